"""mix= without a GPU: tools/mix_model.py against torch's CPU expressions — the roll form, timm's flip form, a per-sample-lam loop,
CutMix's slice assignment —, mj_host_mix — the mix launch's own rule and box test — against the model on exactly sized buffers,
normalize_mix's and mj_host_mix's refusals by message, and cutmix_box."""
import math

import numpy as np
import pytest

from mix_cases import DTYPES, FLOATS, LAMS, LAYOUTS, STORAGE, entries_for, pairings, same_bits, shape_of, single_boxes, storage

CANVASES = ((23, 17), (24, 16))


def _chw_to(layout, nchw):
    """an (N, C, H, W) array as the outputs of a decoder of ``layout``"""
    C = nchw.shape[1]
    if C == 1:
        return np.ascontiguousarray(nchw[:, 0] if layout in ("rowmajor", "planar_rowmajor") else nchw[:, 0].transpose(0, 2, 1))
    return np.ascontiguousarray({"xmajor": nchw.transpose(0, 3, 2, 1), "rowmajor": nchw.transpose(0, 2, 3, 1), "planar": nchw.transpose(0, 1, 3, 2),
                                 "planar_rowmajor": nchw}[layout])


def _batch(dtype, N=5, C=3, H=17, W=23, seed=1):
    """random normalised values with +-0, the largest finite value and tiny values among them"""
    import torch
    g = torch.Generator().manual_seed(seed)
    if dtype == "uint8":
        return torch.randint(0, 256, (N, C, H, W), generator=g, dtype=torch.uint8)
    tdt = getattr(torch, dtype)
    x = (torch.randn((N, C, H, W), generator=g) * 2.2).to(tdt)
    fi = torch.finfo(tdt)
    special = torch.tensor([0.0, -0.0, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.tiny / 4, fi.smallest_normal * 3, 1e-5, -3e-7, 65000.0, 1.0], dtype=torch.float32).to(tdt)
    flat = x.reshape(N, -1)
    for k in range(N):                  # (at different places in every sample, so that specials meet ordinary values and each other)
        flat[k, 7 * k:7 * k + special.numel()] = special.roll(k)
    return x


@pytest.mark.parametrize("dtype", FLOATS)
def test_the_model_is_torchs_roll_form(dtype):
    """pre.roll(1, 0).mul(1.0 - lam).add_(pre.mul(lam)): torchvision's MixUp, in bit patterns; the four layouts through transposes"""
    from tools import mix_model
    pre = _batch(dtype)
    N = pre.shape[0]
    for lam in LAMS:
        want = storage(pre.roll(1, 0).mul(1.0 - lam).add_(pre.mul(lam)))
        entries = [("mixup", (k - 1) % N, lam) for k in range(N)]
        for layout in LAYOUTS:
            got = mix_model.mix(_chw_to(layout, storage(pre)), entries, layout, dtype)
            assert same_bits(got, _chw_to(layout, want)), (lam, layout)


@pytest.mark.parametrize("dtype", FLOATS)
def test_the_model_is_timms_flip_form(dtype):
    """x_flipped = x.flip(0).mul_(1. - lam); x.mul_(lam).add_(x_flipped) — on a clone — and lam = 1 - lam' as timm's cutmix-off path"""
    from tools import mix_model
    pre = _batch(dtype, seed=2)
    N = pre.shape[0]
    for lam in LAMS:
        x = pre.clone()
        flipped = x.flip(0).mul_(1. - lam)
        x.mul_(lam).add_(flipped)
        got = mix_model.mix(storage(pre), [("mixup", N - 1 - k, lam) for k in range(N)], "planar_rowmajor", dtype)
        assert same_bits(got, storage(x)), lam


@pytest.mark.parametrize("dtype", FLOATS)
def test_the_model_with_a_lam_per_sample(dtype):
    """timm's mode="elem": x[i] = x[i] * lam_i + x_orig[j] * (1 - lam_i), every pairing, the output its own partner included"""
    from tools import mix_model
    pre = _batch(dtype, seed=3)
    N = pre.shape[0]
    for name, partners in pairings(N).items():
        lams = [LAMS[(k + 1) % len(LAMS)] for k in range(N)]
        want = pre.clone()
        for k in range(N):
            want[k] = pre[partners[k]].mul(1.0 - lams[k]).add_(pre[k].mul(lams[k]))
        got = mix_model.mix(storage(pre), [("mixup", partners[k], lams[k]) for k in range(N)], "planar_rowmajor", dtype)
        assert same_bits(got, storage(want)), name
    own = mix_model.mix(storage(pre), [("mixup", k, 0.3) for k in range(N)], "planar_rowmajor", dtype)
    assert not same_bits(own, storage(pre)), "partner == k still runs the arithmetic"


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_model_is_torchs_cutmix(dtype):
    """out = pre.clone(); out[..., y:y+h, x:x+w] = pre.roll(1, 0)[..., y:y+h, x:x+w], every single box, four layouts"""
    from tools import mix_model
    W, H = 23, 17
    pre = _batch(dtype, N=3, seed=4)
    rolled = pre.roll(1, 0)
    for name, (x, y, w, h) in single_boxes(W, H).items():
        want = pre.clone()
        want[..., y:y + h, x:x + w] = rolled[..., y:y + h, x:x + w]
        entries = [("cutmix", (k - 1) % 3, (x, y, w, h)) for k in range(3)]
        for layout in LAYOUTS:
            got = mix_model.mix(_chw_to(layout, storage(pre)), entries, layout, dtype)
            assert got.shape == (3,) + shape_of(layout, W, H, 3)
            assert same_bits(got, _chw_to(layout, storage(want))), (name, layout)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_host_twin_against_the_model(layout, C, dtype):
    """mj_host_mix on exactly sized arrays: every pairing with mixed kinds, every lam with every output, every single box"""
    from pyjpegdecoder_amd import _binding as B
    from tools import mix_model
    li = LAYOUTS.index(layout)
    for (W, H) in CANVASES:
        N = 5
        pre = _chw_to(layout, storage(_batch(dtype, N=N, C=C, H=H, W=W, seed=W + C)))
        assert pre.shape == (N,) + shape_of(layout, W, H, C)
        lists = [entries_for(N, partners, W, H, dtype, seed) for seed, partners in enumerate(pairings(N).values())]
        roll = pairings(N)["roll"]
        if dtype != "uint8":
            lists += [[("mixup", roll[k], lam) for k in range(N)] for lam in LAMS]
        boxes = list(single_boxes(W, H).values())
        lists += [[("cutmix", roll[k], boxes[(j + k) % len(boxes)]) for k in range(N)] for j in range(0, len(boxes), N)]
        changed = 0
        for entries in lists:
            got = B.host_mix(pre, li, dtype, C, W, H, entries)
            want = mix_model.mix(pre, entries, layout, dtype)
            for k in range(N):
                assert same_bits(got[k], want[k]), (layout, C, dtype, (W, H), entries[k])
                assert (entries[k] is None) <= same_bits(got[k], pre[k])
            changed += not same_bits(got, pre)
        # (a CutMix from the output itself and a MixUp with lam = 1.0 may change nothing: at most two lists)
        assert changed >= len(lists) - 2


def test_what_normalize_mix_refuses():
    from pyjpegdecoder_amd.batch import normalize_mix
    size = (10, 8)
    assert normalize_mix(None, None) is None
    assert normalize_mix([None, None], size, 2) is None
    ok = normalize_mix([("mixup", 1, 0.25), None, ["cutmix", np.int64(0), [1, 2, 3, 4]]], size, 3, "float16")
    assert ok == [("mixup", 1, 0.25), None, ("cutmix", 0, (1, 2, 3, 4))]
    assert normalize_mix([("cutmix", 0, (0, 0, 10, 8))], size, 1, "uint8") == [("cutmix", 0, (0, 0, 10, 8))]
    for args, msg in [
        (([("mixup", 0, 0.5)], None), "mix needs size"),
        (([("mixup", 0, 0.5)], size, 1, "float32", True), "mix and return_seams do not go together"),
        ((("mixup", 0, 0.5), size), "there is no one-for-all form"),
        (("mixup", size), "there is no one-for-all form"),
        (([("mixup", 0, 0.5)], size, 2), "mix has 1 entries for 2 outputs"),
        (([None, ("blend", 0, 0.5)], size), "output 1: unknown op 'blend'"),
        (([None, ("mixup", 0)], size), "output 1: an entry is None"),
        (([("mixup", 1, 0.5)], size), "output 0: partner 1 is not the index of an output, an integer 0..0"),
        (([None, ("cutmix", -1, (0, 0, 1, 1))], size), "output 1: partner -1 is not"),
        (([("mixup", 0.0, 0.5)], size), "output 0: partner 0.0 is not"),
        (([("mixup", True, 0.5), None], size), "output 0: partner True is not"),
        (([("mixup", 0, float("nan"))], size), "output 0: lam nan is not a finite number in 0..1"),
        (([("mixup", 0, float("inf"))], size), "lam inf is not"),
        (([("mixup", 0, 1.5)], size), "lam 1.5 is not"),
        (([("mixup", 0, -0.1)], size), "lam -0.1 is not"),
        (([("mixup", 0, "0.5")], size), "lam '0.5' is not"),
        (([None, ("mixup", 0, 0.5)], size, 2, "uint8"), "output 1: \"mixup\" needs a float output"),
        (([("cutmix", 0, (0, 0, 1))], size), "output 0: a box is four integers"),
        (([("cutmix", 0, (0, 0, 1.5, 1))], size), "a box is four integers"),
        (([("cutmix", 0, 0.5)], size), "a box is four integers"),
        (([("cutmix", 0, (0, 0, 0, 1))], size), "width and height must be at least 1, not 0 x 1"),
        (([("cutmix", 0, (0, 0, 2, -1))], size), "width and height must be at least 1"),
        (([("cutmix", 0, (8, 0, 3, 1))], size), r"box \(8, 0, 3, 1\) is not inside the 10 x 8 canvas"),
        (([("cutmix", 0, (0, 7, 1, 2))], size), "is not inside the 10 x 8 canvas"),
        (([("cutmix", 0, (-1, 0, 2, 2))], size), "is not inside the 10 x 8 canvas"),
    ]:
        with pytest.raises(ValueError, match=msg):
            normalize_mix(*args)


def test_mix_is_a_key_of_an_also_entry():
    from pyjpegdecoder_amd.batch import ALSO_PER_OUTPUT, normalize_also
    assert "mix" in ALSO_PER_OUTPUT
    call = dict(dtype="float16")
    groups = normalize_also([dict(size=(8, 8), mix=[("mixup", 0, 0.5)])], call, (10, 8))
    assert groups[0]["mix"] == [("mixup", 0, 0.5)] and groups[0]["dtype"] == "float16"
    assert normalize_also([dict(size=(8, 8))], dict(call, mix=[("mixup", 0, 0.5)]), (10, 8))[0]["mix"] is None      # (never the call's)
    with pytest.raises(ValueError, match=r"also\[0\]: mix: output 0: box \(7, 0, 2, 1\) is not inside the 8 x 8 canvas"):
        normalize_also([dict(size=(8, 8), mix=[("cutmix", 0, (7, 0, 2, 1))])], call, (10, 8))


def test_what_the_host_twin_refuses():
    import ctypes
    from pyjpegdecoder_amd import _binding as B
    W, H = 10, 8
    pre = np.zeros((2, H, W, 3), dtype=np.float32)
    for entries, msg in [
        ([None, B.MixOpC(3, 0, 0, 0, 1, 1, 0.5)], "output 1 .kind 3, partner 0.: a kind that is none of"),
        ([("mixup", 2, 0.5), None], "output 0 .*no such partner"),
        ([None, ("cutmix", -1, (0, 0, 1, 1))], "output 1 .*no such partner"),
        ([("mixup", 0, float("nan")), None], "output 0 .*lam is not a finite number in 0..1"),
        ([("mixup", 0, 1.0000001), None], "lam is not a finite number in 0..1"),
        ([("mixup", 0, -1e-9), None], "lam is not a finite number in 0..1"),
        ([None, ("cutmix", 0, (0, 0, 0, 1))], "output 1 .cutmix, partner 0, x 0, y 0, 0 x 1.: a width or height below 1"),
        ([None, ("cutmix", 0, (8, 0, 3, 1))], "not inside the canvas"),
        ([None, ("cutmix", 0, (0, 7, 1, 2))], "not inside the canvas"),
        ([None, ("cutmix", 0, (0, -1, 1, 2))], "not inside the canvas"),
    ]:
        with pytest.raises(ValueError, match=msg):
            B.host_mix(pre, B.MJ_LAYOUT_ROWMAJOR, "float32", 3, W, H, entries)
    with pytest.raises(ValueError, match="output 1 .*mixup on a uint8 output"):
        B.host_mix(pre.astype(np.uint8), B.MJ_LAYOUT_ROWMAJOR, "uint8", 3, W, H, [None, ("mixup", 0, 0.5)])
    L = B.load_library()
    ops, _keep = B.mix_ops([None, None])
    dst = np.empty_like(pre)
    p, d = pre.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p)

    def refused(*args):
        assert L.mj_host_mix(*args) == B.MJ_ERR_INVALID
        return L.mj_last_error(None).decode()
    f32 = B.DTYPES["float32"]
    assert "NULL" in refused(None, d, 1, f32, 3, W, H, 2, ops)
    assert "NULL" in refused(p, None, 1, f32, 3, W, H, 2, ops)
    assert "NULL" in refused(p, d, 1, f32, 3, W, H, 2, None)
    assert "layout 4" in refused(p, d, 4, f32, 3, W, H, 2, ops)
    assert "dtype 7" in refused(p, d, 1, 7, 3, W, H, 2, ops)
    assert "2 components" in refused(p, d, 1, f32, 2, W, H, 2, ops)
    assert "0 x 8" in refused(p, d, 1, f32, 3, 0, H, 2, ops)
    assert "10 x 65536" in refused(p, d, 1, f32, 3, W, 65536, 2, ops)
    assert "0 outputs" in refused(p, d, 1, f32, 3, W, H, 0, ops)
    assert "overlap" in refused(p, p, 1, f32, 3, W, H, 2, ops)
    inside = ctypes.c_void_p(pre.ctypes.data + pre[0].nbytes)         # (src's second slot)
    assert "overlap" in refused(p, inside, 1, f32, 3, W, H, 2, ops)
    assert "overlap" in refused(p, ctypes.c_void_p(pre.ctypes.data + 4), 1, f32, 3, W, H, 2, ops)
    assert L.mj_host_mix(p, inside, 1, f32, 3, W, H, 1, ops) == B.MJ_OK  # (one slot each, side by side: no overlap)
    # (a byte count that would wrap 64 bits is refused before the overlap test, which it would pass wrongly)
    assert "more than an address holds" in refused(p, p, 1, f32, 3, 65535, 65535, 2**31 - 1, ops)


def test_cutmix_box():
    import torch
    from pyjpegdecoder_amd import cutmix_box
    from pyjpegdecoder_amd.batch import normalize_mix
    g = torch.Generator().manual_seed(5)
    for (W, H) in ((224, 224), (23, 17), (5, 40)):
        for lam in (0.0, 0.1, 0.37, 0.5, 0.8, 0.95):
            for _ in range(20):
                box, adj = cutmix_box((W, H), lam, generator=g)
                if box is None:
                    assert adj == 1.0
                    continue
                x, y, w, h = box
                assert w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= W and y + h <= H
                assert w <= 2 * int(0.5 * math.sqrt(1 - lam) * W) and h <= 2 * int(0.5 * math.sqrt(1 - lam) * H)
                assert adj == 1.0 - w * h / float(W * H)
                assert normalize_mix([("cutmix", 0, box)], (W, H), 1) == [("cutmix", 0, box)]
    assert cutmix_box((224, 224), 1.0, generator=g) == (None, 1.0)        # (r = 0: an empty box)
    assert cutmix_box((3, 3), 0.9, generator=g) == (None, 1.0)            # (half sides that round to 0)
    box, adj = cutmix_box((224, 224), 0.0, generator=g)
    assert box is not None and adj < 1.0
    with pytest.raises(ValueError, match="lam 1.5"):
        cutmix_box((8, 8), 1.5)
