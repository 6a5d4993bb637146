"""mix= on the MI355X (mj_mix; BatchDecoder.decode_device(size=..., mix=...)): MixUp and CutMix over the finished outputs of a call.
The expected elements of every case are tools/mix_model.py — which tests/test_mix_host.py holds to torch's CPU expressions, bit for
bit — applied to the library's own output of the same call without mix=.  Bit patterns, in every layout."""
import numpy as np
import pytest

from mix_cases import DTYPES, FLOATS, LAMS, LAYOUTS, entries_for, model_mix, pairings, same_bits, single_boxes, storage
from test_colour import C440, GREY, KINDS, ODD, raw

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_DEC = {}


@pytest.fixture(scope="module", autouse=True)
def decoders():
    yield
    for dec in _DEC.values():
        dec.close()
    _DEC.clear()


def decoder(layout):
    if layout not in _DEC:
        from pyjpegdecoder_amd import BatchDecoder
        _DEC[layout] = BatchDecoder(device=0, layout=layout)
    return _DEC[layout]


def held_to_the_model(layout, names, mixes, el="uint8", what=None, **kw):
    """the call (``kw``) with every list of ``mixes`` as mix= against the model applied to the same call without it — ``el``: the
    output's element type by name —; returns (without, [with ...]) in storage types"""
    dec = decoder(layout)
    files = [raw(n) for n in names]
    base = storage(dec.decode_device(files, **kw))
    results = []
    for j, mix in enumerate(mixes):
        got = storage(dec.decode_device(files, mix=mix, **kw))
        want = model_mix(base, mix, layout, el)
        assert got.shape == want.shape and got.dtype == want.dtype
        for k in range(len(want)):
            assert same_bits(got[k], want[k]), (what, layout, el, "list", j, "output", k, mix[k])
        assert not same_bits(got, base), (what, j, "the mix changes nothing")
        results.append(got)
    return base, results


def output_kw(dtype):
    if dtype == "uint8":
        return {}
    return dict(dtype=dtype, normalize=(MEAN, STD)) if dtype == "float16" else dict(dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_four_kinds_of_file_in_every_dtype(layout, dtype):
    """several plans into one tensor, so that an output's partner is another plan's: mixup / None / cutmix / mixup with the roll
    pairing, then with the flip pairing"""
    W, H = 40, 28
    p = pairings(4)
    base, (rolled, flipped) = held_to_the_model(layout, KINDS, [entries_for(4, p["roll"], W, H, dtype, 0), entries_for(4, p["flip"], W, H, dtype, 3)],
                                                dtype, size=(W, H), mode="RGB", **output_kw(dtype))
    assert same_bits(rolled[1], base[1]) and same_bits(flipped[1], base[1])
    assert not same_bits(rolled[0], flipped[0])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_box_list_and_the_lams(layout):
    """views of one file on a 23 x 17 canvas — slots of 1173, 2346 and 4692 bytes, none a multiple of 16 —: every single box and every
    lam, the 3-cycle pairing and the outputs their own partners"""
    W, H = 23, 17
    boxes = list(single_boxes(W, H).values())
    n = len(boxes)
    views = [(0, (3 * k, 2 * k, 40, 30)) for k in range(n)]         # (windows of the 70 x 50 file, all different)
    p = pairings(n)
    for dtype in DTYPES:
        mixes = [[("cutmix", p["cycle3"][k], boxes[k]) for k in range(n)], [("cutmix", p["roll"][k], boxes[(k + 4) % n]) for k in range(n)]]
        if dtype != "uint8":
            mixes += [[("mixup", p["flip"][k], LAMS[k % len(LAMS)]) for k in range(n)], [("mixup", k, LAMS[(k + 2) % len(LAMS)]) for k in range(n)]]
        held_to_the_model(layout, [ODD], mixes, dtype, what=(W, H), size=(W, H), views=views, **output_kw(dtype))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_float16_products_in_the_subnormal_range(layout):
    """lam = 1e-5: the output's own share is rounded to float16 as a subnormal (or to zero) before the sum"""
    W, H = 23, 17
    mix = [("mixup", (k - 1) % 4, 1e-5) for k in range(4)]
    base, (got,) = held_to_the_model(layout, KINDS, [mix], "float16", size=(W, H), mode="RGB", dtype="float16", normalize=(MEAN, STD))
    own = np.abs(base.astype(np.float32)) * np.float32(1e-5)
    assert ((own > 0) & (own < 6.2e-5)).any(), "no product in float16's subnormal range"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_component(layout):
    W, H = 23, 17
    p = pairings(4)
    for dtype in ("uint8", "bfloat16"):
        held_to_the_model(layout, KINDS, [entries_for(4, p["roll"], W, H, dtype, 1), entries_for(4, p["cycle3"], W, H, dtype, 5)], dtype,
                          size=(W, H), mode="L", **output_kw(dtype))
    # grey files in their own mode (the same file twice, one mirrored: the outputs differ)
    held_to_the_model(layout, [GREY, GREY], [[("cutmix", 1, (1, 1, 5, 3)), ("cutmix", 0, (0, 0, W, H))]], "uint8", size=(W, H), mirror=[False, True])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_behind_everything_else(layout):
    """with mirror= — boxes are not mirrored —, with color_ops=, with resize_to= and fill=, and with erase=: the mix reads ERASED
    partners, and erased elements of the output itself are blended"""
    W, H = 24, 16
    p = pairings(4)
    f16 = dict(dtype="float16", normalize=(MEAN, STD))
    mixes = [entries_for(4, p["roll"], W, H, "float16", 2), entries_for(4, p["flip"], W, H, "float16", 7)]
    held_to_the_model(layout, KINDS, mixes, "float16", "mirror", size=(W, H), mode="RGB", mirror=[True, False, True, True], **f16)
    held_to_the_model(layout, KINDS, mixes, "float16", "color_ops", size=(W, H), mode="RGB", mirror=[False, True, False, True],
                      color_ops=[[("contrast", 1.4)], None, [("equalize",), ("gaussian_blur", 1.0)], [("adjust_hue", 0.2)]], **f16)
    held_to_the_model(layout, KINDS, [entries_for(4, p["cycle3"], W, H, "uint8", 1)], "uint8", "places", size=(W, H), mode="RGB",
                      resize_to=[(12, 8), (30, 10), (24, 16), (8, 20)], place=[(0, 0), (-3, 3), (0, 0), (10, -2)], fill=(114, 7, 200))
    erase = [(2, 2, 9, 7, 1.5), None, [(0, 0, 5, 5, [0.25, -0.5, 3.0]), (20, 10, 4, 6)], (10, 3, 6, 6, -2.0)]
    mix = [("cutmix", 3, (8, 2, 10, 9)), ("mixup", 0, 0.4), ("mixup", 1, 0.7), None]
    base, (got,) = held_to_the_model(layout, KINDS, [mix], "float16", "erase", size=(W, H), mode="RGB", erase=erase, **f16)
    plain = storage(decoder(layout).decode_device([raw(n) for n in KINDS], size=(W, H), mode="RGB", **f16))
    assert not same_bits(base, plain)           # (the erase is part of what the mix read)
    assert same_bits(got[3], base[3])


def test_nothing_to_mix_is_the_call_without_the_argument(monkeypatch):
    """entries that are all None: no mix launch and no second tensor — the tensor the plans wrote is the one handed out"""
    from pyjpegdecoder_amd import _binding as B
    dec = decoder("rowmajor")
    files = [raw(n) for n in KINDS]
    kw = dict(size=(24, 16), mode="RGB")
    base = storage(dec.decode_device(files, **kw))
    launches = []
    real = B.Context.mix
    monkeypatch.setattr(B.Context, "mix", lambda self, *a, **k: (launches.append(a), real(self, *a, **k))[1])
    for none in (None, [None] * 4):
        assert same_bits(storage(dec.decode_device(files, mix=none, **kw)), base), none
    assert not launches
    got = dec.decode_device(files, mix=[None, ("cutmix", 0, (0, 0, 3, 3)), None, None], **kw)
    assert len(launches) == 1 and got.shape == base.shape


def test_on_a_stream_of_the_callers():
    """the launch goes on torch's current stream: a caller's stream, and what is queued behind it there sees the result"""
    import torch
    dec = decoder("planar_rowmajor")
    files = [raw(n) for n in KINDS]
    kw = dict(size=(40, 28), mode="RGB", dtype="float32")
    mix = [("mixup", (k - 1) % 4, 0.3) for k in range(4)]
    base = storage(dec.decode_device(files, **kw))
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        got = dec.decode_device(files, mix=mix, **kw)
        twice = got * 2
    s.synchronize()
    want = model_mix(base, mix, "planar_rowmajor", "float32")
    assert same_bits(storage(got), want) and same_bits(storage(twice), want * 2)


def test_what_the_call_refuses_before_any_file_is_read():
    dec = decoder("rowmajor")
    not_files = [b"not a jpeg", b"nor this"]
    for kw, msg in [(dict(mix=[("mixup", 1, 0.5), None]), "mix needs size"),
                    (dict(mix=[("mixup", 1, 0.5)], size=(8, 8), dtype="float16"), "mix has 1 entries for 2 outputs"),
                    (dict(mix=[("mixup", 1, 0.5), None], size=(8, 8)), "output 0: \"mixup\" needs a float output"),
                    (dict(mix=[None, ("mixup", 2, 0.5)], size=(8, 8), dtype="float16"), "output 1: partner 2 is not"),
                    (dict(mix=[None, ("cutmix", 0, (4, 4, 5, 1))], size=(8, 8)), "output 1: box .4, 4, 5, 1. is not inside the 8 x 8 canvas"),
                    (dict(mix=[None, ("mixup", 0, 2.0)], size=(8, 8), normalize=(MEAN, STD)), "output 1: lam 2.0 is not"),
                    (dict(mix=[None, None], size=(8, 8), also=[dict(size=(4, 4), mix=[("swap", 0, 0.5), None])]), r"also\[0\]: mix: output 0: unknown op 'swap'")]:
        with pytest.raises(ValueError, match=msg):
            dec.decode_device(not_files, **kw)
        with pytest.raises(ValueError, match=msg):
            dec.decode(not_files, **kw)


# ---- at the C ABI ----------------------------------------------------------------------------------------------------------
def _slots(n, W, H, C, layout, dtype, seed):
    from erase_cases import STORAGE, shape_of
    rng = np.random.default_rng(seed)
    shape = (n,) + shape_of(layout, W, H, C)
    if dtype == "uint8":
        return rng.integers(0, 256, size=shape).astype(np.uint8)
    vals = (rng.standard_normal(shape) * 2).astype(np.float32)
    from tools.erase_model import to_storage
    return to_storage(vals, dtype).astype(STORAGE[dtype], copy=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_pointers_inside_sentinel_filled_buffers(layout, dtype):
    """src and dst inside larger buffers, element-aligned but not 16-byte aligned: congruent mod 16 (the vector path, with a head and
    a tail per slot), not congruent (element by element), and — for multi-byte elements — not aligned to their elements at all; dst is
    written in full and the sentinels around it stay"""
    import torch
    from pyjpegdecoder_amd import _binding as B
    W, H, C, n = 23, 17, 3, 4
    dec = decoder(layout)
    es = B.DTYPE_BYTES[dtype]
    pre = _slots(n, W, H, C, layout, dtype, 5)
    nbytes = pre.nbytes
    entries = entries_for(n, pairings(n)["roll"], W, H, dtype, 1)
    want = model_mix(pre, entries, layout, dtype)
    offsets = [(64 + 3 * es, 64 + 3 * es), (64 + 3 * es, 64 + 5 * es), (32 + es, 48 + es)] + ([(65, 65), (65, 67)] if es > 1 else [])
    for front_s, front_d in offsets:
        src = torch.full((front_s + nbytes + 61,), 0x5A, dtype=torch.uint8, device="cuda:0")
        dst = torch.full((front_d + nbytes + 61,), 0xA5, dtype=torch.uint8, device="cuda:0")
        src[front_s:front_s + nbytes] = torch.from_numpy(pre.reshape(-1).view(np.uint8)).to("cuda:0")
        torch.cuda.synchronize()
        dec.ctx.mix(src.data_ptr() + front_s, dst.data_ptr() + front_d, LAYOUTS.index(layout), dtype, C, W, H, entries)
        torch.cuda.synchronize()            # (the context's stream is not torch's: wait for the device)
        got = dst.cpu().numpy()
        assert (got[:front_d] == 0xA5).all() and (got[front_d + nbytes:] == 0xA5).all(), ("a sentinel was written", front_s, front_d)
        assert same_bits(got[front_d:front_d + nbytes].copy().view(pre.dtype).reshape(pre.shape), want), (front_s, front_d)
        kept = src.cpu().numpy()
        assert same_bits(kept[front_s:front_s + nbytes], pre.reshape(-1).view(np.uint8)) and (kept[:front_s] == 0x5A).all()


def test_two_calls_in_a_row_on_two_streams():
    """different records, different streams, back to back: the second call must not rewrite the records under the first launch"""
    import torch
    W, H, C, n = 40, 28, 3, 6
    layout, dtype = "rowmajor", "float16"
    dec = decoder(layout)
    pre = _slots(n, W, H, C, layout, dtype, 9)
    p = pairings(n)
    first = [("mixup", p["roll"][k], 0.3) for k in range(n)]
    second = [("cutmix", p["flip"][k], (5 + k, 3, 20, 10 + k)) for k in range(n)]
    src = torch.from_numpy(pre).to("cuda:0")
    a, b = torch.zeros_like(src), torch.zeros_like(src)
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    args = (LAYOUTS.index(layout), dtype, C, W, H)
    dec.ctx.mix(src.data_ptr(), a.data_ptr(), *args, first, stream=s1.cuda_stream)
    dec.ctx.mix(src.data_ptr(), b.data_ptr(), *args, second, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert same_bits(storage(a), model_mix(pre, first, layout, dtype))
    assert same_bits(storage(b), model_mix(pre, second, layout, dtype))


def test_what_mj_mix_refuses():
    import torch
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.errors import BackendError
    dec = decoder("rowmajor")
    W, H = 10, 8
    src = torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda:0")
    dst = torch.zeros_like(src)
    u8s, u8d = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda:0"), torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda:0")

    def mix(entries, s=None, d=None, layout=1, dtype="float32", C=3, w=W, h=H):
        dec.ctx.mix(src.data_ptr() if s is None else s, dst.data_ptr() if d is None else d, layout, dtype, C, w, h, entries)
    for entries, msg in [([None, B.MixOpC(3, 0, 0, 0, 1, 1, 0.5)], "mj_mix: output 1 .kind 3, partner 0.: a kind that is none of"),
                         ([("mixup", 2, 0.5), None], "output 0 .*no such partner"),
                         ([None, ("cutmix", -1, (0, 0, 1, 1))], "output 1 .*no such partner"),
                         ([("mixup", 0, float("inf")), None], "output 0 .*lam is not a finite number in 0..1"),
                         ([("mixup", 0, 1.5), None], "lam is not a finite number in 0..1"),
                         ([None, ("cutmix", 0, (0, 0, 1, 0))], "output 1 .*a width or height below 1"),
                         ([None, ("cutmix", 0, (8, 0, 3, 1))], "output 1 .*not inside the canvas")]:
        with pytest.raises(BackendError, match=msg):
            mix(entries)
    with pytest.raises(BackendError, match="output 1 .*mixup on a uint8 output"):
        mix([None, ("mixup", 0, 0.5)], u8s.data_ptr(), u8d.data_ptr(), dtype="uint8")
    ok = [None, None]
    for kw, msg in [(dict(d=src.data_ptr()), "src and dst overlap"), (dict(d=src.data_ptr() + 64), "src and dst overlap"),
                    (dict(layout=4), "layout 4"), (dict(C=2), "2 components"), (dict(w=0), "0 x 8"), (dict(h=65536), "10 x 65536")]:
        with pytest.raises(BackendError, match=msg):
            mix(ok, **kw)
    lib, h = dec.ctx.lib, dec.ctx.handle
    ops, _keep = B.mix_ops(ok)
    f32 = B.DTYPES["float32"]
    assert lib.mj_mix(h, None, None, dst.data_ptr(), 1, f32, 3, W, H, 2, ops) == B.MJ_ERR_INVALID and b"NULL" in lib.mj_last_error(h)
    assert lib.mj_mix(h, None, src.data_ptr(), dst.data_ptr(), 1, f32, 3, W, H, 2, None) == B.MJ_ERR_INVALID and b"NULL" in lib.mj_last_error(h)
    assert lib.mj_mix(h, None, src.data_ptr(), dst.data_ptr(), 1, 9, 3, W, H, 2, ops) == B.MJ_ERR_INVALID and b"dtype 9" in lib.mj_last_error(h)
    assert lib.mj_mix(h, None, src.data_ptr(), dst.data_ptr(), 1, f32, 3, W, H, 0, ops) == B.MJ_ERR_INVALID and b"0 outputs" in lib.mj_last_error(h)
    # a refused call launched nothing
    torch.cuda.synchronize()
    assert not dst.any().item()
