"""erase= without a GPU: tools/erase_model.py against torch's slice assignment on the CPU, mj_host_erase — the erase launch's own
address arithmetic — against the model with guard elements around every slot, normalize_erase's acceptances and refusals by
message, _Request.narrow carrying boxes, and random_erasing_rect."""
import math

import numpy as np
import pytest

from erase_cases import DTYPES, LAYOUTS, STORAGE, box_cases, same_bits, shape_of, storage, with_values

CANVASES = ((23, 17), (40, 28))


def _chw_to(layout, chw):
    """a (C, H, W) array as one output in ``layout``"""
    C = chw.shape[0]
    if C == 1:
        return np.ascontiguousarray(chw[0] if layout in ("rowmajor", "planar_rowmajor") else chw[0].T)
    return np.ascontiguousarray({"xmajor": chw.transpose(2, 1, 0), "rowmajor": chw.transpose(1, 2, 0), "planar": chw.transpose(0, 2, 1),
                                 "planar_rowmajor": chw}[layout])


def _torch_image(C, H, W, dtype, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    if dtype == "uint8":
        return torch.randint(0, 256, (C, H, W), generator=g, dtype=torch.uint8)
    return torch.randn((C, H, W), generator=g).to(getattr(torch, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 3])
def test_the_model_is_torchs_slice_assignment(dtype, C):
    """x[..., y:y+h, x:x+w] = v on CHW tensors, for a number, per-component values and a (C, h, w) float32 tensor; floats as bit
    patterns; the other three layouts against the transposed result"""
    import torch
    from tools import erase_model
    W, H = 23, 17
    img = _torch_image(C, H, W, dtype, 5)
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(11)
    for name, boxes in box_cases(W, H).items():
        vboxes = with_values(boxes, C, dtype, 3)
        want = img.clone()
        for (x, y, w, h, v) in vboxes:
            if isinstance(v, np.ndarray):
                tv = torch.from_numpy(v)
            elif isinstance(v, list):
                tv = torch.tensor(v)[:, None, None]
            else:
                tv = torch.tensor(v)
            want[..., y:y + h, x:x + w] = tv.to(tdt) if isinstance(v, np.ndarray) else tv
        want = storage(want)
        for layout in LAYOUTS:
            got = erase_model.erase(_chw_to(layout, storage(img)), vboxes, layout, dtype)
            assert got.shape == shape_of(layout, W, H, C)
            assert same_bits(got, _chw_to(layout, want)), (name, layout)
    del rng


def test_a_constant_is_rounded_to_float32_first():
    """0.5 + 2^-12 + 2^-40 as a float64 rounds UP to float16 directly; to float32 first it loses the 2^-40, is then the midpoint of
    two float16 neighbours and ties to even, DOWN: torch.tensor(v) is float32, and so are the model's and the library's constants"""
    import torch
    from pyjpegdecoder_amd import _binding as B
    from tools import erase_model
    h = np.float16(0.5)
    v = float(h) + 2.0 ** -12 + 2.0 ** -40            # just above the midpoint between two float16 neighbours of 0.5
    assert np.float16(v) != np.float16(np.float32(v)), "the value does not double-round"
    x = torch.zeros((1, 4, 4), dtype=torch.float16)
    x[..., 1:3, 1:3] = torch.tensor(v)
    base = np.zeros((4, 4), dtype=np.float16)
    got = erase_model.erase(base, [(1, 1, 2, 2, v)], "rowmajor")
    assert same_bits(got, x[0].numpy())
    lib = base.copy()
    B.host_erase(lib, B.MJ_LAYOUT_ROWMAJOR, "float16", 1, 4, 4, 1, [(0, 1, 1, 2, 2, v)])
    assert same_bits(lib, got)


def test_an_array_is_rounded_once_from_its_own_type():
    import torch
    from tools import erase_model
    rng = np.random.default_rng(2)
    v64 = rng.standard_normal((3, 5, 4)) * 3
    for dtype in ("float16", "bfloat16", "float32"):
        want = torch.from_numpy(v64).to(getattr(torch, dtype))
        got = erase_model.erase(np.zeros((3, 5, 4), dtype=STORAGE[dtype]), [(0, 0, 4, 5, v64)], "planar_rowmajor", dtype)
        assert same_bits(got, storage(want)), dtype


GUARD = 3


def _guarded(layout, C, W, H, dtype, seed):
    """three slots with GUARD elements in front, behind and between them: (flat array, element offset of slot 0, slot stride)"""
    rng = np.random.default_rng(seed)
    n = W * H * C
    flat = rng.integers(1, 200, size=GUARD + 3 * n + GUARD).astype(STORAGE[dtype])
    return flat, GUARD, n


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_host_twin_against_the_model(layout, C, dtype):
    """mj_host_erase over the middle slot of three, guards in front and behind and the neighbouring slots as guards: only the boxes'
    elements change, to the model's values — for every box of the list, constants and values; the two orders of the overlapping
    pair differ"""
    from pyjpegdecoder_amd import _binding as B
    from tools import erase_model
    li = LAYOUTS.index(layout)
    for (W, H) in CANVASES:
        results = {}
        for name, boxes in box_cases(W, H).items():
            vboxes = with_values(boxes, C, dtype, 7)
            flat, at, n = _guarded(layout, C, W, H, dtype, 13)
            before = flat.copy()
            blocks, rects, off = [], [], 0
            for (x, y, w, h, v) in vboxes:
                if isinstance(v, np.ndarray):
                    sv = erase_model.to_storage(v, dtype).reshape(-1)
                    rects.append((1, x, y, w, h, ("values", off + 2)))
                    blocks.append(sv)
                    off += sv.size
                else:
                    rects.append((1, x, y, w, h, [float(t) for t in (v if isinstance(v, list) else [v] * C)] + [0.0] * (3 - C)))
            values = np.concatenate([np.zeros(2, dtype=STORAGE[dtype])] + blocks) if blocks else None
            B.host_erase(flat, li, dtype, C, W, H, 2, rects, values, offset=at)       # (two slots from `at`: the third is a guard)
            slot = before[at + n:at + 2 * n].reshape(shape_of(layout, W, H, C))
            want = erase_model.erase(slot, vboxes, layout, dtype)
            assert same_bits(flat[at + n:at + 2 * n].reshape(want.shape), want), (name, W, H)
            assert same_bits(flat[:at + n], before[:at + n]) and same_bits(flat[at + 2 * n:], before[at + 2 * n:]), (name, "a guard changed")
            assert not same_bits(want, slot), (name, "the boxes change nothing")
            results[name] = want
        assert not same_bits(results["overlap"], results["overlap_reversed"]), "the order of overlapping boxes does not matter"


def test_the_host_twin_refuses_by_message():
    from pyjpegdecoder_amd import _binding as B
    a = np.zeros(2 * 6 * 5 * 3, dtype=np.uint8)
    v = np.zeros(100, dtype=np.uint8)

    def run(rect, values=None, dtype="uint8", arr=a):
        B.host_erase(arr, B.MJ_LAYOUT_ROWMAJOR, dtype, 3, 6, 5, 2, [rect], values)
    for rect, values, msg in [((2, 0, 0, 1, 1, 0.0), None, "no such output"), ((-1, 0, 0, 1, 1, 0.0), None, "no such output"),
                              ((0, 0, 0, 0, 1, 0.0), None, "a width or height below 1"), ((0, 0, 0, 1, 0, 0.0), None, "a width or height below 1"),
                              ((0, 5, 0, 2, 1, 0.0), None, "not inside the canvas"), ((0, 0, 4, 1, 2, 0.0), None, "not inside the canvas"),
                              ((0, -1, 0, 2, 1, 0.0), None, "not inside the canvas"), ((0, 0, 0, 1, 1, 256.0), None, "integer 0..255"),
                              ((0, 0, 0, 1, 1, 1.5), None, "integer 0..255"), ((0, 0, 0, 1, 1, ("values", 0)), None, "without values"),
                              ((0, 0, 0, 1, 1, ("values", -1)), v, "negative offset")]:
        with pytest.raises(ValueError, match=msg):
            run(rect, values)
        assert not a.any()
    f = np.zeros(2 * 6 * 5 * 3, dtype=np.float32)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="not finite"):
            run((0, 0, 0, 1, 1, bad), dtype="float32", arr=f)
    r = B.EraseRectC(0, 0, 0, 1, 1, 7)
    with pytest.raises(ValueError, match="a kind that is neither"):
        run(r)
    with pytest.raises(ValueError, match="box 0 .output 0, x 5, y 0, 2 x 1."):
        run((0, 5, 0, 2, 1, 0.0))


# ---- normalize_erase -------------------------------------------------------------------------------------------------------
def test_normalize_erase_accepts():
    from pyjpegdecoder_amd.batch import normalize_erase
    size = (10, 8)
    assert normalize_erase(None, size, 2, 3, "uint8") is None
    assert normalize_erase(None, None) is None
    for none in ([None, None], [None, []], [(), None], [[], []]):
        assert normalize_erase(none, size, 2, 3, "uint8") is None, none
    got = normalize_erase([None, (1, 2, 3, 4), [(0, 0, 2, 2, 1.5), (1, 1, 2, 2, (1, 2, 3))]], size, 3, 3, "float16")
    assert got == [None, ((1, 2, 3, 4, (0.0, 0.0, 0.0)),), ((0, 0, 2, 2, (1.5, 1.5, 1.5)), (1, 1, 2, 2, (1.0, 2.0, 3.0)))]
    assert normalize_erase([(0, 0, 10, 8, 255)], size, 1, 1, "uint8") == [((0, 0, 10, 8, (255.0,)),)]
    assert normalize_erase([(np.int64(0), 0, 10, 8, np.float32(0.5))], size, 1, 1, "float32") == [((0, 0, 10, 8, (0.5,)),)]
    assert normalize_erase([(0, 0, 1, 1, 0.1)], size, 1, 1, "float32")[0][0][4] == (float(np.float32(0.1)),)        # float32 first
    v = np.zeros((3, 4, 5), dtype=np.float32)
    got = normalize_erase([(0, 0, 5, 4, v)], size, 1, 3, "bfloat16")
    assert got[0][0][:4] == (0, 0, 5, 4) and got[0][0][4] is v
    assert normalize_erase([(0, 0, 5, 4, np.zeros((3, 4, 5), dtype=np.uint8))], size, 1, 3, "uint8") is not None
    assert normalize_erase([(0, 0, 5, 4, np.array([1.0, 2.0, 3.0]))], size, 1, 3, "float32")[0][0][4] == (1.0, 2.0, 3.0)
    # what is not known yet is not checked: the counts and the components
    assert normalize_erase([(0, 0, 5, 4, (1, 2, 3))], size) is not None
    import torch
    t = torch.zeros((3, 4, 5))
    assert normalize_erase([(0, 0, 5, 4, t)], size, 1, 3, "float16", device=0)[0][0][4] is t


def test_normalize_erase_refuses_by_message():
    from pyjpegdecoder_amd.batch import normalize_erase
    import torch
    size = (10, 8)
    cases = [
        (dict(erase=[(0, 0, 1, 1)], size=None), "erase needs size"),
        (dict(erase=[(0, 0, 1, 1)], size=size, return_seams=True), "erase and return_seams do not go together"),
        (dict(erase=(0, 0, 1, 1), size=size), "no one-for-all form"),
        (dict(erase=5, size=size), "erase must be None or a list"),
        (dict(erase=[None], size=size, n_outputs=2), "erase has 1 entries for 2 outputs"),
        (dict(erase=[None, (0, 0, 1)], size=size), "output 1, box 0: a box is"),
        (dict(erase=[[(0, 0, 1, 1), (0, 0, 1, 1, 0, 0)]], size=size), "output 0, box 1: a box is"),
        (dict(erase=[5], size=size), "output 0: an entry is None, one box or a list of boxes"),
        (dict(erase=[(0.5, 0, 1, 1)], size=size), "output 0, box 0: x, y, width and height must be integers"),
        (dict(erase=[(0, 0, True, 1)], size=size), "must be integers"),
        (dict(erase=[(0, 0, 0, 1)], size=size), "width and height must be at least 1"),
        (dict(erase=[(0, 0, 1, -2)], size=size), "width and height must be at least 1"),
        (dict(erase=[(8, 0, 3, 1)], size=size), r"box \(8, 0, 3, 1\) is not inside the 10 x 8 canvas"),
        (dict(erase=[(0, 7, 1, 2)], size=size), "is not inside"),
        (dict(erase=[(-1, 0, 1, 1)], size=size), "is not inside"),
        (dict(erase=[(0, 0, 1, 1, float("nan"))], size=size), "is not finite"),
        (dict(erase=[(0, 0, 1, 1, float("inf"))], size=size), "is not finite"),
        (dict(erase=[(0, 0, 1, 1, 1e39)], size=size), "is not finite .as float32."),
        (dict(erase=[(0, 0, 1, 1, (1, float("nan"), 2))], size=size, ncomp=3), "is not finite"),
        (dict(erase=[(0, 0, 1, 1, (1, 2))], size=size, ncomp=3), "2 values for 3 component"),
        (dict(erase=[(0, 0, 1, 1, (1, 2, 3))], size=size, ncomp=1), "3 values for 1 component"),
        (dict(erase=[(0, 0, 1, 1, "x")], size=size), "a value is a number"),
        (dict(erase=[(0, 0, 5, 4, np.zeros((3, 5, 4)))], size=size, ncomp=3), r"values of shape \(3, 5, 4\) for a box of \(3, 4, 5\)"),
        (dict(erase=[(0, 0, 5, 4, np.zeros((1, 4, 5)))], size=size, ncomp=3), "values of shape"),
        (dict(erase=[(0, 0, 5, 4, np.zeros((4, 5)))], size=size, ncomp=1), "values of shape"),
        (dict(erase=[(0, 0, 1, 1, 1.5)], size=size, dtype="uint8"), "a uint8 output takes integers 0..255"),
        (dict(erase=[(0, 0, 1, 1, 256)], size=size, dtype="uint8"), "a uint8 output takes integers 0..255"),
        (dict(erase=[(0, 0, 1, 1, -1)], size=size, dtype="uint8"), "a uint8 output takes integers 0..255"),
        (dict(erase=[(0, 0, 5, 4, np.zeros((3, 4, 5), dtype=np.float32))], size=size, ncomp=3, dtype="uint8"), "a uint8 output takes uint8 arrays"),
        (dict(erase=[(0, 0, 5, 4, np.zeros((3, 4, 5), dtype=np.int32))], size=size, ncomp=3, dtype="float32"), "values of type int32"),
        (dict(erase=[(0, 0, 5, 4, torch.zeros((3, 4, 5)))], size=size, ncomp=3, dtype="float32"), "a torch tensor is accepted on the decode_device calls"),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            normalize_erase(**kw)


def test_the_calls_refuse_before_any_file_is_read():
    """not a JPEG in sight: the refusal comes first (the decoder's context is never asked for anything)"""
    from pyjpegdecoder_amd.batch import BatchDecoder, normalize_also

    class Ctx:
        device = 0
    dec = BatchDecoder.__new__(BatchDecoder)
    dec.ctx = Ctx()
    junk = [b"not a jpeg", b"nor this"]
    for call in (dec.decode, dec.decode_device):
        with pytest.raises(ValueError, match="erase needs size"):
            call(junk, erase=[None, (0, 0, 1, 1)])
        with pytest.raises(ValueError, match="erase has 1 entries for 2 outputs"):
            call(junk, size=(8, 8), erase=[(0, 0, 1, 1)])
        with pytest.raises(ValueError, match="output 1, box 0: .* is not inside the 8 x 8 canvas"):
            call(junk, size=(8, 8), erase=[None, (0, 0, 9, 1)])
    with pytest.raises(ValueError):
        dec.decode(junk, return_seams=True, erase=[None, (0, 0, 1, 1)])
    with pytest.raises(ValueError, match="erase needs size"):
        next(dec.decode_device_iter([junk], erase=[[None, None]]))
    with pytest.raises(ValueError, match=r"also\[0\]: erase: output 0, box 0: .* is not inside the 4 x 4 canvas"):
        normalize_also([dict(size=(4, 4), erase=[(0, 0, 5, 1)])], {}, (8, 8))
    assert normalize_also([dict(size=(4, 4))], dict(erase=[(0, 0, 1, 1)]), (8, 8))[0]["erase"] is None       # the group's own, never the call's


def test_narrow_carries_the_boxes():
    from pyjpegdecoder_amd.batch import _Request
    files = [b"a", b"b", b"c", b"d"]
    boxes = [None, ((1, 1, 2, 2, (0.0,)),), None, ((0, 0, 1, 1, (1.0,)), (3, 3, 1, 1, (2.0,)))]
    req = _Request(files, size=(8, 8), erase=boxes)
    sub = req.narrow([3, 1])
    assert sub.files == [b"d", b"b"] and sub.erase == [boxes[3], boxes[1]]
    assert req.narrow([0, 2]).erase is None                               # no box among them: the request of a call without erase
    assert req.narrow([2, 3]).erase == [None, boxes[3]]
    # with views the boxes go with the view
    views = [(0, (0, 0, 4, 4)), (2, (0, 0, 4, 4)), (0, (1, 1, 4, 4)), (3, (0, 0, 4, 4)), (2, (2, 2, 4, 4))]
    vb = [((0, 0, 1, 1, (float(k),)),) if k != 3 else None for k in range(5)]
    req = _Request(files, size=(8, 8), views=views, slots=list(range(5)), erase=vb)
    sub = req.narrow([2, 0])
    assert sub.views == [(1, views[0][1]), (0, views[1][1]), (1, views[2][1]), (0, views[4][1])]
    assert sub.erase == [vb[0], vb[1], vb[2], vb[4]] and sub.slots == [0, 1, 2, 4]
    assert req.narrow([3]).erase is None
    # an extra group's boxes follow the files as well
    extra = _Request(files, size=(4, 4), erase=boxes)
    req = _Request(files, size=(8, 8), also=[extra])
    assert req.narrow([1, 3]).also[0].erase == [boxes[1], boxes[3]] and req.narrow([1, 3]).erase is None


# ---- random_erasing_rect ---------------------------------------------------------------------------------------------------
def test_random_erasing_rect():
    import torch
    from pyjpegdecoder_amd import random_erasing_rect
    W, H = 224, 160
    scale, ratio = (0.02, 0.33), (0.3, 3.3)
    g = torch.Generator().manual_seed(1234)
    seen = 0
    for _ in range(200):
        r = random_erasing_rect((W, H), scale, ratio, generator=g)
        if r is None:
            continue
        seen += 1
        x, y, w, h = r
        assert all(isinstance(t, int) for t in r)
        assert 1 <= w < W and 1 <= h < H and 0 <= x and x + w <= W and 0 <= y and y + h <= H
        # the sides are sqrt(area * aspect) and sqrt(area / aspect), each rounded: within half a pixel of a pair inside the bounds
        lo_a, hi_a = scale[0] * W * H, scale[1] * W * H
        assert (w - 0.5) * (h - 0.5) <= hi_a * (1 + 1e-6) and (w + 0.5) * (h + 0.5) >= lo_a * (1 - 1e-6), r
        assert (h - 0.5) / (w + 0.5) <= ratio[1] * (1 + 1e-6) and (h + 0.5) / (w - 0.5 if w > 0.5 else 0.5) >= ratio[0] * (1 - 1e-6), r
    assert seen > 150
    assert random_erasing_rect((8, 8), scale=(1.5, 2.0), generator=g) is None            # no box of that area lies inside
    a = [random_erasing_rect((W, H), generator=torch.Generator().manual_seed(7)) for _ in range(3)]
    assert a[0] == a[1] == a[2] and a[0] is not None
    assert math.isfinite(sum(a[0]))
