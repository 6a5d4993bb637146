"""Colour operations on the MI355X (mj_plan_request.mode with MJ_MODE_COLOUR_OPS, BatchDecoder.decode / decode_device /
decode_device_iter(size=..., color_ops=...)): Pillow's ImageEnhance.* / ImageOps.* on the finished canvas.  The expected bytes of
every case are tools/colour_model.py — which tests/test_colour_host.py holds to Pillow, bit for bit — applied to the library's own
output of the same call without color_ops, without mirror and with dtype uint8; the flip and tools/normalize_model.py come
afterwards.  Byte for byte, in every layout."""
import numpy as np
import pytest

from conftest import GOLDEN
from test_resize import as_layout
from test_roi import LAYOUTS

pytestmark = pytest.mark.gpu

ODD, GREY, C411, C440, FLAT = "70x50_420_pil_opt", "64x64_grey_pil", "100x36_411_dri3", "48x80_440", "48x32_420_flat"
KINDS = [ODD, GREY, C411, C440]
SINGLE = [("brightness", 1.4), ("brightness", 0.05), ("color", 0.3), ("color", 1.9), ("contrast", 1.9), ("contrast", 0.3), ("sharpness", 2.5),
          ("sharpness", 0.3), ("posterize", 3), ("solarize", 100), ("autocontrast",), ("equalize",), ("invert",)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_DEC, _BASE = {}, {}


def raw(name):
    """a golden file by its name; bytes — a file made at run time (tests/colour_cases.py) — as they are"""
    return name if isinstance(name, bytes) else (GOLDEN / "files" / f"{name}.jpg").read_bytes()


def host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def decoders():
    yield
    for dec in _DEC.values():
        dec.close()
    _DEC.clear()
    _BASE.clear()


def decoder(layout):
    if layout not in _DEC:
        from pyjpegdecoder_amd import BatchDecoder
        _DEC[layout] = BatchDecoder(device=0, layout=layout)
    return _DEC[layout]


def to_rowmajor(img, layout):
    """one image as a decoder of this layout returns it -> (H, W, 3), or (H, W) for one component"""
    s = img
    if s.ndim == 3 and layout.startswith("planar"):
        s = np.moveaxis(s, 0, -1)
    if layout in ("xmajor", "planar"):
        s = s.swapaxes(0, 1)
    return np.ascontiguousarray(s[..., 0] if s.ndim == 3 and s.shape[-1] == 1 else s)


def from_rowmajor(rm, layout, shape):
    """... and back, in the shape the decoder gave (one component: with or without an axis of its own)"""
    return as_layout(rm, layout).reshape(shape)


def base(layout, names, key=None, **kw):
    """the library's own uint8 canvases of the call without color_ops and without mirror: computed once per call, never changed"""
    key = (layout, tuple(names), key if key is not None else repr(sorted(kw.items())))
    if key not in _BASE:
        out = host(decoder(layout).decode_device([raw(n) for n in names], **kw)).copy()
        assert out.dtype == np.uint8
        out.setflags(write=False)
        _BASE[key] = out
    return _BASE[key]


def expected(canvases, layout, chains, mirror=None, dtype=None, normalize=True):
    """the model: chain k on canvas k, then the flip, then the output table (bit patterns for a float dtype)"""
    from tools import colour_model, normalize_model
    out = []
    for k, c in enumerate(canvases):
        rm = colour_model.apply_chain(to_rowmajor(c, layout), chains[k])
        if mirror is not None and mirror[k]:
            rm = rm[:, ::-1]
        if dtype is not None:
            rm = normalize_model.normalize(rm, dtype, MEAN if normalize else None, STD if normalize else None)
        out.append(from_rowmajor(rm, layout, c.shape))
    return np.stack(out)


@pytest.mark.parametrize("op", SINGLE, ids=lambda op: "-".join(str(v) for v in op))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_op_alone_on_four_kinds_of_file(layout, op):
    """files of four kinds in one call, hence several plans into one tensor through slots; canvases smaller and larger than the images"""
    for size in ((24, 16), (120, 96)):
        kw = dict(size=size, mode="RGB")
        canv = base(layout, KINDS, **kw)
        got = host(decoder(layout).decode_device([raw(n) for n in KINDS], color_ops=[op], **kw))
        assert got.shape == canv.shape and got.dtype == np.uint8
        want = expected(canv, layout, [[op]] * len(KINDS))
        for k, n in enumerate(KINDS):
            assert np.array_equal(got[k], want[k]), (n, size, op)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_no_chain_is_the_call_without_the_argument(layout):
    kw = dict(size=(40, 28), mode="RGB")
    canv = base(layout, KINDS, **kw)
    dec = decoder(layout)
    files = [raw(n) for n in KINDS]
    for none in (None, [], [None] * 4, [None, [], (), None]):
        assert np.array_equal(host(dec.decode_device(files, color_ops=none, **kw)), canv), none
    # a list with one real chain changes only that output
    got = host(dec.decode_device(files, color_ops=[None, None, [("solarize", 128), ("invert",)], []], **kw))
    want = expected(canv, layout, [None, None, [("solarize", 128), ("invert",)], None])
    assert np.array_equal(got, want) and not np.array_equal(got[2], canv[2])
    for k in (0, 1, 3):
        assert np.array_equal(got[k], canv[k])


CHAINS = {"jitter": [("brightness", 1.3), ("contrast", 0.7), ("color", 1.6)], "jitter-reordered": [("color", 0.2), ("contrast", 1.9), ("brightness", 0.9)],
          "autocontrast-equalize": [("autocontrast",), ("equalize",)], "four": [("sharpness", 1.9), ("contrast", 0.6), ("posterize", 5), ("solarize", 130)]}


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_chains(layout, name):
    kw = dict(size=(40, 28), mode="RGB")
    canv = base(layout, KINDS, **kw)
    got = host(decoder(layout).decode_device([raw(n) for n in KINDS], color_ops=CHAINS[name], **kw))
    assert np.array_equal(got, expected(canv, layout, [CHAINS[name]] * 4)), name


@pytest.mark.parametrize("layout", LAYOUTS)
def test_chains_of_different_lengths_in_one_call(layout):
    """the outputs whose chain has ended are copied from canvas to canvas while the others go on (ODD twice: one plan, two lengths)"""
    names = [ODD, GREY, ODD, C440, C411]
    chains = [CHAINS["four"], [("equalize",)], [("sharpness", 0.0), ("autocontrast",)], None, CHAINS["jitter"]]
    kw = dict(size=(33, 21), mode="RGB")
    canv = base(layout, names, **kw)
    got = host(decoder(layout).decode_device([raw(n) for n in names], color_ops=chains, **kw))
    want = expected(canv, layout, chains)
    for k in range(len(names)):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("size", ((1, 5), (5, 1), (2, 7), (7, 2), (3, 3), (3, 2), (1, 1)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", LAYOUTS)
def test_canvases_with_a_side_of_one_two_and_three(layout, size):
    """sharpness copies the first and last row and column: a side below 3 leaves the canvas as it was, a 3 x 3 one has one filtered pixel"""
    names = [ODD, C440]
    chain = [("sharpness", 2.5), ("contrast", 1.3), ("sharpness", 0.0)]
    canv = base(layout, names, size=size)
    got = host(decoder(layout).decode_device([raw(n) for n in names], size=size, color_ops=chain))
    assert np.array_equal(got, expected(canv, layout, [chain] * 2))
    only = host(decoder(layout).decode_device([raw(n) for n in names], size=size, color_ops=[("sharpness", 2.5)]))
    if min(size) < 3:
        assert np.array_equal(only, canv)
    else:
        assert np.array_equal(only, expected(canv, layout, [[("sharpness", 2.5)]] * 2)) and not np.array_equal(only, canv)


@pytest.mark.parametrize("op", (("contrast", 1.5), ("autocontrast",), ("equalize",)), ids=lambda op: op[0])
@pytest.mark.parametrize("layout", ("xmajor", "planar_rowmajor"))
def test_a_bin_above_65535_and_the_merge_of_many_workgroups(layout, op):
    """a flat file on a 300 x 300 canvas: 90 000 pixels in very few bins, counted by 22 workgroups per output; the second output's
    histogram is wide (its workgroups' bins differ).  The flat file's fullest bin holds about 30 000 pixels of such a canvas, so a
    second call pads the canvas: 87 600 fill pixels in one bin of every component."""
    names = [FLAT, ODD]
    canv = base(layout, names, size=(300, 300))
    assert np.bincount(to_rowmajor(canv[0], layout)[..., 0].ravel(), minlength=256).max() > 20000         # (few bins, none above 16 bits)
    got = host(decoder(layout).decode_device([raw(n) for n in names], size=(300, 300), color_ops=[op]))
    want = expected(canv, layout, [[op]] * 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    kw = dict(size=(300, 300), resize_to=(60, 40), fill=(7, 99, 200))
    canv = base(layout, names, **kw)
    rm = to_rowmajor(canv[1], layout)
    assert all(np.bincount(rm[..., c].ravel(), minlength=256).max() > 65535 for c in range(3))
    got = host(decoder(layout).decode_device([raw(n) for n in names], color_ops=[[op], [op, ("invert",)]], **kw))
    want = expected(canv, layout, [[op], [op, ("invert",)]])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_component_outputs(layout):
    """mode="L": color is the identity and contrast's mean is the image's own"""
    kw = dict(size=(40, 28), mode="L")
    canv = base(layout, KINDS, **kw)
    assert canv[0].size == 40 * 28
    dec = decoder(layout)
    files = [raw(n) for n in KINDS]
    assert np.array_equal(host(dec.decode_device(files, color_ops=[("color", 0.3)], **kw)), canv)
    for chain in ([("contrast", 1.7)], [("color", 2.0), ("equalize",), ("sharpness", 1.8)], [("autocontrast",), ("brightness", 0.6)]):
        got = host(dec.decode_device(files, color_ops=chain, **kw))
        assert np.array_equal(got, expected(canv, layout, [chain] * 4)), chain
    # a grey file in its own components
    one = base(layout, [GREY], size=(24, 16))
    got = host(dec.decode_device([raw(GREY)], size=(24, 16), color_ops=[("contrast", 0.4), ("posterize", 2)]))
    assert np.array_equal(got, expected(one, layout, [[("contrast", 0.4), ("posterize", 2)]]))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fill_pixels_take_part_in_the_statistics(layout):
    """a letterbox: the padding is part of the canvas — of its histograms — and goes through the ops"""
    names = [C411, C440, ODD]
    kw = dict(size=(48, 48), resize_to="contain", fill=(7, 99, 200))
    canv = base(layout, names, **kw)
    rm = to_rowmajor(canv[0], layout)
    assert (rm[0, 0] == (7, 99, 200)).all() and (rm.reshape(-1, 3) == (7, 99, 200)).all(axis=1).mean() > 0.3
    for chain in ([("contrast", 1.6)], [("equalize",), ("invert",)], [("autocontrast",), ("sharpness", 2.0)]):
        got = host(decoder(layout).decode_device([raw(n) for n in names], color_ops=chain, **kw))
        assert np.array_equal(got, expected(canv, layout, [chain] * 3)), chain
    from tools import colour_model
    assert not np.array_equal(colour_model.apply_op(rm, ("equalize",))[0, 0], rm[0, 0])        # (the fill itself changes)
    # resize_to=256-style placing: the shorter side to 40, centre crop
    kw = dict(size=(32, 32), resize_to=40)
    canv = base(layout, names, **kw)
    got = host(decoder(layout).decode_device([raw(n) for n in names], color_ops=CHAINS["jitter"], **kw))
    assert np.array_equal(got, expected(canv, layout, [CHAINS["jitter"]] * 3))


@pytest.mark.parametrize("layout", ("planar_rowmajor", "xmajor"))
def test_mirror_and_the_output_table_come_afterwards(layout):
    import torch
    names = [ODD, C440, C411, ODD]
    mirror = [True, False, True, False]
    chains = [CHAINS["jitter"], [("sharpness", 2.2)], None, [("equalize",)]]
    kw = dict(size=(40, 28))
    canv = base(layout, names, **kw)
    dec = decoder(layout)
    files = [raw(n) for n in names]
    got = host(dec.decode_device(files, color_ops=chains, mirror=mirror, **kw))
    assert np.array_equal(got, expected(canv, layout, chains, mirror))
    got = dec.decode_device(files, color_ops=chains, mirror=mirror, dtype=torch.float16, normalize=(MEAN, STD), **kw)
    assert got.dtype == torch.float16
    bits = got.cpu().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bits, expected(canv, layout, chains, mirror, "float16"))
    # the output whose chain is None is the output of the call without the argument
    plain = dec.decode_device(files, mirror=mirror, dtype=torch.float16, normalize=(MEAN, STD), **kw)
    assert torch.equal(plain[2], got[2])
    got = dec.decode_device(files, color_ops=chains, mirror=mirror, dtype=torch.float32, **kw)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), expected(canv, layout, chains, mirror, "float32", normalize=False))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_with_views_windows_affine_and_two_step_resize(layout):
    dec = decoder(layout)
    a, b = [("contrast", 1.8), ("color", 0.4)], [("equalize",)]
    # two views of one file with different chains, and a whole image without one
    views = [(0, (5, 3, 40, 30)), (0, (33, 11, 37, 39)), 0]
    canv = base(layout, [ODD], key="views", size=(24, 16), views=views)
    got = host(dec.decode_device([raw(ODD)], size=(24, 16), views=views, color_ops=[a, b, None]))
    assert np.array_equal(got, expected(canv, layout, [a, b, None]))
    names = [ODD, C411, C440]
    files = [raw(n) for n in names]
    chains = [a, b, [("autocontrast",), ("sharpness", 1.5)]]
    kw = dict(size=(24, 16), rois=[(0, 0, 31, 22), (100 - 17, 0, 17, 36), (8, 16, 32, 48)])
    canv = base(layout, names, key="rois", **kw)
    assert np.array_equal(host(dec.decode_device(files, color_ops=chains, **kw)), expected(canv, layout, chains))
    kw = dict(size=(24, 16), affine=(0.9, 0.3, -2.0, -0.3, 0.9, 14.0), affine_resample="bilinear", affine_fill=(7, 99, 200))
    canv = base(layout, names, key="affine", **kw)
    assert np.array_equal(host(dec.decode_device(files, color_ops=chains, **kw)), expected(canv, layout, chains))
    kw = dict(size=(12, 9), reducing_gap=2.0, orientation=[6, 1, 3])
    canv = base(layout, names, key="gap", **kw)
    assert np.array_equal(host(dec.decode_device(files, color_ops=chains, **kw)), expected(canv, layout, chains))


@pytest.mark.parametrize("layout", ("rowmajor", "planar"))
def test_decode_and_the_iterator_are_decode_device(layout):
    dec = decoder(layout)
    files = [raw(n) for n in KINDS]
    chains = [CHAINS["jitter"], [("equalize",)], None, CHAINS["four"]]
    kw = dict(size=(40, 28), mode="RGB", mirror=[False, True, True, False])
    got = host(dec.decode_device(files, color_ops=chains, **kw))
    assert np.array_equal(got, expected(base(layout, KINDS, size=(40, 28), mode="RGB"), layout, chains, kw["mirror"]))
    assert np.array_equal(dec.decode(files, color_ops=chains, **kw), got)
    kw.pop("mirror")
    every = host(dec.decode_device(files, color_ops=CHAINS["jitter"], **kw))
    one, two, three = list(dec.decode_device_iter([files, files[:1], files], color_ops=[chains, [CHAINS["jitter"]], None], **kw))
    assert np.array_equal(host(one), host(dec.decode_device(files, color_ops=chains, **kw))) and np.array_equal(host(two)[0], every[0])
    assert np.array_equal(host(three), base(layout, KINDS, size=(40, 28), mode="RGB"))
    (again,) = list(dec.decode_device_iter([files], color_ops=CHAINS["jitter"], **kw))
    assert np.array_equal(host(again), every)


def test_refusals_name_what_is_wrong():
    dec = decoder("xmajor")
    with pytest.raises(ValueError, match="color_ops needs size"):
        dec.decode_device([raw(ODD)], color_ops=[("invert",)])
    with pytest.raises(ValueError, match="return_seams do not go together"):
        dec.decode([raw(ODD)], size=(24, 16), color_ops=[("invert",)], return_seams=True)
    with pytest.raises(ValueError, match="unknown op 'hue'"):
        dec.decode_device([raw(ODD)], size=(24, 16), color_ops=[("hue", 0.1)])
    with pytest.raises(ValueError, match="5 ops in one chain"):
        dec.decode_device([raw(ODD)], size=(24, 16), color_ops=[("invert",)] * 5)
    with pytest.raises(ValueError, match="is not finite"):
        dec.decode_device([raw(ODD)], size=(24, 16), color_ops=[("contrast", float("nan"))])
    with pytest.raises(ValueError, match="posterize takes 1..8 bits"):
        dec.decode_device([raw(ODD)], size=(24, 16), color_ops=[("posterize", 9)])
    with pytest.raises(ValueError, match="color_ops has 2 entries for 1 outputs"):
        dec.decode([raw(ODD)], size=(24, 16), color_ops=[None, [("invert",)]])
    with pytest.raises(ValueError, match="color_ops needs size"):
        list(dec.decode_device_iter([[raw(ODD)]], color_ops=[("invert",)]))
