"""adjust_hue on the host (no GPU): tools/colour_model.py's two conversions against Pillow's Image.convert over all 2^24 inputs, its
adjust_hue against torchvision's F.adjust_hue restated here with Pillow's own calls, the library's host twin mj_host_colour_ops
against the model over all 2^24 colours, the numbers and the refusals of the request, and the file of tests/hue_cases.py against the
colours and the branches it is meant to reach.  Bytes, not tolerances."""
import ctypes
import io
import math

import numpy as np
import pytest

import hue_cases
from conftest import ROOT
from test_colour_host import _batch, _normal

# factor -> the shift torchvision's np.array(factor * 255).astype(np.uint8) gives on x86-64
SHIFTS = {0.5: 127, 0.1: 25, 0.004: 1, -0.003: 0, -1 / 255: 255, -0.1: 231, -0.5: 129}
FACTORS = tuple(SHIFTS) + (0.0,)
CHUNK = 1 << 22


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


def triples(chunk: int) -> np.ndarray:
    """the chunk-th 2^22 of all 2^24 byte triples, as a (2048, 2048, 3) image"""
    n = np.arange(chunk * CHUNK, (chunk + 1) * CHUNK, dtype=np.uint32)
    return np.stack([n >> 16 & 255, n >> 8 & 255, n & 255], axis=-1).astype(np.uint8).reshape(2048, 2048, 3)


def torchvision_adjust_hue(a: np.ndarray, factor: float) -> np.ndarray:
    """F.adjust_hue's PIL branch, call for call: split the HSV image, add in uint8 with wrap-around, merge, convert"""
    from PIL import Image
    if a.ndim == 2:             # (input_mode in {"L", "1", "I", "F"}: return img)
        return a
    h, s, v = Image.fromarray(a, "RGB").convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(all="ignore"):         # (a negative product's conversion to uint8 is the platform's: x86-64 truncates and wraps)
        shift = np.array(factor * 255).astype(np.uint8)
        assert int(shift) == SHIFTS.get(factor, 0), "this platform's float-to-uint8 conversion is not the one the rule restates"
        np_h = np_h + shift
    return np.asarray(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))


def test_both_conversions_are_pillows_over_all_inputs():
    from PIL import Image
    from tools import colour_model
    to_hsv = to_rgb = 0
    for chunk in range(4):
        a = triples(chunk)
        to_hsv += int((colour_model.rgb_to_hsv(a) != np.asarray(Image.fromarray(a, "RGB").convert("HSV"))).any(axis=-1).sum())
        to_rgb += int((colour_model.hsv_to_rgb(a) != np.asarray(Image.fromarray(a, "HSV").convert("RGB"))).any(axis=-1).sum())
    assert (to_hsv, to_rgb) == (0, 0)


def test_the_shift_is_the_table():
    from tools import colour_model
    assert {f: colour_model.hue_shift(f) for f in SHIFTS} == SHIFTS
    assert colour_model.hue_shift(0.0) == 0 and colour_model.hue_shift(-0.0) == 0
    # numpy on this machine agrees where its float-to-uint8 conversion is defined at all (factors that are not negative)
    for f in (0.5, 0.1, 0.004, 0.0):
        assert int(np.array(f * 255).astype(np.uint8)) == SHIFTS.get(f, 0)


@pytest.mark.parametrize("factor", FACTORS, ids=lambda f: f"{f:.4f}")
def test_the_model_is_torchvisions_adjust_hue(factor):
    """a fixed sample of 2^20 colours plus the corners and the grey axis, as an image"""
    from tools import colour_model
    rng = np.random.default_rng(24)
    a = rng.integers(0, 256, (1024, 1040, 3), dtype=np.uint8)
    a[:, 1024:1032] = rng.integers(0, 2, (1024, 8, 3), dtype=np.uint8) * 255              # the cube's corners
    a[:, 1032:] = np.arange(1024 * 8, dtype=np.uint32).reshape(1024, 8, 1) & 255          # greys
    got = colour_model.apply_op(a, ("adjust_hue", factor))
    assert np.array_equal(got, torchvision_adjust_hue(a, factor))
    if factor == 0.0:           # the round trip is not the identity, and must not be short-circuited
        assert 0.5 < (got != a).any(axis=-1).mean() < 0.95 and int(np.abs(got.astype(int) - a.astype(int)).max()) <= 7
    grey = a[..., 0]
    assert colour_model.apply_op(grey, ("adjust_hue", factor)) is not None and np.array_equal(colour_model.apply_op(grey, ("adjust_hue", factor)), grey)
    assert np.array_equal(colour_model.apply_chain(a, [("adjust_hue", factor), ("invert",)]), 255 - got)


def test_the_model_refuses_what_torchvision_refuses():
    from tools import colour_model
    a = np.zeros((2, 2, 3), dtype=np.uint8)
    for bad in (0.500001, -0.500001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="adjust_hue takes a factor of -0.5..0.5"):
            colour_model.apply_op(a, ("adjust_hue", bad))
    with pytest.raises(ValueError, match="no colour op"):
        colour_model.apply_op(a, ("adjust_hue",))
    with pytest.raises(ValueError, match="no colour op"):
        colour_model.apply_op(a, ("hue", 0.1))


@pytest.mark.parametrize("factor,shift", [(0.0, 0), (0.004, 1), (0.1, 25), (0.5, 127), (-0.5, 129), (-0.1, 231), (-1 / 255, 255)], ids=lambda v: str(v)[:6])
def test_the_host_twin_is_the_model_over_all_colours(lib, factor, shift):
    from pyjpegdecoder_amd import _binding as B
    from tools import colour_model
    assert colour_model.hue_shift(factor) == shift
    bad = 0
    for chunk in range(4):
        a = triples(chunk)
        bad += int((B.colour_ops(a, [("adjust_hue", factor)]) != colour_model.adjust_hue(a, factor)).any(axis=-1).sum())
    assert bad == 0


def test_the_host_twin_on_one_component_and_in_chains(lib):
    from pyjpegdecoder_amd import _binding as B
    from tools import colour_model
    rng = np.random.default_rng(7)
    grey = rng.integers(0, 256, (17, 23), dtype=np.uint8)
    assert np.array_equal(B.colour_ops(grey, [("adjust_hue", 0.3)]), grey)
    chain = [("adjust_hue", -0.2), ("contrast", 1.4)]
    assert np.array_equal(B.colour_ops(grey, chain), colour_model.apply_chain(grey, chain)) and not np.array_equal(B.colour_ops(grey, chain), grey)
    rgb = rng.integers(0, 256, (17, 23, 3), dtype=np.uint8)
    for chain in ([("brightness", 1.3), ("contrast", 0.7), ("color", 1.6), ("adjust_hue", 0.1)], [("adjust_hue", -0.1), ("gaussian_blur", 1.0)],
                  [("adjust_hue", 0.25), ("adjust_hue", -0.25)], [("equalize",), ("adjust_hue", 0.0), ("sharpness", 2.0)]):
        assert np.array_equal(B.colour_ops(rgb, chain), colour_model.apply_chain(rgb, chain)), chain


def test_the_numbers(lib):
    from pyjpegdecoder_amd import _binding as B
    header = (ROOT / "include" / "mijpeg.h").read_text()
    assert "#define MJ_COLOUR_ADJUST_HUE   13" in header and B.COLOUR_OPS["adjust_hue"] == 13 and "adjust_hue" in B.COLOUR_VALUED
    assert 12 not in B.COLOUR_OPS.values() and "hue" not in B.COLOUR_OPS
    assert lib.mj_version() == 2 and ctypes.sizeof(B.ColourChainC) == 36 and ctypes.sizeof(B.ColourOpC) == 8
    c = B.colour_chain([("adjust_hue", -0.25)])
    assert (c.n, c.op[0].kind, c.op[0].value) == (1, 13, -0.25)


def test_normalize_color_ops_takes_the_op_and_refuses_what_is_out_of_range():
    from pyjpegdecoder_amd.batch import normalize_color_ops
    size = (24, 16)
    jitter = [("brightness", 1.2), ("contrast", 0.8), ("color", 1.1), ("adjust_hue", -0.05)]
    assert normalize_color_ops(jitter, size, 2) == [tuple(jitter)] * 2
    assert normalize_color_ops([None, [("adjust_hue", 0)]], size, 2) == [None, (("adjust_hue", 0.0),)]           # (factor 0 is an op)
    assert normalize_color_ops([("adjust_hue", 0.5)], size, 1) == [(("adjust_hue", 0.5),)] and normalize_color_ops([("adjust_hue", -0.5)], size, 1)
    for bad in (0.500001, -0.500001, 1, -7):
        with pytest.raises(ValueError, match=r"output 1: adjust_hue takes a factor of -0\.5\.\.0\.5"):
            normalize_color_ops([None, [("invert",), ("adjust_hue", bad)]], size, 2)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="output 1: 'adjust_hue': .* is not finite"):
            normalize_color_ops([None, [("adjust_hue", bad)]], size, 2)
    with pytest.raises(ValueError, match="takes one number"):
        normalize_color_ops([("adjust_hue",)], size, 1)
    with pytest.raises(ValueError, match=r"unknown op 'hue' .*adjust_hue"):
        normalize_color_ops([("hue", 0.1)], size, 1)


def test_the_request_with_the_op(lib):
    from pyjpegdecoder_amd import _binding as B
    batch, keep = _batch([(128, 64), (50, 70)])
    rc, out, msg = _normal(lib, batch, colour=[None, (("adjust_hue", 0.1),)])
    assert rc == B.MJ_OK and out.mode == 0 and bool(out.colour) and out.n_slots == 2, msg
    r, keep_r = B.plan_request(2, size=(24, 16), colour=[None, (("adjust_hue", 0.1),)])
    assert (r.colour[1].n, r.colour[1].op[0].kind, r.colour[0].n) == (1, 13, 0) and math.isclose(r.colour[1].op[0].value, 0.1, rel_tol=1e-6)
    rc, out, msg = _normal(lib, batch, colour=[(("adjust_hue", 0.0),), None], mode="L")
    assert rc == B.MJ_OK and out.mode == B.MJ_MODE_L and bool(out.colour), msg          # (factor 0 on "L" is still a chain)
    rc, out, msg = _normal(lib, batch, colour=[(("brightness", 1.2), ("contrast", 0.8), ("color", 1.1), ("adjust_hue", -0.5)), (("adjust_hue", 0.5),)])
    assert rc == B.MJ_OK and bool(out.colour), msg
    for bad, why in ((((13, 0.500001),), "adjust_hue takes a factor of -0.5..0.5"), (((13, -0.500001),), "adjust_hue takes a factor of -0.5..0.5"),
                     ((("adjust_hue", float("nan")),), "an op's value is not finite"), ((("adjust_hue", float("inf")),), "an op's value is not finite"),
                     ((("adjust_hue", -float("inf")),), "an op's value is not finite"), (((12, 0.1),), "an op's kind is none of MJ_COLOUR_*"),
                     (((14, 0.1),), "an op's kind is none of MJ_COLOUR_*")):
        rc, _, msg = _normal(lib, batch, colour=[None, bad])
        assert rc == B.MJ_ERR_INVALID and "colour_ops: output 1: " + why in msg, (bad, msg)
    rgb = np.zeros((2, 2, 3), dtype=np.uint8)
    for bad in ([(13, 0.6)], [(12, 0.1)], [("adjust_hue", float("nan"))]):
        with pytest.raises(ValueError, match="mj_host_colour_ops"):
            B.colour_ops(rgb, bad)


def test_the_crafted_file_is_its_colours_and_reaches_every_branch(lib):
    """Pillow's decode and the oracle's give the blocks their colours; with them every class of the census occurs under every shift the
    GPU test uses, and the model's bytes for two blocks are the ones worked out by hand from the rules"""
    from PIL import Image
    from oracle import oracle
    from tools import colour_model
    want = hue_cases.intended()
    assert want.shape == (hue_cases.SIZE[1], hue_cases.SIZE[0], 3)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(hue_cases.raw())).convert("RGB")), want)
    assert np.array_equal(oracle.decode(hue_cases.raw())["rgb"].swapaxes(0, 1), want)
    for f in (-0.5, -0.1, 0.0, 0.25, 0.5):
        assert hue_cases.census([want], colour_model.hue_shift(f)) == hue_cases.CLASSES, f
    assert hue_cases.census([want[:8, :24]], 0) == {"r is max", "g is max", "b is max", "i % 6 == 0", "i % 6 == 2", "i % 6 == 4"}       # (the census tells canvases apart)
    # red (254, 0, 0): H 0, S 255, V 254; shift 127 -> hf = 2.988.., sextant 2: (p, V, t) = (0, 254, round(254 * 0.988..)) = (0, 254, 251)
    assert tuple(colour_model.adjust_hue(want[:1, :1], 0.5)[0, 0]) == (0, 254, 251)
    # a grey stays what it is under any shift
    assert np.array_equal(colour_model.adjust_hue(want[24:, 32:], 0.3), want[24:, 32:])
