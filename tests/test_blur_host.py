"""The blurs of color_ops= on the host (no GPU): tools/colour_model.py's statement of Pillow's BoxBlur.c — gaussian_box_radius,
box_pass — against Pillow itself (Image.filter with ImageFilter.GaussianBlur / BoxBlur), the library's host twin
mj_host_colour_ops against the model, and the request: batch.normalize_color_ops and the C ABI's checks through
mj_debug_normalise_request.  Bytes, not tolerances."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT
from test_colour_host import _batch, _normal

GAUSSIAN = (0, 0.1, 0.5, 1.0, 1.41, 1.42, 2.0, 2.44, 2.45, 3.0, 13.37, 1024)
BOX = (0, 0.25, 1, 1.5, 3.3, 40)
SIZES = ((1, 1), (1, 7), (5, 3), (33, 21), (40, 28))          # (width, height)
# the box radius of a Gaussian's three passes at fixed radii, to the decimals written here
FIXED = ((0.1, "0.00167224"), (0.5, "0.04545455"), (1.0, "0.25000003"), (1.41, "0.98236"), (1.42, "1.00246"), (2.0, "1.375"), (2.44, "1.98082"),
         (2.45, "2.00030"), (3.0, "2.4166667"))
MIXED = ([("contrast", 0.6), ("gaussian_blur", 1.7), ("solarize", 128)], [("box_blur", 1.5), ("gaussian_blur", 0.8)])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


def drawn():
    """twenty radii from the range the self-supervised recipes draw from"""
    return [float(v) for v in np.random.default_rng(2021).uniform(0.1, 2.0, 20)]


def ops():
    return [("gaussian_blur", r) for r in GAUSSIAN + tuple(drawn())] + [("box_blur", r) for r in BOX]


def images():
    rng = np.random.default_rng(21)
    out = []
    for w, h in SIZES:
        for C in (3, 1):
            out.append((f"random {w}x{h}x{C}", rng.integers(0, 256, (h, w, 3) if C == 3 else (h, w), dtype=np.uint8)))
    board = ((np.add.outer(np.arange(21), np.arange(33)) & 1) * 255).astype(np.uint8)
    out.append(("checkerboard x1", board))
    out.append(("checkerboard x3", np.ascontiguousarray(np.stack([board, 255 - board, board], axis=-1))))
    return out


def pillow(im, op):
    from PIL import ImageFilter
    return im.filter(ImageFilter.GaussianBlur(op[1]) if op[0] == "gaussian_blur" else ImageFilter.BoxBlur(op[1]))


def test_model_is_pillows_filter():
    from PIL import Image
    from tools import colour_model as M
    for name, a in images():
        im = Image.fromarray(a)
        for op in ops():
            assert np.array_equal(M.apply_op(a, op), np.asarray(pillow(im, op))), (name, op)
        # radius 0 is the identity, and the width passes come first: the other order gives other bytes
        assert np.array_equal(M.apply_op(a, ("gaussian_blur", 0)), a) and np.array_equal(M.apply_op(a, ("box_blur", 0)), a)
    a = dict(images())["random 33x21x3"]
    fr = M.gaussian_box_radius(1.7)
    swapped = a
    for axis in (0, 0, 0, 1, 1, 1):
        swapped = M.box_pass(swapped, fr, axis)
    assert not np.array_equal(swapped, M.apply_op(a, ("gaussian_blur", 1.7)))


def test_gaussian_box_radius_at_the_fixed_points():
    from tools import colour_model as M
    for radius, fr in FIXED:
        got = M.gaussian_box_radius(radius)
        assert got.dtype == np.float32 and f"{float(got):.{len(fr) - 2}f}" == fr, (radius, got, fr)
    assert M.gaussian_box_radius(1.0) == np.float32(0.25000003) and M.gaussian_box_radius(2.0) == np.float32(1.375)
    assert M.gaussian_box_radius(3.0) == np.float32(2.4166667)
    assert M.gaussian_box_radius(0) == 0
    # the range of the recipes runs with r = 0 or r = 1
    assert {M.box_weights(M.gaussian_box_radius(r))[0] for r in np.linspace(0.1, 2.0, 200)} == {0, 1}
    assert M.box_weights(np.float32(0)) == (0, 1 << 24, 0)


def test_host_twin_is_the_model(lib):
    from pyjpegdecoder_amd import _binding as B
    from tools import colour_model as M
    named = dict(images())
    for name in ("random 33x21x3", "random 33x21x1", "random 5x3x3", "random 5x3x1"):
        a = named[name]
        for op in ops():
            assert np.array_equal(B.colour_ops(a, [op]), M.apply_op(a, op)), (name, op)
        for chain in MIXED:
            assert np.array_equal(B.colour_ops(a, chain), M.apply_chain(a, chain)), (name, chain)


def test_host_twin_refuses_a_radius_out_of_range(lib):
    from pyjpegdecoder_amd import _binding as B
    a = np.zeros((4, 5, 3), dtype=np.uint8)
    out = np.empty_like(a)
    for name in ("gaussian_blur", "box_blur"):
        for value, rc in ((0, B.MJ_OK), (1024, B.MJ_OK), (-0.5, B.MJ_ERR_INVALID), (1024.5, B.MJ_ERR_INVALID), (float("nan"), B.MJ_ERR_INVALID),
                          (float("inf"), B.MJ_ERR_INVALID)):
            c = B.colour_chain([(name, value)])
            assert lib.mj_host_colour_ops(a.ctypes.data, 5, 4, 3, ctypes.byref(c), out.ctypes.data) == rc, (name, value)


def test_normalize_color_ops_takes_the_blurs():
    from pyjpegdecoder_amd.batch import normalize_color_ops
    size = (24, 16)
    assert normalize_color_ops([("gaussian_blur", 1.7)], size, 2) == [(("gaussian_blur", 1.7),)] * 2
    assert normalize_color_ops([("box_blur", np.int64(3)), ("gaussian_blur", np.float32(0.5))], size, 1) == [(("box_blur", 3.0), ("gaussian_blur", 0.5))]
    assert normalize_color_ops([[("gaussian_blur", 0)], None, [("box_blur", 1024)]], size, 3) == [(("gaussian_blur", 0.0),), None, (("box_blur", 1024.0),)]
    for name in ("gaussian_blur", "box_blur"):
        with pytest.raises(ValueError, match=f"output 1: '{name}' takes one number"):
            normalize_color_ops([None, [(name,)]], size, 2)
        with pytest.raises(ValueError, match="takes one number"):
            normalize_color_ops([(name, (1.0, 2.0))], size, 1)
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match=f"output 1: '{name}': .* is not finite"):
                normalize_color_ops([None, [(name, bad)]], size, 2)
        for bad in (-0.5, 1024.5):
            with pytest.raises(ValueError, match=f"output 1: {name} takes a radius of 0..1024, not {bad}"):
                normalize_color_ops([None, [("invert",), (name, bad)]], size, 2)


def test_a_chain_with_a_blur_is_no_unknown_op():
    """what the library refused before it had the blurs: ValueError("... unknown op 'gaussian_blur' ...")"""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import normalize_color_ops
    chain = [("contrast", 0.6), ("gaussian_blur", 1.7), ("solarize", 128)]
    assert normalize_color_ops(chain, (24, 16), 1) == [(("contrast", 0.6), ("gaussian_blur", 1.7), ("solarize", 128.0))]
    assert B.COLOUR_OPS["gaussian_blur"] == 10 and B.COLOUR_OPS["box_blur"] == 11
    c = B.colour_chain(chain)
    assert c.n == 3 and c.op[1].kind == 10 and c.op[1].value == np.float32(1.7)


def test_the_request_takes_kinds_10_and_11_and_refuses_a_radius_out_of_range(lib):
    from pyjpegdecoder_amd import _binding as B
    header = (ROOT / "include" / "mijpeg.h").read_text()
    assert "#define MJ_COLOUR_GAUSSIAN_BLUR 10" in header and "#define MJ_COLOUR_BOX_BLUR     11" in header
    batch, keep = _batch([(128, 64), (50, 70)])
    for chain in (((10, 1.5),), ((11, 2.0),), ((10, 0.0), (11, 1024.0)), (("gaussian_blur", 0.3), ("invert",), ("box_blur", 0.25))):
        rc, out, msg = _normal(lib, batch, colour=[None, chain])
        assert rc == B.MJ_OK and out.mode == 0 and bool(out.colour), (chain, msg)
    for kind in (10, 11):
        for bad, why in ((-1.0, "a blur takes a radius of 0..1024"), (2000.0, "a blur takes a radius of 0..1024"), (float("nan"), "an op's value is not finite"),
                         (float("inf"), "an op's value is not finite")):
            rc, _, msg = _normal(lib, batch, colour=[None, ((kind, bad),)])
            assert rc == B.MJ_ERR_INVALID and "colour_ops: output 1: " + why in msg, (kind, bad, msg)
    # the kinds around them stay what they were
    for kind in (0, 12):
        rc, _, msg = _normal(lib, batch, colour=[None, ((kind, 1.0),)])
        assert rc == B.MJ_ERR_INVALID and "colour_ops: output 1: an op's kind is none of MJ_COLOUR_*" in msg
