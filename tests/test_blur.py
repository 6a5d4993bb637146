"""The blurs of color_ops= on the MI355X: ("gaussian_blur", radius) and ("box_blur", radius), Pillow's
im.filter(ImageFilter.GaussianBlur(radius) / BoxBlur(radius)) on the finished canvas.  As in tests/test_colour.py the expected bytes
are tools/colour_model.py — which tests/test_blur_host.py holds to Pillow — applied to the library's own uint8 canvases of the same
call without color_ops; the flip and the output table come afterwards.  Byte for byte: the plane-resident launch (the canvas in
LDS), the pass launches (canvases LDS does not hold, and option MJ_BLUR=passes), every layout."""
import numpy as np
import pytest

from test_colour import C411, C440, GREY, KINDS, MEAN, ODD, STD, base, decoder, expected, host, raw
from test_roi import LAYOUTS

pytestmark = pytest.mark.gpu

GAUSSIAN = (0, 0.1, 1.0, 1.42, 2.0, 3.0, 13.37, 1024)
BOX = (0.25, 1.5, 40)
SINGLE = [("gaussian_blur", r) for r in GAUSSIAN] + [("box_blur", r) for r in BOX]
# one call, five outputs: a blur at step 0, at step 2 behind a histogram op and color, as the last of four, two blurs, no chain
NAMES = [ODD, GREY, ODD, C440, C411]
CHAINS = [[("gaussian_blur", 1.3), ("solarize", 128)], [("contrast", 0.6), ("color", 1.7), ("box_blur", 2.5)],
          [("sharpness", 1.9), ("equalize",), ("posterize", 5), ("gaussian_blur", 0.7)], [("box_blur", 1.5), ("gaussian_blur", 0.8)], None]
MIRROR = [True, False, True, False, True]


@pytest.fixture(scope="module", autouse=True)
def decoders():
    """the decoders and canvases are tests/test_colour.py's, made on first use; this module closes what it opened"""
    import test_colour
    yield
    for dec in test_colour._DEC.values():
        dec.close()
    test_colour._DEC.clear()
    test_colour._BASE.clear()


@pytest.fixture
def passes():
    """the pass launches whatever the canvas's size (read when a plan is created)"""
    from pyjpegdecoder_amd import _binding as B
    B.set_option("MJ_BLUR", "passes")
    yield
    B.set_option("MJ_BLUR", None)


def files(names):
    return [raw(n) for n in names]


@pytest.mark.parametrize("op", SINGLE, ids=lambda op: "-".join(str(v) for v in op))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_each_blur_alone_on_four_kinds_of_file(layout, op):
    for size in ((24, 16), (33, 21)):
        kw = dict(size=size, mode="RGB")
        canv = base(layout, KINDS, **kw)
        got = host(decoder(layout).decode_device(files(KINDS), color_ops=[op], **kw))
        assert got.shape == canv.shape and got.dtype == np.uint8
        want = expected(canv, layout, [[op]] * len(KINDS))
        for k, n in enumerate(KINDS):
            assert np.array_equal(got[k], want[k]), (n, size, op)
        assert op[1] < 1 or not np.array_equal(got, canv)


@pytest.mark.parametrize("size", ((3, 5), (1, 7)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", LAYOUTS)
def test_canvases_narrower_than_the_taps_and_than_a_dword(layout, size):
    names = [ODD, C440]
    canv = base(layout, names, size=size)
    for op in (("gaussian_blur", 3.0), ("box_blur", 1.5)):
        got = host(decoder(layout).decode_device(files(names), size=size, color_ops=[op]))
        assert np.array_equal(got, expected(canv, layout, [[op]] * 2)), op


def five_outputs(layout, size):
    import torch
    kw = dict(size=size, mode="RGB")
    canv = base(layout, NAMES, **kw)
    dec = decoder(layout)
    got = host(dec.decode_device(files(NAMES), color_ops=CHAINS, **kw))
    want = expected(canv, layout, CHAINS)
    for k in range(len(NAMES)):
        assert np.array_equal(got[k], want[k]), k
    # the blur launch's own last-step store: the flip, the output table
    got = host(dec.decode_device(files(NAMES), color_ops=CHAINS, mirror=MIRROR, **kw))
    assert np.array_equal(got, expected(canv, layout, CHAINS, MIRROR))
    got = dec.decode_device(files(NAMES), color_ops=CHAINS, mirror=MIRROR, dtype=torch.float16, normalize=(MEAN, STD), **kw)
    assert got.dtype == torch.float16
    assert np.array_equal(got.cpu().view(torch.int16).numpy().view(np.uint16), expected(canv, layout, CHAINS, MIRROR, "float16"))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_blurs_beside_histogram_ops_table_ops_and_ended_chains(layout):
    five_outputs(layout, (33, 21))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_pass_launches_on_the_same_five_outputs(layout, passes):
    five_outputs(layout, (33, 21))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_component_outputs(layout):
    names = [GREY, ODD]
    kw = dict(size=(40, 28), mode="L")
    canv = base(layout, names, **kw)
    assert canv[0].size == 40 * 28
    got = host(decoder(layout).decode_device(files(names), color_ops=[("gaussian_blur", 2.0)], **kw))
    assert np.array_equal(got, expected(canv, layout, [[("gaussian_blur", 2.0)]] * 2))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_views_with_radii_of_their_own(layout):
    names = [ODD, C440]
    views = [(0, (5, 3, 40, 30)), (1, (8, 16, 32, 48)), 0]
    chains = [[("gaussian_blur", 0.3)], [("gaussian_blur", 1.9)], None]
    canv = base(layout, names, key="blur views", size=(24, 16), views=views)
    got = host(decoder(layout).decode_device(files(names), size=(24, 16), views=views, color_ops=chains))
    assert np.array_equal(got, expected(canv, layout, chains))
    assert np.array_equal(got[2], canv[2]) and not np.array_equal(got[1], canv[1])


@pytest.mark.parametrize("layout", ("rowmajor", "planar_rowmajor"))
def test_the_canvas_of_the_recipes(layout):
    """224 x 224: two planes of 50 176 bytes in LDS, more than the 64 KB a launch gets unasked"""
    kw = dict(size=(224, 224))
    drawn = float(np.random.default_rng(7).uniform(0.1, 2.0))
    canv = base(layout, [ODD, ODD], **kw)
    chains = [[("gaussian_blur", 2.0)], [("gaussian_blur", drawn)]]
    got = host(decoder(layout).decode_device(files([ODD, ODD]), color_ops=chains, **kw))
    want = expected(canv, layout, chains)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), drawn


@pytest.mark.parametrize("layout", ("rowmajor", "xmajor"))
def test_the_largest_canvas_that_lds_holds(layout):
    """256 x 320: two planes are exactly the 163 840 bytes of LDS a workgroup can have, so the plane-resident launch still runs, with
    all of it as dynamic LDS; 260 x 316 is the step beyond (two planes of 260 x 316: 164 320 bytes), pass by pass"""
    for size in ((256, 320), (260, 316)):
        canv = base(layout, [C440], size=size)
        chain = [("gaussian_blur", 1.6), ("invert",)]
        got = host(decoder(layout).decode_device(files([C440]), size=size, color_ops=chain))
        assert np.array_equal(got, expected(canv, layout, [chain])), size


@pytest.mark.parametrize("layout", ("rowmajor", "xmajor"))
def test_a_canvas_whose_planes_lds_does_not_hold(layout):
    """304 x 272: two planes are 165 376 bytes, so the plan blurs pass by pass through its third canvas"""
    import torch
    names = [ODD, C411]
    kw = dict(size=(304, 272))
    canv = base(layout, names, **kw)
    dec = decoder(layout)
    chains = [[("gaussian_blur", 2.0)], [("box_blur", 1.5)]]
    got = host(dec.decode_device(files(names), color_ops=chains, **kw))
    want = expected(canv, layout, chains)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    chains = [[("contrast", 1.4), ("gaussian_blur", 1.1)], [("invert",), ("box_blur", 3.3), ("gaussian_blur", 0.6)]]
    got = dec.decode_device(files(names), color_ops=chains, mirror=[True, False], dtype=torch.float16, normalize=(MEAN, STD), **kw)
    assert np.array_equal(got.cpu().view(torch.int16).numpy().view(np.uint16), expected(canv, layout, chains, [True, False], "float16"))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_calls_with_radii_of_their_own(layout):
    """nothing of an earlier call shows through the plan-owned canvases: each call gives its own bytes, in either order"""
    kw = dict(size=(33, 21), mode="RGB")
    canv = base(layout, KINDS, **kw)
    dec = decoder(layout)
    for radius in (1.9, 0.4, 1.9):
        got = host(dec.decode_device(files(KINDS), color_ops=[("gaussian_blur", radius), ("invert",)], **kw))
        assert np.array_equal(got, expected(canv, layout, [[("gaussian_blur", radius), ("invert",)]] * 4)), radius
    # ... on the pass launches too, whose first canvas a blur overwrites
    from pyjpegdecoder_amd import _binding as B
    B.set_option("MJ_BLUR", "passes")
    try:
        for radius in (1.9, 0.4):
            got = host(dec.decode_device(files(KINDS), color_ops=[("gaussian_blur", radius)], **kw))
            assert np.array_equal(got, expected(canv, layout, [[("gaussian_blur", radius)]] * 4)), radius
    finally:
        B.set_option("MJ_BLUR", None)


def test_decode_and_the_iterator_are_decode_device():
    dec = decoder("xmajor")
    kw = dict(size=(24, 16), mode="RGB")
    chains = [[("gaussian_blur", 1.2)], None, [("box_blur", 0.25), ("equalize",)], [("color", 0.0), ("gaussian_blur", 1.8), ("solarize", 128)]]
    want = expected(base("xmajor", KINDS, **kw), "xmajor", chains)
    assert np.array_equal(host(dec.decode_device(files(KINDS), color_ops=chains, **kw)), want)
    assert np.array_equal(dec.decode(files(KINDS), color_ops=chains, **kw), want)
    (one,) = list(dec.decode_device_iter([files(KINDS)], color_ops=[chains], **kw))
    assert np.array_equal(host(one), want)
    with pytest.raises(ValueError, match="output 0: gaussian_blur takes a radius of 0..1024"):
        dec.decode_device(files(KINDS), color_ops=[[("gaussian_blur", -0.5)], None, None, None], **kw)
