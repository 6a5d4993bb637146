"""("adjust_hue", f) of color_ops= on the MI355X: torchvision's F.adjust_hue on a PIL image — Pillow's HSV round trip with a shift
added to H —, the fourth knob of ColorJitter, on the finished canvas.  As in tests/test_colour.py the expected bytes are
tools/colour_model.py — which tests/test_hue_host.py holds to Pillow over all 2^24 inputs — applied to the library's own uint8
canvases of the same call without color_ops and without mirror; the flip and tools/normalize_model.py come afterwards.  Byte for
byte, in every layout: the hue launch (four pixels per lane, the tail of a canvas that is no multiple of four), the outputs it and
the blur launch take from k_colour_apply in one plan, steps without an apply launch, and one-component outputs, where the op is
k_colour_apply's copy."""
import numpy as np
import pytest

import hue_cases
from test_colour import C411, C440, GREY, KINDS, MEAN, ODD, STD, base, decoder, expected, host, raw, to_rowmajor
from test_roi import LAYOUTS

pytestmark = pytest.mark.gpu

FACTORS = (-0.5, -0.1, 0.0, 0.25, 0.5)
SIZES = ((24, 16), (120, 96), (23, 17))             # (23 x 17: neither the width nor the 391 pixels are a multiple of four)
JITTER = [("brightness", 1.3), ("contrast", 0.7), ("color", 1.6)]


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
    """the blurs' pass launches whatever the canvas's size (read when a plan is created)"""
    from pyjpegdecoder_amd import _binding as B
    B.set_option("MJ_BLUR", "passes")
    yield
    B.set_option("MJ_BLUR", None)


def files(names):
    return [raw(n) for n in names]


def check(layout, names, chains, key=None, **kw):
    """the call with these chains (one for all, or one per output) against the model on the call's own canvases; -> (canvases, got)"""
    canv = base(layout, names, key=key, **kw)
    got = host(decoder(layout).decode_device(files(names), color_ops=chains, **kw))
    per_output = chains if chains and not isinstance(chains[0], tuple) else [chains] * len(canv)
    want = expected(canv, layout, per_output)
    assert got.shape == canv.shape and got.dtype == np.uint8
    for k in range(len(canv)):
        assert np.array_equal(got[k], want[k]), (k, per_output[k])
    return canv, got


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_op_alone_on_four_kinds_of_file(layout, factor):
    """files of four kinds in one call, hence several plans into one tensor through slots; factor 0 is the round trip, not a copy"""
    for size in SIZES:
        canv, got = check(layout, KINDS, [("adjust_hue", factor)], size=size, mode="RGB")
        assert not np.array_equal(got, canv), size
        assert np.array_equal(got[1], canv[1])          # (the grey file's R = G = B: max == min, whatever the shift)


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_branch_of_the_arithmetic(layout, factor):
    """the crafted file at its own size — the canvas is its flat blocks — and shrunk to 23 x 17, where the blocks' borders mix; the
    census is taken over the library's own canvases, so the comparison cannot pass on inputs that miss a branch"""
    from tools import colour_model
    name = hue_cases.raw()
    for size in (hue_cases.SIZE, (23, 17)):
        canv, got = check(layout, [name], [("adjust_hue", factor)], key=f"crafted {size}", size=size)
        rm = to_rowmajor(canv[0], layout)
        if size == hue_cases.SIZE:
            assert np.array_equal(rm, hue_cases.intended())
        assert hue_cases.census([rm], colour_model.hue_shift(factor)) == hue_cases.CLASSES, size


CHAINS = {"hue-first": [("adjust_hue", 0.1)] + JITTER, "hue-in-the-middle": JITTER[:2] + [("adjust_hue", -0.1)] + JITTER[2:],
          "hue-last": JITTER + [("adjust_hue", 0.05)], "hue-twice": [("adjust_hue", 0.5), ("equalize",), ("adjust_hue", -0.5)]}


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_colorjitter_chain_in_its_orders(layout, name):
    check(layout, KINDS, CHAINS[name], size=(40, 28), mode="RGB")
    check(layout, [ODD, C440], CHAINS[name], size=(23, 17))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_hue_last_with_mirror_and_the_output_table(layout):
    import torch
    names = [ODD, C440, C411, ODD]
    mirror = [True, False, True, False]
    chains = [CHAINS["hue-last"], [("adjust_hue", -0.3)], None, [("equalize",), ("adjust_hue", 0.0)]]
    for size in ((40, 28), (23, 17)):
        kw = dict(size=size)
        canv = base(layout, names, **kw)
        dec = decoder(layout)
        got = host(dec.decode_device(files(names), color_ops=chains, mirror=mirror, **kw))
        assert np.array_equal(got, expected(canv, layout, chains, mirror))
        got = dec.decode_device(files(names), color_ops=chains, mirror=mirror, dtype=torch.float16, normalize=(MEAN, STD), **kw)
        assert got.dtype == torch.float16
        bits = got.cpu().view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(bits, expected(canv, layout, chains, mirror, "float16"))
        got = dec.decode_device(files(names), color_ops=chains, mirror=mirror, dtype=torch.float32, **kw)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), expected(canv, layout, chains, mirror, "float32", normalize=False))


def hue_and_blur(layout):
    """both leave-out lists active in one plan: hue then a blur, a blur then hue, and both at one step in different outputs"""
    names = [ODD, ODD, ODD, ODD]
    chains = [[("adjust_hue", 0.2), ("gaussian_blur", 1.3)], [("gaussian_blur", 0.9), ("adjust_hue", -0.2)],
              [("box_blur", 1.5), ("adjust_hue", 0.4), ("gaussian_blur", 0.6), ("adjust_hue", -0.4)], [("adjust_hue", 0.3), ("box_blur", 0.75)]]
    for size in ((40, 28), (23, 17)):
        check(layout, names, chains, size=size)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_hue_and_blur_in_one_plan(layout):
    hue_and_blur(layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_hue_and_blur_in_one_plan_pass_by_pass(layout, passes):
    hue_and_blur(layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_four_kinds_of_op_at_one_step(layout):
    """step 0: hue, brightness, a blur and nothing, in one plan (ODD four times); step 1 swaps them round; a fifth output of another plan"""
    names = [ODD, ODD, ODD, ODD, C440]
    chains = [[("adjust_hue", 0.15), ("brightness", 1.2)], [("brightness", 0.8), ("adjust_hue", -0.15)], [("gaussian_blur", 1.1), ("adjust_hue", 0.45)], None,
              [("adjust_hue", 0.0)]]
    canv, got = check(layout, names, chains, size=(33, 21))
    assert np.array_equal(got[3], canv[3])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_step_at_which_every_output_is_hue(layout):
    """no apply launch at step 0 (every output is the hue launch's); at step 1 every output is hue or a blur: none there either"""
    names = [ODD, ODD, ODD]
    chains = [[("adjust_hue", 0.1), ("adjust_hue", 0.2), ("invert",)], [("adjust_hue", -0.25), ("box_blur", 1.0)], [("adjust_hue", 0.5), ("adjust_hue", -0.5)]]
    for size in ((24, 16), (23, 17)):
        check(layout, names, chains, size=size)
    check(layout, names, [("adjust_hue", 0.37)], size=(23, 17))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_component_outputs_are_left_as_they_are(layout):
    """mode="L" and a grey file in its own components: the op is the identity — a copy that takes up its step —, and the op behind it
    is still applied"""
    dec = decoder(layout)
    kw = dict(size=(23, 17), mode="L")
    canv = base(layout, KINDS, **kw)
    assert canv[0].size == 23 * 17
    assert np.array_equal(host(dec.decode_device(files(KINDS), color_ops=[("adjust_hue", 0.3)], **kw)), canv)
    for chain in ([("adjust_hue", 0.3), ("contrast", 1.7)], [("invert",), ("adjust_hue", -0.5), ("adjust_hue", 0.0), ("posterize", 3)]):
        got = host(dec.decode_device(files(KINDS), color_ops=chain, **kw))
        assert np.array_equal(got, expected(canv, layout, [chain] * 4)) and not np.array_equal(got, canv), chain
    one = base(layout, [GREY], size=(24, 16))
    assert np.array_equal(host(dec.decode_device([raw(GREY)], size=(24, 16), color_ops=[("adjust_hue", 0.5)])), one)
    chain = [("adjust_hue", 0.5), ("box_blur", 1.0), ("solarize", 100)]
    got = host(dec.decode_device([raw(GREY)], size=(24, 16), color_ops=chain))
    assert np.array_equal(got, expected(one, layout, [chain])) and not np.array_equal(got, one)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_views_of_one_file_with_different_factors(layout):
    views = [(0, (5, 3, 40, 30)), (0, (5, 3, 40, 30)), (0, (33, 11, 37, 39)), 0]
    chains = [[("adjust_hue", 0.25)], [("adjust_hue", -0.25)], [("contrast", 1.8), ("adjust_hue", 0.1)], None]
    canv, got = check(layout, [ODD], chains, key="hue views", size=(23, 17), views=views)
    assert np.array_equal(canv[0], canv[1]) and not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_second_execute_of_the_plan_gives_the_same_bytes(layout):
    """the canvases, the lists and the tables are the plan's: nothing of the first execute is left over for the second"""
    import torch
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    dec = decoder(layout)
    names = [ODD, ODD, ODD]
    chains = [JITTER + [("adjust_hue", 0.1)], [("adjust_hue", -0.2), ("gaussian_blur", 1.0)], None]
    size = (23, 17)
    want = expected(base(layout, names, size=size), layout, chains)
    prep = prepare_batch(files(names), dec.layout, 0)
    plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 3}, size=size, colour=chains)
    try:
        for sentinel in (0x5A, 0xA5):
            out = torch.full((want.size,), sentinel, dtype=torch.uint8, device=torch.device("cuda", dec.ctx.device))
            plan.execute(0, out.data_ptr())
            plan.sync()
            assert not plan.read(rgb=False)["status"].any()
            assert np.array_equal(out.cpu().numpy().reshape(want.shape), want), sentinel
    finally:
        plan.close()


@pytest.mark.parametrize("layout", ("rowmajor", "planar"))
def test_decode_and_the_iterator_are_decode_device(layout):
    dec = decoder(layout)
    chains = [CHAINS["hue-last"], [("adjust_hue", -0.4)], None, CHAINS["hue-first"]]
    kw = dict(size=(23, 17), mode="RGB", mirror=[False, True, True, False])
    got = host(dec.decode_device(files(KINDS), color_ops=chains, **kw))
    assert np.array_equal(got, expected(base(layout, KINDS, size=(23, 17), mode="RGB"), layout, chains, kw["mirror"]))
    assert np.array_equal(dec.decode(files(KINDS), color_ops=chains, **kw), got)
    kw.pop("mirror")
    one, two = list(dec.decode_device_iter([files(KINDS), files(KINDS)[:1]], color_ops=[chains, [[("adjust_hue", -0.4)]]], **kw))
    assert np.array_equal(host(one), host(dec.decode_device(files(KINDS), color_ops=chains, **kw)))
    assert np.array_equal(host(two), host(dec.decode_device(files(KINDS)[:1], color_ops=[("adjust_hue", -0.4)], **kw)))


def test_refusals_name_what_is_wrong():
    dec = decoder("xmajor")
    for bad in (0.500001, -0.500001):
        with pytest.raises(ValueError, match=r"output 1: adjust_hue takes a factor of -0\.5\.\.0\.5"):
            dec.decode_device(files([ODD, ODD]), size=(24, 16), color_ops=[None, [("adjust_hue", bad)]])
    with pytest.raises(ValueError, match="is not finite"):
        dec.decode_device(files([ODD]), size=(24, 16), color_ops=[("adjust_hue", float("nan"))])
    with pytest.raises(ValueError, match=r"unknown op 'hue' .*adjust_hue"):
        dec.decode_device(files([ODD]), size=(24, 16), color_ops=[("hue", 0.1)])
