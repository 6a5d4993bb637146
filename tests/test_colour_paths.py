"""The paths of the colour launches (csrc/colour.hip) that tests/test_colour.py and tests/test_blur.py do not reach on purpose, on
the MI355X: the data-dependent branches of k_colour_tables on crafted canvases (a flat band, a zero step, quotients above 255, the
.5 tie of contrast's mean) and every entry of every table; k_colour_hist on canvases of exactly one chunk, of one chunk and a pixel,
and of fewer pixels than one chunk has lanes; the blurs' dword forms on rows whose last dword is half padding, on one row, and with
radii at and beyond the canvas's sides, plane-resident and pass by pass; and a call of 70 outputs whose histogram and blur lists
are sparse.  The cases are tests/colour_cases.py's, which tests/test_colour_paths_host.py holds — on the CPU — to what they are meant
to reach and to the wrong variants they must tell apart.

As in tests/test_colour.py the expected bytes are tools/colour_model.py applied to the library's own canvases of the same call
without color_ops; for the crafted files those canvases are first held to the oracle's pixels, so that the host file's census is
a census of what the GPU was given.  Byte for byte; floats as bit patterns.

Left out: the idle tail of the grids beyond kResizeGridX = 1 << 20 workgroups.  Nothing here looks at generated code."""
from contextlib import contextmanager

import numpy as np
import pytest

import colour_cases as CC
from test_colour import C411, GREY, MEAN, ODD, STD, base, decoder, expected, host, raw, to_rowmajor
from test_roi import LAYOUTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def decoders():
    """the decoders and canvases are tests/test_colour.py's, made on first use; this module closes what it opened"""
    import test_colour
    yield
    for dec in test_colour._DEC.values():
        dec.close()
    test_colour._DEC.clear()
    test_colour._BASE.clear()


@contextmanager
def blur_route(route):
    """"plane": the plane-resident launch where LDS holds the canvas; "passes": the pass launches (read when a plan is created)"""
    from pyjpegdecoder_amd import _binding as B
    B.set_option("MJ_BLUR", "passes" if route == "passes" else None)
    try:
        yield
    finally:
        B.set_option("MJ_BLUR", None)


def crafted(layout, name, colour=False, mode=None):
    """(the file, the call's keywords, the library's canvas of it) — the canvas held to the oracle's pixels"""
    kw = dict(size=CC.size_of(name))
    if mode is not None:
        kw["mode"] = mode
    one = base(layout, [CC.raw(name, colour)], **kw)
    assert np.array_equal(to_rowmajor(one[0], layout), CC.canvas(name, colour, mode)), (name, colour, mode, "the canvas is not the crafted one")
    return CC.raw(name, colour), kw, one


def run_chains(layout, file, kw, one, chains, what, singly=()):
    """ONE call whose outputs are the file once per chain — so the plan's lists name some outputs and not others at every step —,
    then the chains of ``singly`` in calls of their own"""
    dec = decoder(layout)
    canv = np.concatenate([one] * len(chains))
    got = host(dec.decode_device([file] * len(chains), color_ops=list(chains), **kw))
    want = expected(canv, layout, chains)
    assert got.shape == want.shape and got.dtype == np.uint8, what
    for k, chain in enumerate(chains):
        assert np.array_equal(got[k], want[k]), (what, chain, int((got[k] != want[k]).sum()), "bytes differ")
    for chain in singly:
        got = host(dec.decode_device([file], color_ops=[chain], **kw))
        assert np.array_equal(got, expected(one, layout, [chain])), (what, "alone", chain)


VARIANTS = {"grey": ("all_levels", False, None), "grey_as_RGB": ("all_levels", False, "RGB"), "444": ("all_levels", True, None),
            "444_as_L": ("all_levels", True, "L"), "colour": (CC.COLOUR, True, None), "colour_as_L": (CC.COLOUR, True, "L")}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_entry_of_every_table(layout, variant):
    """a canvas that has every level 0..255: brightness and contrast at 0, 0.3, 1, 1.9 and -0.5, posterize 1 and 8, solarize 0 and
    256, invert, autocontrast and equalize — alone and as the second op of a chain —, in one component, in three that are equal and
    (the colour file) in three with histograms of their own and an L of its own"""
    name, colour, mode = VARIANTS[variant]
    file, kw, one = crafted(layout, name, colour, mode)
    run_chains(layout, file, kw, one, CC.chains_of(name), variant, singly=[(("equalize",),), (("contrast", 1.9),)])


RARE = ("one_level_77", "one_level_255", "two_levels", "zero_step", "clips", "mean_tie")


@pytest.mark.parametrize("name", RARE)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_rare_branches_of_the_tables(layout, name):
    """hi <= lo and nz <= 1 on a flat canvas, autocontrast to {0, 255}, equalize with a zero step and with quotients above 255, the
    .5 tie of contrast's mean: autocontrast, equalize and contrast on each, alone, behind an op that changes nothing (the
    statistics are canvas 1's) and behind invert; the grey file, its 4:4:4 twin, and each in the other mode"""
    stats = [c for c in CC.chains_of(name) if not any(op in CC.BLURS for op in c)]
    for colour, mode in ((False, None), (True, None), (False, "RGB"), (True, "L")):
        file, kw, one = crafted(layout, name, colour, mode)
        run_chains(layout, file, kw, one, stats, (name, colour, mode), singly=stats[:len(CC.STATISTICS)] if mode is None else ())


@pytest.mark.parametrize("route", ("plane", "passes"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_blurs_of_a_flat_canvas_and_of_the_board(layout, route):
    """255 everywhere stays 255 (the weights sum to 1 << 24 exactly); the board is a blur at full contrast in both directions"""
    import torch
    chains = [c for c in CC.chains_of("board") if any(op in CC.BLURS for op in c)]
    with blur_route(route):
        for name in ("one_level_255", "board"):
            for colour in (False, True):
                file, kw, one = crafted(layout, name, colour)
                run_chains(layout, file, kw, one, chains, (name, colour, route), singly=[(op,) for op in CC.BLURS])
                if name == "one_level_255":
                    got = host(decoder(layout).decode_device([file], color_ops=[CC.BLURS[0]], **kw))
                    assert (got == 255).all()
        # once through the blur launch's own last-step store: mirrored, normalised, float16
        file, kw, one = crafted(layout, "board", True)
        both = [(CC.BLURS[0],), (("invert",), CC.BLURS[1])]
        got = decoder(layout).decode_device([file, file], color_ops=both, mirror=[True, False], dtype=torch.float16, normalize=(MEAN, STD), **kw)
        assert got.dtype == torch.float16
        want = expected(np.concatenate([one] * 2), layout, both, [True, False], "float16")
        assert np.array_equal(got.cpu().view(torch.int16).numpy().view(np.uint16), want)


def natural_chains(layout, names, chains, what, **kw):
    """every file under every chain, in ONE call"""
    files = [n for n in names for _ in chains]
    every = [c for _ in names for c in chains]
    canv = base(layout, files, **kw)
    got = host(decoder(layout).decode_device([raw(n) for n in files], color_ops=every, **kw))
    want = expected(canv, layout, every)
    for k in range(len(files)):
        assert np.array_equal(got[k], want[k]), (what, files[k], every[k], int((got[k] != want[k]).sum()), "bytes differ")


@pytest.mark.parametrize("size", CC.HIST_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", ("rowmajor", "xmajor", "planar"))
def test_the_histogram_launch_at_one_chunk_one_pixel_more_and_fewer_pixels_than_lanes(layout, size):
    """64 x 64: exactly one chunk of 4096 pixels; 17 x 241 and 241 x 17: a second chunk of ONE pixel — the last of a row in one
    layout, of a column in the other; 23 x 7: 161 pixels, so most lanes have none and one has a single pixel.  Three components
    (four histograms) and one."""
    natural_chains(layout, [ODD, C411], CC.HIST_CHAINS, size, size=size, mode="RGB")
    natural_chains(layout, [GREY, C411], CC.HIST_CHAINS, size, size=size, mode="L")


@pytest.mark.parametrize("route", ("plane", "passes"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_blurs_at_row_ends_on_one_row_and_with_radii_at_and_beyond_the_sides(layout, route):
    """widths 2, 6 and 34: the last dword of a row holds two pixels and two bytes of padding; 7 x 1: one row, so every tap across
    is that row; 6 x 5 with box radii 3, 4, 5 and 6: r = n - 2, n - 1, n and beyond, where every tap is clamped"""
    with blur_route(route):
        for size in CC.BLUR_SIZES:
            natural_chains(layout, [ODD, C411], CC.BLUR_CHAINS, (size, route), size=size, mode="RGB")
            natural_chains(layout, [GREY], CC.BLUR_CHAINS, (size, route), size=size)
        radii = [(("box_blur", float(r)),) for r in CC.BOX_RADII] + [(("box_blur", r + 0.5), ("gaussian_blur", float(r))) for r in CC.BOX_RADII]
        natural_chains(layout, [ODD], radii, ("radii", route), size=(6, 5))
        natural_chains(layout, [GREY], radii, ("radii", route), size=(6, 5))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_seventy_views_with_chains_of_their_own(layout):
    """one file as 70 views, view k's chain from a cycle of seven with its factor or radius from k: the histogram list and the blur
    list of every step name some outputs of more than one wavefront's worth and not the others, and step 1 has fewer blur outputs
    than step 0.  Held view by view; then once more with alternating mirror flags as float32."""
    import torch
    views, chains = CC.many_views(70, 50), CC.many_chains()
    kw = dict(size=CC.MANY_SIZE, views=views)
    canv = base(layout, [ODD], key="seventy views", **kw)
    assert len(canv) == CC.MANY
    dec = decoder(layout)
    got = host(dec.decode_device([raw(ODD)], color_ops=chains, **kw))
    want = expected(canv, layout, chains)
    for k in range(CC.MANY):
        assert np.array_equal(got[k], want[k]), ("view", k, chains[k])
        assert chains[k] is not None or np.array_equal(got[k], canv[k])
    mirror = [bool(k & 1) for k in range(CC.MANY)]
    got = dec.decode_device([raw(ODD)], color_ops=chains, mirror=mirror, dtype=torch.float32, **kw)
    assert got.dtype == torch.float32
    bits, want = got.cpu().numpy().view(np.uint32), expected(canv, layout, chains, mirror, "float32", normalize=False)
    for k in range(CC.MANY):
        assert np.array_equal(bits[k], want[k]), ("view", k, chains[k], "mirrored" if mirror[k] else "as it is")
