"""The cases of tests/colour_cases.py, without a GPU: every crafted file decodes — by the oracle — to the levels it was written
for, and the resize at its own size is the identity; every case reaches what it is there for, with the quantities spelled out (the
step, the quotients, lo and hi, the non-empty bins, the mean before it is rounded); every case tells the wrong variant it is aimed
at from the right one; and the library's host twin mj_host_colour_ops gives the model's bytes on every crafted canvas.  Everything
comes from the oracle's pixels and tools/colour_model.py, never from the library's decode: tests/test_colour_paths.py then runs the
same cases on the MI355X, after it has held the library's canvases to these."""
import numpy as np
import pytest

import colour_cases as CC
from conftest import GOLDEN
from routes_common import differ

ODD, GREY, C411 = "70x50_420_pil_opt", "64x64_grey_pil", "100x36_411_dri3"
TWINS = [(n, c) for n in CC.LEVELS for c in (False, True)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


def natural(name: str, size, mode=None) -> np.ndarray:
    """a natural file's canvas at ``size``: tools/resize_model.py on the golden pixels, row-major"""
    from tools import mode_model, resize_model
    full = np.load(GOLDEN / "files" / f"{name}.npz")["rgb"]
    rm = np.ascontiguousarray(full.swapaxes(0, 1))
    rm = rm[..., 0] if rm.ndim == 3 and rm.shape[2] == 1 else rm
    return resize_model.resize(mode_model.convert(rm, mode), size)


def hist(a):
    return np.bincount(np.asarray(a).ravel(), minlength=256)


def test_every_crafted_file_decodes_to_its_levels_and_the_resize_is_the_identity():
    from tools import resize_model
    for name, colour in TWINS:
        px = CC.pixels(name, colour)
        assert px.shape[:2] == CC.size_of(name)[::-1] and px.ndim == (3 if colour else 2), (name, colour, px.shape)
        assert np.array_equal(px, CC.intended(name, colour)), (name, colour)
        assert np.array_equal(resize_model.resize(px, CC.size_of(name)), px), (name, colour)
    px = CC.pixels(CC.COLOUR)
    assert px.shape == (32, 32, 3)
    blocks = px.reshape(4, 8, 4, 8, 3)
    assert (blocks == blocks[:, :1, :, :1]).all(), "a block of the colour file is not flat"
    assert np.array_equal(resize_model.resize(px, (32, 32)), px)
    # a grey file as "RGB" and a twin as "L" are the twin and the grey file
    for name in CC.LEVELS:
        assert np.array_equal(CC.canvas(name, False, "RGB"), CC.intended(name, True)) and np.array_equal(CC.canvas(name, True, "L"), CC.intended(name))


def test_every_case_reaches_what_it_is_for():
    from tools import colour_model as M
    identity = np.arange(256)
    assert (hist(CC.pixels("all_levels")) == 64).all() and CC.size_of("all_levels") == (128, 128)
    for level in (77, 255):
        a = CC.pixels(f"one_level_{level}")
        h = hist(a)
        nz = np.flatnonzero(h)
        assert len(nz) == 1 and nz[0] == nz[-1] == level                       # nz <= 1 and hi <= lo
        assert sum(i * int(h[i]) for i in range(256)) / int(h.sum()) == float(level) and M.contrast_mean(a) == level
        assert np.array_equal(M.autocontrast_table(h), identity) and np.array_equal(M.equalize_table(h), identity)
        for layout in ("rowmajor", "xmajor"):                                  # every lane of the histogram launch: one run
            lanes = CC.memory_order(a, layout).reshape(-1, CC.LANE_PIXELS)
            assert (lanes == lanes[:, :1]).all()
    for op in CC.BLURS:
        assert (M.apply_op(CC.pixels("one_level_255"), op) == 255).all()
    two = CC.pixels("two_levels")
    nz = np.flatnonzero(hist(two))
    assert list(nz) == [10, 200] and set(np.unique(M.apply_op(two, ("autocontrast",)))) == {0, 255}
    h = hist(CC.pixels("zero_step"))
    assert [int(v) for v in h[np.flatnonzero(h)]] == [64, 64, 64, 832] and CC.equalize_quantities(h) == (0, [])
    assert np.array_equal(M.equalize_table(h), identity)
    h = hist(CC.pixels("clips"))
    assert list(np.flatnonzero(h)) == [3, 50, 100, 150, 200, 240]
    assert CC.equalize_quantities(h) == (1, [0, 64, 128, 192, 256, 320])
    assert [int(M.equalize_table(h)[v]) for v in (200, 240)] == [255, 255]
    tie = CC.pixels("mean_tie")
    h = hist(tie)
    assert sum(i * int(h[i]) for i in range(256)) / int(h.sum()) == 10.5 and M.contrast_mean(tie) == 11
    assert (M.apply_op(tie, ("contrast", 0)) == 11).all()
    board = CC.pixels("board")
    assert set(np.unique(board)) == {0, 255} and board.shape == (24, 40)
    for op in CC.BLURS:
        fr = M.gaussian_box_radius(op[1]) if op[0] == "gaussian_blur" else np.float32(op[1])
        along, across = M.box_pass(board, fr, 1), M.box_pass(board, fr, 0)
        assert differ(along, board) and differ(across, board) and differ(along, across)
    # the colour file: four histograms of their own, and an L whose mean is no component's
    px = CC.pixels(CC.COLOUR)
    hs = CC.histograms(px)
    keys = list(hs)
    assert keys == [0, 1, 2, "L"]
    for i, a in enumerate(keys):
        for b in keys[:i]:
            assert not np.array_equal(hs[a], hs[b]), (a, b)
    means = {k: CC.mean_of(hs[k]) for k in keys}
    assert all(means["L"] != means[c] for c in (0, 1, 2)), means
    assert all(len(np.flatnonzero(hs[c])) >= 12 for c in keys)
    for c in (0, 1, 2):
        step, q = CC.equalize_quantities(hs[c])
        assert step == 3 and step // 2 == 1 and max(q) > 255 and len(set(q)) >= 12, (c, step, q)


def test_the_exposed_model_is_the_model():
    """colour_cases.histograms / table_op / blur_variant with nothing changed are tools/colour_model.py's ops"""
    from tools import colour_model as M
    canvases = [CC.canvas(n, c) for n, c in TWINS] + [CC.pixels(CC.COLOUR), natural(ODD, (17, 241)), natural(GREY, (23, 7))]
    for a in canvases:
        for layout in ("rowmajor", "xmajor"):
            hs = CC.histograms(a, layout)
            for op in CC.STATISTICS:
                assert np.array_equal(CC.table_op(a, op, hs), M.apply_op(a, op)), (a.shape, op, layout)
        if a.size <= 4096 * 3:
            for op in CC.BLURS:
                assert np.array_equal(CC.blur_variant(a, op), M.apply_op(a, op)), (a.shape, op)


def test_every_case_tells_its_wrong_variant_from_the_right_one():
    from tools import colour_model as M
    colour = CC.pixels(CC.COLOUR)
    eq, ac = ("equalize",), ("autocontrast",)
    # equalize that starts at n = 0: the colour file (step 3, n starts at 1)
    assert differ(CC.table_op(colour, eq, CC.histograms(colour), equalize=CC.equalize_from_zero), M.apply_op(colour, eq))
    # equalize that wraps instead of clipping: the quotients 256 and 320
    for twin in (False, True):
        a = CC.pixels("clips", twin)
        assert differ(CC.table_op(a, eq, CC.histograms(a), equalize=CC.equalize_wrapping), M.apply_op(a, eq))
        assert differ(CC.table_op(colour, eq, CC.histograms(colour), equalize=CC.equalize_wrapping), M.apply_op(colour, eq))
    # autocontrast without its identity branch: a flat band
    for name in ("one_level_77", "one_level_255"):
        a = CC.pixels(name)
        assert differ(CC.table_op(a, ac, CC.histograms(a), autocontrast=CC.autocontrast_always_stretching), M.apply_op(a, ac)), name
    two = CC.pixels("two_levels")                # (where the band is not flat the variant is the model)
    assert np.array_equal(CC.table_op(two, ac, CC.histograms(two), autocontrast=CC.autocontrast_always_stretching), M.apply_op(two, ac))
    # contrast's mean truncated: the tie
    tie = CC.pixels("mean_tie")
    for f in (0, 0.3, 1.9):
        assert differ(CC.table_op(tie, ("contrast", f), CC.histograms(tie), round_half_up=False), M.apply_op(tie, ("contrast", f))), f
    # contrast's mean from component 0 instead of L: the colour file
    for f in (0, 0.3, 1.9):
        assert differ(CC.table_op(colour, ("contrast", f), CC.histograms(colour), mean_band=0), M.apply_op(colour, ("contrast", f))), f
    # a histogram that loses the pixels beyond the last whole chunk: every crafted canvas but the one of exactly four chunks, and
    # the canvases of 4097 pixels in either order, where ONE pixel is lost
    for name in CC.NAMES:
        a = CC.pixels(name)
        lost = CC.histograms(a, whole_chunks_only=True)
        if name == "all_levels":
            assert np.array_equal(lost[0], hist(a))
            continue
        assert int(lost[0].sum()) == 0
        op = ("contrast", 0.3) if name.startswith("one_level") else eq if name in ("clips", CC.COLOUR) else ("contrast", 0.3) if name == "board" else ac if name == "two_levels" else ("contrast", 0)
        assert differ(CC.table_op(a, op, lost), M.apply_op(a, op)), name
    for size in ((17, 241), (241, 17)):
        for mode in ("RGB", "L"):
            a = natural(ODD, size, mode)
            for layout in ("rowmajor", "xmajor"):
                lost = CC.histograms(a, layout, whole_chunks_only=True)
                assert int(lost["L"].sum()) == 4096
                assert differ(CC.table_op(a, eq, lost), M.apply_op(a, eq)), (size, mode, layout)
    # a histogram that loses a lane's last run
    for name, op in (("one_level_77", ("contrast", 0.3)), ("two_levels", ac), ("clips", eq), ("mean_tie", ("contrast", 0)), ("board", ("contrast", 0.3)), (CC.COLOUR, eq)):
        a = CC.pixels(name)
        for layout in ("rowmajor", "xmajor"):
            lost = CC.histograms(a, layout, without_last_runs=True)
            assert int(lost[0].sum()) < a.shape[0] * a.shape[1]
            assert differ(CC.table_op(a, op, lost), M.apply_op(a, op)), (name, layout)
    for size in CC.HIST_SIZES:             # (161 pixels: equalize's step is 0, so autocontrast and contrast tell it, on the second file)
        a = natural(ODD if size != (23, 7) else C411, size)
        lost = CC.histograms(a, without_last_runs=True)
        for op in ((eq,) if size != (23, 7) else (ac, ("contrast", 0.3))):
            assert differ(CC.table_op(a, op, lost), M.apply_op(a, op)), (size, op)
    # a blur whose taps clamp at the row's padded width, with zero padding: the canvases whose width is no multiple of four
    for size in CC.BLUR_SIZES:
        a = natural(ODD, size)
        for op in CC.BLURS:
            assert differ(CC.blur_variant(a, op, padded=True), M.apply_op(a, op)), (size, op)
    a = natural(ODD, (6, 5))
    for r in CC.BOX_RADII:
        assert differ(CC.blur_variant(a, ("box_blur", r), padded=True), M.apply_op(a, ("box_blur", r))), r
    # a blur with the height passes first: the board
    # (the board is symmetric enough for one box pass each way to commute: the box blur is told on a natural canvas)
    board = CC.pixels("board")
    assert differ(CC.blur_variant(board, CC.BLURS[0], height_first=True), M.apply_op(board, CC.BLURS[0]))
    for size in CC.BLUR_SIZES[1:3]:
        a = natural(ODD, size)
        for op in CC.BLURS:
            assert differ(CC.blur_variant(a, op, height_first=True), M.apply_op(a, op)), (size, op)


def test_the_geometries_are_what_they_are_for():
    assert [w * h for w, h in CC.HIST_SIZES] == [CC.HIST_PIXELS, CC.HIST_PIXELS + 1, CC.HIST_PIXELS + 1, 161] and 161 < 256 * CC.LANE_PIXELS and 161 % CC.LANE_PIXELS
    assert [w % 4 for w, _ in CC.BLUR_SIZES[:3]] == [2, 2, 2] and CC.BLUR_SIZES[3][1] == 1
    assert set(CC.BOX_RADII) >= {6 - 2, 6 - 1, 6, 5 - 2, 5 - 1, 5} and max(CC.BOX_RADII) > 5          # (beyond the height; the width's n - 2, n - 1 and n)
    chains = CC.many_chains()
    assert len(chains) == CC.MANY == len(set(CC.many_views(70, 50))) > 64
    real = [c for c in chains if c is not None]
    assert len(set(real)) == len(real) == 60
    at = lambda kinds, s: [k for k, c in enumerate(chains) if c is not None and len(c) > s and c[s][0] in kinds]          # noqa: E731
    hists, blurs = ("contrast", "autocontrast", "equalize"), ("gaussian_blur", "box_blur")
    assert len(at(blurs, 0)) == 20 > len(at(blurs, 1)) == 10 and len(at(blurs, 3)) == 10 and not at(blurs, 2)
    for s in (0, 1):                            # sparse index lists that reach beyond the first 64 outputs
        assert 0 < len(at(hists, s)) < CC.MANY and max(at(hists, s)) >= 64
    assert max(at(blurs, 0)) >= 64
    assert {op[0] for c in real for op in c} >= {"sharpness", "color", "solarize", "posterize", "invert", "brightness"}


@pytest.mark.parametrize("name", CC.NAMES)
def test_the_host_twin_gives_the_models_bytes_on_every_crafted_canvas(lib, name):
    from pyjpegdecoder_amd import _binding as B
    from tools import colour_model as M
    canvases = [CC.pixels(CC.COLOUR), CC.canvas(CC.COLOUR, mode="L")] if name == CC.COLOUR else [CC.pixels(name), CC.pixels(name, True)]
    for a in canvases:
        for chain in CC.chains_of(name):
            assert np.array_equal(B.colour_ops(a, chain), M.apply_chain(a, chain)), (name, a.shape, chain)
