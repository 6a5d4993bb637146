"""The paths of k_reduce (csrc/reduce.hip) that tests/test_reduce.py does not reach, on the MI355X: row segments staged in pieces
with a cell across the piece boundary, in the colour, the LUMA and the grey instance; two tiles along the contiguous axis under a
phase; tile rows of 500 and more bytes with a tail store; a small image whose second tile returns early; views whose pitch is not
their length, on rows staged in pieces; a cell of 65536 pixels, and the refusal of the next size.  The cases are
tests/reduce_cases.py's, which tests/test_reduce_paths_host.py holds — on the CPU — to the paths they are meant to reach and to the
wrong variants of the kernel's loop they must tell apart.

Every output is byte for byte tools/reduce_model.resize of the oracle's pixels, converted (tools/mode_model.py), oriented
(tools/orient_model.py) and cropped as tests/test_reduce.py and tests/test_views_host.py do it; expected values never come from
the library.  Before any pixel is compared, the plan's own numbers are held to the census: mj_debug_reduce_shape (that it reduces
at all, the factors, phases and reduced size of every output) and mj_debug_reduce_launch (tiles and the staged piece) — a plan
that ran the single step, or a launch cut otherwise than the census says, fails here and not silently.  The row-major layouts run
the wide files, the x-major ones the files with width and height exchanged.

Left out: the idle tail of the grid beyond 1 << 20 workgroups, which needs a batch no test should build."""
import numpy as np
import pytest

import reduce_cases as RC
from test_resize import as_layout

pytestmark = pytest.mark.gpu

_expected = {}


def host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def want(c: RC.Case, k: int, layout: str, filter: str = "bilinear") -> np.ndarray:
    """the model's bytes of output k of case c, once per (case, output, filter) and left unchanged: the layouts share them"""
    key = (c.name, c.fast, k, filter)
    if key not in _expected:
        _expected[key] = RC.expected(c, c.slots[k], filter)
    return as_layout(_expected[key], layout)


def call_args(c: RC.Case):
    """(files, keywords) of the one call — and the one plan — that case c is"""
    kw = {"size": c.size, "reducing_gap": c.gap}
    if c.mode is not None:
        kw["mode"] = c.mode
    if c.views:
        assert len({(s.file, s.orientation) for s in c.slots}) == 1
        files = [RC.raw(c.slots[0].file, c.fast)]
        kw["views"] = [(0, s.window) for s in c.slots]
        turns = [c.slots[0].orientation]
    else:
        files = [RC.raw(s.file, c.fast) for s in c.slots]
        if any(s.window is not None for s in c.slots):
            kw["rois"] = [s.window for s in c.slots]
        turns = [s.orientation for s in c.slots]
    if any(o != 1 for o in turns):
        kw["orientation"] = turns
    return files, kw


def assert_plan_is_the_census(dec, c: RC.Case, filter: str = "bilinear"):
    """the plan these files make with these keywords reduces, output by output, with the factors, phases and reduced sizes the census
    names, and its launch is cut into the census's tiles and pieces"""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    files, kw = call_args(c)
    n = RC.census(c)
    prep = prepare_batch(files, dec.layout, 0)
    plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(files)}, filter=filter, **kw)
    try:
        shapes = [plan.reduce_shape(k) for k in range(len(c.slots))]
        cut = plan.reduce_launch()
    finally:
        plan.close()
    for k, s in enumerate(shapes):
        assert s["reduces"], (c.name, k, s)
        assert (s["fx"], s["fy"], s["phase_x"], s["phase_y"], s["width"], s["height"]) == n["slots"][k]["record"].shape, (c.name, k, s)
    assert cut == n["launch"], (c.name, cut, n["launch"])
    return n


def run(dec, c: RC.Case, layout: str, filters=("bilinear",), how: str = "decode"):
    assert RC.fast_of(layout) == c.fast
    files, kw = call_args(c)
    out = None
    for filter in filters:
        assert_plan_is_the_census(dec, c, filter)
        got = host(getattr(dec, how)(files, resample=filter, **kw))
        assert len(got) == len(c.slots)
        for k in range(len(c.slots)):
            exp = want(c, k, layout, filter)
            assert got[k].shape == exp.shape, (c.name, k, got[k].shape, exp.shape)
            assert np.array_equal(got[k], exp), (c.name, layout, k, filter, int((got[k] != exp).sum()), "bytes differ")
        out = got if out is None else out
    return out


def ids(t: dict, *rows):
    return [k for k in t if k.split("_")[0] in rows]


@pytest.mark.parametrize("layout", ("rowmajor", "xmajor"))
def test_pieces_two_tiles_under_a_phase_and_full_lanes(layout):
    """P1, P2, P3, T, PT and G of the table: bilinear throughout, bicubic once more on P1 and Lanczos once more on T (the second
    step is held elsewhere: the filters carry an error in the reduced image through to the output)"""
    from pyjpegdecoder_amd import BatchDecoder
    t = RC.table(RC.fast_of(layout))
    names = ids(t, "P1", "P2", "P3", "T", "PT", "G")
    assert len(names) == 8
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for name in names:
            extra = {"P1": ("bicubic",), ids(t, "T")[0]: ("lanczos",)}.get(name, ())
            run(dec, t[name], layout, ("bilinear",) + extra)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("planar_rowmajor", "planar"))
def test_p1_and_t_in_the_planar_layouts(layout):
    from pyjpegdecoder_amd import BatchDecoder
    t = RC.table(RC.fast_of(layout))
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for name in ids(t, "P1", "T"):
            run(dec, t[name], layout, how="decode_device")
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("rowmajor", "xmajor"))
def test_a_small_image_beside_one_of_two_tiles(layout):
    """B: the small image's workgroup for the second tile returns early — both slots of the one output tensor are the model's;
    upright, and with both long axes reversed (the large image's second tile then starts inside a phased grid)"""
    from pyjpegdecoder_amd import BatchDecoder
    t = RC.table(RC.fast_of(layout))
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for name in ids(t, "B"):
            got = run(dec, t[name], layout, how="decode_device")
            assert got.shape[0] == 2
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("rowmajor", "xmajor"))
def test_views_of_a_long_file_read_with_the_images_pitch(layout):
    """V: the whole file and two windows of it as views of ONE decode — rows staged in pieces at a pitch that is not the window's
    length, window origins at odd byte offsets —, upright and with the long axis reversed; held to the model, and to the call on
    the file repeated with rois= as tests/test_views.py does it"""
    from pyjpegdecoder_amd import BatchDecoder
    t = RC.table(RC.fast_of(layout))
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for name in ids(t, "V"):
            c = t[name]
            got = run(dec, c, layout)
            files, kw = call_args(c)
            views = kw.pop("views")
            o = kw.pop("orientation", None)
            again = dec.decode(files * len(views), rois=[w for _, w in views], orientation=o * len(views) if o else None, **kw)
            assert again.shape == got.shape and np.array_equal(again, got), name
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("rowmajor", "xmajor"))
def test_the_largest_cell_and_the_first_refused(layout):
    """C: 512 x 512 to 2 x 2 with gap 1.0 — cells of 65536 pixels, on a photograph and on an all-white image (the largest sum);
    to 1 x 2 the cells would hold 131072 pixels: refused by decode, by decode_device and by the plan's constructor"""
    from pyjpegdecoder_amd import BatchDecoder, UnsupportedJpeg
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    t = RC.table(RC.fast_of(layout))
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for name in ids(t, "C"):
            run(dec, t[name], layout)
        raw = RC.raw(RC.BIG)
        refusal = "takes cells of more than 65536 pixels"
        for call in (dec.decode, dec.decode_device):
            with pytest.raises((ValueError, UnsupportedJpeg), match=refusal):
                call([raw], size=(1, 2), reducing_gap=1.0)
        prep = prepare_batch([raw], dec.layout, 0)
        with pytest.raises((ValueError, UnsupportedJpeg), match=refusal):
            B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 1}, size=(1, 2), reducing_gap=1.0).close()
        # ... and the decoder goes on working
        run(dec, t["C"], layout)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("rowmajor", "xmajor"))
def test_sweep_of_windows_targets_and_gaps_every_orientation(layout):
    """One 1501 x 157 file (157 x 1501 for the x-major layout); per orientation 1..8 one call of twelve windows as rois=, a target
    and a gap drawn per call (reduce_cases.sweep) — factors from 1 to 40, at least four windows per call staged in pieces.  The
    host file holds what the draw reaches: all four kinds of cell, pieces, several tiles and early returns together in single
    plans."""
    from pyjpegdecoder_amd import BatchDecoder
    cases = RC.sweep(RC.fast_of(layout))
    dec = BatchDecoder(device=0, layout=layout)
    pairs = 0
    try:
        for c in cases:
            got = run(dec, c, layout)
            pairs += len(got)
    finally:
        dec.close()
    assert pairs == 8 * 12
