"""The paths of k_affine (csrc/affine.hip) that tests/test_affine.py does not reach, on the MI355X: NEAREST by index tables with
offsets, origins and runs of -1; the bicubic clamp below 0 and above 255 in three components and in one; every orientation through
StoredFetch under every filter and all four <CS, CO> instantiations; plans whose windows differ strongly in size, more than two
tiles along the contiguous axis, and the word-or-bytes split at a row's end for every remainder.  The cases are
tests/affine_cases.py's, which tests/test_affine_paths_host.py holds — on the CPU — to what they are meant to reach and to the
wrong variants they must tell apart.

The expected bytes are tools/affine_model.expected on the library's own plain decode of the file, as in tests/test_affine.py.
Unless a test is about the steps behind the launch, the call's size is the windows' common size under the default bilinear
resize, which is the identity there (asserted on the CPU in the host file): the output is the affine buffer itself, byte for byte,
so one wrong pixel of the launch is one wrong pixel of the output.

Left out: the idle tail of the grid beyond kResizeGridX = 1 << 20 workgroups, which needs over a million tiles in one plan.
Nothing here looks at generated code."""
import numpy as np
import pytest

import affine_cases as AC
from test_resize import as_layout
from test_roi import LAYOUTS

pytestmark = pytest.mark.gpu

_PLAIN, _BUFFERS = {}, {}


def plain(name):
    """the library's own plain decode of the file, row-major, in the file's components: computed once, never changed"""
    if name not in _PLAIN:
        from pyjpegdecoder_amd import BatchDecoder
        dec = BatchDecoder(device=0, layout="rowmajor")
        try:
            (img,) = dec.decode([AC.raw(name)])
        finally:
            dec.close()
        img = img[:, :, 0] if img.ndim == 3 and img.shape[2] == 1 else img
        img.setflags(write=False)
        _PLAIN[name] = img
    return _PLAIN[name]


def host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def want(c: AC.Case, layout: str, size=None, filter="bilinear") -> np.ndarray:
    """affine_model.expected for case c (for the 512 x 512 file the model transforms the case's window only: the same bytes by the
    model's own statement of a window, without half a second per view)"""
    from tools import affine_model, views_model
    size = tuple(size or c.size)
    if c.file != AC.BIG:
        rm = affine_model.expected(plain(c.file), c.a, c.window, size, resample=c.resample, affine_fill=c.fill, filter=filter,
                                   orientation=c.orientation, mode=c.mode)
    else:
        key = (c.file, c.a, c.resample, c.window, c.orientation, c.mode)
        if key not in _BUFFERS:
            _BUFFERS[key] = AC.buffer(c, plain(c.file))
        rm = views_model.expected(_BUFFERS[key], None, size, filter)
    return as_layout(rm, layout)


def run(dec, cases, size=None, **kw):
    """ONE call — so one plan per kind of file and orientation class — whose outputs are the cases, as views of the files they name"""
    files, views = [], []
    for c in cases:
        key = (c.file, c.orientation)
        if key not in [(f, o) for f, o, _ in files]:
            files.append((c.file, c.orientation, AC.raw(c.file)))
        views.append(([(f, o) for f, o, _ in files].index(key), c.window))
    first = cases[0]
    assert all((c.resample, c.mode, c.fill) == (first.resample, first.mode, first.fill) for c in cases)
    return host(dec.decode_device([r for _, _, r in files], views=views, size=tuple(size or first.size), affine=[c.a for c in cases],
                                  affine_resample=first.resample, affine_fill=first.fill, mode=first.mode,
                                  orientation=[o for _, o, _ in files] if any(o != 1 for _, o, _ in files) else None, **kw))


def check(got, cases, layout, size=None, filter="bilinear"):
    assert len(got) == len(cases)
    for k, c in enumerate(cases):
        exp = want(c, layout, size, filter)
        assert got[k].shape == exp.shape, (c.name, got[k].shape, exp.shape)
        assert np.array_equal(got[k], exp), (c.name, layout, int((got[k] != exp).sum()), "bytes differ")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_nearest_by_tables_with_offsets_origins_and_runs_outside(layout):
    """ten views of one file in one plan: scale matrices (index tables, kind 1) on windows that hang over the tables' leading and
    trailing -1 runs, the flip, the sub-pixel shift, two rotations (fixed point, kind 2) and an untransformed view — then the same
    call with the outputs in reversed order, where every view gets other table offsets"""
    from pyjpegdecoder_amd import BatchDecoder
    cases = AC.table_cases()
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = run(dec, cases)
        check(got, cases, layout)
        back = run(dec, cases[::-1])
        check(back, cases[::-1], layout)
        assert np.array_equal(back[::-1], got)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bicubic_clamps_below_0_and_above_255(layout):
    """the RGB noise files and the checker fixtures — as colour, as "L", as grey and as grey to RGB — with the window the image and
    with a corner window; every case is a call of its own size"""
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for c in AC.clamp_cases():
            check(run(dec, [c]), [c], layout)
    finally:
        dec.close()


@pytest.mark.parametrize("resample", AC.FILTERS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_orientation_under_every_filter(layout, resample):
    """eight copies of a file with orientation 1..8 — one plan per orientation class in one call —, a window off the origin of
    each oriented image and a matrix per output; each file in its own components and in the other mode: k_affine<3, 3>, <3, 1>,
    <1, 1> and <1, 3>"""
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for file in (AC.ODD, AC.GREY):
            for mode in (None, AC.other_mode(file)):
                cases = AC.orientation_cases(file, resample, mode)
                check(run(dec, cases), cases, layout)
    finally:
        dec.close()


@pytest.mark.parametrize("resample", ("bilinear", "bicubic"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_edge_of_the_image_under_every_orientation(layout, resample):
    """every output the WHOLE oriented image, rotated so that the source's frame crosses it on all four sides, at its own size —
    the taps clipped at ix == -1, ix + 1 >= w, iy == -1 and iy + 1 >= h are bytes of the result; orientations 1..4 in one call,
    5..8 (the other shape) in another, a colour and a grey file"""
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for file in (AC.ODD, AC.GREY):
            for cases in AC.edge_cases(file, resample):
                check(run(dec, cases), cases, layout)
    finally:
        dec.close()


@pytest.mark.parametrize("resample", ("bilinear", "bicubic"))
@pytest.mark.parametrize("layout", ("rowmajor", "xmajor", "planar_rowmajor"))
def test_windows_of_one_pixel_one_tile_and_256_tiles_in_one_plan(layout, resample):
    """the whole 512 x 512 image (8 x 32 tiles), a 1 x 1 window, one tile, a pixel more than a tile along each axis and a 300 x 20
    window in one plan: most workgroups of the smaller windows return early.  Resized to 48 x 32 behind the launch."""
    from pyjpegdecoder_amd import BatchDecoder
    cases = AC.tile_cases(resample, layout)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        check(run(dec, cases, size=AC.TILE_SIZE), cases, layout, size=AC.TILE_SIZE)
    finally:
        dec.close()


@pytest.mark.parametrize("mode", (None, "L"))
@pytest.mark.parametrize("layout", ("rowmajor", "xmajor", "planar_rowmajor"))
def test_row_tails_of_every_remainder(layout, mode):
    """windows of 64 + r pixels along the contiguous axis, r = 1..4, three per call at different origins, in three components and
    in one: the last tile of a row holds r * CO bytes — every remainder modulo 4 of the word-or-bytes split — and rows start at
    every alignment"""
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for r in (1, 2, 3, 4):
            cases = AC.row_tail_cases(r, layout, mode)
            check(run(dec, cases), cases, layout)
    finally:
        dec.close()
