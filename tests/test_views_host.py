"""Views on the host (no GPU): batch.normalize_views and the routing that drops the files no view names, the request's checks and
its default rule through mj_debug_normalise_request, the layout of mj_view, of the request and of the structure that encloses it
for a request with views (C against ctypes),
and tools/views_model.py — the statement of what a view is — against Pillow's crop().resize()."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


# ---- batch.normalize_views ----------------------------------------------------------------------------------------------------
DIMS = [(128, 64), (50, 70)]


def test_normalize_views_forms():
    from pyjpegdecoder_amd.batch import normalize_views
    assert normalize_views(None, DIMS, None) is None
    got = normalize_views([1, (0, None), (0, (3, 5, 61, 40)), (1, [13, 21, 30, 30]), np.int64(0)], DIMS, (24, 16))
    assert got == [(1, (0, 0, 50, 70)), (0, (0, 0, 128, 64)), (0, (3, 5, 61, 40)), (1, (13, 21, 30, 30)), (0, (0, 0, 128, 64))]
    # a file whose header has not been read: the first pass leaves its windows as given
    assert normalize_views([(1, (1, 2, 3, 4)), 0, (1, None)], [(128, 64), None], (8, 8)) == [(1, (1, 2, 3, 4)), (0, (0, 0, 128, 64)), (1, None)]
    assert normalize_views([], DIMS, (8, 8)) == []


def test_normalize_views_refusals():
    from pyjpegdecoder_amd.batch import normalize_views
    with pytest.raises(ValueError, match=r"views needs size=\(width, height\)"):
        normalize_views([0], DIMS, None)
    with pytest.raises(ValueError, match="views and rois do not go together"):
        normalize_views([0], DIMS, (8, 8), rois=[(0, 0, 4, 4)] * 2)
    with pytest.raises(ValueError, match="views and return_seams do not go together"):
        normalize_views([0], DIMS, (8, 8), return_seams=True)
    with pytest.raises(ValueError, match="views must be None or a list"):
        normalize_views(3, DIMS, (8, 8))
    for bad in ((0, 1), (0, (1, 2, 3)), "0", (0, None, None), (0.0, None), (True, None), (0, (1, 2, 3, 4.0))):
        with pytest.raises(ValueError, match="view 1: .* is none of"):
            normalize_views([0, bad], DIMS, (8, 8))
    with pytest.raises(ValueError, match="view 0: file 2 is not one of the 2 files"):
        normalize_views([2], DIMS, (8, 8))
    with pytest.raises(ValueError, match="view 0: file -1 is not one of the 2 files"):
        normalize_views([(-1, None)], DIMS, (8, 8))
    for bad in ((0, 0, 0, 4), (0, 0, 4, 0), (-1, 0, 4, 4), (0, -1, 4, 4), (48, 0, 3, 4), (0, 67, 4, 4)):
        with pytest.raises(ValueError, match=r"view 1 \(file 7\): window \(x=.*\) is empty or not inside the 50x70 image"):
            normalize_views([0, (1, bad)], DIMS, (8, 8), index=[5, 7])


def test_per_view_lists_have_one_entry_per_view():
    from pyjpegdecoder_amd.batch import normalize_output, normalize_places, normalize_views
    views = normalize_views([0, (0, (3, 5, 61, 40)), 1], DIMS, (24, 16))
    vdims = [r[2:] for _, r in views]
    assert normalize_output(None, None, [True, False, True], (24, 16), len(views), 3).mirror == [True, False, True]
    with pytest.raises(ValueError, match="mirror has 2 entries for 3"):
        normalize_output(None, None, [True, False], (24, 16), len(views), 3)
    places = normalize_places([32, (24, 16), "contain"], [(0, 0), None, None], (24, 16), vdims, [0, 0, 1])
    assert len(places) == 3 and places[0] == (64, 32, 0, 0) and places[1] == (24, 16, 0, 0)
    with pytest.raises(ValueError, match="resize_to has 2 entries for 3"):
        normalize_places([32, 32], None, (24, 16), vdims)
    with pytest.raises(ValueError, match="place has 2 entries for 3"):
        normalize_places(32, [(0, 0), None], (24, 16), vdims)
    # the binding: places and the mirror flags per view, orientations per image
    from pyjpegdecoder_amd import _binding as B
    r, keep = B.plan_request(2, size=(24, 16), views=views, places=places, orientation=[1, 6], output=("uint8", None, None, [1, 0, 1]))
    assert r.n_views == 3 and (r.views[1].image, r.views[1].window.x, r.views[1].window.width) == (0, 3, 61)
    with pytest.raises(ValueError, match="places: 2 entries, not one for each of the 3 views"):
        B.plan_request(2, size=(24, 16), views=views, places=places[:2])
    with pytest.raises(ValueError, match="mirror: 2 entries, not one for each of the 3 views"):
        B.plan_request(2, size=(24, 16), views=views, output=("uint8", None, None, [1, 0]))
    with pytest.raises(ValueError, match="orientation: 3 entries, not one for each of the 2 images"):
        B.plan_request(2, size=(24, 16), views=views, orientation=[1, 1, 1])
    with pytest.raises(ValueError, match="views needs size"):
        B.plan_request(2, views=views)


# ---- files no view names are not looked at ---------------------------------------------------------------------------------------
def _up_to_planning(files, views, size=(24, 16), orientation=None):
    """what decode / decode_device do with views before any plan is made: which files are read, their headers, the views against
    them, the files sorted by kind"""
    from pyjpegdecoder_amd import batch
    index, entries = batch.select_view_files(files, views, size)
    orientation = batch._per_file_of(orientation, len(files), index, "orientation")
    kept = [files[i] for i in index]
    info = [batch._named(index, i, batch._image_info, f) for i, f in enumerate(kept)]
    orient = batch.normalize_orientation(orientation, kept)
    vs = batch.normalize_views(entries, batch._oriented_dims([t[:2] for t in info], orient), size, index=index)
    groups = batch._group_by_kind(kept, range(len(kept)), {}, False, index=index)
    return index, vs, groups


def test_a_bad_file_counts_only_when_a_view_names_it():
    from pyjpegdecoder_amd.errors import JpegError
    good = (GOLDEN / "files" / "128x64_420_dri3.jpg").read_bytes()
    grey = (GOLDEN / "files" / "50x70_grey_dri4.jpg").read_bytes()
    garbage = b"\xff\xd8" + b"not a jpeg at all" * 4
    lossless = good.replace(b"\xff\xc0", b"\xff\xc3", 1)             # SOF3: a frame type the decoder does not take
    for bad, exc in ((garbage, JpegError), (lossless, JpegError)):
        files = [good, bad, grey, good]
        index, vs, groups = _up_to_planning(files, [(3, (3, 5, 61, 40)), 0, (2, None), (0, (1, 1, 4, 4))], orientation=[1, 1, 6, 1])
        assert index == [0, 2, 3]
        assert vs == [(2, (3, 5, 61, 40)), (0, (0, 0, 128, 64)), (1, (0, 0, 70, 50)), (0, (1, 1, 4, 4))]      # file 2 is turned: 70 x 50
        assert sorted(sum(groups, [])) == [0, 1, 2] and len(groups) == 2
        with pytest.raises(exc, match="file 1: "):
            _up_to_planning(files, [0, (1, None)])
    # a per-file list still has one entry per file of the CALLER's list
    with pytest.raises(ValueError, match="orientation has 2 entries for 4 files"):
        _up_to_planning([good, garbage, grey, good], [0], orientation=[1, 1])


def test_narrow_takes_a_files_views_with_it():
    from pyjpegdecoder_amd.batch import OutputSpec, _Request
    req = _Request([b"a", b"b", b"c"], None, (8, 8), OutputSpec("uint8", mirror=[True, False, False, True, True]), None, [0, 1, 2, 3, 4], [4, 6, 9],
                   [1, 6, 1], places=[(8, 8, 0, 0), (9, 9, 1, 1), (8, 8, 2, 2), (8, 8, 3, 3), (8, 8, 4, 4)],
                   views=[(2, (0, 0, 1, 1)), (0, (0, 0, 2, 2)), (1, (0, 0, 3, 3)), (2, (0, 0, 4, 4)), (0, (0, 0, 5, 5))])
    sub = req.narrow([2, 0])
    assert sub.files == [b"c", b"a"] and sub.index == [9, 4] and sub.orient is None
    assert sub.views == [(0, (0, 0, 1, 1)), (1, (0, 0, 2, 2)), (0, (0, 0, 4, 4)), (1, (0, 0, 5, 5))]
    assert sub.slots == [0, 1, 3, 4] and sub.output.mirror == [True, False, True, True]
    assert sub.places == [(8, 8, 0, 0), (9, 9, 1, 1), (8, 8, 3, 3), (8, 8, 4, 4)] and sub.n_outputs == 4
    one = req.narrow([1])
    assert one.views == [(0, (0, 0, 3, 3))] and one.slots == [2] and one.orient == [6] and one.output.mirror == [False]
    kw = one.plan_kwargs(3)
    assert kw["views"] == one.views and kw["rois"] is None and kw["slots"] is None      # (no tensor to name slots of)


# ---- the request: mj_debug_normalise_request ---------------------------------------------------------------------------------
def _batch(sizes):
    from pyjpegdecoder_amd import _binding as B
    images = (B.ImageDescC * len(sizes))()
    for d, (w, h) in zip(images, sizes):
        d.width, d.height, d.ncomp = w, h, 3
    b = B.BatchC()
    b.n_images = len(sizes)
    b.images = ctypes.cast(images, ctypes.POINTER(B.ImageDescC))
    return b, images


def _normal(lib, batch, **kw):
    from pyjpegdecoder_amd import _binding as B
    size = kw.pop("size", (24, 16))
    r, keep = B.plan_request(batch.n_images, size=(24, 16), **kw)
    if size is None:
        r.out_width = r.out_height = 0
    out = B.PlanRequestC()
    rc = lib.mj_debug_normalise_request(ctypes.byref(batch), ctypes.byref(r), ctypes.byref(out))
    return rc, out, lib.mj_last_error(None).decode()


def test_request_identity_views_come_back_absent(lib):
    from pyjpegdecoder_amd import _binding as B
    batch, keep = _batch([(128, 64), (50, 70)])
    for views in ([(0, None), (1, None)], [(0, (0, 0, 128, 64)), (1, None)]):
        rc, out, msg = _normal(lib, batch, views=views)
        assert rc == B.MJ_OK and out.n_views == 0 and out.n_slots == 2, msg
    rc, out, _ = _normal(lib, batch, views=[(0, None), (1, (0, 0, 70, 50))], orientation=[1, 6])     # whole, as the orientation shows it
    assert rc == B.MJ_OK and out.n_views == 0 and not out.views
    # the count switches views on: an array that comes with n_views == 0 is not looked at — the request is the plain one —,
    # from C and from plan_request(views=[])
    rc, plain_out, _ = _normal(lib, batch)
    r, keep_r = B.plan_request(2, size=(24, 16), views=[(1, None), (0, (1, 1, 4, 4))])
    r.n_views = 0
    for req in (r, B.plan_request(2, size=(24, 16), views=[])[0]):
        assert bool(req.views) and req.n_views == 0
        out = B.PlanRequestC()
        assert lib.mj_debug_normalise_request(ctypes.byref(batch), ctypes.byref(req), ctypes.byref(out)) == B.MJ_OK
        assert not out.views and out.n_views == 0 and out.n_slots == 2 and bytes(out) == bytes(plain_out)
    # anything else stays: another order, a window, a file twice — and n_slots defaults to the views
    for views in ([(1, None), (0, None)], [(0, None), (1, (0, 0, 50, 69))], [(0, None), (1, None), (0, None)]):
        rc, out, msg = _normal(lib, batch, views=views)
        assert rc == B.MJ_OK and out.n_views == len(views) and out.n_slots == len(views), msg
    rc, out, _ = _normal(lib, batch, views=[(0, None), (1, None), (0, None)], slots=([5, 1, 0], 7))
    assert rc == B.MJ_OK and out.n_slots == 7
    # the first step's default rule looks at the views' windows and the views' places
    rc, out, _ = _normal(lib, batch, views=[(0, None), (1, None), (0, (3, 5, 61, 40))], reducing_gap=2.0)
    assert rc == B.MJ_OK and out.reducing_gap == 2.0                   # 128 / 24 / 2 = 2.67
    rc, out, _ = _normal(lib, batch, views=[(0, (3, 5, 61, 40)), (1, (0, 5, 50, 60)), (0, (0, 0, 90, 60))], reducing_gap=2.0)
    assert rc == B.MJ_OK and out.reducing_gap == 0.0 and out.n_views == 3     # 90 / 24 / 2 and 60 / 16 / 2 stay below 2


def test_request_refusals(lib):
    from pyjpegdecoder_amd import _binding as B
    batch, keep = _batch([(128, 64), (50, 70)])
    both = [(0, None), (1, (1, 1, 4, 4))]
    rc, _, msg = _normal(lib, batch, views=both, size=None)
    assert rc == B.MJ_ERR_INVALID and "views needs a size" in msg
    rc, _, msg = _normal(lib, batch, views=both, rois=[(0, 0, 4, 4), (0, 0, 4, 4)])
    assert rc == B.MJ_ERR_INVALID and "views and rois do not go together" in msg
    rc, _, msg = _normal(lib, batch, views=[(0, None), (2, None), (1, None)])
    assert rc == B.MJ_ERR_INVALID and "view 1: image 2 outside the 2 images of the batch" in msg
    rc, _, msg = _normal(lib, batch, views=[(0, None), (-1, None), (1, None)])
    assert rc == B.MJ_ERR_INVALID and "view 1: image -1 outside" in msg
    for bad in ((0, 0, 0, 4), (0, 0, 4, -1), (-1, 0, 4, 4), (48, 0, 3, 4), (0, 67, 4, 4), (0, 0, 70, 50)):
        rc, _, msg = _normal(lib, batch, views=[(0, None), (0, (1, 1, 4, 4)), (1, bad)])
        assert rc == B.MJ_ERR_INVALID and "view 2: window" in msg and "is empty or not inside the oriented image" in msg, (bad, msg)
    rc, _, msg = _normal(lib, batch, views=[(0, None), (1, (0, 0, 70, 50))], orientation=[1, 1])
    assert rc == B.MJ_ERR_INVALID and "view 1: window" in msg
    rc, _, msg = _normal(lib, batch, views=[(1, None), (1, (1, 1, 4, 4))])
    assert rc == B.MJ_ERR_INVALID and "image 0: no view names it" in msg
    rc, _, msg = _normal(lib, batch, views=both, slots=([0, 2], 2))
    assert rc == B.MJ_ERR_INVALID and "view 1: slot 2 outside the 2 slots" in msg
    r, keep_r = B.plan_request(2, size=(24, 16), views=both)
    r.n_views = -1
    out = B.PlanRequestC()
    assert lib.mj_debug_normalise_request(ctypes.byref(batch), ctypes.byref(r), ctypes.byref(out)) == B.MJ_ERR_INVALID
    assert "n_views = -1" in lib.mj_last_error(None).decode()
    r.n_views = 2
    r.views = None                                           # (the count without the array)
    assert lib.mj_debug_normalise_request(ctypes.byref(batch), ctypes.byref(r), ctypes.byref(out)) == B.MJ_ERR_INVALID
    assert "n_views = 2" in lib.mj_last_error(None).decode()


# ---- the struct ----------------------------------------------------------------------------------------------------------------
def test_mj_view_and_the_request_with_views_are_laid_out_as_the_binding_assumes(lib, tmp_path):
    from pyjpegdecoder_amd import _binding as B
    gcc = shutil.which("gcc")
    assert gcc is not None, "the header is held to a C compiler"
    flags = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include")]
    vfields = [f for f, _ in B.ViewC._fields_]
    assert vfields == ["image", "window"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(
        ['#include <stdio.h>', '#include <stddef.h>', '#include "mijpeg.h"', 'int main(void) {', '  mj_plan_request zeroed = {0};',
         '  printf("%zu", sizeof(mj_view));'] +
        [f'  printf(" %zu", offsetof(mj_view, {f}));' for f in vfields] +
        ['  printf(" %d\\n", zeroed.views == 0 && zeroed.n_views == 0);', '  return 0;', '}']))
    exe = tmp_path / "layout"
    subprocess.run([gcc] + flags + [str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(B.ViewC)] + [getattr(B.ViewC, f).offset for f in vfields] + [1]
    assert ctypes.sizeof(B.ViewC) == 20
    # (the request's own layout, views and n_views included: test_plan_request_host)
    r = B.PlanRequestC()
    r.n_views = 7
    assert r.n_views == 7 and r.n_slots == 0 and not r.output and not r.slots and not r.views
    header = (ROOT / "include" / "mijpeg.h").read_text()
    assert "int32_t n_views;" in header and "const mj_view *views;" in header


# ---- the model against Pillow ----------------------------------------------------------------------------------------------------
WINDOWS = ((3, 5, 61, 40), (1, 1, 125, 63), None)


@pytest.mark.parametrize("filter", ("bilinear", "bicubic"))
def test_model_is_pillows_crop_then_resize(filter):
    Image = pytest.importorskip("PIL.Image")
    from tools import views_model
    _, vec = load_golden("128x64_420_dri3")                      # the oracle's decode, (W, H, 3)
    pixels = np.ascontiguousarray(vec["rgb"].transpose(1, 0, 2))
    img = Image.fromarray(pixels)
    for window in WINDOWS:
        for gap in (None, 2.0):
            for orientation, mode, mirror in ((1, None, False), (6, None, True), (3, "L", False)):
                w = window
                if w is not None and orientation == 6:
                    w = (w[1], w[0], w[3], w[2])                 # (a window of the turned, 64 x 128 image)
                kw = dict(filter=filter, orientation=orientation, mode=mode, reducing_gap=gap, mirror=mirror)
                want = views_model.pillow_expression(img, w, (24, 16), **kw)
                got = views_model.expected(pixels, w, (24, 16), **kw)
                assert np.array_equal(got, want), (window, gap, orientation, mode)
    # the factors come from the window, not from the image: this window reduces by 2 x 1, the whole image by 2 x 2
    from tools import reduce_model
    assert reduce_model.reduce_factors(125, 63, 24, 16, 2.0) == (2, 1) and reduce_model.reduce_factors(128, 64, 24, 16, 2.0) == (2, 2)
    assert reduce_model.reduce_factors(61, 40, 24, 16, 2.0) == (1, 1)


def test_equivalent_calls_restate_a_view_as_a_call_on_one_file():
    from tools import views_model
    calls = views_model.equivalent_calls([b"a", b"b"], [(1, (1, 2, 3, 4)), 0, (1, None)], size=(24, 16), mirror=[True, False, True],
                                         orientation=[1, 6], resize_to=[32, "contain", (9, 9)], place=None, resample="bicubic")
    assert [c[0] for c in calls] == [[b"b"], [b"a"], [b"b"]]
    assert calls[0][1] == dict(size=(24, 16), mirror=[True], orientation=[6], resize_to=[32], place=None, resample="bicubic", rois=[(1, 2, 3, 4)])
    assert calls[1][1]["rois"] is None and calls[1][1]["orientation"] == [1] and calls[1][1]["resize_to"] == ["contain"]
    assert calls[2][1]["mirror"] == [True] and calls[2][1]["resize_to"] == [(9, 9)]
