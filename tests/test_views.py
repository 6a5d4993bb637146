"""Views on the MI355X (mj_plan_request.views, BatchDecoder.decode / decode_device / decode_device_iter(size=..., views=...)): several
sized crops per file from one decode.  The reference of every case is the path that was there before: the call on the files
REPEATED, one per view, with rois= — which tests/test_resize.py, test_place.py, test_orientation.py, test_mode.py and test_reduce.py
hold to Pillow's arithmetic on the oracle's pixels.  Byte for byte, in every layout; one case is also held to the model
(tools/views_model.py, which tests/test_views_host.py holds to Pillow) directly."""
import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from test_resize import as_layout
from test_roi import LAYOUTS

pytestmark = pytest.mark.gpu

SIZE = (24, 16)
COLOUR, GREY, NODRI, PROG = "128x64_420_dri3", "50x70_grey_dri4", "64x48_422_pil", "prog_70x50_420_pil"
# (file, window): interleaved across the files, so that every plan's views land in slots that are not its own run
CASE1 = ((0, None), (1, (0, 0, 50, 70)), (2, (0, 0, 64, 48)), (3, (2, 3, 60, 40)), (0, (3, 5, 61, 40)), (1, (13, 21, 30, 30)),
         (0, (100, 30, 28, 34)), (2, (5, 7, 33, 20)), (0, (64, 0, 7, 64)), (3, (35, 10, 35, 40)), (0, (17, 9, 1, 1)))
MIRROR1 = [False, True, False, True, True, False, False, True, True, False, True]


def raw(name):
    return (GOLDEN / "files" / f"{name}.jpg").read_bytes()


def repeated(dec, files, views, how="decode_device", **kw):
    """the existing path: every view's file listed once per view, its window as rois=; per-file lists follow the files"""
    idx = [v if isinstance(v, int) else v[0] for v in views]
    if isinstance(kw.get("orientation"), list):
        kw["orientation"] = [kw["orientation"][i] for i in idx]
    return getattr(dec, how)([files[i] for i in idx], rois=[None if isinstance(v, int) else v[1] for v in views], **kw)


def same(got, want):
    import torch
    if isinstance(got, np.ndarray):
        return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))


def differing(got, want):
    return [k for k in range(len(want))] if got.shape != want.shape else [k for k in range(len(want)) if not same(got[k], want[k])]


@pytest.mark.parametrize("filter", ("bilinear", "bicubic"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_views_of_four_kinds_of_file_are_the_repeated_files_call(layout, filter):
    from pyjpegdecoder_amd import BatchDecoder
    files = [raw(COLOUR), raw(GREY), raw(NODRI), raw(PROG)]
    kw = dict(size=SIZE, resample=filter, mode="RGB", mirror=MIRROR1)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        want = repeated(dec, files, CASE1, **kw)
        # (a file no view names is not looked at: this one is no JPEG at all)
        got = dec.decode_device(files + [b"not a jpeg"], views=list(CASE1), **kw)
        assert got.shape[0] == len(CASE1) and not differing(got, want), differing(got, want)
        if layout == "rowmajor":
            host = dec.decode(files + [b"not a jpeg"], views=list(CASE1), **kw)
            assert same(host, want.cpu().numpy())
            kw.pop("mirror")
            (one, two) = list(dec.decode_device_iter([files, files[:1]], views=[list(CASE1), [0, (0, (3, 5, 61, 40))]], mirror=[MIRROR1, [True, False]], **kw))
            assert not differing(one, want)
            assert not differing(two, repeated(dec, files[:1], [0, (0, (3, 5, 61, 40))], mirror=[True, False], **kw))
    finally:
        dec.close()


def test_a_view_is_the_models_crop_then_resize():
    """held to tools/views_model.py on the oracle's pixels directly, not through the other path"""
    from pyjpegdecoder_amd import BatchDecoder
    from tools import views_model
    pixels = np.ascontiguousarray(load_golden(COLOUR)[1]["rgb"].transpose(1, 0, 2))
    views = [(0, (3, 5, 61, 40)), 0, (0, (100, 30, 28, 34))]
    for layout in ("xmajor", "planar_rowmajor"):
        dec = BatchDecoder(device=0, layout=layout)
        try:
            got = dec.decode([raw(COLOUR)], size=SIZE, resample="bicubic", views=views, mirror=[False, True, False])
            for k, v in enumerate(views):
                want = views_model.expected(pixels, None if isinstance(v, int) else v[1], SIZE, "bicubic", mirror=k == 1)
                assert np.array_equal(got[k], as_layout(want, layout)), (layout, k)
        finally:
            dec.close()


def test_model_ready_views():
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    files = [raw(COLOUR), raw(NODRI)]
    views = [(0, (3, 5, 61, 40)), (1, None), 0, (1, (5, 7, 33, 20)), (0, (64, 0, 7, 64))]
    kw = dict(size=SIZE, dtype=torch.float16, normalize=((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), mirror=[True, False, False, True, False])
    dec = BatchDecoder(device=0, layout="planar_rowmajor")
    try:
        want = repeated(dec, files, views, **kw)
        got = dec.decode_device(files, views=views, **kw)
        assert got.dtype == torch.float16 and got.shape == (5, 3, 16, 24) and not differing(got, want), differing(got, want)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_views_of_turned_files_are_windows_of_the_oriented_images(layout):
    from pyjpegdecoder_amd import BatchDecoder
    files = [raw(COLOUR), raw("128x64_420_pil_rst")]
    # file 0 is shown 64 x 128 (orientation 6: the transposing class), file 1 128 x 64 rotated by 180 (the flipping class)
    views = [(0, (5, 3, 40, 61)), (1, (3, 5, 61, 40)), 0, (1, (100, 30, 28, 34)), (0, (30, 100, 34, 28)), 1, (0, (0, 64, 64, 7))]
    kw = dict(size=SIZE, orientation=[6, 3], mirror=[False, False, True, True, False, False, True], resample="bicubic")
    dec = BatchDecoder(device=0, layout=layout)
    try:
        want = repeated(dec, files, views, **kw)
        got = dec.decode_device(files, views=views, **kw)
        assert not differing(got, want), differing(got, want)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_view_has_its_own_place(layout):
    from pyjpegdecoder_amd import BatchDecoder
    files = [raw(COLOUR)]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        # one view cropped by its place, one padded
        views = [0, (0, (3, 5, 61, 40))]
        kw = dict(size=SIZE, resize_to=[(48, 24), (12, 8)], place=[(-10, -4), (5, 3)], fill=(114, 114, 114), mirror=[False, True])
        want = repeated(dec, files, views, **kw)
        got = dec.decode_device(files, views=views, **kw)
        assert not differing(got, want), differing(got, want)
        # TenCrop: the shorter side to 32 (64 x 32), the four corners and the centre of a 24 x 24 canvas, each also mirrored
        five = [(0, 0), (-40, 0), (0, -8), (-40, -8), (-20, -4)]
        kw = dict(size=(24, 24), resize_to=32, place=five + five, mirror=[False] * 5 + [True] * 5)
        want = repeated(dec, files, [0] * 10, **kw)
        got = dec.decode_device(files, views=[0] * 10, **kw)
        assert got.shape[0] == 10 and not differing(got, want), differing(got, want)
        assert differing(got[:5], got[5:]) == list(range(5))         # (the mirrored crops are other bytes)
    finally:
        dec.close()


def _plan(dec, raws, **kw):
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    prep = prepare_batch(raws, dec.layout, 0)
    return B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(raws)}, **kw)


GAP_VIEWS = [(0, None), (0, (1, 1, 125, 63)), (0, (3, 5, 61, 40))]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_step_views_reduce_their_own_windows(layout):
    from pyjpegdecoder_amd import BatchDecoder
    files = [raw(COLOUR)]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        # every view its own factors, from its window: 2 x 2; 2 x 1 with a partial last cell and an origin off the image's grid; 1 x 1
        plan = _plan(dec, files, size=SIZE, reducing_gap=2.0, views=GAP_VIEWS)
        try:
            shapes = [plan.reduce_shape(k) for k in range(3)]
        finally:
            plan.close()
        assert [(s["fx"], s["fy"], s["width"], s["height"], s["reduces"]) for s in shapes] == [(2, 2, 64, 32, True), (2, 1, 63, 63, True), (1, 1, 61, 40, True)]
        for extra in ({}, {"mode": "L"}, {"orientation": [6]}):
            views = GAP_VIEWS if "orientation" not in extra else [(0, None), (0, (1, 1, 63, 125)), (0, (5, 3, 40, 61))]
            kw = dict(size=SIZE, reducing_gap=2.0, mirror=[False, True, False], **extra)
            want = repeated(dec, files, views, **kw)
            got = dec.decode_device(files, views=views, **kw)
            assert not differing(got, want), (extra, differing(got, want))
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("xmajor", "rowmajor"))
def test_a_file_is_decoded_once(layout):
    from pyjpegdecoder_amd import BatchDecoder
    files = [raw(COLOUR)]
    views = [v for v in CASE1 if v[0] == 0]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        plain = _plan(dec, files)
        plan = _plan(dec, files, size=SIZE, views=views)
        try:
            assert (plan.info.total_blocks, plan.info.entropy_bytes) == (plain.info.total_blocks, plain.info.entropy_bytes)
            assert plan.info.rgb_bytes == len(views) * SIZE[0] * SIZE[1] * 3 and plan.info.total_pixels == len(views) * SIZE[0] * SIZE[1]
            a, b = plan.shape(), plain.shape()
            assert a[:2] == b[:2] and a[20:28] == b[20:28] and a[3] == b[3]      # the stage-1 form, the fused words, the restart segments
            plan.fill_source(0xAA)              # every view reads what THIS execute decoded
            plan.execute()
            plan.sync()
            out = plan.read()
            assert not out["status"].any() and out["status"].size == 1        # status stays per image
            got = out["rgb"].reshape((len(views),) + dec._shape(SIZE[0], SIZE[1], 3))
            _, source_bytes = plan.time_resize(1)
            assert source_bytes == 128 * 64 * 3                                # what was decoded: the image, once
        finally:
            plan.close()
            plain.close()
        want = repeated(dec, files, views, size=SIZE).cpu().numpy()
        assert not differing(got, want), differing(got, want)
    finally:
        dec.close()
