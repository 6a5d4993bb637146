"""Derived plans on the MI355X (mj_plan_derive, BatchDecoder.decode / decode_device / decode_device_iter(size=..., also=[...])): several
groups of outputs — each with its own size, views and everything behind the decode — from ONE decode.  The reference of every case is
the path that was there before: the call made with one group's arguments alone, which tests/test_views.py, test_resize.py,
test_place.py, test_orientation.py, test_mode.py, test_reduce.py, test_affine.py, test_perspective.py and test_colour.py hold to the
models on the oracle's pixels.  Byte for byte; one case is also held to the model (tools/views_model.py) directly."""
import numpy as np
import pytest

from conftest import load_golden
from test_resize import as_layout
from test_roi import LAYOUTS
from test_views import CASE1, COLOUR, GREY, MIRROR1, NODRI, PROG, differing, raw, same

pytestmark = pytest.mark.gpu

SIZE, SMALL, TINY = (24, 16), (12, 10), (7, 9)
RST = "128x64_420_pil_rst"
# (file, window) of the second group: other windows of the same four files, again interleaved
CASE2 = ((2, (5, 7, 33, 20)), (0, (64, 0, 7, 64)), (3, None), (1, (13, 21, 30, 30)), (0, (3, 5, 61, 40)), (3, (35, 10, 35, 40)), (1, None))
MIRROR2 = [True, False, False, True, False, True, True]
JUNK = b"not a jpeg"


def alone(dec, files, call, group, how="decode_device", **more):
    """the existing path: the call made with one group's arguments alone — an extra group's, as normalize_also completes them"""
    from pyjpegdecoder_amd.batch import ALSO_CALL_WIDE
    kw = {k: v for k, v in call.items() if k in ALSO_CALL_WIDE} if group is not call else {}
    kw.update(group)
    return getattr(dec, how)(files, **kw, **more)


def check(got, dec, files, call, also, **more):
    """every element of the result is the call with that group's arguments alone"""
    assert isinstance(got, tuple) and len(got) == 1 + len(also)
    for g, (element, group) in enumerate(zip(got, [call] + list(also))):
        want = alone(dec, files, call, group, **more)
        if isinstance(element, np.ndarray):
            want = want.cpu().numpy()
        assert not differing(element, want), (g, differing(element, want))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_three_groups_over_four_kinds_of_file(layout):
    from pyjpegdecoder_amd import BatchDecoder
    files = [raw(COLOUR), raw(GREY), raw(NODRI), raw(PROG), JUNK]       # (a file no group names is not looked at: this one is no JPEG)
    call = dict(size=SIZE, views=list(CASE1), mirror=MIRROR1, mode="RGB", resample="bicubic")
    also = [dict(size=SMALL, views=list(CASE2), mirror=MIRROR2), dict(size=TINY, views=[0, 1, 2, 3])]       # (whole images: bare file indices)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode_device(files, also=also, **call)
        assert [tuple(t.shape[:1]) for t in got] == [(len(CASE1),), (len(CASE2),), (4,)]
        check(got, dec, files, call, also)
        assert same(dec.decode_device(files, also=[], **call), got[0]) and same(dec.decode_device(files, also=None, **call), got[0])
        if layout == "rowmajor":
            # an extra group without views has one output per file: every file is then named
            whole = [dict(size=SMALL, views=list(CASE2), mirror=MIRROR2), dict(size=TINY, mirror=[True, False, False, True])]
            check(dec.decode_device(files[:4], also=whole, **call), dec, files[:4], call, whole)
            host = dec.decode(files, also=also, **call)
            assert all(isinstance(a, np.ndarray) for a in host)
            check(host, dec, files, call, also)
            # two batches, the second with other groups
            call2 = dict(call, views=[0, (0, (3, 5, 61, 40))], mirror=[True, False])
            also2 = [dict(size=TINY, views=[(0, (100, 30, 28, 34))])]
            per = dict(call)
            per.pop("views"), per.pop("mirror")
            one, two = list(dec.decode_device_iter([files, files[:1]], views=[call["views"], call2["views"]], mirror=[MIRROR1, call2["mirror"]],
                                                   also=[also, also2], **per))
            check(one, dec, files, call, also)
            check(two, dec, files[:1], call2, also2)
            with pytest.raises(ValueError, match="also yields fewer entries than there are batches"):
                list(dec.decode_device_iter([files[:1], files[:1]], also=[also2], size=SIZE))
    finally:
        dec.close()


def test_a_derived_group_is_the_models_crop_then_resize():
    """held to tools/views_model.py on the oracle's pixels directly, not through the other path"""
    from pyjpegdecoder_amd import BatchDecoder
    from tools import views_model
    pixels = np.ascontiguousarray(load_golden(COLOUR)[1]["rgb"].transpose(1, 0, 2))
    views = [(0, (3, 5, 61, 40)), 0, (0, (100, 30, 28, 34))]
    for layout in ("xmajor", "planar_rowmajor"):
        dec = BatchDecoder(device=0, layout=layout)
        try:
            big, small = dec.decode([raw(COLOUR)], size=SIZE, also=[dict(size=SMALL, resample="bicubic", views=views, mirror=[False, True, False])])
            assert np.array_equal(big[0], as_layout(views_model.expected(pixels, None, SIZE), layout)), layout
            for k, v in enumerate(views):
                want = views_model.expected(pixels, None if isinstance(v, int) else v[1], SMALL, "bicubic", mirror=k == 1)
                assert np.array_equal(small[k], as_layout(want, layout)), (layout, k)
        finally:
            dec.close()


@pytest.mark.parametrize("layout", ("rowmajor", "planar_rowmajor"))
def test_everything_behind_the_decode_in_extra_groups(layout):
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd.batch import rotation_matrix
    files = [raw(COLOUR), raw(NODRI)]
    call = dict(size=SIZE)                                              # (the primary has no transform, no chain, no place)
    also = [
        dict(size=SMALL, resample="bicubic", reducing_gap=2.0, mode="L", dtype=torch.float16, normalize=(0.45, 0.225)),
        dict(size=SMALL, resize_to=[(20, 6), (6, 14)], place=[(-3, 2), (4, -2)], fill=(114, 7, 200)),
        dict(size=TINY, color_ops=[[("contrast", 1.3), ("gaussian_blur", 1.5), ("adjust_hue", 0.1)], [("adjust_hue", -0.25), ("contrast", 0.6)]]),
        dict(size=SMALL, affine=[rotation_matrix(30.0, (128, 64)), None], affine_resample="bilinear", affine_fill=(9, 8, 7)),
        dict(size=TINY, perspective=[None, (0.9, 0.1, 2.0, -0.05, 1.1, 1.0, 0.001, 0.002)], affine_resample="bicubic"),
    ]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode_device(files, also=also, **call)
        assert got[1].dtype == torch.float16 and got[1].shape == (2, 10, 12)
        check(got, dec, files, call, also)
        # the call-wide keys are the call's where an entry is silent
        call = dict(size=SIZE, resample="lanczos", mode="L", dtype=torch.float32, normalize=(0.5, 0.25))
        also = [dict(size=SMALL), dict(size=TINY, mode="RGB", normalize=((0.4, 0.5, 0.6), (0.2, 0.3, 0.4)))]
        got = dec.decode_device(files, also=also, **call)
        assert got[1].dtype == torch.float32 and got[1].shape == (2, 10, 12) and got[2].shape[0] == 2 and got[2].numel() == 2 * 7 * 9 * 3
        check(got, dec, files, call, also)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("xmajor", "rowmajor"))
def test_three_orientation_classes_with_an_extra_group(layout):
    from pyjpegdecoder_amd import BatchDecoder
    files = [raw(COLOUR), raw(RST), raw(COLOUR), raw(NODRI)]
    # shown 128 x 64 as stored, 128 x 64 rotated by 180, 64 x 128 (orientation 6) and 48 x 64 (orientation 8)
    views = [(2, (5, 3, 40, 61)), (0, (3, 5, 61, 40)), (1, (100, 30, 28, 34)), (3, (2, 3, 40, 50)), (2, None), (3, (0, 0, 48, 7))]
    call = dict(size=SIZE, mirror=[False, True, True, False])
    also = [dict(size=SMALL, views=views, mirror=[True, False, False, True, False, True], resample="bicubic")]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode_device(files, orientation=[1, 3, 6, 8], also=also, **call)
        check(got, dec, files, call, also, orientation=[1, 3, 6, 8])
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("xmajor", "planar_rowmajor"))
def test_a_file_named_only_by_an_extra_group(layout):
    """the grey file's kind has no output in the call's own group: the extra group makes the plan that decodes it"""
    from pyjpegdecoder_amd import BatchDecoder
    files = [raw(COLOUR), JUNK, raw(GREY)]
    call = dict(size=SIZE, views=[(0, (3, 5, 61, 40)), 0], mode="RGB")
    also = [dict(size=SMALL, views=[(2, None), (0, (64, 0, 7, 64)), (2, (13, 21, 30, 30))], mirror=[False, True, True])]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        check(dec.decode_device(files, also=also, **call), dec, files, call, also)
        # ... and a file of the SAME kind that only the extra group names is a plan of its own, made by that group
        files = [raw(COLOUR), raw(RST)]
        also = [dict(size=SMALL, views=[(1, (100, 30, 28, 34)), (0, None), 1])]
        check(dec.decode_device(files, also=also, **call), dec, files, call, also)
    finally:
        dec.close()


VIEWS6 = [(0, (3, 5, 61, 40)), (0, None), (0, (100, 30, 28, 34))]
VIEWS6B = [(0, (64, 0, 7, 64)), (0, (17, 9, 30, 30)), (0, None), (0, (0, 0, 128, 8))]
MIRROR6B = [True, False, False, True]


def _plans(dec, ctx=None):
    """(prepared batch, plain plan, parent, derived) over the one colour file"""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    ctx = ctx or dec.ctx
    prep = prepare_batch([raw(COLOUR)], dec.layout, 0)
    keep = {"prep": prep, "n_images": 1}
    plain = B.Plan(ctx, prep.to_c(), keep)
    parent = B.Plan(ctx, prep.to_c(), keep, size=SIZE, views=VIEWS6)
    derived = parent.derive(prep, size=SMALL, views=VIEWS6B, output=("uint8", None, None, MIRROR6B))
    return prep, plain, parent, derived


def test_decoded_once_and_kept_for_as_long_as_a_derived_plan_lives():
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    dec = BatchDecoder(device=0, layout="rowmajor")
    try:
        want = dec.decode_device([raw(COLOUR)], size=SMALL, views=VIEWS6B, mirror=MIRROR6B).cpu().numpy()
        want_parent = dec.decode_device([raw(COLOUR)], size=SIZE, views=VIEWS6).cpu().numpy()
        before = dec.ctx.cache_stats()
        prep, plain, parent, derived = _plans(dec)
        try:
            # the parent is the plan it was; the derived plan decodes nothing and reports its own output
            assert (parent.info.total_blocks, parent.info.entropy_bytes) == (plain.info.total_blocks, plain.info.entropy_bytes)
            assert parent.info.total_blocks > 0 and parent.info.entropy_bytes > 0
            assert derived.info.total_blocks == 0 and derived.info.entropy_bytes == 0 and derived.info.total_mcus == 0
            assert derived.info.rgb_bytes == len(VIEWS6B) * SMALL[0] * SMALL[1] * 3 and derived.info.total_pixels == len(VIEWS6B) * SMALL[0] * SMALL[1]
            assert parent.info.rgb_bytes == len(VIEWS6) * SIZE[0] * SIZE[1] * 3
            plain.close()
            shape = (len(VIEWS6B),) + dec._shape(SMALL[0], SMALL[1], 3)
            parent.fill_source(0xAA)              # every derived view reads what THIS execute of the parent decoded
            parent.execute()
            derived.execute()
            derived.sync()
            out = derived.read()
            assert out["status"].size == 1 and not out["status"].any()
            got = out["rgb"].reshape(shape)
            assert not differing(got, want), differing(got, want)
            assert not differing(parent.read()["rgb"].reshape(want_parent.shape), want_parent)
            _, source_bytes = derived.time_resize(1)
            assert source_bytes == 128 * 64 * 3                                  # what it reads: the parent's decoded image
            # the derived plan reads the parent's buffer and decodes nothing: poison it, leave the parent alone, execute the derived
            parent.fill_source(0x55)
            derived.execute()
            derived.sync()
            assert (derived.read()["rgb"] == 0x55).all()
            # what only a decoding plan has is refused
            for call in (derived.execute_stage1, derived.execute_stage2, lambda: derived.fill_coef(0), lambda: derived.fill_source(0),
                         lambda: derived.write_coef(np.zeros(0, dtype=np.int16)), derived.time_stages, derived.tune_placement, derived.idct_levels):
                with pytest.raises(B.BackendError):
                    call()
            seam = np.zeros(64, dtype=np.int16)
            for at in (2, 3, 4):                  # mj_plan_read: its output and a status per image, and nothing else
                args = [None] * 5
                args[at - 1] = seam.ctypes.data
                assert dec.ctx.lib.mj_plan_read(derived.handle, *args) == B.MJ_ERR_INVALID
            with pytest.raises(B.BackendError, match="the parent is itself derived"):
                derived.derive(prep, size=TINY)
            # lifetime: the parent goes first; its buffers stay for the derived plan, which still computes the same bytes from them
            parent.execute()
            parent.sync()
            both = dec.ctx.cache_stats()
            parent.close()
            assert dec.ctx.cache_stats()[:2] == both[:2], "the parent's buffers went back while a derived plan holds them"
            derived.execute()
            derived.sync()
            assert not differing(derived.read()["rgb"].reshape(shape), want)
            derived.close()
            after = dec.ctx.cache_stats()
            assert after[:2] == before[:2], "a buffer is still handed out"
        finally:
            for p in (derived, parent, plain):
                p.close()
    finally:
        dec.close()


def _cache_counts(capfd, follow: bool):
    """(hits, misses) of a context's buffer cache — printed when it goes, with MJ_CACHE_STATS set — over a parent and a derived plan,
    closed parent first, and (follow) a plan of the parent's request after them"""
    import re
    from pyjpegdecoder_amd import _binding as B

    class Dec:
        layout = B.MJ_LAYOUT_ROWMAJOR
    ctx = B.Context(0)
    try:
        prep, plain, parent, derived = _plans(Dec, ctx)
        plain.close()
        parent.execute()
        derived.execute()
        parent.close()
        derived.sync()
        derived.close()
        if follow:
            again = B.Plan(ctx, prep.to_c(), {"prep": prep, "n_images": 1}, size=SIZE, views=VIEWS6)
            again.execute()
            again.sync()
            again.close()
    finally:
        capfd.readouterr()
        ctx.close()
    m = re.search(r"device buffer cache: (\d+) hits, (\d+) misses", capfd.readouterr().err)
    assert m, "the context did not report its cache"
    return int(m.group(1)), int(m.group(2))


def test_the_buffers_return_to_the_cache_for_the_next_plan(capfd, monkeypatch):
    monkeypatch.setenv("MJ_CACHE_STATS", "1")
    hits0, misses0 = _cache_counts(capfd, follow=False)
    hits1, misses1 = _cache_counts(capfd, follow=True)
    # the following plan's buffers — the parent's, back in the cache once both plans had gone — are all hits: nothing new is allocated
    assert misses1 == misses0 and hits1 > hits0


def test_refusals_of_the_entry_point():
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    dec = BatchDecoder(device=0, layout="rowmajor")
    try:
        prep = prepare_batch([raw(COLOUR)], dec.layout, 0)
        other = prepare_batch([raw(NODRI)], dec.layout, 0)
        two = prepare_batch([raw(COLOUR), raw(COLOUR)], dec.layout, 0)
        keep = {"prep": prep, "n_images": 1}
        before = dec.ctx.cache_stats()
        cases = [(dict(size=SIZE), prep, dict(), "needs a size"),
                 (dict(size=SIZE), prep, dict(size=SMALL, rois=[(0, 0, 4, 4)]), "rois: a derived plan's windows are views"),
                 (dict(size=SIZE), other, dict(size=SMALL), "not the one the parent was made from"),
                 (dict(size=SIZE), two, dict(size=SMALL), "not the one the parent was made from"),
                 (dict(), prep, dict(size=SMALL), "the parent has no size"),
                 (dict(orientation=[6]), prep, dict(size=SMALL), "the parent has no size"),
                 (dict(size=SIZE, rois=[(8, 8, 32, 32)]), prep, dict(size=SMALL), "the parent is a window plan"),
                 (dict(size=SIZE), prep, dict(size=SMALL, views=[(0, (100, 30, 29, 34))]), "view 0: window .* is empty or not inside"),
                 (dict(size=SIZE), prep, dict(size=SMALL, colour=[[(12, 1.0)]]), "colour_ops: output 0")]
        for parent_kw, batch, kw, message in cases:
            parent = B.Plan(dec.ctx, prep.to_c(), keep, **parent_kw)
            try:
                with pytest.raises(B.BackendError, match=message):
                    parent.derive(batch, **kw)
            finally:
                parent.close()
        assert dec.ctx.cache_stats()[:2] == before[:2], "a refused derive left a buffer handed out"
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("xmajor", "rowmajor"))
def test_a_file_the_marker_scan_hands_back_is_right_in_every_group(layout):
    from pyjpegdecoder_amd import BatchDecoder
    from routes_common import with_com
    clean = [raw(COLOUR), raw(RST), raw(COLOUR)]
    files = [clean[0], with_com(clean[1]), with_com(clean[2])]          # (MJ_ST_TAIL: bytes behind the scan; the second round is the host's)
    call = dict(size=SIZE, mirror=[False, True, False])
    also = [dict(size=SMALL, views=[(1, (100, 30, 28, 34)), (0, None), (2, (3, 5, 61, 40)), 1], mirror=[True, False, True, False])]
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        got = dec.decode_device(files, also=also, **call)
        check(got, dec, clean, call, also)
        one, = list(dec.decode_device_iter([files], also=[also], size=SIZE, mirror=[call["mirror"]]))      # (per batch: one list of flags)
        check(one, dec, clean, call, also)
        check(dec.decode(files, also=also, **call), dec, clean, call, also)
    finally:
        dec.close()


def test_a_large_call_in_two_parts():
    from pyjpegdecoder_amd import BatchDecoder
    # (one kind of file — 4:2:0 with restart markers —, so that each part is one plan of the batches in flight)
    files = [raw(n) for n in (COLOUR, RST, "100x36_420_dri7", COLOUR, RST, "100x36_420_dri7", COLOUR, RST)]
    views = [(7, (100, 30, 28, 34)), (0, None), (3, (3, 5, 61, 40)), (4, (1, 2, 50, 60)), (2, None), (6, (0, 0, 100, 36)), (5, (64, 0, 7, 36)), (1, None), (4, None)]
    call = dict(size=SIZE, mirror=[k % 3 == 0 for k in range(8)])
    also = [dict(size=SMALL, views=views, mirror=[k % 2 == 1 for k in range(len(views))], resample="bicubic")]
    dec = BatchDecoder(device=0, layout="rowmajor", segment="gpu", gpu_segment_min_files=1)
    try:
        got = dec.decode_device(files, parts=2, also=also, **call)
        check(got, dec, files, call, also)
    finally:
        dec.close()
