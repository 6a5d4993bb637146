"""Decode to a fixed size on the MI355X (mj_plan_request.out_width / out_height, BatchDecoder.decode / decode_device(size=...)): every output
is byte for byte tools/resize_model.py — which tests/test_resize_host.py pins to Pillow's resize(size, Image.BILINEAR) —
applied to the oracle's pixels of the image or window, in every layout, for shrinking, enlarging and unchanged axes."""
import numpy as np
import pytest

from conftest import GOLDEN, oracle_rgb_all
from test_roi import LAYOUTS, _fixture_files, mcu_size, window_kinds

pytestmark = pytest.mark.gpu

_cache = {}


def rowmajor_window(full: np.ndarray, win) -> np.ndarray:
    """The oracle's (W, H[, 3]) image, sliced to the window, seen row-major: (h, w[, 3])."""
    x, y, w, h = win
    return np.ascontiguousarray(full[x:x + w, y:y + h].swapaxes(0, 1))


def as_layout(img_rm: np.ndarray, layout: str) -> np.ndarray:
    """A row-major (oh, ow[, 3]) image laid out as a decoder of this layout returns one image."""
    s = img_rm
    if layout in ("xmajor", "planar"):
        s = s.swapaxes(0, 1)
    if layout.startswith("planar") and s.ndim == 3:
        s = np.moveaxis(s, -1, 0)
    return np.ascontiguousarray(s)


def expect(key, full, win, size, layout):
    """model(oracle window) in the decoder's layout (the model's result is kept per (file, window, size): four layouts share it)."""
    from tools import resize_model
    k = (key, tuple(win), tuple(size))
    if k not in _cache:
        _cache[k] = resize_model.resize(rowmajor_window(full, win), size)
    return as_layout(_cache[k], layout)


@pytest.fixture(scope="module")
def fixtures():
    from oracle import oracle
    files = _fixture_files()
    out = [(name, raw, oracle.decode(raw)["rgb"], mcu_size(raw)) for name, raw in files]
    # grouped by component count: one call fills one array
    return {nc: [f for f in out if (f[2].ndim == 3) == (nc == 3)] for nc in (1, 3)}


SIZES = {"shrink_both": (13, 9), "enlarge_both": (301, 257), "shrink_w_enlarge_h": (11, 263), "enlarge_w_shrink_h": (270, 7),
         "one_by_one": (1, 1)}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_fixture_every_size_whole_and_windows(fixtures, layout):
    """Every fixture file x sizes that shrink both axes, enlarge both, shrink one and enlarge the other, 1 x 1 — whole images
    and every kind of window of tests/test_roi.py."""
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for nc, group in fixtures.items():
            assert group
            raws = [f[1] for f in group]
            kinds = [window_kinds(f[2].shape[0], f[2].shape[1], *f[3]) for f in group]
            for sname, size in SIZES.items():
                for kind in [None] + list(kinds[0]):
                    wins = None if kind is None else [k[kind] for k in kinds]
                    got = dec.decode(raws, rois=wins, size=size)
                    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
                    assert got.shape == (len(group),) + dec._shape(size[0], size[1], nc), (sname, kind)
                    for i, (name, _, full, _) in enumerate(group):
                        win = (0, 0, full.shape[0], full.shape[1]) if wins is None else wins[i]
                        assert np.array_equal(got[i], expect(name, full, win, size, layout)), (name, sname, kind, win)
    finally:
        dec.close()


def unchanged_sizes(w: int, h: int):
    """Sizes that leave the width, the height or both of a w x h source as they are (the other axis enlarged or shrunk)."""
    return {"w_same_h_up": (w, 2 * h + 3), "w_same_h_down": (w, max(1, h // 3)), "h_same_w_up": (3 * w + 1, h),
            "h_same_w_down": (max(1, w // 2), h), "identity": (w, h)}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_unchanged_axes_and_identity_every_fixture_every_window_kind(fixtures, layout):
    """Width unchanged, height unchanged, both unchanged (the identity), for every fixture file — the 1920 x 1080 golden
    included — whole and through every kind of window.  An unchanged axis depends on the source's own size, so the files of one
    call are those whose sources (image or window) have one size."""
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    done = 0
    try:
        for nc, group in fixtures.items():
            kinds = [window_kinds(f[2].shape[0], f[2].shape[1], *f[3]) for f in group]
            for kind in [None] + list(kinds[0]):
                by_size = {}
                for i, (name, raw, full, _) in enumerate(group):
                    win = None if kind is None else kinds[i][kind]
                    w, h = (full.shape[0], full.shape[1]) if win is None else (win[2], win[3])
                    by_size.setdefault((w, h), []).append((name, raw, full, win))
                for (w, h), members in by_size.items():
                    for sname, size in unchanged_sizes(w, h).items():
                        got = dec.decode([m[1] for m in members], rois=None if kind is None else [m[3] for m in members], size=size)
                        assert got.shape == (len(members),) + dec._shape(size[0], size[1], nc), (kind, sname, w, h)
                        for k, (name, _, full, win) in enumerate(members):
                            win = win or (0, 0, full.shape[0], full.shape[1])
                            assert np.array_equal(got[k], expect(name, full, win, size, layout)), (name, kind, win, sname)
                            if sname == "identity":            # ... which is the plain decode
                                assert np.array_equal(got[k], as_layout(rowmajor_window(full, win), layout)), (name, kind, win)
                            done += 1
        assert done == sum(len(g) for g in fixtures.values()) * 11 * 5
    finally:
        dec.close()


def test_pillow_itself_on_the_oracles_pixels(fixtures):
    """Pillow applied to the oracle's pixels, not the model: whole images and windows, to several sizes, through decode_device."""
    Image = pytest.importorskip("PIL.Image")
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout="rowmajor")
    try:
        for nc, group in fixtures.items():
            raws = [f[1] for f in group]
            kinds = [window_kinds(f[2].shape[0], f[2].shape[1], *f[3]) for f in group]
            for size in ((224, 224), (17, 40), (90, 31)):
                for kind in (None, "inner", "last_mcu"):
                    wins = None if kind is None else [k[kind] for k in kinds]
                    got = dec.decode_device(raws, rois=wins, size=size).cpu().numpy()
                    for i, (name, _, full, _) in enumerate(group):
                        win = (0, 0, full.shape[0], full.shape[1]) if wins is None else wins[i]
                        want = np.asarray(Image.fromarray(rowmajor_window(full, win)).resize(size, Image.BILINEAR))
                        assert np.array_equal(got[i], want), (name, size, kind)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
@pytest.mark.parametrize("segment", ["host", "gpu"])
def test_mixed_kinds_into_one_tensor_in_input_order(segment, layout):
    """Different image sizes, sampling layouts, baseline and progressive, with and without restart markers, one call: one tensor,
    every slot its file's expectation."""
    import torch
    from oracle import oracle
    from pyjpegdecoder_amd import BatchDecoder
    from tools import synth
    g = np.load(GOLDEN / "odd_layouts.npz")
    odd = sorted(k for k in g.files if k.endswith(".jpg"))[0]
    files = [synth.synth_jpeg(41, 200, 120, 85, "420", 13), synth.synth_jpeg(44, 96, 64, 85, "444", 0),
             synth.synth_jpeg(42, 333, 77, 85, "420", 0), (GOLDEN / "files" / "prog_70x50_420_pil.jpg").read_bytes(),
             g[odd].tobytes(), synth.synth_jpeg(43, 200, 120, 85, "420", 7), (GOLDEN / "files" / "64x48_422_pil.jpg").read_bytes(),
             synth.synth_jpeg(45, 640, 480, 90, "422", 40), synth.synth_jpeg(46, 1920, 1080, 85, "420", 120)]
    fulls = [oracle.decode(r)["rgb"] for r in files]
    wins = [(37, 21, 90, 50), None, (150, 10, 5, 3), (10, 9, 33, 21), None, None, (17, 3, 40, 40), None, (736, 316, 448, 448)]
    size = (224, 224)
    for min_files in (64, 1):                    # a handful of files on the host-parsed route, or the native front end + GPU scan
        dec = BatchDecoder(device=0, layout=layout, segment=segment, gpu_segment_min_files=min_files)
        shape = dec._shape(224, 224, 3)
        try:
            for rois in (None, wins):
                got = dec.decode_device(files, rois=rois, size=size)
                assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and got.is_cuda
                assert tuple(got.shape) == (len(files),) + shape
                host = got.cpu().numpy()
                arr = dec.decode(files, rois=rois, size=size)
                for i, full in enumerate(fulls):
                    win = (rois[i] if rois is not None else None) or (0, 0, full.shape[0], full.shape[1])
                    want = expect(("mixed", i), full, win, size, layout)
                    assert np.array_equal(host[i], want), (segment, min_files, i)
                    assert np.array_equal(arr[i], want), (segment, min_files, i)
            per_batch = list(dec.decode_device_iter([files[:4], files[4:]], size=size))
            assert [tuple(t.shape) for t in per_batch] == [(4,) + shape, (5,) + shape]
            both = torch.cat(per_batch).cpu().numpy()
            for i, full in enumerate(fulls):
                assert np.array_equal(both[i], expect(("mixed", i), full, (0, 0, full.shape[0], full.shape[1]), size, layout)), i
        finally:
            dec.close()


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
@pytest.mark.parametrize("windows", [False, True], ids=["whole", "centred_448"])
def test_at_size_1024_x_1080p_to_224(windows, layout):
    """1 024 x 1080p 4:2:0 (256 distinct files, one restart interval per MCU row) to 224 x 224 on decode_device's default route,
    whole images and centred 448 x 448 windows, x-major and as the NCHW batch (planar_rowmajor): every distinct image held to model(oracle), every copy to its first instance."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from tools import synth
    W, H, n, distinct = 1920, 1080, 1024, 256
    blob, offs = synth.synth_batch(distinct, 8800, W, H, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(distinct)]
    files = [raws[(5 * i + i // distinct) % distinct] for i in range(n)]
    win = ((W - 448) // 2, (H - 448) // 2, 448, 448) if windows else None
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode_device(files, rois=win, size=(224, 224))
        assert tuple(got.shape) == (n,) + dec._shape(224, 224, 3)
        first = {}
        for i in range(n):
            first.setdefault((5 * i + i // distinct) % distinct, i)
        for i in range(n):
            d = (5 * i + i // distinct) % distinct
            if first[d] != i:
                assert torch.equal(got[i], got[first[d]]), i
        host = got.cpu().numpy()
    finally:
        dec.close()
    for d, full in enumerate(oracle_rgb_all(raws)):
        want = expect(("at_size", d), full, win or (0, 0, W, H), (224, 224), layout)
        assert np.array_equal(host[first[d]], want), d


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("segment", ["host", "gpu"])
def test_sentinels_slots_and_a_poisoned_intermediate(layout, segment):
    """Bytes behind the output array and the slots a plan does not name are untouched, and what the intermediate buffer held
    before the execute does not show in the result (stage 2 writes every byte the resize reads)."""
    import torch
    from oracle import oracle
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth
    files = [synth.synth_jpeg(31 + k, 200, 120, 85, "420", ri) for k, ri in enumerate((13, 7, 0))]
    wins = [(37, 21, 90, 50), (101, 40, 60, 3), (3, 5, 7, 100)]
    fulls = [oracle.decode(r)["rgb"] for r in files]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for size in ((24, 40), (130, 9)):
            per = size[0] * size[1] * 3
            n_slots = 5
            for rois in (wins, None):
                buf = torch.full((n_slots * per + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                slot_of = {0: 3, 1: 0, 2: 4}                  # slots 1 and 2 belong to no plan
                for group in ([0, 1], [2]):                   # (files with and without restart markers are separate plans)
                    sub = [files[i] for i in group]
                    parsed = [parse_jpeg(f, headers_only=True) for f in sub] if segment == "gpu" else None
                    prep = prepare_batch(sub, dec.layout, 0, parsed)
                    plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(sub)},
                                  rois=[rois[i] for i in group] if rois else None, size=size,
                                  slots=([slot_of[i] for i in group], n_slots))
                    try:
                        assert plan.info.rgb_bytes == n_slots * per
                        plan.fill_coef(0x5B)
                        plan.fill_source(0xC3)
                        plan.execute(0, buf.data_ptr())
                        plan.sync()
                        assert not plan.read(rgb=False)["status"].any()
                    finally:
                        plan.close()
                host = buf.cpu().numpy()
                assert (host[n_slots * per:] == 0xA5).all(), "bytes written behind the output"
                for s in (1, 2):
                    assert (host[s * per:(s + 1) * per] == 0xA5).all(), "a slot of no plan was written"
                for i, s in slot_of.items():
                    win = rois[i] if rois else (0, 0, 200, 120)
                    want = expect(("sentinel", i), fulls[i], win, size, layout)
                    assert np.array_equal(host[s * per:(s + 1) * per].reshape(want.shape), want), (i, layout, segment, size)
    finally:
        dec.close()


def test_resized_plans_refuse_what_they_cannot_do():
    import ctypes
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth
    files = [synth.synth_jpeg(51, 200, 120, 85, "420", 13), synth.synth_jpeg(52, 200, 120, 85, "420", 13)]
    dec = BatchDecoder(device=0)
    try:
        L = dec.ctx.lib
        prep = prepare_batch(files)
        bc = prep.to_c()
        h = ctypes.c_void_p()
        from routes_common import create_with
        for ow, oh in ((0, 5), (5, 0), (-1, 5), (70000, 5)):
            assert create_with(L, dec.ctx.handle, bc, h, out_width=ow, out_height=oh) == B.MJ_ERR_INVALID
            assert b"output size" in L.mj_last_error(dec.ctx.handle)
        for bad in ([0, 2], [-1, 0]):
            sl = np.asarray(bad, dtype=np.int32)
            assert create_with(L, dec.ctx.handle, bc, h, out_width=8, out_height=8, slots=sl, n_slots=2) == B.MJ_ERR_INVALID
            assert b"slot" in L.mj_last_error(dec.ctx.handle)
        for flag in (B.MJ_FLAG_KEEP_PLANES, B.MJ_FLAG_KEEP_IDCT):
            bc2 = prepare_batch(files, flags=flag).to_c()
            assert create_with(L, dec.ctx.handle, bc2, h, out_width=8, out_height=8) == B.MJ_ERR_INVALID
        rois = (B.RoiC * 2)(B.RoiC(0, 0, 5, 5), B.RoiC(190, 0, 11, 5))
        assert create_with(L, dec.ctx.handle, bc, h, rois=rois, out_width=8, out_height=8) == B.MJ_ERR_INVALID
        assert b"image 1" in L.mj_last_error(dec.ctx.handle)
        plain = B.Plan(dec.ctx, bc, {"prep": prep, "n_images": 2})
        try:
            assert L.mj_plan_fill_source(plain.handle, 1) == B.MJ_ERR_INVALID
        finally:
            plain.close()
        grey = (GOLDEN / "files" / "50x70_grey_dri4.jpg").read_bytes()
        for bad in ((0, 5), (5,), 224, (2.0, 3)):
            for call in (dec.decode, dec.decode_device):
                with pytest.raises(ValueError, match="size"):
                    call(files, size=bad)
            with pytest.raises(ValueError, match="size"):
                next(dec.decode_device_iter([files], size=bad))
        with pytest.raises(ValueError, match="return_seams"):
            dec.decode(files, size=(8, 8), return_seams=True)
        for call in (dec.decode, dec.decode_device):
            with pytest.raises(ValueError, match="file 2"):
                call(files + [grey], size=(8, 8))
            with pytest.raises(ValueError, match="file 1"):          # windows are still checked against the files' headers
                call(files, rois=[None, (190, 0, 11, 5)], size=(8, 8))
        # no files: an empty batch of the colour shape, from every entry point
        assert dec.decode([], size=(8, 6)).shape == (0, 8, 6, 3)
        assert tuple(dec.decode_device([], size=(8, 6)).shape) == (0, 8, 6, 3)
        outs = list(dec.decode_device_iter([[], files], size=(8, 6)))
        assert [tuple(t.shape) for t in outs] == [(0, 8, 6, 3), (2, 8, 6, 3)]
    finally:
        dec.close()
