"""Region-of-interest decode on the MI355X (mj_plan_request.rois, BatchDecoder.decode / decode_device(rois=...)): every window
equals the oracle's whole image, sliced, in every layout; only the restart segments the windows need are decoded; nothing
outside the windows is read or written."""
import ctypes

import numpy as np
import pytest

from conftest import GOLDEN, oracle_rgb_all

pytestmark = pytest.mark.gpu

LAYOUTS = ("xmajor", "rowmajor", "planar", "planar_rowmajor")


def expect(full: np.ndarray, win, layout: str) -> np.ndarray:
    """The oracle's (W, H[, 3]) image, sliced to the window and laid out as the decoder returns it."""
    x, y, w, h = win
    s = full[x:x + w, y:y + h]
    if layout in ("rowmajor", "planar_rowmajor"):
        s = s.swapaxes(0, 1)
    if layout.startswith("planar") and s.ndim == 3:
        s = np.moveaxis(s, -1, 0)
    return np.ascontiguousarray(s)


def mcu_size(raw: bytes):
    from pyjpegdecoder_amd._parse import parse_jpeg
    p = parse_jpeg(raw)
    comps = list(p.color_components.values())
    if len(comps) == 1:
        return 8, 8
    return 8 * max(c.horizontal_sampling for c in comps), 8 * max(c.vertical_sampling for c in comps)


def window_kinds(W: int, H: int, mw: int, mh: int):
    """The windows every file is decoded through: whole image, 1x1 corners, MCU-aligned, inside MCUs, one row, one column,
    ending in the last (partial) MCU."""
    ax, ay = (mw if W > mw else 0), (mh if H > mh else 0)
    ix, iy = min(3, W - 1), min(5, H - 1)
    lw, lh = min(W, 11), min(H, 13)
    return {
        "full": (0, 0, W, H),
        "corner_tl": (0, 0, 1, 1), "corner_tr": (W - 1, 0, 1, 1), "corner_bl": (0, H - 1, 1, 1), "corner_br": (W - 1, H - 1, 1, 1),
        "aligned": (ax, ay, min(mw, W - ax), min(mh, H - ay)),
        "inner": (ix, iy, max(1, min(W - ix - 1, mw + 7)), max(1, min(H - iy - 1, mh + 5))),
        "row": (0, H // 2, W, 1),
        "column": (W // 2, 0, 1, H),
        "last_mcu": (W - lw, H - lh, lw, lh),
    }


def _fixture_files():
    """Every golden file, the odd sampling layouts and the crafted progressive scripts: (name, raw)."""
    out = [(f.stem, f.read_bytes()) for f in sorted((GOLDEN / "files").glob("*.jpg"))]
    g = np.load(GOLDEN / "odd_layouts.npz")
    out += [("odd_" + k[:-4], g[k].tobytes()) for k in sorted(g.files) if k.endswith(".jpg")]
    gp = np.load(GOLDEN / "crafted_progressive.npz")
    out += [("cprog_" + k[:-4], gp[k].tobytes()) for k in sorted(gp.files) if k.endswith(".jpg")]
    return out


@pytest.fixture(scope="module")
def fixtures():
    from oracle import oracle
    files = _fixture_files()
    return [(name, raw, oracle.decode(raw)["rgb"], mcu_size(raw)) for name, raw in files]


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact_only"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_fixture_through_every_window_kind(fixtures, layout, exact):
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout, exact_only=exact)
    try:
        raws = [f[1] for f in fixtures]
        kinds = [window_kinds(f[2].shape[0], f[2].shape[1], *f[3]) for f in fixtures]
        for kind in kinds[0]:
            wins = [k[kind] for k in kinds]
            got = dec.decode(raws, rois=wins)
            for (name, _, full, _), win, img in zip(fixtures, wins, got):
                want = expect(full, win, layout)
                assert img.shape == want.shape, (name, kind, win)
                assert np.array_equal(img, want), (name, kind, win)
    finally:
        dec.close()


# ---- restart intervals, both segmentations, segments that span rows --------------------------------------------------------
W2, H2 = 200, 120          # 4:2:0: 13 x 8 MCUs of 16 x 16


def _needed_segments(ri: int, mch: int, mcv: int, win, mw: int, mh: int):
    """Which restart segments hold an MCU of the window (raster order, enumerated MCU by MCU)."""
    x, y, w, h = win
    mcus = mch * mcv
    n = -(-mcus // ri) if ri else 1
    rect = lambda m: x // mw <= m % mch <= (x + w - 1) // mw and y // mh <= m // mch <= (y + h - 1) // mh
    return [s for s in range(n) if any(rect(m) for m in range(s * ri if ri else 0, min((s + 1) * ri, mcus) if ri else mcus))]


def _interval_files():
    from tools import craft_jpeg, synth
    files = {ri: [synth.synth_jpeg(11 + ri, W2, H2, 85, "420", ri), synth.synth_jpeg(23 + ri, W2, H2, 85, "420", ri)]
             for ri in (1, 7, 13, 26, 0)}
    files["422_ri7"] = [craft_jpeg.craft_baseline(W2, H2, [(2, 1), (1, 1), (1, 1)], seed=3, restart_interval=7)] * 2
    return files


INTERVAL_WINDOWS = [(37, 21, 90, 50), (150, 100, 5, 3), (0, 0, W2, H2), (101, 40, 60, 1)]


@pytest.mark.parametrize("segment", ["host", "gpu"])
def test_restart_intervals_and_both_segmentations(segment):
    from oracle import oracle
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, segment=segment, gpu_segment_min_files=1)
    try:
        for key, files in _interval_files().items():
            fulls = [oracle.decode(r)["rgb"] for r in files]
            for win in INTERVAL_WINDOWS:
                got = dec.decode(files, rois=win)
                for full, img in zip(fulls, got):
                    assert np.array_equal(img, expect(full, win, "xmajor")), (key, win)
                gd = dec.decode_device(files, rois=[win, None])
                assert np.array_equal(gd[0].cpu().numpy(), expect(fulls[0], win, "xmajor")), (key, win)
                assert np.array_equal(gd[1].cpu().numpy(), fulls[1]), key
    finally:
        dec.close()


def test_host_segmented_plans_decode_only_the_needed_segments():
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    dec = BatchDecoder(device=0)
    try:
        for key, files in _interval_files().items():
            mw = 16
            mh = 8 if key == "422_ri7" else 16
            ri = 7 if key == "422_ri7" else key
            mch, mcv = -(-W2 // mw), -(-H2 // mh)
            for win in INTERVAL_WINDOWS:
                prep = prepare_batch(files)
                assert not (prep.flags & B.MJ_FLAG_GPU_SEGMENT)
                plain = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(files)})
                roi = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(files)}, rois=[win] * len(files))
                try:
                    need = _needed_segments(ri, mch, mcv, win, mw, mh)
                    lens = prep.seg_end - prep.seg_begin
                    per = len(lens) // len(files)
                    want = sum(int(lens[i * per + s]) for i in range(len(files)) for s in need)
                    assert roi.info.entropy_bytes == want, (key, win)
                    assert plain.info.entropy_bytes == int(lens.sum())
                    if len(need) < per:
                        assert roi.info.entropy_bytes < plain.info.entropy_bytes
                    assert roi.info.rgb_bytes == len(files) * win[2] * win[3] * 3
                    assert roi.info.total_pixels == len(files) * win[2] * win[3]
                    assert roi.image_offsets(1)[1] == win[2] * win[3] * 3
                finally:
                    plain.close()
                    roi.close()
    finally:
        dec.close()


# ---- skipping is real ------------------------------------------------------------------------------------------------------
def _corrupt_segment(raw: bytes, seg: int) -> bytes:
    """Restart segment `seg` of the file's scan with 32 bytes of 0xFF 0x00 (all ones after destuffing: no Huffman code)
    written into its middle; markers and length stay."""
    from pyjpegdecoder_amd._parse import parse_jpeg
    so = parse_jpeg(raw).scans[0].segment_offsets
    b, e = int(so[seg]), int(so[seg + 1]) - 2
    assert e - b > 48
    pos = b + (e - b) // 2 - 16
    while raw[pos - 1] == 0xFF:
        pos += 1
    bad = bytearray(raw)
    bad[pos:pos + 32] = b"\xFF\x00" * 16
    return bytes(bad)


@pytest.mark.parametrize("segment", ["host", "gpu"])
def test_a_damaged_segment_outside_the_window_is_not_decoded(segment):
    from oracle import oracle
    from pyjpegdecoder_amd import BatchDecoder, CorruptedJpeg
    from tools import synth
    clean = synth.synth_jpeg(7, W2, H2, 85, "420", 13)           # DRI = one MCU row
    bad = _corrupt_segment(clean, 1)                              # MCU row 1: pixel rows 16..31
    with pytest.raises(RuntimeError):
        oracle.decode(bad)
    full = oracle.decode(clean)["rgb"]
    win = (20, 70, 100, 40)                                       # MCU rows 4..6
    dec = BatchDecoder(device=0, segment=segment, gpu_segment_min_files=1)
    try:
        with pytest.raises(CorruptedJpeg):
            dec.decode([bad])
        (img,) = dec.decode([bad], rois=[win])
        assert np.array_equal(img, expect(full, win, "xmajor"))
        (dv,) = dec.decode_device([bad], rois=win)
        assert np.array_equal(dv.cpu().numpy(), expect(full, win, "xmajor"))
        with pytest.raises(CorruptedJpeg):
            dec.decode([bad], rois=[(0, 16, 8, 1)])               # a window in the damaged row
    finally:
        dec.close()


# ---- nothing outside the windows is read or written -----------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("segment", ["host", "gpu"])
def test_poisoned_coefficients_and_sentinel_tail(layout, segment):
    import torch
    from oracle import oracle
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth
    files = [synth.synth_jpeg(31 + k, W2, H2, 85, "420", ri) for k, ri in enumerate((13, 7, 0))]
    wins = [(37, 21, 90, 50), (101, 40, 60, 3), (3, 5, 7, 100)]
    fulls = [oracle.decode(r)["rgb"] for r in files]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for group in ([0, 1], [2]):          # (files with and without restart markers are separate plans)
            sub = [files[i] for i in group]
            parsed = [parse_jpeg(f, headers_only=True) for f in sub] if segment == "gpu" else None
            prep = prepare_batch(sub, dec.layout, 0, parsed)
            plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(sub)}, rois=[wins[i] for i in group])
            try:
                assert not (plan.stage1_form() & B.MJ_FORM_FUSED)
                n = plan.info.rgb_bytes
                buf = torch.full((n + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                plan.fill_coef(0x5B)
                plan.execute(0, buf.data_ptr())
                plan.sync()
                st = plan.read(rgb=False)["status"]
                assert not st.any()
                host = buf.cpu().numpy()
                assert (host[n:] == 0xA5).all(), "bytes written behind the windows"
                off = 0
                for i in group:
                    want = expect(fulls[i], wins[i], layout)
                    got = host[off:off + want.size].reshape(want.shape)
                    assert np.array_equal(got, want), (i, layout, segment)
                    off += want.size
                assert off == n
            finally:
                plan.close()
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["xmajor", "rowmajor"])
@pytest.mark.parametrize("segment", ["host", "gpu"])
def test_full_frame_windows_equal_the_plain_plan(layout, segment):
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth
    blob, offs = synth.synth_batch(8, 515, 1920, 1080, 85, "420", 120)
    files = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(8)]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        parsed = [parse_jpeg(f, headers_only=True) for f in files] if segment == "gpu" else None
        prep = prepare_batch(files, dec.layout, 0, parsed)
        plain = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 8})
        roi = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 8}, rois=[(0, 0, 1920, 1080)] * 8)
        try:
            assert not (roi.stage1_form() & B.MJ_FORM_FUSED)
            assert roi.info.rgb_bytes == plain.info.rgb_bytes
            assert roi.info.entropy_bytes == plain.info.entropy_bytes
            for p in (plain, roi):
                p.execute()
                p.sync()
            a, b = plain.read(), roi.read()
            assert not a["status"].any() and not b["status"].any()
            assert np.array_equal(a["rgb"], b["rgb"])
        finally:
            plain.close()
            roi.close()
    finally:
        dec.close()


def test_mixed_kinds_with_per_file_windows_in_input_order():
    from oracle import oracle
    from pyjpegdecoder_amd import BatchDecoder
    from tools import synth
    g = np.load(GOLDEN / "odd_layouts.npz")
    odd = sorted(k for k in g.files if k.endswith(".jpg"))[0]
    files = [synth.synth_jpeg(41, W2, H2, 85, "420", 13), (GOLDEN / "files" / "50x70_grey_dri4.jpg").read_bytes(),
             synth.synth_jpeg(42, W2, H2, 85, "420", 0), (GOLDEN / "files" / "prog_70x50_420_pil.jpg").read_bytes(),
             g[odd].tobytes(), synth.synth_jpeg(43, W2, H2, 85, "420", 7), (GOLDEN / "files" / "64x48_422_pil.jpg").read_bytes()]
    fulls = [oracle.decode(r)["rgb"] for r in files]
    wins = [(37, 21, 90, 50), None, (150, 100, 5, 3), (10, 9, 33, 21), (1, 2, 3, 4), None, (17, 3, 40, 40)]
    for min_files in (8, 1):                     # host segmentation for a handful of files, or the GPU scan + native front end
        dec = BatchDecoder(device=0, gpu_segment_min_files=min_files)
        try:
            got = dec.decode(files, rois=wins)
            gotd = dec.decode_device(files, rois=wins)
            for i, full in enumerate(fulls):
                win = wins[i] or (0, 0, full.shape[0], full.shape[1])
                want = expect(full, win, "xmajor")
                assert np.array_equal(got[i], want), (min_files, i)
                assert np.array_equal(gotd[i].cpu().numpy(), want), (min_files, i)
        finally:
            dec.close()


def test_at_size_centred_224_windows_on_the_default_route():
    """1024 distinct 1080p files, DRI = one MCU row, centred 224 x 224 windows: decode_device's default route (native front end,
    GPU segmentation, parts).  Every image against the oracle, sliced."""
    from pyjpegdecoder_amd import BatchDecoder
    from tools import synth
    n, W, H = 1024, 1920, 1080
    blob, offs = synth.synth_batch(n, 9000, W, H, 85, "420", 120)
    files = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
    win = ((W - 224) // 2, (H - 224) // 2, 224, 224)
    dec = BatchDecoder(device=0)
    try:
        got = dec.decode_device(files, rois=win)
        host = [t.cpu().numpy() for t in got]
    finally:
        dec.close()
    for i, full in enumerate(oracle_rgb_all(files)):
        assert np.array_equal(host[i], expect(full, win, "xmajor")), i


def test_invalid_windows_and_seam_flags_are_rejected():
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth
    files = [synth.synth_jpeg(51, W2, H2, 85, "420", 13), synth.synth_jpeg(52, W2, H2, 85, "420", 13)]
    dec = BatchDecoder(device=0)
    try:
        for bad in [(0, 0, 0, 5), (190, 0, 11, 5), (0, 115, 5, 6), (-1, 0, 5, 5)]:
            with pytest.raises(ValueError, match="file 1"):
                dec.decode(files, rois=[None, bad])
            with pytest.raises(ValueError, match="file 1"):
                dec.decode_device(files, rois=[None, bad])
        with pytest.raises(ValueError):
            dec.decode(files, rois=(0, 0, 5, 5), return_seams=True)
        L = dec.ctx.lib
        prep = prepare_batch(files)
        bc = prep.to_c()
        h = ctypes.c_void_p()
        from routes_common import create_with
        for bad in [(0, 0, 0, 5), (190, 0, 11, 5), (0, 115, 5, 6), (-1, 0, 5, 5)]:
            rois = (B.RoiC * 2)(B.RoiC(0, 0, 5, 5), B.RoiC(*bad))
            assert create_with(L, dec.ctx.handle, bc, h, rois=rois) == B.MJ_ERR_INVALID
            assert b"image 1" in L.mj_last_error(dec.ctx.handle)
        rois = (B.RoiC * 2)(B.RoiC(0, 0, 5, 5), B.RoiC(0, 0, 5, 5))
        for flag in (B.MJ_FLAG_KEEP_COEF, B.MJ_FLAG_KEEP_PLANES, B.MJ_FLAG_KEEP_IDCT):
            prep2 = prepare_batch(files, flags=flag)
            bc2 = prep2.to_c()
            assert create_with(L, dec.ctx.handle, bc2, h, rois=rois) == B.MJ_ERR_INVALID
        # NULL windows: whole images, mj_plan_create's plan
        assert create_with(L, dec.ctx.handle, bc, h, rois=None) == B.MJ_OK
        L.mj_plan_destroy(h)
    finally:
        dec.close()
