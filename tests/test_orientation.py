"""EXIF orientation on the MI355X (mj_plan_request.orientations with and without a size, BatchDecoder's ``orientation=``):
every output is tools/orient_model.py — and, with ``size``, tools/resize_model.py on top of it — applied to the oracle's
pixels, never to the library's own output.  tests/test_orientation_host.py pins both models to Pillow on the CPU."""
import struct

import numpy as np
import pytest

from conftest import oracle_rgb_all
from test_resize import as_layout
from test_roi import LAYOUTS, _fixture_files, mcu_size, window_kinds

pytestmark = pytest.mark.gpu

ODD_SIZES = ((70, 50), (100, 36), (37, 29), (50, 70))


def exif_app1(o: int, order: str = "<") -> bytes:
    """An APP1 segment holding an EXIF block whose IFD0 is the Orientation tag alone."""
    tiff = (b"II*\0" if order == "<" else b"MM\0*") + struct.pack(order + "I", 8) + struct.pack(order + "H", 1)
    tiff += struct.pack(order + "HHIHH", 0x0112, 3, 1, o, 0) + struct.pack(order + "I", 0)
    payload = b"Exif\0\0" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def tagged(raw: bytes, o: int, order: str = "<") -> bytes:
    return raw[:2] + exif_app1(o, order) + raw[2:]


def oriented(full: np.ndarray, o: int, win=None) -> np.ndarray:
    """The oracle's (W, H[, 3]) image as orientation ``o`` shows it, row-major, sliced to a window (x, y, w, h) of THAT image."""
    from tools import orient_model
    a = orient_model.orient(full.swapaxes(0, 1), o)
    if win is not None:
        x, y, w, h = win
        a = a[y:y + h, x:x + w]
    return np.ascontiguousarray(a)


def expected(full, o, layout, win=None, size=None):
    from tools import resize_model
    a = oriented(full, o, win)
    if size is not None:
        a = resize_model.resize(a, size)
    return as_layout(a, layout)


@pytest.fixture(scope="module")
def fixtures():
    """Every golden kind (4:2:0, 4:2:2, 4:4:0, 4:1:1, 4:4:4, grey, non-interleaved, progressive, with and without DRI, the odd
    layouts) plus the odd sizes: (name, raw, oracle pixels, MCU size)."""
    from oracle import oracle
    from tools import synth
    files = _fixture_files()
    for k, (w, h) in enumerate(ODD_SIZES):
        files.append((f"synth_{w}x{h}_420", synth.synth_jpeg(900 + k, w, h, 85, "420", 0)))
        files.append((f"synth_{w}x{h}_444_dri", synth.synth_jpeg(910 + k, w, h, 85, "444", 3)))
    return [(name, raw, oracle.decode(raw)["rgb"], mcu_size(raw)) for name, raw in files]


def test_the_fixtures_hold_the_odd_sizes(fixtures):
    sizes = {f[2].shape[:2] for f in fixtures}
    assert all(s in sizes for s in ODD_SIZES)
    assert any(f[2].ndim == 2 for f in fixtures) and any(f[2].ndim == 3 for f in fixtures)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_fixture_every_orientation_own_size(fixtures, layout):
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    raws = [f[1] for f in fixtures]
    try:
        for o in range(1, 9):
            got = dec.decode(raws, orientation=o)
            for (name, _, full, _), img in zip(fixtures, got):
                want = expected(full, o, layout)
                assert img.shape == want.shape, (name, o)
                assert np.array_equal(img, want), (name, o)
    finally:
        dec.close()


def _mixed(fixtures):
    """a per-file orientation that follows neither the kinds nor the positions, some files upright, some None"""
    turns = [(5 * i + i // 8) % 8 + 1 for i in range(len(fixtures))]
    return [None if (i % 7 == 3) else t for i, t in enumerate(turns)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_batch_of_mixed_orientations_and_kinds_three_routes(fixtures, layout):
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    raws = [f[1] for f in fixtures]
    turns = _mixed(fixtures)
    assert len({t for t in turns}) == 9
    dec = BatchDecoder(device=0, layout=layout, gpu_segment_min_files=1)
    try:
        want = [expected(f[2], t or 1, layout) for f, t in zip(fixtures, turns)]
        host = dec.decode(raws, orientation=turns)
        dev = dec.decode_device(raws, orientation=turns)
        cut = len(raws) // 2
        it = list(dec.decode_device_iter([raws[:cut], raws[cut:]], orientation=[turns[:cut], turns[cut:]]))
        torch.cuda.synchronize()
        streamed = it[0] + it[1]
        for i, w in enumerate(want):
            name = fixtures[i][0]
            assert np.array_equal(host[i], w), ("decode", name, turns[i])
            assert np.array_equal(dev[i].cpu().numpy(), w), ("decode_device", name, turns[i])
            assert np.array_equal(streamed[i].cpu().numpy(), w), ("decode_device_iter", name, turns[i])
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_windows_are_windows_of_the_oriented_image(fixtures, layout):
    """Every window kind of tests/test_roi.py (every edge, the 1 x 1 corners, rows, columns) taken on the ORIENTED image, and
    per-file None windows."""
    from tools import orient_model
    from pyjpegdecoder_amd import BatchDecoder
    raws = [f[1] for f in fixtures]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for o in range(2, 9):
            dims = [orient_model.oriented_size(o, f[2].shape[0], f[2].shape[1]) for f in fixtures]
            kinds = [window_kinds(w, h, *f[3]) for (w, h), f in zip(dims, fixtures)]
            for kind in kinds[0]:
                wins = [None if (i + o) % 5 == 0 else k[kind] for i, k in enumerate(kinds)]
                got = dec.decode(raws, rois=wins, orientation=o)
                for (name, _, full, _), win, img in zip(fixtures, wins, got):
                    assert np.array_equal(img, expected(full, o, layout, win)), (name, o, kind, win)
    finally:
        dec.close()


def test_a_window_outside_the_oriented_image_is_refused(fixtures):
    from pyjpegdecoder_amd import BatchDecoder
    name, raw, full, _ = next(f for f in fixtures if f[2].shape[:2] == (70, 50))
    dec = BatchDecoder(device=0)
    try:
        assert dec.decode([raw], rois=(0, 0, 50, 70), orientation=6)[0].shape[:2] == (50, 70)
        with pytest.raises(ValueError):
            dec.decode([raw], rois=(0, 0, 70, 50), orientation=6)
    finally:
        dec.close()


SIZES = {"shrink": (13, 9), "enlarge": (150, 131), "mixed": (11, 140)}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_size_is_the_resize_of_the_oriented_image(fixtures, layout):
    """Enlarging and shrinking, whole images and windows, all eight orientations in ONE call per component count."""
    from tools import orient_model
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for nc in (1, 3):
            group = [f for f in fixtures if (f[2].ndim == 3) == (nc == 3)]
            raws = [f[1] for f in group]
            turns = [(i + i // 8) % 8 + 1 for i in range(len(group))]
            for sname, size in SIZES.items():
                for kind in (None, "inner", "last_mcu", "corner_br"):
                    wins = None
                    if kind is not None:
                        wins = [window_kinds(*orient_model.oriented_size(t, f[2].shape[0], f[2].shape[1]), *f[3])[kind]
                                for f, t in zip(group, turns)]
                    got = dec.decode(raws, rois=wins, size=size, orientation=turns)
                    assert got.shape == (len(group),) + dec._shape(size[0], size[1], nc)
                    for i, f in enumerate(group):
                        want = expected(f[2], turns[i], layout, None if wins is None else wins[i], size)
                        assert np.array_equal(got[i], want), (f[0], turns[i], sname, kind)
    finally:
        dec.close()


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("layout", ["rowmajor", "planar_rowmajor", "xmajor"])
def test_size_with_dtype_normalize_and_mirror(fixtures, layout, dtype):
    """The model-ready output of an oriented decode: torchvision's Normalize(to_tensor()) of the resized oriented bytes, a
    flagged file mirrored AFTER its orientation."""
    from routes_common import bits_of
    from tools import normalize_model, resize_model
    from pyjpegdecoder_amd import BatchDecoder
    group = [f for f in fixtures if f[2].ndim == 3]
    raws = [f[1] for f in group]
    turns = [(5 * i) % 8 + 1 for i in range(len(group))]
    mirror = [bool((i // 3) % 2) for i in range(len(group))]
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    size = (40, 28)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode_device(raws, size=size, dtype=dtype, normalize=norm, mirror=mirror, orientation=turns)
        bits = bits_of(got)
        for i, f in enumerate(group):
            a = resize_model.resize(oriented(f[2], turns[i]), size)
            if mirror[i]:
                a = a[:, ::-1]
            want = as_layout(normalize_model.normalize(np.ascontiguousarray(a), dtype, norm[0], norm[1]), layout)
            assert bits[i].shape == want.shape and np.array_equal(bits[i], want), (f[0], turns[i], mirror[i])
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["xmajor", "rowmajor"])
def test_sweep_of_source_and_target_sizes_every_orientation(layout):
    """Several dozen (source size, target size) pairs per orientation — the sources are windows of one file, so that one call
    holds many source sizes.  The flips are implemented on the SOURCE side (reversed tap tables, integer sums of the same
    products), so this sweep licenses nothing: it holds them to the definition like everything else."""
    from oracle import oracle
    from tools import orient_model, synth
    from pyjpegdecoder_amd import BatchDecoder
    raw = synth.synth_jpeg(321, 211, 157, 90, "420", 5)
    full = oracle.decode(raw)["rgb"]
    rng = np.random.default_rng(7)
    dec = BatchDecoder(device=0, layout=layout)
    pairs = 0
    try:
        for o in range(2, 9):
            wo, ho = orient_model.oriented_size(o, 211, 157)
            for size in ((16, 16), (33, 7), (5, 61), (224, 224), (97, 180)):
                wins = []
                for _ in range(12):
                    w, h = int(rng.integers(1, wo + 1)), int(rng.integers(1, ho + 1))
                    wins.append((int(rng.integers(0, wo - w + 1)), int(rng.integers(0, ho - h + 1)), w, h))
                got = dec.decode([raw] * len(wins), rois=wins, size=size, orientation=o)
                for k, win in enumerate(wins):
                    assert np.array_equal(got[k], expected(full, o, layout, win, size)), (o, size, win)
                    pairs += 1
    finally:
        dec.close()
    assert pairs == 7 * 60


def test_exif_equals_the_explicit_integer(fixtures):
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    base = [f for f in fixtures if f[2].ndim == 3][:10]
    turns = [i % 8 + 1 for i in range(len(base))]
    files = [tagged(f[1], t, "<>"[i % 2]) for i, (f, t) in enumerate(zip(base, turns))]
    dec = BatchDecoder(device=0, gpu_segment_min_files=1)
    try:
        a = dec.decode(files, orientation="exif")
        b = dec.decode([f[1] for f in base], orientation=turns)
        c = dec.decode_device(files, orientation="exif")
        d = dec.decode_device(files, orientation=["exif"] * len(files), size=(31, 17))
        e = dec.decode([f[1] for f in base], orientation=turns, size=(31, 17))
        torch.cuda.synchronize()
        for i, f in enumerate(base):
            want = expected(f[2], turns[i], "xmajor")
            assert np.array_equal(a[i], want) and np.array_equal(b[i], want) and np.array_equal(c[i].cpu().numpy(), want), (f[0], turns[i])
            assert np.array_equal(d[i].cpu().numpy(), expected(f[2], turns[i], "xmajor", None, (31, 17))), (f[0], turns[i])
        assert np.array_equal(d.cpu().numpy(), e)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
def test_a_second_round_file_keeps_its_orientation_and_its_slot(layout):
    """Files the GPU marker scan hands back (MJ_ST_TAIL: a COM segment behind the scan, as tests/routes_common.py forces it) go
    round again through the host parse: with their orientation, their window and into their slot."""
    import torch
    from oracle import oracle
    from routes_common import with_com
    from tools import synth
    from pyjpegdecoder_amd import BatchDecoder
    s = synth.synth_jpeg
    raws = [s(601, 200, 120, 85, "420", 1), with_com(s(602, 200, 120, 85, "420", 1)), s(603, 200, 120, 85, "420", 1),
            with_com(s(604, 200, 120, 85, "420", 1)), s(605, 200, 120, 85, "420", 1)]
    turns = [6, 8, 1, 3, 5]
    wins = [(3, 5, 100, 150), (10, 20, 60, 31), None, (150, 100, 50, 20), (0, 0, 120, 200)]
    fulls = [oracle.decode(r)["rgb"] for r in raws]
    dec = BatchDecoder(device=0, layout=layout, gpu_segment_min_files=1)
    try:
        own = dec.decode_device(raws, orientation=turns)
        own_w = dec.decode(raws, rois=wins, orientation=turns)
        sized = dec.decode_device(raws, rois=wins, size=(40, 28), orientation=turns)
        streamed = list(dec.decode_device_iter([raws], orientation=[turns], size=(40, 28)))[0]
        torch.cuda.synchronize()
        for i, full in enumerate(fulls):
            assert np.array_equal(own[i].cpu().numpy(), expected(full, turns[i], layout)), i
            assert np.array_equal(own_w[i], expected(full, turns[i], layout, wins[i])), i
            assert np.array_equal(sized[i].cpu().numpy(), expected(full, turns[i], layout, wins[i], (40, 28))), i
            assert np.array_equal(streamed[i].cpu().numpy(), expected(full, turns[i], layout, None, (40, 28))), i
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_none_and_one_are_a_call_without_the_argument(fixtures, layout):
    from pyjpegdecoder_amd import BatchDecoder
    group = [f for f in fixtures if f[2].ndim == 3]
    raws = [f[1] for f in group]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        plain, sized = dec.decode(raws), dec.decode(raws, size=(40, 28))
        for o in (None, 1, [1] * len(raws), [None] * len(raws), "exif"):
            for a, b in zip(plain, dec.decode(raws, orientation=o)):
                assert np.array_equal(a, b)
            assert np.array_equal(sized, dec.decode(raws, size=(40, 28), orientation=o))
            for a, b in zip(plain, dec.decode_device(raws, orientation=o)):
                assert np.array_equal(a, b.cpu().numpy())
    finally:
        dec.close()


def test_c_abi_rules():
    """All ones is the plain plan; a byte outside 1..8 and the seam flags are refused; image offsets stay those of the packing."""
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth
    raws = [synth.synth_jpeg(71, 70, 50, 85, "420", 0), synth.synth_jpeg(72, 37, 29, 85, "420", 0)]
    dec = BatchDecoder(device=0, layout="rowmajor")
    try:
        prep = prepare_batch(raws, dec.layout, 0, [parse_jpeg(r) for r in raws])
        keep = {"prep": prep, "n_images": 2}
        for bad in ([6, 0], [9, 1]):
            with pytest.raises(B.BackendError, match="image [01]: orientation"):
                B.Plan(dec.ctx, prep.to_c(), keep, orientation=bad)
            with pytest.raises(B.BackendError, match="image [01]: orientation"):
                B.Plan(dec.ctx, prep.to_c(), keep, orientation=bad, size=(8, 8))
        seams = prepare_batch(raws, dec.layout, B.MJ_FLAG_KEEP_PLANES, [parse_jpeg(r) for r in raws])
        with pytest.raises(B.BackendError, match="seam"):
            B.Plan(dec.ctx, seams.to_c(), {"prep": seams, "n_images": 2}, orientation=[6, 6])
        with pytest.raises(Exception, match="exchange width and height"):
            B.Plan(dec.ctx, prep.to_c(), keep, orientation=[6, 3], size=(8, 8))
        plain, turned = B.Plan(dec.ctx, prep.to_c(), keep), B.Plan(dec.ctx, prep.to_c(), keep, orientation=[6, 3])
        try:
            assert plain.info.rgb_bytes == turned.info.rgb_bytes == (70 * 50 + 37 * 29) * 3
            assert plain.image_offsets(1) == turned.image_offsets(1)
        finally:
            plain.close()
            turned.close()
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
def test_at_size_256_x_1080p_orientation_6(layout):
    """256 distinct 1080p 4:2:0 files, all orientation 6, on decode_device's default route: every one against the oracle through
    the models, at its own size (1080 x 1920) and resized to 224 x 224."""
    from pyjpegdecoder_amd import BatchDecoder
    from tools import synth
    W, H, n = 1920, 1080, 256
    blob, offs = synth.synth_batch(n, 8800, W, H, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        own = [t.cpu().numpy() for t in dec.decode_device(raws, orientation=6)]
        sized = dec.decode_device(raws, size=(224, 224), orientation=6).cpu().numpy()
    finally:
        dec.close()
    assert own[0].shape == dec._shape(H, W, 3)
    for d, full in enumerate(oracle_rgb_all(raws)):
        assert np.array_equal(own[d], expected(full, 6, layout)), d
        assert np.array_equal(sized[d], expected(full, 6, layout, None, (224, 224))), d
