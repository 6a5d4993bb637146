"""Resample filters of a decode to a fixed size on the MI355X (mj_plan_request.filter, BatchDecoder.decode /
decode_device / decode_device_iter(size=..., resample=...)): every output is byte for byte tools/resize_model.py with that filter
— which tests/test_resample_host.py pins to Pillow's resize(size, filter) — applied to the oracle's pixels of the image or
window, in every layout.  Expected values never come from the library."""
import numpy as np
import pytest

from conftest import GOLDEN, oracle_rgb_all
from test_resize import as_layout, rowmajor_window
from test_roi import LAYOUTS, _fixture_files, mcu_size, window_kinds

pytestmark = pytest.mark.gpu

FILTERS = ("bilinear", "box", "hamming", "bicubic", "lanczos")
SIGNED = ("bicubic", "lanczos")

_cache = {}


def model(key, img_rm: np.ndarray, size, filter: str) -> np.ndarray:
    """tools/resize_model.py of a row-major image, computed once per (key, size, filter) and left unchanged: the layouts share it."""
    from tools import resize_model
    k = (key, tuple(size), filter)
    if k not in _cache:
        _cache[k] = resize_model.resize(img_rm, size, filter)
        _cache[k].setflags(write=False)
    return _cache[k]


def expect(key, full, win, size, layout, filter):
    """model(oracle window) in the decoder's layout"""
    return as_layout(model((key, tuple(win)), rowmajor_window(full, win), size, filter), layout)


@pytest.fixture(scope="module")
def fixtures():
    """test_resize.py's fixture set, by component count (one call fills one array): (name, raw, oracle pixels, MCU size)."""
    files = _fixture_files()
    fulls = oracle_rgb_all([raw for _, raw in files])
    out = [(name, raw, full, mcu_size(raw)) for (name, raw), full in zip(files, fulls)]
    return {nc: [f for f in out if (f[2].ndim == 3) == (nc == 3)] for nc in (1, 3)}


CLAMP_FILES = ("64x64_444_q98_pil", "96x64_420_q100_noise", "ni_37x29_444_dri4")


@pytest.mark.parametrize("filter", SIGNED)
def test_both_clamps_are_reached_in_both_passes(fixtures, filter):
    """The condition first: on these three files at (150, 100) the model's sums fall below 0 and rise above 255 in the width pass
    and again in the height pass — so a kernel that clamps at one end only, or in one pass only, cannot pass the comparison that
    follows (every layout).  No greyscale fixture reaches the clamps: the one-component instances of the signed kernels are held
    to the model by parity alone (test_every_filter_every_layout_every_fixture)."""
    from tools import resize_model
    from pyjpegdecoder_amd import BatchDecoder
    size = (150, 100)
    group = [f for f in fixtures[3] if f[0] in CLAMP_FILES]
    assert len(group) == 3
    for name, _, full, _ in group:
        clipped = []
        resize_model.resize(rowmajor_window(full, (0, 0, full.shape[0], full.shape[1])), size, filter, clipped=clipped)
        assert len(clipped) == 2, name
        for p, (below, above) in enumerate(clipped):
            assert below >= 1 and above >= 1, (name, filter, "width pass" if p == 0 else "height pass", below, above)
    for layout in LAYOUTS:
        dec = BatchDecoder(device=0, layout=layout)
        try:
            got = dec.decode([f[1] for f in group], size=size, resample=filter)
            for i, (name, _, full, _) in enumerate(group):
                assert np.array_equal(got[i], expect(name, full, (0, 0, full.shape[0], full.shape[1]), size, layout, filter)), (name, layout)
        finally:
            dec.close()


# shrink both, shrink strongly, shrink to a handful — and (64, 36): the width of the 64-wide files and the height of the 36-high ones unchanged
SIZES = ((150, 100), (33, 21), (7, 5), (64, 36))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("filter", FILTERS)
def test_every_filter_every_layout_every_fixture(fixtures, filter, layout):
    """Every fixture file of tests/test_resize.py, whole and through one kind of window (inside MCUs), colour and greyscale."""
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    unchanged = 0
    try:
        for nc, group in fixtures.items():
            assert group
            raws = [f[1] for f in group]
            inner = [window_kinds(f[2].shape[0], f[2].shape[1], *f[3])["inner"] for f in group]
            for size in SIZES:
                for wins in (None, inner):
                    got = dec.decode(raws, rois=wins, size=size, resample=filter)
                    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
                    assert got.shape == (len(group),) + dec._shape(size[0], size[1], nc), (size, wins is None)
                    for i, (name, _, full, _) in enumerate(group):
                        win = (0, 0, full.shape[0], full.shape[1]) if wins is None else wins[i]
                        unchanged += win[2] == size[0] or win[3] == size[1]
                        assert np.array_equal(got[i], expect(name, full, win, size, layout, filter)), (name, size, win)
        assert unchanged >= 4
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["rowmajor", "xmajor"])
@pytest.mark.parametrize("filter", SIGNED)
def test_several_tiles_on_both_axes_with_the_widest_taps(filter, layout):
    """One 1920 x 1080 file to 224 x 224: 27 (bicubic) and 53 (Lanczos) taps per pixel along the width.  The launch has more than
    one tile along x and along y (a single image makes the row-major plan give up columns, the small batch rows), and the tiles
    fit the 64 KB a workgroup's LDS is budgeted with."""
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    raw = (GOLDEN / "files" / "c3_1920x1080_420_dri120.jpg").read_bytes()
    full = oracle_rgb_all([raw])[0]
    size = (224, 224)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        prep = prepare_batch([raw], dec.layout, 0)
        plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 1}, size=size, filter=filter)
        try:
            shape = plan.resize_shape()
            assert shape["signed"] and shape["filter"] == B.FILTERS[filter]
            assert shape["max_ksize"] == {"bicubic": 37, "lanczos": 53}[filter]
            assert shape["tiles_x"] > 1 and shape["tiles_y"] > 1, shape
            assert shape["tiles_x"] == -(-224 // shape["tile_cols"]) and shape["tiles_y"] == -(-224 // shape["tile_rows"])
            assert 0 < shape["lds_bytes"] <= 64 * 1024, shape
            plan.execute()
            plan.sync()
            out = plan.read(rgb=True)
            assert not out["status"].any()
            want = expect("c3", full, (0, 0, 1920, 1080), size, layout, filter)
            assert np.array_equal(out["rgb"].reshape(want.shape), want)
        finally:
            plan.close()
    finally:
        dec.close()


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def test_bicubic_with_float16_normalize_and_per_file_mirror(fixtures):
    """planar_rowmajor, the NCHW batch: the float16 table and the per-file flips stay inside the one (signed) resize launch."""
    from routes_common import bits_of
    from tools import normalize_model
    from pyjpegdecoder_amd import BatchDecoder
    group = fixtures[3]
    raws = [f[1] for f in group]
    mirror = [bool((i // 2) % 2) for i in range(len(group))]
    assert any(mirror) and not all(mirror)
    size, layout = (40, 28), "planar_rowmajor"
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for call in (dec.decode, dec.decode_device):
            bits = bits_of(call(raws, size=size, dtype="float16", normalize=(MEAN, STD), mirror=mirror, resample="bicubic"))
            for i, (name, _, full, _) in enumerate(group):
                a = model((name, "whole"), rowmajor_window(full, (0, 0, full.shape[0], full.shape[1])), size, "bicubic")
                if mirror[i]:
                    a = a[:, ::-1]
                want = as_layout(normalize_model.normalize(np.ascontiguousarray(a), "float16", MEAN, STD), layout)
                assert bits[i].shape == want.shape and np.array_equal(bits[i], want), (name, mirror[i])
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_lanczos_of_oriented_images_and_oriented_windows(fixtures, layout):
    """Orientations 1, 2, 3, 6 and 8 in one call (three plans: upright, turned, width and height exchanged), whole and through
    windows of the ORIENTED images: the model chained behind tools/orient_model.py."""
    from tools import orient_model
    from pyjpegdecoder_amd import BatchDecoder
    group = fixtures[3]
    raws = [f[1] for f in group]
    cycle = (1, 2, 3, 6, 8)
    turns = [cycle[i % 5] for i in range(len(group))]
    size = (33, 21)

    def oriented(full, o):
        return np.ascontiguousarray(orient_model.orient(full.swapaxes(0, 1), o))
    wins = []
    for (_, _, full, _), o in zip(group, turns):
        h, w = oriented(full, o).shape[:2]
        wins.append((min(2, w - 1), min(3, h - 1), max(1, w - 5), max(1, h - 7)))
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for rois in (None, wins):
            got = dec.decode_device(raws, rois=rois, size=size, orientation=turns, resample="lanczos").cpu().numpy()
            for i, (name, _, full, _) in enumerate(group):
                a = oriented(full, turns[i])
                if rois is not None:
                    x, y, w, h = rois[i]
                    a = np.ascontiguousarray(a[y:y + h, x:x + w])
                want = as_layout(model((name, turns[i], rois[i] if rois else None), a, size, "lanczos"), layout)
                assert np.array_equal(got[i], want), (name, turns[i], rois is not None)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
@pytest.mark.parametrize("segment", ["host", "gpu"])
def test_every_route_resamples_with_the_calls_filter(segment, layout):
    """Files of several kinds (sampling layouts, baseline and progressive, with and without restart markers, two the GPU marker
    scan hands back for a second round) in one call with resample="bicubic": one tensor in input order from decode,
    decode_device, decode_device in parts and decode_device_iter over two batches; a greyscale file among them is refused as
    ever."""
    import torch
    from routes_common import with_com
    from pyjpegdecoder_amd import BatchDecoder
    from tools import synth
    g = np.load(GOLDEN / "odd_layouts.npz")
    odd = sorted(k for k in g.files if k.endswith(".jpg"))[0]
    files = [synth.synth_jpeg(41, 200, 120, 85, "420", 13), synth.synth_jpeg(44, 96, 64, 85, "444", 0),
             with_com(synth.synth_jpeg(42, 333, 77, 85, "420", 21)), (GOLDEN / "files" / "prog_70x50_420_pil.jpg").read_bytes(),
             g[odd].tobytes(), synth.synth_jpeg(43, 200, 120, 85, "420", 7), (GOLDEN / "files" / "64x48_422_pil.jpg").read_bytes(),
             with_com(synth.synth_jpeg(45, 200, 120, 85, "420", 13))]
    grey = (GOLDEN / "files" / "50x70_grey_dri4.jpg").read_bytes()
    fulls = oracle_rgb_all(files)
    wins = [(37, 21, 90, 50), None, (150, 10, 5, 3), (10, 9, 33, 21), None, None, (17, 3, 40, 40), (3, 5, 190, 100)]
    size, filter = (56, 40), "bicubic"

    def check(host, rois, what):
        for i, full in enumerate(fulls):
            win = (rois[i] if rois is not None else None) or (0, 0, full.shape[0], full.shape[1])
            assert np.array_equal(host[i], expect(("routes", i), full, win, size, layout, filter)), (what, segment, i)
    for min_files in (64, 1):                    # a handful of files on the host-parsed route, or the native front end + GPU scan
        dec = BatchDecoder(device=0, layout=layout, segment=segment, gpu_segment_min_files=min_files)
        shape = dec._shape(size[0], size[1], 3)
        try:
            for rois in (None, wins):
                got = dec.decode_device(files, rois=rois, size=size, resample=filter)
                assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and tuple(got.shape) == (len(files),) + shape
                check(got.cpu().numpy(), rois, "decode_device")
                check(dec.decode(files, rois=rois, size=size, resample=filter), rois, "decode")
                check(dec.decode_device(files, rois=rois, size=size, resample=filter, parts=2).cpu().numpy(), rois, "parts")
            per_batch = list(dec.decode_device_iter([files[:3], files[3:]], size=size, resample=filter))
            assert [tuple(t.shape) for t in per_batch] == [(3,) + shape, (5,) + shape]
            check(torch.cat(per_batch).cpu().numpy(), None, "iter")
            for call in (dec.decode, dec.decode_device):
                with pytest.raises(ValueError, match="file 8"):
                    call(files + [grey], size=size, resample=filter)
        finally:
            dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("segment", ["host", "gpu"])
def test_sentinels_slots_and_a_poisoned_intermediate_lanczos(layout, segment):
    """A signed filter: bytes behind the output array and the slots a plan does not name are untouched, and what the
    intermediate buffer held before the execute does not show in the result."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth
    files = [synth.synth_jpeg(31 + k, 200, 120, 85, "420", ri) for k, ri in enumerate((13, 7, 0))]
    wins = [(37, 21, 90, 50), (101, 40, 60, 3), (3, 5, 7, 100)]
    fulls = oracle_rgb_all(files)
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
                                  slots=([slot_of[i] for i in group], n_slots), filter="lanczos")
                    try:
                        assert plan.info.rgb_bytes == n_slots * per and plan.resize_shape()["signed"]
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
                    want = expect(("sentinel", i), fulls[i], win, size, layout, "lanczos")
                    assert np.array_equal(host[s * per:(s + 1) * per].reshape(want.shape), want), (i, layout, segment, size)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_default_is_unchanged(fixtures, layout):
    """resample=None, "bilinear" and Pillow's BILINEAR are a call without the argument: identical outputs from plans that are
    cut the same way and run the unsigned instances — as box and hamming plans do, with another table."""
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    group = fixtures[3]
    raws = [f[1] for f in group]
    same = [None, "bilinear", "BILINEAR", 2]
    try:
        from PIL import Image
        same.append(Image.Resampling.BILINEAR)
    except ImportError:
        pass
    size = (33, 21)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        plain = dec.decode(raws, size=size)
        plain_dev = dec.decode_device(raws, size=size).cpu().numpy()
        for i, (name, _, full, _) in enumerate(group):
            assert np.array_equal(plain[i], expect(name, full, (0, 0, full.shape[0], full.shape[1]), size, layout, "bilinear")), name
        for r in same:
            assert np.array_equal(dec.decode(raws, size=size, resample=r), plain), r
            assert np.array_equal(dec.decode_device(raws, size=size, resample=r).cpu().numpy(), plain_dev), r
            assert np.array_equal(next(dec.decode_device_iter([raws], size=size, resample=r)).cpu().numpy(), plain_dev), r
        one = [group[0][1]]
        prep = prepare_batch(one, dec.layout, 0)
        shapes = {}
        for f in (None, "bilinear", "box", "hamming", "bicubic"):
            plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 1}, size=size, filter=f)
            try:
                shapes[f] = plan.resize_shape()
            finally:
                plan.close()
        assert shapes[None] == shapes["bilinear"] and shapes[None]["filter"] == 0 and not shapes[None]["signed"]
        assert not shapes["box"]["signed"] and not shapes["hamming"]["signed"] and shapes["bicubic"]["signed"]
        for call in (dec.decode, dec.decode_device):
            with pytest.raises(ValueError, match="resample needs size"):
                call(raws, resample="bicubic")
            with pytest.raises(ValueError, match="not a convolution"):
                call(raws, size=size, resample="nearest")
        with pytest.raises(ValueError, match="resample must be one of"):
            next(dec.decode_device_iter([raws], size=size, resample="cubic"))
    finally:
        dec.close()
