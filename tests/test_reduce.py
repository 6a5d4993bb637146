"""The two-step resize on the MI355X (mj_plan_request.reducing_gap, BatchDecoder.decode / decode_device /
decode_device_iter(size=..., reducing_gap=...)): every output is byte for byte tools/reduce_model.py — which
tests/test_reduce_host.py pins to Pillow's resize(size, filter, reducing_gap=g) — applied to the oracle's pixels of the image or
window, in every layout.  Expected values never come from the library, and every test first asserts through
mj_debug_reduce_shape that the plan reduces with the factors it names: one that ran the single step would show nothing."""
import numpy as np
import pytest

from conftest import GOLDEN, oracle_rgb_all
from test_resize import as_layout, rowmajor_window
from test_roi import LAYOUTS

pytestmark = pytest.mark.gpu

FILTERS = ("bilinear", "box", "hamming", "bicubic", "lanczos")

_files = {}
_cache = {}


def fixture(name):
    """(raw bytes, the oracle's (W, H[, 3]) pixels) of tests/golden/files/<name>.jpg, decoded once"""
    if name not in _files:
        raw = (GOLDEN / "files" / f"{name}.jpg").read_bytes()
        full = oracle_rgb_all([raw])[0]
        full.setflags(write=False)
        _files[name] = (raw, full)
    return _files[name]


def model(key, img_rm, size, filter, gap):
    """tools/reduce_model.py of a row-major image, once per key and left unchanged: the layouts share it.  The case first: Pillow's
    other pass order (an image more than 100 times taller than wide) is not what is being compared."""
    from tools import reduce_model
    k = (key, tuple(size), filter, gap)
    if k not in _cache:
        h, w = img_rm.shape[:2]
        fx, fy = reduce_model.reduce_factors(w, h, size[0], size[1], gap) if gap is not None else (1, 1)
        assert not reduce_model.tall(-(-w // fx), -(-h // fy), size[1]), k
        _cache[k] = reduce_model.resize(img_rm, size, filter, gap)
        _cache[k].setflags(write=False)
    return _cache[k]


def whole(full):
    return (0, 0, full.shape[0], full.shape[1])


def plan_shapes(dec, raws, **kw):
    """mj_debug_reduce_shape of every image of the one plan these files of one kind make with these Plan keywords"""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    prep = prepare_batch(raws, dec.layout, 0)
    plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(raws)}, **kw)
    try:
        return [plan.reduce_shape(i) for i in range(len(raws))]
    finally:
        plan.close()


def assert_reduces(dec, raw, size, gap, factors, **kw):
    s = plan_shapes(dec, [raw], size=size, reducing_gap=gap, **kw)[0]
    assert s["reduces"] and (s["fx"], s["fy"]) == tuple(factors), s
    return s


# (fixture, size, gap, factors): what each exercises is the issue's table — partial cells on both axes with rows that start at
# every byte alignment (row pitch 210 bytes); a cell wider than a lane's 16 bytes; one axis untouched; the shift cases 2 x 2 and
# 4 x 4; remainder 1; remainders 1 and 1; one component.  (Rows staged in pieces, several tiles under a phase, tile rows of 500 bytes
# and more, the early return along the contiguous axis, the largest cell: tests/reduce_cases.py, test_reduce_paths_host.py, test_reduce_paths.py.)
ROWS = (("70x50_420_pil_opt", (8, 7), 2.0, (4, 3)),
        ("128x64_420_dri3", (4, 4), 1.0, (32, 16)),
        ("100x36_420_dri7", (12, 18), 2.0, (4, 1)),
        ("64x64_420_pil", (16, 16), 2.0, (2, 2)),
        ("64x64_420_pil", (16, 16), 1.0, (4, 4)),
        ("64x64_420_pil", (10, 10), 2.0, (3, 3)),
        ("ni_37x29_444_dri4", (5, 4), 1.5, (4, 4)),
        ("64x64_grey_pil", (10, 10), 2.0, (3, 3)),
        ("50x70_grey_dri4", (6, 5), 2.0, (4, 7)))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_row_of_the_table_in_every_layout(layout):
    """All five filters on the first row, two on the others."""
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for r, (name, size, gap, factors) in enumerate(ROWS):
            raw, full = fixture(name)
            s = assert_reduces(dec, raw, size, gap, factors)
            assert (s["width"], s["height"]) == (-(-full.shape[0] // factors[0]), -(-full.shape[1] // factors[1])) and s["phase_x"] == s["phase_y"] == 0
            for filter in (FILTERS if r == 0 else ("bilinear", "lanczos")):
                got = dec.decode([raw], size=size, resample=filter, reducing_gap=gap)
                want = as_layout(model(name, rowmajor_window(full, whole(full)), size, filter, gap), layout)
                assert got.shape[1:] == want.shape and np.array_equal(got[0], want), (name, size, gap, filter)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["rowmajor", "xmajor"])
def test_the_workloads_own_factors(layout):
    """One 1920 x 1080 file to 224 x 224 with gap 2.0: 4 x 2, many tiles of the reduce launch on both axes."""
    from pyjpegdecoder_amd import BatchDecoder
    raw, full = fixture("c3_1920x1080_420_dri120")
    size = (224, 224)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        s = assert_reduces(dec, raw, size, 2.0, (4, 2), filter="bicubic")
        assert (s["width"], s["height"]) == (480, 540)
        got = dec.decode([raw], size=size, resample="bicubic", reducing_gap=2.0)
        assert np.array_equal(got[0], as_layout(model("c3", rowmajor_window(full, whole(full)), size, "bicubic", 2.0), layout))
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_plan_of_files_whose_factors_differ_some_1x1(layout):
    """Three 4:2:0 images in one plan: 4 x 2, 1 x 1 (a small window; the identity cell: all images go through the reduce launch)
    and 3 x 1."""
    from pyjpegdecoder_amd import BatchDecoder
    names = ("128x64_420_dri3", "128x64_420_dri3", "100x36_420_dri7")
    wins = [(0, 0, 128, 64), (1, 1, 25, 21), (0, 0, 100, 36)]
    size, gap = (20, 20), 1.5
    raws = [fixture(n)[0] for n in names]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        shapes = plan_shapes(dec, raws, size=size, reducing_gap=gap, rois=wins)
        assert [(s["fx"], s["fy"], s["reduces"]) for s in shapes] == [(4, 2, True), (1, 1, True), (3, 1, True)]
        got = dec.decode(raws, rois=wins, size=size, reducing_gap=gap)
        for i, n in enumerate(names):
            full = fixture(n)[1]
            assert np.array_equal(got[i], as_layout(model((n, wins[i]), rowmajor_window(full, wins[i]), size, "bilinear", gap), layout)), (n, wins[i])
        # every factor 1: the plan without the argument
        (s,) = plan_shapes(dec, raws[1:2], size=size, reducing_gap=gap, rois=wins[1:2])
        assert not s["reduces"] and (s["fx"], s["fy"], s["width"], s["height"]) == (1, 1, 25, 21)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_windows_at_odd_offsets(layout):
    """The cells are the window's: exif_transpose(img).crop(window).resize(size, reducing_gap=g)."""
    from pyjpegdecoder_amd import BatchDecoder
    cases = (("70x50_420_pil_opt", (3, 5, 61, 43), (7, 5), 2.0, (4, 4)), ("50x70_grey_dri4", (7, 1, 41, 66), (5, 6), 1.0, (8, 11)))
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for name, win, size, gap, factors in cases:
            raw, full = fixture(name)
            s = assert_reduces(dec, raw, size, gap, factors, rois=[win])
            assert (s["width"], s["height"]) == (-(-win[2] // factors[0]), -(-win[3] // factors[1]))
            got = dec.decode([raw], rois=[win], size=size, resample="hamming", reducing_gap=gap)
            assert np.array_equal(got[0], as_layout(model((name, win), rowmajor_window(full, win), size, "hamming", gap), layout)), name
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("o", [2, 3, 6, 7])
def test_orientations_phases_and_exchanged_factors(o, layout):
    """Pillow reduces the ORIENTED image: along a stored axis the orientation reverses the partial cell comes first (phase =
    size mod f), and orientations 5..8 exchange the factors.  Whole, and through a window of the oriented image."""
    from tools import orient_model
    from pyjpegdecoder_amd import BatchDecoder
    name, gap = "70x50_420_pil_opt", 2.0
    raw, full = fixture(name)
    a = np.ascontiguousarray(orient_model.orient(full.swapaxes(0, 1), o))
    turned = o in (6, 7)
    # of the oriented image: 50 x 70 -> (8, 4) is 3 x 8, 70 x 50 -> (8, 7) is 4 x 3; every remainder is above 0
    size, factors = ((8, 4), (3, 8)) if turned else ((8, 7), (4, 3))
    # which stored axes the orientation reverses, from the model: the stored coordinates, oriented, run downwards
    ys, xs = np.mgrid[0:50, 0:70]
    back = []
    for coord in (xs, ys):
        t = orient_model.orient(coord, o)
        back.append(bool(t[0, 0] > t[0, -1] or t[0, 0] > t[-1, 0]))
    dec = BatchDecoder(device=0, layout=layout)
    try:
        s = plan_shapes(dec, [raw], size=size, reducing_gap=gap, orientation=[o])[0]
        stored = (factors[1], factors[0]) if turned else factors
        assert s["reduces"] and (s["fx"], s["fy"]) == stored, s
        assert (s["phase_x"], s["phase_y"]) == (70 % stored[0] if back[0] else 0, 50 % stored[1] if back[1] else 0), s
        assert any(back) and 70 % stored[0] and 50 % stored[1]
        got = dec.decode([raw], size=size, orientation=o, resample="bicubic", reducing_gap=gap)
        assert np.array_equal(got[0], as_layout(model((name, o), a, size, "bicubic", gap), layout))
        h, w = a.shape[:2]
        win = (3, 2, w - 4, h - 7)
        got = dec.decode([raw], rois=[win], size=size, orientation=o, reducing_gap=gap)
        x, y, ww, hh = win
        assert np.array_equal(got[0], as_layout(model((name, o, win), np.ascontiguousarray(a[y:y + hh, x:x + ww]), size, "bilinear", gap), layout))
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_modes_convert_before_the_reduce(layout):
    """mode="L" on a colour file: the reduce launch converts where it reads (convert, then reduce, then resample); mode="RGB" on
    a greyscale file: the byte is replicated at the resize's store, which commutes with everything in between."""
    from tools import mode_model
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for name, mode, size, gap, factors in (("70x50_420_pil_opt", "L", (8, 7), 2.0, (4, 3)), ("50x70_grey_dri4", "RGB", (6, 5), 2.0, (4, 7))):
            raw, full = fixture(name)
            assert_reduces(dec, raw, size, gap, factors, mode=mode)
            a = mode_model.convert(rowmajor_window(full, whole(full)), mode)
            got = dec.decode([raw], size=size, mode=mode, resample="lanczos", reducing_gap=gap)
            want = as_layout(model((name, mode), np.ascontiguousarray(a), size, "lanczos", gap), layout)
            assert got.shape[1:] == want.shape and np.array_equal(got[0], want), (name, mode)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_contain_with_fill(layout):
    """resize_to="contain": the factors come from the PLACE's size, and the fill surrounds the two-step result."""
    from tools import place_model
    from pyjpegdecoder_amd import BatchDecoder
    name, canvas, gap, fill = "100x36_420_dri7", (20, 20), 2.0, (9, 200, 77)
    raw, full = fixture(name)
    resized = place_model.resized_size("contain", 100, 36, canvas)
    xy = place_model.centred("contain", resized, canvas)
    assert resized == (20, 7)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        assert_reduces(dec, raw, canvas, gap, (2, 2), places=[tuple(resized) + tuple(xy)], fill=fill)
        got = dec.decode([raw], size=canvas, resize_to="contain", fill=fill, resample="bicubic", reducing_gap=gap)
        small = model((name, "contain"), rowmajor_window(full, whole(full)), resized, "bicubic", gap)
        want = np.empty((20, 20, 3), dtype=np.uint8)
        want[...] = np.asarray(fill, dtype=np.uint8)
        want[xy[1]:xy[1] + 7, xy[0]:xy[0] + 20] = small
        assert np.array_equal(got[0], as_layout(want, layout))
    finally:
        dec.close()


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def test_mirror_float16_normalize_and_the_three_calls():
    """planar_rowmajor, the NCHW batch: mirror + float16 + normalize behind the two steps; decode_device and decode_device_iter
    equal decode."""
    from routes_common import bits_of
    from tools import normalize_model
    from pyjpegdecoder_amd import BatchDecoder
    names = ("64x64_420_pil", "128x64_420_dri3")
    size, gap, layout = (16, 12), 1.5, "planar_rowmajor"
    raws = [fixture(n)[0] for n in names]
    mirror = [True, False]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        shapes = plan_shapes(dec, raws, size=size, reducing_gap=gap)
        assert [(s["fx"], s["fy"], s["reduces"]) for s in shapes] == [(2, 3, True), (5, 3, True)]
        kw = dict(size=size, dtype="float16", normalize=(MEAN, STD), mirror=mirror, resample="bicubic", reducing_gap=gap)
        host = bits_of(dec.decode(raws, **kw))
        for i, n in enumerate(names):
            full = fixture(n)[1]
            a = model(n, rowmajor_window(full, whole(full)), size, "bicubic", gap)
            if mirror[i]:
                a = a[:, ::-1]
            want = as_layout(normalize_model.normalize(np.ascontiguousarray(a), "float16", MEAN, STD), layout)
            assert host[i].shape == want.shape and np.array_equal(host[i], want), n
        assert np.array_equal(bits_of(dec.decode_device(raws, **kw)), host)
        # (the iterator takes its mirror flags batch by batch)
        assert np.array_equal(bits_of(next(dec.decode_device_iter([raws], **dict(kw, mirror=[mirror])))), host)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_call_without_the_argument_returns_what_it_returned(layout):
    """reducing_gap=None is a call without it — tests/test_resample.py's expectation — and so is a gap under which no factor
    exceeds 1; the argument's refusals."""
    from test_resample import expect
    from pyjpegdecoder_amd import BatchDecoder
    name, size = "70x50_420_pil_opt", (33, 21)
    raw, full = fixture(name)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        want = expect(name, full, whole(full), size, layout, "bicubic")
        assert np.array_equal(dec.decode([raw], size=size, resample="bicubic")[0], want)
        assert np.array_equal(dec.decode([raw], size=size, resample="bicubic", reducing_gap=None)[0], want)
        (s,) = plan_shapes(dec, [raw], size=size, reducing_gap=2.0, filter="bicubic")
        assert not s["reduces"]
        assert np.array_equal(dec.decode([raw], size=size, resample="bicubic", reducing_gap=2.0)[0], want)
        for call in (dec.decode, dec.decode_device):
            with pytest.raises(ValueError, match="reducing_gap needs size"):
                call([raw], reducing_gap=2.0)
            with pytest.raises(ValueError, match="reducing_gap must be 1.0 or greater"):
                call([raw], size=size, reducing_gap=0.5)
        with pytest.raises(ValueError, match="reducing_gap must be 1.0 or greater"):
            next(dec.decode_device_iter([[raw]], size=size, reducing_gap=float("nan")))
    finally:
        dec.close()
