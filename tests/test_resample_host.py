"""Resample filters of a decode to a fixed size, the parts that need no GPU: the NumPy model (tools/resize_model.py) is Pillow's
Image.resize(size, filter) byte for byte for BILINEAR, BOX, HAMMING, BICUBIC and LANCZOS; the library's tap tables
(mj_host_resize_table_filtered) are the model's, entry for entry; the taps stay inside what the kernels' arithmetic holds;
resample= is checked before any GPU work; the new entry points are exported and declared as plain C."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FILTERS = ("bilinear", "box", "hamming", "bicubic", "lanczos")


def _cases():
    """((in_w, in_h), (out_w, out_h), channels, kind of data): 40 seeded cases with sources up to 100 x 64 and outputs up to 224 x
    224, then sizes 1 and 2 on either side, an unchanged axis either way, both unchanged, a strong shrink and a strong growth."""
    rng = np.random.default_rng(1764)
    cases = []
    for k in range(40):
        iw, ih = int(rng.integers(1, 101)), int(rng.integers(1, 65))
        ow, oh = (int(v) for v in rng.integers(1, 225, 2))
        cases.append(((iw, ih), (ow, oh), 3 if k % 2 else 1, ("noise", "binary", "white")[k % 3]))
    edge = [((1, 1), (1, 1)), ((1, 1), (9, 5)), ((2, 1), (1, 2)), ((2, 2), (7, 1)), ((1, 2), (2, 31)), ((37, 29), (1, 1)), ((37, 29), (2, 2)),
            ((50, 2), (2, 50)), ((37, 29), (37, 11)), ((37, 29), (90, 29)), ((37, 29), (37, 29)), ((250, 5), (7, 5)), ((250, 6), (7, 3)),
            ((7, 3), (250, 6)), ((3, 250), (5, 7)), ((5, 7), (3, 250))]
    cases += [(i, o, 3 if k % 2 else 1, ("binary", "noise")[k % 2]) for k, (i, o) in enumerate(edge)]
    return cases


def _data(rng, w, h, c, kind):
    shape = (h, w, 3) if c == 3 else (h, w)
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "binary":                 # two levels: the sums of the filters with side lobes leave 0..255 at every edge
        return (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    return np.full(shape, 255, dtype=np.uint8)


@pytest.mark.parametrize("filter", FILTERS)
def test_model_is_pillow_byte_for_byte(filter):
    Image = pytest.importorskip("PIL.Image")
    from tools import resize_model
    pil = getattr(Image.Resampling, filter.upper())
    rng = np.random.default_rng(11)
    cases = _cases()
    bad = []
    reached = [0, 0]
    for (iw, ih), (ow, oh), c, kind in cases:
        a = _data(rng, iw, ih, c, kind)
        want = np.asarray(Image.fromarray(a).resize((ow, oh), pil))
        clipped = []
        got = resize_model.resize(a, (ow, oh), filter, clipped=clipped)
        for below, above in clipped:
            reached[0] += below
            reached[1] += above
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append(((iw, ih), (ow, oh), c, kind))
    assert len(cases) == 56
    assert not bad, f"{filter}: {len(bad)} of {len(cases)} cases differ from Pillow, first {bad[:5]}"
    if filter in ("bicubic", "lanczos"):      # ... and the comparison has seen both clamps at work
        assert reached[0] > 0 and reached[1] > 0, reached


def test_existing_callers_of_the_model_see_the_bilinear_filter():
    from tools import resize_model
    for i, o in ((1080, 224), (7, 250), (33, 33), (1, 9)):
        for x, y in zip(resize_model.axis_table(i, o), resize_model.axis_table(i, o, "bilinear")):
            assert np.array_equal(x, y)
        assert (resize_model.axis_table(i, o)[2] >= 0).all()
    a = np.random.default_rng(3).integers(0, 256, (29, 37, 3), dtype=np.uint8)
    assert np.array_equal(resize_model.resize(a, (50, 11)), resize_model.resize(a, (50, 11), "bilinear"))
    assert np.array_equal(resize_model.resample_axis(a, 9, 1), resize_model.resample_axis(a, 9, 1, filter="bilinear"))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


PAIRS = [(1080, 224), (1920, 224), (375, 256), (7, 250), (250, 7)] + [(n, n) for n in (1, 2, 33, 224)] + \
        [(n, 1) for n in (1, 2, 33, 1080)] + [(1, n) for n in (2, 33, 224)]


@pytest.mark.parametrize("filter", FILTERS)
def test_library_tap_tables_are_the_models(lib, filter):
    from pyjpegdecoder_amd import _binding as B
    from tools import resize_model
    import math
    support = resize_model.FILTERS[filter][0]
    fid = B.FILTERS[filter]
    assert list(B.FILTERS) == list(resize_model.FILTERS) and list(B.FILTERS.values()) == [0, 1, 2, 3, 4]
    for i, o in PAIRS:
        xmin, count, taps = B.resize_table(i, o, filter)
        mxmin, mcount, mtaps = resize_model.axis_table(i, o, filter)
        assert taps.shape[1] == int(math.ceil(support * max(i / o, 1.0))) * 2 + 1, (i, o)
        assert np.array_equal(xmin, mxmin), (i, o)
        assert np.array_equal(count, mcount), (i, o)
        assert taps.shape == mtaps.shape and np.array_equal(taps, mtaps), (i, o)
        for x, y in zip(B.resize_table(i, o, fid), (xmin, count, taps)):       # (by number as by name)
            assert np.array_equal(x, y)
        if filter == "bilinear":           # filter 0: the table of the function that was there before
            for x, y in zip(B.resize_table(i, o), (xmin, count, taps)):
                assert np.array_equal(x, y), (i, o)
    if filter in ("bicubic", "lanczos"):
        assert (B.resize_table(7, 250, filter)[2] < 0).any() and (B.resize_table(250, 7, filter)[2] < 0).any()
    # a wider row than the table needs: the tail is zeros; a narrower one is refused
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ks = ctypes.c_int32()
    assert lib.mj_host_resize_table_filtered(fid, 100, 30, None, None, None, 0, ctypes.byref(ks)) == B.MJ_OK
    want = resize_model.axis_table(100, 30, filter)[2]
    assert ks.value == want.shape[1]
    xmin, count = np.zeros(30, np.int32), np.zeros(30, np.int32)
    wide = np.full((30, ks.value + 3), -1, np.int32)
    assert lib.mj_host_resize_table_filtered(fid, 100, 30, p(xmin), p(count), p(wide), ks.value + 3, None) == B.MJ_OK
    assert np.array_equal(wide[:, :ks.value], want) and not wide[:, ks.value:].any()
    assert lib.mj_host_resize_table_filtered(fid, 100, 30, p(xmin), p(count), p(wide), ks.value - 1, None) == B.MJ_ERR_INVALID
    for i, o in ((0, 5), (5, 0), (70000, 5), (5, 70000)):
        assert lib.mj_host_resize_table_filtered(fid, i, o, None, None, None, 0, ctypes.byref(ks)) == B.MJ_ERR_INVALID


def test_unknown_filters_are_refused(lib):
    from pyjpegdecoder_amd import _binding as B
    ks = ctypes.c_int32()
    for bad in (-1, 5, 6, 1 << 20):
        assert lib.mj_host_resize_table_filtered(bad, 100, 30, None, None, None, 0, ctypes.byref(ks)) == B.MJ_ERR_INVALID
    for bad in ("nearest", "cubic", 5, -1, True, 2.0):
        with pytest.raises(ValueError, match="filter"):
            B.resize_table(100, 30, bad)
    assert [B.MJ_FILTER_BILINEAR, B.MJ_FILTER_BOX, B.MJ_FILTER_HAMMING, B.MJ_FILTER_BICUBIC, B.MJ_FILTER_LANCZOS] == [0, 1, 2, 3, 4]
    header = (ROOT / "include" / "mijpeg.h").read_text()
    for name, value in (("BILINEAR", 0), ("BOX", 1), ("HAMMING", 2), ("BICUBIC", 3), ("LANCZOS", 4)):
        assert any(line.split() == ["#define", f"MJ_FILTER_{name}", str(value)] for line in header.splitlines()), name


def test_taps_stay_inside_what_the_kernels_arithmetic_holds(lib):
    """Every table for source and output sizes 1..129, every filter.  The unsigned kernel instances (bilinear, box, hamming)
    need taps >= 0 and below 2^24 and 2^21 + 255 * sum(tap) below 2^32; the signed ones (bicubic, Lanczos) |tap| < 2^23 and
    2^21 + 255 * sum |tap| <= 2^31 - 1.  Measured over these sizes, in units of 2^22 for the taps and of 2^31 for the sums:
        bilinear  largest tap 1.000000   least tap 0          largest sum 0.4990
        box       largest tap 1.000000   least tap 0          largest sum 0.4990
        hamming   largest tap 1.000000   least tap 0          largest sum 0.4990
        bicubic   largest |tap| 1.124495 least tap -522169    largest sum 0.6329
        lanczos   largest |tap| 1.283256 least tap -1188062   largest sum 0.7836
    (the sums of the first three are 255 * (2^22 + rounding) + 2^21).  Plan creation makes the same check for every table it builds and refuses a plan whose table breaks a bound."""
    from pyjpegdecoder_amd import _binding as B
    N = 129
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    xmin, count = np.zeros(N, np.int32), np.zeros(N, np.int32)
    buf = np.zeros(N * (3 * N * 2 + 3), np.int32)
    ks = ctypes.c_int32()
    seen = {}
    for filter in FILTERS:
        fid = B.FILTERS[filter]
        big = least = top = 0
        for i in range(1, N + 1):
            for o in range(1, N + 1):
                assert lib.mj_host_resize_table_filtered(fid, i, o, None, None, None, 0, ctypes.byref(ks)) == B.MJ_OK
                assert lib.mj_host_resize_table_filtered(fid, i, o, p(xmin), p(count), p(buf), ks.value, None) == B.MJ_OK
                t = buf[:o * ks.value].reshape(o, ks.value).astype(np.int64)
                mag = np.abs(t)
                big, least = max(big, int(mag.max())), min(least, int(t.min()))
                top = max(top, (1 << 21) + 255 * int(mag.sum(axis=1).max()))
        seen[filter] = (round(big / (1 << 22), 6), least, round(top / (1 << 31), 4))
        if filter in ("bicubic", "lanczos"):
            assert least < 0 and big < (1 << 23) and top <= (1 << 31) - 1, (filter, seen[filter])
        else:
            assert least >= 0 and big < (1 << 24) and top <= (1 << 32) - 1, (filter, seen[filter])
    print(seen)


def test_resample_argument_checks_need_no_gpu():
    """What decode / decode_device / decode_device_iter accept as resample=, as the plain function they call."""
    from pyjpegdecoder_amd.batch import _Request, normalize_resample
    size = (8, 8)
    for same in (None, "bilinear", "BILINEAR", "Bilinear", 2, np.int64(2)):
        assert normalize_resample(same, size) is None
    for name, number in (("lanczos", 1), ("bicubic", 3), ("box", 4), ("hamming", 5)):
        for given in (name, name.upper(), name.capitalize(), number, np.int32(number)):
            assert normalize_resample(given, size) == name, given
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert normalize_resample(Image.Resampling.BILINEAR, size) is None and normalize_resample(Image.BILINEAR, size) is None
        for name in ("lanczos", "bicubic", "box", "hamming"):
            assert normalize_resample(getattr(Image.Resampling, name.upper()), size) == name
        with pytest.raises(ValueError, match="not a convolution"):
            normalize_resample(Image.Resampling.NEAREST, size)
    for nearest in ("nearest", "NEAREST", 0, np.int64(0)):
        with pytest.raises(ValueError, match="not a convolution.*affine transform.*not offered"):
            normalize_resample(nearest, size)
    for junk in ("cubic", "", 6, -1, 2.0, True, False, (3,), b"box", object()):
        with pytest.raises(ValueError, match="resample must be one of"):
            normalize_resample(junk, size)
    for given in ("bicubic", "bilinear", 2, "junk", 0):          # without size: refused whatever it is, as dtype= is
        with pytest.raises(ValueError, match="resample needs size"):
            normalize_resample(given, None)
    assert normalize_resample(None, None) is None
    # the filter travels with the request; a bilinear request is the request of a call without the argument
    req = _Request([b"a", b"b", b"c"], None, size, resample="lanczos")
    assert req.narrow([2, 0]).resample == "lanczos" and req.narrow([1]).plan_kwargs()["filter"] == "lanczos"
    plain = _Request([b"a", b"b"], None, size, resample=normalize_resample("bilinear", size))
    assert plain == _Request([b"a", b"b"], None, size) and "filter" not in plain.plan_kwargs()
    assert plain.narrow([1]).plan_kwargs() == _Request([b"b"], None, size, index=[1]).plan_kwargs()


def test_new_entry_points_are_exported_and_declared_as_c(lib, tmp_path):
    from pyjpegdecoder_amd import _binding as B
    for name in ("mj_host_resize_table_filtered", "mj_debug_resize_shape"):
        assert name in B.EXPORTS and hasattr(lib, name), name
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    # the prototypes the binding assumes, assigned from the header's declarations (a mismatch is a compile error)
    src = tmp_path / "proto.c"
    src.write_text("""
#include "mijpeg.h"
int main(void) {
  int (*a)(int32_t, int32_t, int32_t, int32_t *, int32_t *, int32_t *, int32_t, int32_t *) = mj_host_resize_table_filtered;
  int (*c)(const mj_plan *, int32_t *) = mj_debug_resize_shape;
  int filters[MJ_FILTER_BILINEAR == 0 && MJ_FILTER_LANCZOS == 4 ? 1 : -1] = {MJ_FILTER_BOX + MJ_FILTER_HAMMING + MJ_FILTER_BICUBIC};
  (void)a; (void)c; (void)filters;
  return 0;
}
""")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-c", str(src), "-o", str(tmp_path / "proto.o")],
                   check=True)
    # without a context nothing is created and nothing crashes: an unknown filter and a missing context are both refused
    h = ctypes.c_void_p()
    from routes_common import create_with
    assert create_with(lib, None, None, h, out_width=8, out_height=8, filter=7) == B.MJ_ERR_INVALID
    assert create_with(lib, None, None, h, out_width=8, out_height=8, filter=B.MJ_FILTER_LANCZOS) == B.MJ_ERR_INVALID
    assert lib.mj_debug_resize_shape(None, (ctypes.c_int32 * 8)()) == B.MJ_ERR_INVALID
