"""Decode to a fixed size, the parts that need no GPU: the NumPy model of the resize (tools/resize_model.py) is Pillow's
Image.resize(size, Image.BILINEAR) byte for byte; the library's tap tables (mj_host_resize_table) are the model's, entry for
entry; decode(size=...) refuses bad arguments before any GPU work; the new entry points are exported and declared as plain C."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NAMED = [((1920, 1080), (224, 224)), ((1920, 1080), (640, 360)), ((640, 480), (224, 224)), ((500, 375), (256, 256)),
         ((300, 200), (1024, 768))]


def _sweep():
    """300 seeded cases: ((in_w, in_h), (out_w, out_h), channels, kind of data); sizes 1..260, shrinking and enlarging, a fifth
    with the width or the height unchanged; then the named large ones."""
    rng = np.random.default_rng(20260)
    cases = []
    for k in range(300):
        iw, ih, ow, oh = (int(v) for v in rng.integers(1, 261, 4))
        if k % 10 == 3:
            ow = iw
        if k % 10 == 7:
            oh = ih
        cases.append(((iw, ih), (ow, oh), 3 if k % 2 else 1, ("noise", "binary", "smooth")[k % 3]))
    cases += [(i, o, 3, "noise") for i, o in NAMED]
    return cases


def _data(rng, w, h, c, kind):
    shape = (h, w, 3) if c == 3 else (h, w)
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (127.5 + 127.5 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.uint8)
    return np.stack([base, base[::-1], 255 - base], axis=-1) if c == 3 else base


def test_model_is_pillow_bilinear_byte_for_byte():
    Image = pytest.importorskip("PIL.Image")
    from tools import resize_model
    rng = np.random.default_rng(7)
    cases = _sweep()
    bad = []
    for (iw, ih), (ow, oh), c, kind in cases:
        a = _data(rng, iw, ih, c, kind)
        want = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))
        got = resize_model.resize(a, (ow, oh))
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append(((iw, ih), (ow, oh), c, kind))
    assert len(cases) == 305
    assert not bad, f"{len(bad)} of {len(cases)} cases differ from Pillow, first {bad[:5]}"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


def test_library_tap_tables_are_the_models(lib):
    from pyjpegdecoder_amd import _binding as B
    from tools import resize_model
    pairs = set()
    for (iw, ih), (ow, oh), _, _ in _sweep():
        pairs.add((iw, ow))
        pairs.add((ih, oh))
    pairs |= {(1080, 224), (1920, 224), (375, 256), (7, 250), (250, 7)}
    pairs |= {(n, n) for n in (1, 2, 33, 224)} | {(n, 1) for n in (1, 2, 33, 1080)} | {(1, n) for n in (2, 33, 224)}
    for i, o in sorted(pairs):
        xmin, count, taps = B.resize_table(i, o)
        mxmin, mcount, mtaps = resize_model.axis_table(i, o)
        assert np.array_equal(xmin, mxmin), (i, o)
        assert np.array_equal(count, mcount), (i, o)
        assert taps.shape == mtaps.shape and np.array_equal(taps, mtaps), (i, o)
    # a wider row than the table needs: the tail is zeros; a narrower one is refused
    ks = ctypes.c_int32()
    assert lib.mj_host_resize_table(100, 30, None, None, None, 0, ctypes.byref(ks)) == B.MJ_OK and ks.value == 9
    xmin, count = np.zeros(30, np.int32), np.zeros(30, np.int32)
    wide = np.full((30, 12), -1, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.mj_host_resize_table(100, 30, p(xmin), p(count), p(wide), 12, None) == B.MJ_OK
    assert np.array_equal(wide[:, :9], resize_model.axis_table(100, 30)[2]) and not wide[:, 9:].any()
    assert lib.mj_host_resize_table(100, 30, p(xmin), p(count), p(wide), 8, None) == B.MJ_ERR_INVALID
    for i, o in ((0, 5), (5, 0), (70000, 5), (5, 70000)):
        assert lib.mj_host_resize_table(i, o, None, None, None, 0, ctypes.byref(ks)) == B.MJ_ERR_INVALID


def test_decode_size_argument_checks_need_no_gpu():
    """The rules decode / decode_device / decode_device_iter apply to `size` and to the files' component counts before any GPU
    work, as the plain functions they call (tests/test_resize.py raises the same through a decoder)."""
    from pyjpegdecoder_amd.batch import _image_dims, _image_info, normalize_size, one_component_count
    colour = (GOLDEN / "files" / "64x48_422_pil.jpg").read_bytes()
    grey = (GOLDEN / "files" / "50x70_grey_dri4.jpg").read_bytes()
    for bad in ((0, 5), (5, 0), (-3, 5), (5,), (5, 6, 7), 224, "ab", (2.0, 3), (None, 3), (70000, 3), (True, 3)):
        with pytest.raises(ValueError, match="size"):
            normalize_size(bad)
    assert normalize_size(None) is None and normalize_size([np.int64(3), 4]) == (3, 4) and normalize_size((65535, 1)) == (65535, 1)
    assert _image_info(colour) == (64, 48, 3) and _image_info(grey) == (50, 70, 1)
    for name, raw in [(f.stem, f.read_bytes()) for f in sorted((GOLDEN / "files").glob("*.jpg"))]:
        assert _image_info(raw)[:2] == _image_dims(raw), name
    assert one_component_count([3, 3, 3]) == 3 and one_component_count([1]) == 1 and one_component_count([]) == 3
    for ncomps, odd in (([3, 3, 1, 3], 2), ([1, 3], 1)):
        with pytest.raises(ValueError, match=f"file {odd}"):
            one_component_count(ncomps)


def test_new_entry_points_are_exported_and_declared_as_c(lib, tmp_path):
    from pyjpegdecoder_amd import _binding as B
    names = ("mj_plan_fill_source", "mj_plan_time_resize", "mj_host_resize_table")
    for name in names:
        assert name in B.EXPORTS and hasattr(lib, name), name
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    # the prototypes the binding assumes, assigned from the header's declarations (a mismatch is a compile error); mj_roi is the
    # struct the windows of a resized plan come in
    src = tmp_path / "proto.c"
    src.write_text("""
#include <stdio.h>
#include "mijpeg.h"
int main(void) {
  int (*b)(mj_plan *, int) = mj_plan_fill_source;
  int (*c)(mj_plan *, int, uint8_t *, float *, int64_t *) = mj_plan_time_resize;
  int (*d)(int32_t, int32_t, int32_t *, int32_t *, int32_t *, int32_t, int32_t *) = mj_host_resize_table;
  (void)b; (void)c; (void)d;
  printf("%zu\\n", sizeof(mj_roi));
  return 0;
}
""")
    obj = tmp_path / "proto.o"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-c", str(src), "-o", str(obj)], check=True)
    assert ctypes.sizeof(B.RoiC) == 16
