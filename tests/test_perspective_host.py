"""The perspective transform on the host (no GPU): tools/perspective_model.py — the statement of Pillow's Image.transform(size,
PERSPECTIVE, ..) — against Pillow itself, the library's host twin mj_host_perspective against the model (windows, the 0 / 0 pixel and
component changes included), perspective_coeffs against torchvision's corner rule, and the request: batch.normalize_perspective, the
binding's structures against the header, and the checks and the default rule through mj_debug_normalise_request."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

FILTERS = ("nearest", "bilinear", "bicubic")
GOLDEN_FILES = ("70x50_420_pil_opt", "48x80_440", "100x36_411_dri3", "64x64_grey_pil")
IDENT = (1, 0, 0, 0, 1, 0, 0, 0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


def images():
    """(name, row-major uint8 image): two random ones and the golden files' recorded pixels"""
    rng = np.random.default_rng(2200)
    out = [("rgb48x40", rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)), ("l21x33", rng.integers(0, 256, (33, 21), dtype=np.uint8))]
    for name in GOLDEN_FILES:
        rgb = np.load(GOLDEN / "files" / f"{name}.npz")["rgb"]          # (x-major: width, height[, C])
        out.append((name, np.ascontiguousarray(rgb.transpose(1, 0, 2) if rgb.ndim == 3 else rgb.T)))
    return out


def keystone(w, h):
    from tools import perspective_model as pm
    return pm.coeffs(pm.corners(w, h), [(0.1 * w, 0.15 * h), (0.95 * w, 0.05 * h), (0.85 * w, 0.9 * h), (0.05 * w, 0.8 * h)])


def coefficient_sets(w, h):
    """(name, coefficients) for a w x h image"""
    from tools import perspective_model as pm
    return [("identity", IDENT),
            ("affine only", (1.1, 0.1, -3, 0.05, 0.9, 2, 0, 0)),
            ("mild keystone", (1, 0, 0, 0, 1, 0, 0.002, 0.001)),
            ("strong keystone", keystone(w, h)),
            ("flip with perspective", (-1, 0, w, 0, 1, 0, 0.004, 0.002)),
            ("zoom out", (3, 0, -w, 0, 3, -h, 0.001, 0)),
            ("pole inside the frame", (1, 0, 0, 0, 1, 0, -0.05, 0)),
            ("pole on a column of pixel centres", (1, 0, 0, 0, 1, 0, -1 / 20.5, 0)),
            ("1e300", (1e300, 0, 0, 0, 1e300, 0, 0, 0)),
            ("1e300 in the denominator", (1, 0, 0, 0, 1, 0, 1e300, -1e300)),
            ("torchvision corners", pm.coeffs(pm.corners(w, h), [(3, 2), (w - 5, 1), (w - 2, h - 4), (1, h - 2)]))]


def fill_of(img):
    return (7, 99, 200) if img.ndim == 3 else 55


def cases():
    """(image's name, image, set's name, coefficients, window): the image's own size, and an output larger than the source"""
    for name, img in images():
        h, w = img.shape[:2]
        for cname, c in coefficient_sets(w, h):
            for window in ((0, 0, w, h), (0, 0, w + 9, h + 7)):
                yield name, img, cname, c, window


# ---- the model is Pillow; the host twin is the model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", FILTERS)
def test_model_is_pillows_perspective_transform(resample):
    Image = pytest.importorskip("PIL.Image")
    from tools import perspective_model as pm
    n, fills = 0, {}
    for name, img, cname, c, window in cases():
        want = np.asarray(Image.fromarray(img).transform(window[2:], Image.PERSPECTIVE, c, getattr(Image.Resampling, resample.upper()), fillcolor=fill_of(img)))
        got = pm.transform(img, c, resample, fill_of(img), window=window)
        assert np.array_equal(got, want), (resample, name, cname, window)
        fills[cname] = max(fills.get(cname, 0.0), pm.fill_share(img, c))
        n += 1
    assert n == 6 * 11 * 2
    # the sets are what their names say: nothing, most, and — at a pole inside the frame — a good part of the frame is fill
    assert fills["identity"] == 0.0 and fills["zoom out"] > 0.8 and fills["pole inside the frame"] > 0.5 and fills["1e300"] > 0.9


def test_a_pole_inside_the_frame_has_source_pixels_on_both_sides():
    """the denominator changes sign inside the frame; Pillow's answer is defined on both sides, and at a pixel centre ON the pole
    (x + 0.5 == 20.5: d == 0 exactly) the coordinates are infinite, hence fill"""
    Image = pytest.importorskip("PIL.Image")
    from tools import perspective_model as pm
    img = np.random.default_rng(3).integers(1, 256, (40, 48), dtype=np.uint8)
    c = (1, 0, 0, 0, 1, 0, -1 / 20.5, 0)
    X, Y = np.meshgrid(np.arange(48), np.arange(40))
    xin, yin = pm.source_coords(c, X, Y)
    assert np.isinf(xin[:, 20]).all() and (xin[:, :20] > 0).all() and (xin[:, 21:] < 0).all()
    got = pm.transform(img, c, "bilinear", 0)
    assert (got[:, 20] == 0).all() and (got[:, :5] != 0).any()
    assert np.array_equal(got, np.asarray(Image.fromarray(img).transform((48, 40), Image.PERSPECTIVE, c, Image.Resampling.BILINEAR, fillcolor=0)))
    # a negative denominator that maps back INTO the image: the source is sampled beyond the pole, as Pillow samples it
    c = (-1, 0, 0, 0, -1, 0, -1 / 10.25, 0)
    share = pm.fill_share(img, c)
    assert 0.0 < share < 1.0
    xin, _ = pm.source_coords(c, X, Y)
    d = -1 / 10.25 * (X + 0.5) + 1
    assert ((d < 0) & (xin >= 0) & (xin < 48)).any()
    for resample in FILTERS:
        want = np.asarray(Image.fromarray(img).transform((48, 40), Image.PERSPECTIVE, c, getattr(Image.Resampling, resample.upper()), fillcolor=9))
        assert np.array_equal(pm.transform(img, c, resample, 9), want), resample


@pytest.mark.parametrize("kind", ("444", "grey"))
def test_bicubic_keystone_of_the_checker_clamps_at_both_ends(lib, kind):
    Image = pytest.importorskip("PIL.Image")
    from pyjpegdecoder_amd import _binding as B
    from tools import perspective_model as pm
    img = np.asarray(Image.open(GOLDEN / "affine" / f"checker_48x40_{kind}.jpg"))
    c, fill = keystone(48, 40), (fill_of(img))
    want = np.asarray(Image.fromarray(img).transform((48, 40), Image.PERSPECTIVE, c, Image.Resampling.BICUBIC, fillcolor=fill))
    got = pm.transform(img, c, "bicubic", fill)
    assert np.array_equal(got, want) and np.array_equal(B.perspective(img, c, "bicubic", fill), got)
    X, Y = np.meshgrid(np.arange(48), np.arange(40))
    xin, yin = pm.source_coords(c, X, Y)
    inside = (xin >= 0) & (xin < 48) & (yin >= 0) & (yin < 40)
    assert (got[inside] == 0).any() and (got[inside] == 255).any()
    # ... and the clamps are clamps: the bilinear result, which cannot overshoot, has neither value there more often
    lin = pm.transform(img, c, "bilinear", fill)
    assert (got[inside] == 0).sum() > (lin[inside] == 0).sum() and (got[inside] == 255).sum() > (lin[inside] == 255).sum()


@pytest.mark.parametrize("resample", FILTERS)
def test_host_twin_is_the_model(lib, resample):
    from pyjpegdecoder_amd import _binding as B
    from tools import perspective_model as pm
    for name, img, cname, c, window in cases():
        want = pm.transform(img, c, resample, fill_of(img), window=window)
        got = B.perspective(img, c, resample, fill_of(img), window=window)
        assert got.shape == want.shape and np.array_equal(got, want), (resample, name, cname, window)


@pytest.mark.parametrize("resample", FILTERS)
def test_a_window_is_the_transform_at_the_windows_absolute_coordinates(lib, resample):
    from pyjpegdecoder_amd import _binding as B
    from tools import perspective_model as pm
    for name, img in images()[:3]:
        h, w = img.shape[:2]
        for cname, c in coefficient_sets(w, h)[2:8]:
            whole = pm.transform(img, c, resample, fill_of(img))
            # the four corners of the frame, and one in the middle
            for x, y, ww, wh in ((0, 0, 7, 5), (w - 6, 0, 6, 9), (0, h - 4, 11, 4), (w - 9, h - 8, 9, 8), (3, 7, 11, 13)):
                want = whole[y:y + wh, x:x + ww]
                assert np.array_equal(pm.transform(img, c, resample, fill_of(img), window=(x, y, ww, wh)), want), (name, cname, x, y)
                assert np.array_equal(B.perspective(img, c, resample, fill_of(img), window=(x, y, ww, wh)), want), (name, cname, x, y)


@pytest.mark.parametrize("resample", FILTERS)
def test_zero_over_zero_is_fill(lib, resample):
    """c = (0,0,0, 0,1,0, -2,0): in column 0 the numerator of xin and the denominator are both zero — NaN, which Pillow's C converts
    to an int (undefined); the library and the model make that pixel fill.  The other columns are ordinary (xin == 0)."""
    from pyjpegdecoder_amd import _binding as B
    from tools import perspective_model as pm
    img = np.random.default_rng(4).integers(1, 256, (10, 12, 3), dtype=np.uint8)
    c = (0, 0, 0, 0, 1, 0, -2, 0)
    xin, yin = pm.source_coords(c, *np.meshgrid(np.arange(12), np.arange(10)))
    assert np.isnan(xin[:, 0]).all() and np.isinf(yin[:, 0]).all() and not np.isnan(xin[:, 1:]).any()
    got = B.perspective(img, c, resample, (7, 99, 200))
    assert np.array_equal(got, pm.transform(img, c, resample, (7, 99, 200)))
    assert (got[:, 0] == np.array((7, 99, 200), np.uint8)).all()


def test_host_twin_refuses_what_the_request_refuses(lib):
    from pyjpegdecoder_amd import _binding as B
    img = np.zeros((8, 8, 3), np.uint8)
    assert B.perspective(img, IDENT, "nearest").shape == (8, 8, 3)
    for bad in ((1, 0, float("nan"), 0, 1, 0, 0, 0), (1, 0, 0, 0, 1, 0, float("inf"), 0)):
        with pytest.raises(ValueError, match="mj_host_perspective"):
            B.perspective(img, bad, "bilinear")
    for filt in (0, 4, 9, 0x11):
        with pytest.raises(ValueError, match="mj_host_perspective"):
            B.perspective(img, IDENT, filt)
    for window in ((0, 0, 0, 4), (-1, 0, 4, 4), (32760, 0, 8, 8)):
        with pytest.raises(ValueError, match="mj_host_perspective"):
            B.perspective(img, IDENT, "nearest", window=window)
    # no magnitude is refused
    from tools import perspective_model as pm
    img = np.random.default_rng(5).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    for huge in ((1e300, 0, -1e300, 0, 1e300, 0, 1e300, 1e300), (1e308, 1e308, 0, 0, 1e308, 0, 0, 0), (1, 0, 0, 0, 1, 0, -1e308, -1e308)):
        assert np.array_equal(B.perspective(img, huge, "bicubic", 5), pm.transform(img, huge, "bicubic", 5)), huge


@pytest.mark.parametrize("resample", FILTERS)
def test_the_model_of_a_call_converts_then_orients_then_transforms(lib, resample):
    """3 -> 1 and 1 -> 3: the kernel converts every tap where it fetches (mj_host_perspective has the file's components in and out,
    so the conversions are held on the model's side: transform(convert(img)) is what a tap-wise conversion gives, since convert is
    per pixel) — and the host twin agrees on both sides of the conversion"""
    from pyjpegdecoder_amd import _binding as B
    from tools import mode_model
    from tools import perspective_model as pm
    (_, rgb), (_, grey) = images()[:2]
    for img, mode in ((rgb, "L"), (grey, "RGB")):
        h, w = img.shape[:2]
        c = keystone(w, h)
        conv = mode_model.convert(img, mode)
        fill = fill_of(conv)
        want = pm.expected(img, c, None, (w, h), resample=resample, affine_fill=fill, mode=mode, filter="box")
        # (a box resize to the image's own size is the identity: the expected bytes are the transformed image's)
        assert np.array_equal(want, pm.transform(conv, c, resample, fill))
        assert np.array_equal(B.perspective(conv, c, resample, fill), want)


# ---- perspective_coeffs ---------------------------------------------------------------------------------------------------------------
def test_perspective_coeffs_map_the_end_points_to_the_start_points():
    """750 corner draws by torchvision's get_params rule: every end point maps to its start point within 1e-9 of a pixel (the
    worst seen was 3.6e-12; the bound leaves two orders of magnitude for another LAPACK), and at distortion 0.9 some draw has a
    non-positive denominator at a corner of the output — the pole case is in the set"""
    from pyjpegdecoder_amd import perspective_coeffs
    from tools import perspective_model as pm
    rng = np.random.default_rng(750)
    n, worst, poles = 0, 0.0, 0
    for (w, h) in ((70, 50), (64, 64), (100, 36), (48, 80), (1920, 1080)):
        for scale in (0.3, 0.5, 0.9):
            for _ in range(50):
                start, end = pm.get_params(w, h, scale, rng)
                c = perspective_coeffs(start, end)
                assert c == pm.coeffs(start, end) and len(c) == 8 and all(isinstance(v, float) for v in c)
                for (sx, sy), (ex, ey) in zip(start, end):
                    d = c[6] * ex + c[7] * ey + 1
                    worst = max(worst, abs((c[0] * ex + c[1] * ey + c[2]) / d - sx), abs((c[3] * ex + c[4] * ey + c[5]) / d - sy))
                if scale == 0.9:
                    poles += any(c[6] * (x + 0.5) + c[7] * (y + 0.5) + 1 <= 0 for x in (0, w - 1) for y in (0, h - 1))
                n += 1
    print(f"perspective_coeffs: {n} draws, worst end point error {worst:.3g} pixels, {poles} draws at 0.9 with a pole inside the frame")
    assert n == 750 and worst < 1e-9
    assert poles >= 1


def test_perspective_coeffs_refusals():
    from pyjpegdecoder_amd import perspective_coeffs
    sq = [(0, 0), (9, 0), (9, 9), (0, 9)]
    got = perspective_coeffs(sq, sq)
    assert np.allclose(got, IDENT, atol=1e-12)
    for bad in (None, sq[:3], [(0, 0, 0)] * 4, [(0, "1")] * 4, [(0, float("nan"))] * 4, [(0, True)] * 4):
        with pytest.raises(ValueError, match="must be four"):
            perspective_coeffs(bad, sq)
        with pytest.raises(ValueError, match="must be four"):
            perspective_coeffs(sq, bad)
    with pytest.raises(ValueError, match="determine no perspective transform"):
        perspective_coeffs(sq, [(0, 0)] * 4)


# ---- the arguments ---------------------------------------------------------------------------------------------------------------------
def test_normalize_perspective():
    from pyjpegdecoder_amd.batch import AffineSpec, normalize_perspective, normalize_transform
    c = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.001, 0.0)
    assert normalize_perspective(None, None, None, (8, 8), 2) is None
    assert normalize_perspective([None, None], None, None, (8, 8), 2) is None
    spec = normalize_perspective(c, None, None, (8, 8), 2)
    assert spec == AffineSpec([c, c], "nearest", (0,), True)
    spec = normalize_perspective([None, list(c)], "BiCubic", (1, 2, 3), (8, 8), 2, ncomp=3)
    assert spec == AffineSpec([None, c], "bicubic", (1, 2, 3), True)
    assert normalize_perspective(np.array(c), 2, 9, (8, 8), 1, ncomp=3) == AffineSpec([c], "bilinear", (9, 9, 9), True)
    assert normalize_perspective(c, "nearest", 3, (8, 8), None).matrices == []         # (what needs no file)
    assert normalize_transform(None, c, None, None, (8, 8), 1).perspective
    assert not normalize_transform((1, 0, 0, 0, 1, 0), None, None, None, (8, 8), 1).perspective
    assert normalize_transform(None, None, None, None, (8, 8), 1) is None


def test_normalize_perspective_refusals():
    from pyjpegdecoder_amd.batch import AffineSpec, check_affine, normalize_affine, normalize_perspective, normalize_transform, perspective_fault
    with pytest.raises(ValueError, match=r"perspective needs size=\(width, height\)"):
        normalize_perspective(IDENT, None, None, None, 1)
    with pytest.raises(ValueError, match="perspective and return_seams do not go together"):
        normalize_perspective(IDENT, None, None, (8, 8), 1, return_seams=True)
    with pytest.raises(ValueError, match="perspective and reducing_gap do not go together yet"):
        normalize_perspective(IDENT, None, None, (8, 8), 1, reducing_gap=2.0)
    with pytest.raises(ValueError, match="affine and perspective do not go together"):
        normalize_transform((1, 0, 0, 0, 1, 0), IDENT, None, None, (8, 8), 1)
    with pytest.raises(ValueError, match="perspective has 2 entries for 3 outputs"):
        normalize_perspective([IDENT, None], None, None, (8, 8), 3)
    for bad in (3, "keystone", (1, 0, 0, 0, 1, 0), (1, 0, 0, 0, 1, 0, 0), [(1, 0, 0, 0, 1, 0, 0, "0")], [IDENT, 5], (1, 0, 0, 0, True, 0, 0, 0),
                (1, 0, 0, 0, 1, 0, 0, 0, 0)):
        with pytest.raises(ValueError, match="perspective must be None, one sequence"):
            normalize_perspective(bad, None, None, (8, 8), 2)
    for bad in (float("nan"), float("inf"), -float("inf")):         # (reported with the output's file: check_affine's)
        spec = normalize_perspective([IDENT, (1, 0, 0, 0, 1, 0, bad, 0)], None, None, (8, 8), 2)
        with pytest.raises(ValueError, match=r"perspective: output 1 \(file 7\): a coefficient is not finite"):
            check_affine(spec, [(0, None), (1, None)], [(64, 64), (20, 30)], index=[5, 7])
    with pytest.raises(ValueError, match="perspective: output 0: coefficients that are all zero"):
        normalize_perspective([(0,) * 8], None, None, (8, 8), 1)
    with pytest.raises(ValueError, match="affine_resample must be one of nearest, bilinear, bicubic"):
        normalize_perspective(IDENT, "lanczos", None, (8, 8), 1)
    with pytest.raises(ValueError, match="affine_fill has 3 bytes for outputs of 1 component"):
        normalize_perspective(IDENT, None, (1, 2, 3), (8, 8), 1, ncomp=1)
    # against the images: a side of 32768 or more — and nothing else: no magnitude is refused
    from tools import perspective_model as pm
    assert perspective_fault(IDENT, 32768, 30) == pm.fault(IDENT, 32768, 30) == "an image with a side of 32768 or more"
    assert perspective_fault((1e300, 0, -1e300, 0, 1, 0, 1e300, 0), 20, 30) is None and pm.fault((1e300,) * 8, 20, 30) is None
    with pytest.raises(ValueError, match=r"perspective: output 1 \(file 7\): an image with a side of 32768 or more"):
        check_affine(AffineSpec([None, IDENT], "nearest", (0,), True), [(0, (0, 0, 4, 4)), (1, (0, 0, 4, 4))], [(64, 64), (30, 32768)], index=[5, 7])
    # the affine messages keep matching their pinned patterns
    with pytest.raises(ValueError, match="affine_resample and affine_fill need affine"):
        normalize_affine(None, "bilinear", None, (8, 8), 1)
    with pytest.raises(ValueError, match="affine_resample and affine_fill need affine"):
        normalize_perspective(None, None, 3, (8, 8), 1)
    with pytest.raises(ValueError, match=r"affine needs size=\(width, height\)"):
        normalize_transform((1, 0, 0, 0, 1, 0), None, None, None, None, 1)
    with pytest.raises(ValueError, match="affine and reducing_gap do not go together yet"):
        normalize_transform((1, 0, 0, 0, 1, 0), None, None, None, (8, 8), 1, reducing_gap=2.0)
    with pytest.raises(ValueError, match="affine must be None, one matrix"):
        normalize_transform(IDENT[:5], None, None, None, (8, 8), 1)


def test_narrow_takes_the_coefficients_with_the_views():
    from pyjpegdecoder_amd.batch import AffineSpec, _Request
    c1, c2 = (1, 0, 1, 0, 1, 0, 0.001, 0), (1, 0, 2, 0, 1, 0, 0, 0.002)
    req = _Request([b"a", b"b"], None, (8, 8), None, None, [0, 1, 2], None, None, views=[(1, (0, 0, 1, 1)), (0, (0, 0, 2, 2)), (1, (0, 0, 3, 3))],
                   affine=AffineSpec([c1, None, c2], "bilinear", (1, 2, 3), True))
    sub = req.narrow([1])
    assert sub.affine.matrices == [c1, c2] and sub.affine.perspective and sub.slots == [0, 2]
    kw = sub.plan_kwargs(3)
    assert kw["perspective"] == ([c1, c2], "bilinear", (1, 2, 3)) and "affine" not in kw
    none = req.narrow([0])
    assert none.affine is None and "perspective" not in none.plan_kwargs(3) and "affine" not in none.plan_kwargs(3)


# ---- the request: structures and mj_debug_normalise_request -----------------------------------------------------------------------------
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


def test_the_request_with_a_perspective_transform_is_laid_out_as_the_binding_assumes(lib, tmp_path):
    from pyjpegdecoder_amd import _binding as B
    gcc = shutil.which("gcc")
    assert gcc is not None, "the header is held to a C compiler"
    flags = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include")]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(
        ['#include <stdio.h>', '#include <stddef.h>', '#include "mijpeg.h"', 'int main(void) {', '  mj_plan_request zeroed = {0};',
         '  printf("%zu", sizeof(mj_perspective));',
         '  printf(" %d\\n", zeroed.perspective == 0 && zeroed.affine == 0 && zeroed.transform_filter == 0);', '  return 0;', '}']))
    exe = tmp_path / "layout"
    subprocess.run([gcc] + flags + [str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(B.PerspectiveC), 1] and got[0] == 64
    # (the request's own layout, `perspective` included: test_plan_request_host)
    # plan_request: the filter, the fill bytes, the coefficients (None: all zero), one per output; the matrices' pointer stays NULL
    c = (0.5, 0.25, 3.0, -0.25, 0.5, 1.5, 0.001, -0.002)
    r, keep = B.plan_request(2, size=(24, 16), perspective=([c, None], "bicubic", (7, 99, 200)))
    assert r.transform_filter == B.MJ_AFFINE_BICUBIC and tuple(r.transform_fill) == (7, 99, 200) and r.n_views == 0
    assert tuple(r.perspective[0].a) == c and tuple(r.perspective[1].a) == (0.0,) * 8 and not r.affine and not r.colour
    r, keep = B.plan_request(2, size=(24, 16), views=[(1, None), (0, (1, 1, 4, 4)), (1, None)], perspective=([c, None, c], "nearest", (5,)),
                             colour=[None, [("invert",)], None])
    assert r.n_views == 3 and r.transform_filter == B.MJ_AFFINE_NEAREST and tuple(r.transform_fill) == (5, 0, 0)
    assert r.views[1].window.width == 4 and r.colour[1].n == 1 and r.mode == 0
    with pytest.raises(ValueError, match="perspective: 1 entries, not one for each of the 2 images"):
        B.plan_request(2, size=(24, 16), perspective=([c], "nearest", (0,)))
    with pytest.raises(ValueError, match="perspective: 2 entries, not one for each of the 3 views"):
        B.plan_request(2, size=(24, 16), views=[(0, None), (1, None), (0, None)], perspective=([c, c], "nearest", (0,)))
    with pytest.raises(ValueError, match="perspective needs size"):
        B.plan_request(2, perspective=([c, c], "nearest", (0,)))
    with pytest.raises(ValueError, match="affine and perspective do not go together"):
        B.plan_request(2, size=(24, 16), perspective=([c, c], "nearest", (0,)), affine=([None, None], "nearest", (0,)))
    header = (ROOT / "include" / "mijpeg.h").read_text()
    assert "const mj_perspective *perspective;" in header
    assert "mj_host_perspective" in B.EXPORTS and hasattr(lib, "mj_host_perspective")


def test_no_transform_is_the_zeroed_request(lib):
    """None and lists of None make the byte-identical request of a call without the argument — in Python — and all-zero
    coefficients normalise to the field's absence in the library"""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import _Request, normalize_perspective
    plain = _Request([b"a", b"b"], None, (24, 16))
    for persp in (None, [None, None]):
        req = _Request([b"a", b"b"], None, (24, 16), affine=normalize_perspective(persp, None, None, (24, 16), 2))
        a, _ = B.plan_request(2, **req.plan_kwargs(3))
        b, _ = B.plan_request(2, **plain.plan_kwargs(3))
        assert bytes(a) == bytes(b) and req.plan_kwargs(3) == plain.plan_kwargs(3)
    batch, keep = _batch([(128, 64), (50, 70)])
    rc, out, msg = _normal(lib, batch, perspective=([None, None], "bilinear", (1, 2, 3)))
    assert rc == B.MJ_OK and not out.affine and not out.perspective and out.transform_filter == 0 and bytes(out.transform_fill) == bytes(3), msg
    assert out.n_views == 0 and out.n_slots == 2
    rc, plain_out, _ = _normal(lib, batch)
    assert bytes(out) == bytes(plain_out)
    # a request with a transform: its windows, or whole images, become one view per image; the array stays the caller's
    c = (0.9, 0.3, -2.0, -0.3, 0.9, 4.0, 0.001, 0.0)
    rc, out, msg = _normal(lib, batch, perspective=([c, None], "bilinear", (1, 2, 3)))
    assert rc == B.MJ_OK and bool(out.perspective) and not out.affine and out.transform_filter == 2 and tuple(out.transform_fill) == (1, 2, 3), msg
    assert out.n_views == 2 and out.n_slots == 2 and not out.rois and not out.views
    rc, out, msg = _normal(lib, batch, perspective=([c, c], "nearest", (0,)), rois=[(1, 1, 4, 4), (0, 0, 50, 70)])
    assert rc == B.MJ_OK and out.n_views == 2 and not out.rois, msg
    rc, out, msg = _normal(lib, batch, perspective=([c, None, c], "bicubic", (0,)), views=[(1, None), (0, (1, 1, 4, 4)), (1, None)])
    assert rc == B.MJ_OK and out.n_views == 3 and out.n_slots == 3, msg
    # no magnitude is refused
    rc, out, msg = _normal(lib, batch, perspective=([(1e300, 0, 0, 0, 1e300, 0, -1e300, 0), c], "nearest", (0,)))
    assert rc == B.MJ_OK, msg


def test_request_refusals(lib):
    from pyjpegdecoder_amd import _binding as B
    batch, keep = _batch([(128, 64), (50, 70)])
    c = (0.9, 0.3, -2.0, -0.3, 0.9, 4.0, 0.001, -0.001)
    ok = ([c, c], "bilinear", (0,))
    rc, _, msg = _normal(lib, batch, perspective=ok, size=None)
    assert rc == B.MJ_ERR_INVALID and "perspective needs a size" in msg
    rc, _, msg = _normal(lib, batch, perspective=ok, reducing_gap=2.0)
    assert rc == B.MJ_ERR_INVALID and "perspective and reducing_gap do not go together yet" in msg
    for bad_filter in (9, 4, 0):
        rc, _, msg = _normal(lib, batch, perspective=([c, c], bad_filter, (0,)))
        assert rc == B.MJ_ERR_INVALID and f"affine: filter {bad_filter} is none of MJ_AFFINE_*" in msg
    for good in (1, 2, 3):
        assert _normal(lib, batch, perspective=([c, c], good, (0,)))[0] == B.MJ_OK
    rc, _, msg = _normal(lib, batch, perspective=ok, rois=[(1, 1, 4, 4), (0, 0, 51, 70)])
    assert rc == B.MJ_ERR_INVALID and "view 1: window" in msg
    for bad in (float("nan"), float("inf")):
        for at in (2, 6):
            cc = list(c)
            cc[at] = bad
            rc, _, msg = _normal(lib, batch, perspective=([c, tuple(cc)], "nearest", (0,)))
            assert rc == B.MJ_ERR_INVALID and "perspective: output 1: a coefficient is not finite" in msg, msg
    big, keep_big = _batch([(128, 64), (40000, 8)])
    rc, _, msg = _normal(lib, big, perspective=ok)
    assert rc == B.MJ_ERR_INVALID and "perspective: output 1: an image with a side of 32768 or more" in msg
    rc, _, msg = _normal(lib, big, perspective=ok, orientation=[1, 6])
    assert rc == B.MJ_ERR_INVALID and "perspective: output 1: an image with a side of 32768 or more" in msg
    r, keep_r = B.plan_request(2, size=(24, 16), perspective=ok)
    r.perspective = None                                        # (the filter without an array)
    out = B.PlanRequestC()
    assert lib.mj_debug_normalise_request(ctypes.byref(batch), ctypes.byref(r), ctypes.byref(out)) == B.MJ_ERR_INVALID
    assert "transform_filter / transform_fill without an array" in lib.mj_last_error(None).decode()
    # both arrays in one request
    r, keep_r = B.plan_request(2, size=(24, 16), perspective=ok)
    keep_a = r.affine = (B.AffineC * 2)()
    assert lib.mj_debug_normalise_request(ctypes.byref(batch), ctypes.byref(r), ctypes.byref(out)) == B.MJ_ERR_INVALID
    assert "affine and perspective do not go together" in lib.mj_last_error(None).decode()
    # the affine refusals, with their messages as they were
    m = (0.9, 0.3, -2.0, -0.3, 0.9, 4.0)
    rc, _, msg = _normal(lib, batch, affine=([m, m], "bilinear", (0,)), size=None)
    assert rc == B.MJ_ERR_INVALID and "affine needs a size" in msg
    rc, _, msg = _normal(lib, batch, affine=([m, m], "bilinear", (0,)), reducing_gap=2.0)
    assert rc == B.MJ_ERR_INVALID and "affine and reducing_gap do not go together yet" in msg
    rc, _, msg = _normal(lib, batch, affine=([m, m], 9, (0,)))
    assert rc == B.MJ_ERR_INVALID and "affine: filter 9 is none of MJ_AFFINE_*" in msg
    rc, _, msg = _normal(lib, batch, affine=([m, (1, 0, float("nan"), 0, 1, 0)], "bilinear", (0,)))
    assert rc == B.MJ_ERR_INVALID and "affine: output 1: a matrix entry is not finite" in msg
