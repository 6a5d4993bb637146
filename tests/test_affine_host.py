"""The affine transform on the host (no GPU): tools/affine_model.py — the statement of Pillow's Image.transform(size, AFFINE, ..) —
against Pillow itself, the library's host twin mj_host_affine against the model, a window of the transform, rotation_matrix against
Image.rotate, and the request: batch.normalize_affine, the binding's structures against the header, and the checks and the default
rule through mj_debug_normalise_request."""
import ctypes
import math
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FILTERS = ("nearest", "bilinear", "bicubic")
SIZES = ((23, 31), (17, 40))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


def image(w, h, C, seed=0):
    rng = np.random.default_rng(1000 * w + 10 * h + C + seed)
    return rng.integers(0, 256, (h, w, 3) if C == 3 else (h, w), dtype=np.uint8)


def matrices(w, h, n_random=10):
    """the special matrices, then random rotate + scale + shear ones about the centre"""
    out = [(1, 0, 0, 0, 1, 0), (1, 0, 0.37, 0, 1, -2.61), (1.7, 0, 0.3, 0, 0.6, 1.2), (-1, 0, w, 0, 1, 0), (0, 1, 0, 1, 0, 0),
           (1, 0, -0.5 * w, 0, 1, 0.75 * h)]
    rng = np.random.default_rng(w * h)
    for _ in range(n_random):
        th, sc, sh = rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 1.8), rng.uniform(-0.5, 0.5)
        a0, a1, a3, a4 = sc * math.cos(th), sc * (math.sin(th) + sh), -sc * math.sin(th), sc * math.cos(th)
        cx, cy = w / 2, h / 2
        out.append((a0, a1, cx - a0 * cx - a1 * cy + rng.uniform(-3, 3), a3, a4, cy - a3 * cx - a4 * cy + rng.uniform(-3, 3)))
    return out


def cases():
    """(image, matrix, output size, fill): RGB and L, sizes that are no multiple of 8, outputs of the source's size, larger, smaller"""
    for w, h in SIZES:
        for C in (3, 1):
            img = image(w, h, C)
            for m in matrices(w, h):
                for size in ((w, h), (w + 9, h + 5), (w - 6, h - 7)):
                    yield img, m, size, (7, 99, 200) if C == 3 else 55


# ---- the model is Pillow; the host twin is the model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", FILTERS)
def test_model_is_pillows_affine_transform(resample):
    Image = pytest.importorskip("PIL.Image")
    from tools import affine_model
    n = 0
    for img, m, size, fill in cases():
        want = np.asarray(Image.fromarray(img).transform(size, Image.AFFINE, m, getattr(Image.Resampling, resample.upper()), fillcolor=fill))
        got = affine_model.transform(img, m, resample, fill, window=(0, 0) + size)
        assert np.array_equal(got, want), (resample, m, size, img.shape)
        n += 1
    assert n == 2 * 2 * 16 * 3


def test_fix_rounds_to_nearest_as_pillow_does_for_negative_values():
    """the 16.16 form of NEAREST: a matrix whose entries are negative and lie near the middle between two fixed-point values —
    truncating v * 65536 + 0.5 toward zero gives another A there, floor gives Pillow's"""
    Image = pytest.importorskip("PIL.Image")
    from tools import affine_model
    assert affine_model.fix(-0.75 / 65536) == -1 and affine_model.fix(-0.25 / 65536) == 0 and affine_model.fix(-1.5 / 65536) == -1
    assert affine_model.fix(0.5 / 65536) == 1 and affine_model.fix(-0.5 / 65536) == 0
    img = image(23, 31, 3)
    rng = np.random.default_rng(5)
    for _ in range(40):
        th = rng.uniform(-math.pi, math.pi)
        m = (math.cos(th), math.sin(th), rng.uniform(-12, 12), -math.sin(th), math.cos(th), rng.uniform(-12, 12))
        want = np.asarray(Image.fromarray(img).transform((23, 31), Image.AFFINE, m, Image.Resampling.NEAREST, fillcolor=(1, 2, 3)))
        assert np.array_equal(affine_model.transform(img, m, "nearest", (1, 2, 3)), want), m


@pytest.mark.parametrize("resample", FILTERS)
def test_host_twin_is_the_model(lib, resample):
    from pyjpegdecoder_amd import _binding as B
    from tools import affine_model
    for img, m, size, fill in cases():
        want = affine_model.transform(img, m, resample, fill, window=(0, 0) + size)
        got = B.affine(img, m, resample, fill, window=(0, 0) + size)
        assert got.shape == want.shape and np.array_equal(got, want), (resample, m, size, img.shape)


@pytest.mark.parametrize("resample", FILTERS)
def test_a_window_is_the_transform_at_the_windows_absolute_coordinates(lib, resample):
    from pyjpegdecoder_amd import _binding as B
    from tools import affine_model
    for w, h in SIZES:
        img = image(w, h, 3)
        for m in matrices(w, h, 4):
            whole = affine_model.transform(img, m, resample, (7, 99, 200))
            for x, y, ww, wh in ((0, 0, 5, 4), (w - 6, h - 9, 6, 9), (3, 7, 11, 13), (w - 1, 0, 1, h)):
                want = whole[y:y + wh, x:x + ww]
                assert np.array_equal(affine_model.transform(img, m, resample, (7, 99, 200), window=(x, y, ww, wh)), want), (m, x, y)
                assert np.array_equal(B.affine(img, m, resample, (7, 99, 200), window=(x, y, ww, wh)), want), (m, x, y)


def test_host_twin_refuses_what_the_request_refuses(lib):
    from pyjpegdecoder_amd import _binding as B
    img = image(23, 31, 3)
    for bad in ((float("nan"), 0, 0, 0, 1, 0), (1, 0, float("inf"), 0, 1, 0), (1, 0, 40000, 0, 1, 0), (2000, 0, 0, 0, 1, 0)):
        with pytest.raises(ValueError, match="mj_host_affine"):
            B.affine(img, bad, "bilinear")
    with pytest.raises(ValueError, match="mj_host_affine"):
        B.affine(img, (1, 0, 0, 0, 1, 0), 7)
    with pytest.raises(ValueError, match="mj_host_affine"):
        B.affine(img, (1, 0, 0, 0, 1, 0), "nearest", window=(0, 0, 0, 4))


# ---- rotation_matrix ---------------------------------------------------------------------------------------------------------------------
def test_rotation_matrix_is_image_rotates():
    Image = pytest.importorskip("PIL.Image")
    import pyjpegdecoder_amd
    from tools import affine_model
    for w, h in SIZES:
        img = image(w, h, 3)
        pil = Image.fromarray(img)
        for angle in (30.0, -17.5, 45, 133.25, 271, 359.5, 725.0):
            for kw in ({}, {"center": (3.5, 9.0)}, {"translate": (2, -3)}, {"center": (w - 1, 0), "translate": (-1.5, 4)}):
                m = pyjpegdecoder_amd.rotation_matrix(angle, (w, h), **kw)
                assert m == affine_model.rotation_matrix(angle, (w, h), **kw)
                for resample in FILTERS:
                    want = np.asarray(pil.rotate(angle, getattr(Image.Resampling, resample.upper()), fillcolor=(7, 99, 200), **kw))
                    assert np.array_equal(affine_model.transform(img, m, resample, (7, 99, 200)), want), (angle, kw, resample)
    assert "rotation_matrix" in pyjpegdecoder_amd.__all__


# ---- batch.normalize_affine ----------------------------------------------------------------------------------------------------------------
IDENT = (1, 0, 0, 0, 1, 0)


def test_normalize_affine_forms():
    from pyjpegdecoder_amd.batch import normalize_affine, rois_as_views
    assert normalize_affine(None, None, None, (8, 8), 3) is None
    assert normalize_affine([None, None, None], "bicubic", 7, (8, 8), 3) is None          # (no output transformed: the call without)
    s = normalize_affine(IDENT, None, None, (8, 8), 2)
    assert s.matrices == [(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)] * 2 and s.resample == "nearest" and s.fill == (0,)
    s = normalize_affine([None, np.array([1, 0, 2.5, 0, 1, 0])], "BiLinear", (7, 99, 200), (8, 8), 2, ncomp=3)
    assert s.matrices == [None, (1.0, 0.0, 2.5, 0.0, 1.0, 0.0)] and s.resample == "bilinear" and s.fill == (7, 99, 200)
    assert normalize_affine(IDENT, 3, 9, (8, 8), 1, ncomp=3).fill == (9, 9, 9)
    assert normalize_affine(IDENT, 3, 9, (8, 8), 1).resample == "bicubic" and normalize_affine(IDENT, 0, 9, (8, 8), 1).resample == "nearest"
    assert normalize_affine(IDENT, 2, (9,), (8, 8), 1, ncomp=1).fill == (9,)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert normalize_affine(IDENT, Image.Resampling.BICUBIC, None, (8, 8), 1).resample == "bicubic"
    # what needs no file
    assert normalize_affine(IDENT, "nearest", 3, (8, 8), None).matrices == []
    # rois become views, one per file
    assert rois_as_views(None, 2) == [(0, None), (1, None)]
    assert rois_as_views((1, 2, 3, 4), 2) == [(0, (1, 2, 3, 4)), (1, (1, 2, 3, 4))]
    assert rois_as_views([None, [1, 2, 3, 4]], 2) == [(0, None), (1, (1, 2, 3, 4))]
    with pytest.raises(ValueError, match="rois must be None"):
        rois_as_views([(1, 2, 3, 4)], 2)


def test_normalize_affine_refusals():
    from pyjpegdecoder_amd.batch import AffineSpec, affine_fault, check_affine, normalize_affine
    with pytest.raises(ValueError, match=r"affine needs size=\(width, height\)"):
        normalize_affine(IDENT, None, None, None, 1)
    with pytest.raises(ValueError, match="affine and return_seams do not go together"):
        normalize_affine(IDENT, None, None, (8, 8), 1, return_seams=True)
    with pytest.raises(ValueError, match="affine and reducing_gap do not go together yet"):
        normalize_affine(IDENT, None, None, (8, 8), 1, reducing_gap=2.0)
    with pytest.raises(ValueError, match="affine_resample and affine_fill need affine"):
        normalize_affine(None, "bilinear", None, (8, 8), 1)
    with pytest.raises(ValueError, match="affine has 2 entries for 3 outputs"):
        normalize_affine([IDENT, None], None, None, (8, 8), 3)
    for bad in (3, "rotate", (1, 0, 0, 0, 1), [(1, 0, 0, 0, 1, "0")], [IDENT, 5], (1, 0, 0, 0, True, 0)):
        with pytest.raises(ValueError, match="affine must be None, one matrix"):
            normalize_affine(bad, None, None, (8, 8), 2)
    for bad in ("lanczos", "box", 1, 4, 5, True, 2.0):
        with pytest.raises(ValueError, match="affine_resample must be one of nearest, bilinear, bicubic"):
            normalize_affine(IDENT, bad, None, (8, 8), 1)
    for bad in (256, -1, (1, 2), (1, 2, 300), "red", 1.5):
        with pytest.raises(ValueError, match="affine_fill must be one byte"):
            normalize_affine(IDENT, None, bad, (8, 8), 1)
    with pytest.raises(ValueError, match="affine_fill has 3 bytes for outputs of 1 component"):
        normalize_affine(IDENT, None, (1, 2, 3), (8, 8), 1, ncomp=1)
    with pytest.raises(ValueError, match="affine: output 1: a matrix entry is not finite"):
        normalize_affine([IDENT, (1, 0, float("nan"), 0, 1, 0)], None, None, (8, 8), 2)
    with pytest.raises(ValueError, match="affine: output 0: a matrix that is all zero"):
        normalize_affine([(0,) * 6], None, None, (8, 8), 1)
    # against the images: the four refusals, as the library words them
    from tools import affine_model
    for m, resample, dims, why in (((1, 0, float("inf"), 0, 1, 0), "bilinear", (20, 30), "not finite"),
                                   (IDENT, "bilinear", (32768, 30), "a side of 32768 or more"),
                                   ((1, 0, 32768, 0, 1, 0), "bicubic", (20, 30), "source coordinate of magnitude 32768 or more"),
                                   ((1700, 0, 0, 0, 1, 0), "bilinear", (20, 30), "source coordinate of magnitude 32768 or more"),
                                   # (the corner pixels' centres pass, Pillow's check_fixed corner (w, h) does not)
                                   ((1638.4, 0, 0, 0, 1, 0), "nearest", (20, 30), "source coordinate of magnitude 32768 or more"),
                                   ((40000, 0.001, -20000, 0, 1, 0), "nearest", (1, 1), "16.16 fixed point")):
        assert why in affine_fault(m, resample, *dims) and affine_fault(m, resample, *dims) == affine_model.fault(m, resample, *dims)
        with pytest.raises(ValueError, match=r"affine: output 1 \(file 7\): "):
            check_affine(AffineSpec([None, m], resample, (0,)), [(0, (0, 0, 4, 4)), (1, (0, 0, 4, 4))], [(64, 64), dims], index=[5, 7])
    assert affine_fault((1638.4, 0, 0, 0, 1, 0), "bilinear", 20, 30) is None
    assert affine_fault((0.9, 0.3, -2, -0.3, 0.9, 4), "nearest", 1920, 1080) is None


def test_narrow_takes_the_matrices_with_the_views():
    from pyjpegdecoder_amd.batch import AffineSpec, _Request
    m1, m2 = (1, 0, 1, 0, 1, 0), (1, 0, 2, 0, 1, 0)
    req = _Request([b"a", b"b"], None, (8, 8), None, None, [0, 1, 2], None, None, views=[(1, (0, 0, 1, 1)), (0, (0, 0, 2, 2)), (1, (0, 0, 3, 3))],
                   affine=AffineSpec([m1, None, m2], "bilinear", (1, 2, 3)))
    sub = req.narrow([1])
    assert sub.views == [(0, (0, 0, 1, 1)), (0, (0, 0, 3, 3))] and sub.affine.matrices == [m1, m2] and sub.slots == [0, 2]
    assert sub.plan_kwargs(3)["affine"] == ([m1, m2], "bilinear", (1, 2, 3))
    none = req.narrow([0])                       # (its one output is not transformed: the request of a call without)
    assert none.affine is None and "affine" not in none.plan_kwargs(3)


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


def test_the_request_with_an_affine_transform_is_laid_out_as_the_binding_assumes(lib, tmp_path):
    from pyjpegdecoder_amd import _binding as B
    gcc = shutil.which("gcc")
    assert gcc is not None, "the header is held to a C compiler"
    flags = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include")]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(
        ['#include <stdio.h>', '#include <stddef.h>', '#include "mijpeg.h"', 'int main(void) {', '  mj_plan_request zeroed = {0};',
         '  printf("%zu", sizeof(mj_affine));',
         '  printf(" %d %d %d", MJ_AFFINE_NEAREST, MJ_AFFINE_BILINEAR, MJ_AFFINE_BICUBIC);',
         '  printf(" %d\\n", zeroed.affine == 0 && zeroed.transform_filter == 0 && zeroed.transform_fill[2] == 0);', '  return 0;', '}']))
    exe = tmp_path / "layout"
    subprocess.run([gcc] + flags + [str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(B.AffineC), B.MJ_AFFINE_NEAREST, B.MJ_AFFINE_BILINEAR, B.MJ_AFFINE_BICUBIC, 1]
    assert ctypes.sizeof(B.AffineC) == 48
    # (the request's own layout, these fields included: test_plan_request_host)
    # plan_request: the filter, the fill bytes, the matrices (None: all zero), one per output
    m = (0.5, 0.25, 3.0, -0.25, 0.5, 1.5)
    r, keep = B.plan_request(2, size=(24, 16), affine=([m, None], "bicubic", (7, 99, 200)))
    assert r.transform_filter == B.MJ_AFFINE_BICUBIC and tuple(r.transform_fill) == (7, 99, 200) and r.n_views == 0 and not r.views and not r.perspective
    assert tuple(r.affine[0].a) == m and tuple(r.affine[1].a) == (0.0,) * 6
    r, keep = B.plan_request(2, size=(24, 16), views=[(1, None), (0, (1, 1, 4, 4)), (1, None)], affine=([m, None, m], "nearest", (5,)))
    assert r.n_views == 3 and r.transform_filter == B.MJ_AFFINE_NEAREST and tuple(r.transform_fill) == (5, 0, 0) and r.views[1].window.width == 4
    with pytest.raises(ValueError, match="affine: 1 entries, not one for each of the 2 images"):
        B.plan_request(2, size=(24, 16), affine=([m], "nearest", (0,)))
    with pytest.raises(ValueError, match="affine: 2 entries, not one for each of the 3 views"):
        B.plan_request(2, size=(24, 16), views=[(0, None), (1, None), (0, None)], affine=([m, m], "nearest", (0,)))
    with pytest.raises(ValueError, match="affine needs size"):
        B.plan_request(2, affine=([m, m], "nearest", (0,)))
    header = (ROOT / "include" / "mijpeg.h").read_text()
    assert "int32_t transform_filter;" in header and "uint8_t transform_fill[3];" in header and "const mj_affine *affine;" in header


def test_no_transform_is_the_zeroed_request(lib):
    """None and lists of None make the byte-identical request of a call without the argument — in Python — and all-zero matrices
    normalise to the field's absence in the library"""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import _Request, normalize_affine
    plain = _Request([b"a", b"b"], None, (24, 16))
    for affine in (None, [None, None]):
        req = _Request([b"a", b"b"], None, (24, 16), affine=normalize_affine(affine, None, None, (24, 16), 2))
        a, _ = B.plan_request(2, **req.plan_kwargs(3))
        b, _ = B.plan_request(2, **plain.plan_kwargs(3))
        assert bytes(a) == bytes(b) and req.plan_kwargs(3) == plain.plan_kwargs(3)
    batch, keep = _batch([(128, 64), (50, 70)])
    rc, out, msg = _normal(lib, batch, affine=([None, None], "bilinear", (1, 2, 3)))
    assert rc == B.MJ_OK and not out.affine and not out.perspective and out.transform_filter == 0 and bytes(out.transform_fill) == bytes(3), msg
    assert out.n_views == 0 and out.n_slots == 2
    rc, plain_out, _ = _normal(lib, batch)
    assert bytes(out) == bytes(plain_out)
    # a request with a transform: its windows, or whole images, become one view per image
    m = (0.9, 0.3, -2.0, -0.3, 0.9, 4.0)
    rc, out, msg = _normal(lib, batch, affine=([m, None], "bilinear", (1, 2, 3)))
    assert rc == B.MJ_OK and bool(out.affine) and out.transform_filter == 2 and tuple(out.transform_fill) == (1, 2, 3), msg
    assert out.n_views == 2 and out.n_slots == 2 and not out.rois and not out.views, "the library's own views do not leave it"
    rc, out, msg = _normal(lib, batch, affine=([m, m], "nearest", (0,)), rois=[(1, 1, 4, 4), (0, 0, 50, 70)])
    assert rc == B.MJ_OK and out.n_views == 2 and not out.rois, msg
    rc, out, msg = _normal(lib, batch, affine=([m, None, m], "bicubic", (0,)), views=[(1, None), (0, (1, 1, 4, 4)), (1, None)])
    assert rc == B.MJ_OK and out.n_views == 3 and out.n_slots == 3, msg


def test_request_refusals(lib):
    from pyjpegdecoder_amd import _binding as B
    batch, keep = _batch([(128, 64), (50, 70)])
    m = (0.9, 0.3, -2.0, -0.3, 0.9, 4.0)
    ok = ([m, m], "bilinear", (0,))
    rc, _, msg = _normal(lib, batch, affine=ok, size=None)
    assert rc == B.MJ_ERR_INVALID and "affine needs a size" in msg
    rc, _, msg = _normal(lib, batch, affine=ok, reducing_gap=2.0)
    assert rc == B.MJ_ERR_INVALID and "affine and reducing_gap do not go together yet" in msg
    rc, _, msg = _normal(lib, batch, affine=([m, m], 9, (0,)))
    assert rc == B.MJ_ERR_INVALID and "affine: filter 9 is none of MJ_AFFINE_*" in msg
    rc, _, msg = _normal(lib, batch, affine=ok, rois=[(1, 1, 4, 4), (0, 0, 51, 70)])
    assert rc == B.MJ_ERR_INVALID and "view 1: window" in msg
    for bad, name, why in (((1, 0, float("nan"), 0, 1, 0), "bilinear", "a matrix entry is not finite"),
                           ((1, 0, 32768, 0, 1, 0), "bicubic", "a corner of the output has a source coordinate of magnitude 32768 or more"),
                           ((1638.4, 0, 0, 0, 1, 0), "nearest", "a corner of the output has a source coordinate of magnitude 32768 or more"),
                           ((30000, 0.001, -20000, 0, 1, 0), "nearest", "a corner of the output")):
        rc, _, msg = _normal(lib, batch, affine=([m, bad], name, (0,)))
        assert rc == B.MJ_ERR_INVALID and "affine: output 1: " + why in msg, (bad, msg)
    big, keep_big = _batch([(128, 64), (40000, 8)])
    rc, _, msg = _normal(lib, big, affine=ok)
    assert rc == B.MJ_ERR_INVALID and "affine: output 1: an image with a side of 32768 or more" in msg
    rc, _, msg = _normal(lib, big, affine=ok, orientation=[1, 6])
    assert rc == B.MJ_ERR_INVALID and "affine: output 1: an image with a side of 32768 or more" in msg
    for fill in ((0, 0, 0), (0, 0, 1)):                       # (the filter, or a fill byte, without an array)
        r, keep_r = B.plan_request(2, size=(24, 16), affine=(ok[0], "bilinear" if not any(fill) else 0, fill))
        r.affine = None
        out = B.PlanRequestC()
        assert lib.mj_debug_normalise_request(ctypes.byref(batch), ctypes.byref(r), ctypes.byref(out)) == B.MJ_ERR_INVALID
        assert "transform_filter / transform_fill without an array" in lib.mj_last_error(None).decode()
    # both arrays in one request
    r, keep_r = B.plan_request(2, size=(24, 16), affine=ok)
    keep_p = r.perspective = (B.PerspectiveC * 2)()
    out = B.PlanRequestC()
    assert lib.mj_debug_normalise_request(ctypes.byref(batch), ctypes.byref(r), ctypes.byref(out)) == B.MJ_ERR_INVALID
    assert "affine and perspective do not go together" in lib.mj_last_error(None).decode()
