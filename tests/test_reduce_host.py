"""The two-step resize without a GPU: tools/reduce_model.py is Pillow's Image.reduce and Image.resize(..., reducing_gap=) byte
for byte (and a committed Pillow-made fixture pins it where Pillow is absent); the library's host twins — mj_host_reduce_factors,
mj_host_reduce with its phases, mj_host_resize_table_boxed — are the model's; the request field's refusals and its default rule."""
import ctypes
import itertools

import numpy as np
import pytest

from conftest import GOLDEN
from test_resample_host import PAIRS

FILTERS = ("bilinear", "box", "hamming", "bicubic", "lanczos")
GAPS = (1.0, 1.5, 2.0, 3.0)


def _image(rng, w, h, nc):
    return rng.integers(0, 256, (h, w, 3) if nc == 3 else (h, w), dtype=np.uint8)


def _reduce_cases():
    """(w, h, fx, fy): every factor pair 1..12 x 1..12 with remainders 0, 1 and f - 1 on both axes, then a few large ones"""
    cases = []
    for fx, fy in itertools.product(range(1, 13), range(1, 13)):
        for rx, ry in ((0, 0), (1, 1), (fx - 1, fy - 1)):
            cases.append((3 * fx + rx, 2 * fy + ry, fx, fy))
    return cases + [(300, 9, 291, 2), (128, 64, 32, 16), (70, 513, 3, 256), (600, 3, 600, 3), (257, 300, 256, 256), (40, 40, 41, 50), (301, 300, 300, 300)]


def test_model_reduce_is_pillows():
    Image = pytest.importorskip("PIL.Image")
    from tools import reduce_model
    rng = np.random.default_rng(5)
    cases = _reduce_cases()
    assert len(cases) == 144 * 3 + 7
    for k, (w, h, fx, fy) in enumerate(cases):
        a = _image(rng, w, h, 3 if k % 2 else 1)
        want = np.asarray(Image.fromarray(a).reduce((fx, fy)))
        got = reduce_model.reduce(a, fx, fy)
        assert got.shape == want.shape and np.array_equal(got, want), (w, h, fx, fy)


def _resize_cases(filter):
    """(w, h, out_w, out_h, components, gap), seeded per filter; every one reduces and avoids Pillow's tall-image pass order"""
    from tools import reduce_model
    rng = np.random.default_rng(100 + FILTERS.index(filter))
    cases = []
    while len(cases) < 40:
        gap = GAPS[len(cases) % 4]
        w, h = int(rng.integers(8, 400)), int(rng.integers(8, 300))
        ow, oh = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        fx, fy = reduce_model.reduce_factors(w, h, ow, oh, gap)
        if fx == 1 and fy == 1:
            continue
        assert not reduce_model.tall(-(-w // fx), -(-h // fy), oh), (w, h, ow, oh, gap)
        cases.append((w, h, ow, oh, 3 if len(cases) % 3 else 1, gap))
    return cases


# (w, h, out_w, out_h, gap, seed of a greyscale noise image): found by search — the bytes with the box kept in doubles are not the
# bytes with the float32 box
PARTED = {"bilinear": [(379, 132, 27, 36, 1.0, 0), (69, 163, 6, 19, 1.0, 4), (332, 133, 18, 21, 2.0, 14)],
          "box": [(197, 58, 34, 8, 2.0, 10), (235, 104, 30, 22, 2.0, 46), (305, 178, 20, 9, 2.0, 110)],
          "hamming": [(121, 109, 16, 11, 3.0, 15), (388, 144, 35, 9, 1.5, 17), (341, 95, 34, 32, 3.0, 59)],
          "bicubic": [(213, 199, 32, 32, 1.0, 8), (337, 155, 37, 28, 3.0, 223), (61, 119, 18, 32, 1.0, 224)],
          "lanczos": [(278, 184, 37, 39, 1.5, 293), (367, 124, 37, 11, 1.5, 421), (115, 78, 9, 9, 1.0, 880)]}


@pytest.mark.parametrize("filter", FILTERS)
def test_model_two_step_resize_is_pillows_and_float32_is_part_of_it(filter):
    """The condition first: on three cases per filter a box kept in doubles gives other bytes than the float32 box, and Pillow's
    are the float32 ones — the comparison can tell the two apart.  Then 40 seeded cases over the four gaps."""
    Image = pytest.importorskip("PIL.Image")
    from tools import reduce_model
    pil = getattr(Image.Resampling, filter.upper())
    for w, h, ow, oh, gap, seed in PARTED[filter]:
        a = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
        fx, fy = reduce_model.reduce_factors(w, h, ow, oh, gap)
        assert not reduce_model.tall(-(-w // fx), -(-h // fy), oh)
        want = np.asarray(Image.fromarray(a).resize((ow, oh), pil, reducing_gap=gap))
        assert not np.array_equal(reduce_model.resize(a, (ow, oh), filter, gap, box32=False), want), (w, h, ow, oh, gap)
        assert np.array_equal(reduce_model.resize(a, (ow, oh), filter, gap), want), (w, h, ow, oh, gap)
    rng = np.random.default_rng(17)
    bad = []
    cases = _resize_cases(filter)
    assert len(cases) == 40 and {c[5] for c in cases} == set(GAPS)
    for w, h, ow, oh, nc, gap in cases:
        a = _image(rng, w, h, nc)
        want = np.asarray(Image.fromarray(a).resize((ow, oh), pil, reducing_gap=gap))
        got = reduce_model.resize(a, (ow, oh), filter, gap)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append((w, h, ow, oh, nc, gap))
    assert not bad, f"{filter}: {len(bad)} cases differ from Pillow, first {bad[:5]}"


def test_model_is_pinned_by_the_pillow_made_fixture():
    """tests/golden/reduce_blocks.npz (tools/make_reduce_golden.py): holds where Pillow is not installed."""
    from tools import reduce_model
    g = np.load(GOLDEN / "reduce_blocks.npz")
    assert len(g["reduce_args"]) == 9 and len(g["resize_args"]) == 20
    for k, (fx, fy) in enumerate(g["reduce_args"]):
        assert np.array_equal(reduce_model.reduce(g[f"reduce_in_{k}"], int(fx), int(fy)), g[f"reduce_out_{k}"]), k
    seen = set()
    for k, (ow, oh, f, gap) in enumerate(g["resize_args"]):
        a = g[f"resize_in_{k}"]
        assert reduce_model.reduce_factors(a.shape[1], a.shape[0], int(ow), int(oh), float(gap)) != (1, 1)
        assert np.array_equal(reduce_model.resize(a, (int(ow), int(oh)), FILTERS[int(f)], float(gap)), g[f"resize_out_{k}"]), k
        seen.add((int(f), float(gap)))
    assert len(seen) == 20


def test_multiplier_values():
    """m(n) = (uint32)(float32(2^32) / float32(256 n)): powers of two divide exactly — the shift cases — and 2^24 is the identity
    cell's; up to the library's largest cell the float32 quotient truncates to what the exact quotient truncates to."""
    from tools import reduce_model
    assert reduce_model.multiplier(1) == 1 << 24 and reduce_model.multiplier(4) == 1 << 22 and reduce_model.multiplier(16) == 1 << 20
    assert reduce_model.multiplier(3) == 5592405 and reduce_model.multiplier(65536) == 256
    assert all(reduce_model.multiplier(n) == (1 << 24) // n for n in range(1, reduce_model.MAX_CELL + 1, 7))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


def test_library_factors_are_the_models(lib):
    from pyjpegdecoder_amd import _binding as B
    from tools import reduce_model
    rng = np.random.default_rng(23)
    cases = [(1920, 1080, 224, 224), (70, 50, 8, 7), (65535, 65535, 1, 1), (1, 1, 1, 1), (5, 9, 65535, 3)]
    cases += [tuple(int(v) for v in rng.integers(1, 5000, 4)) for _ in range(200)]
    for case in cases:
        for gap in GAPS + (1.0000001, 2.5, 7.25, 1e9):
            assert B.reduce_factors(*case, gap) == reduce_model.reduce_factors(*case, gap), (case, gap)
    fx, fy = ctypes.c_int32(), ctypes.c_int32()
    for bad in ((0, 5, 1, 1, 2.0), (5, 5, 0, 1, 2.0), (65536, 5, 1, 1, 2.0), (5, 5, 1, 1, 0.5), (5, 5, 1, 1, float("nan")), (5, 5, 1, 1, float("inf")),
                (5, 5, 1, 1, 0.0)):
        assert lib.mj_host_reduce_factors(*bad, ctypes.byref(fx), ctypes.byref(fy)) == B.MJ_ERR_INVALID, bad
    assert lib.mj_host_reduce_factors(5, 5, 1, 1, 2.0, None, ctypes.byref(fy)) == B.MJ_ERR_INVALID


def test_library_reduce_is_the_models_phases_included(lib):
    """Phases against the model applied to the FLIPPED array: reducing in stored order with the partial cell first is reducing
    the reversed axis Pillow's way."""
    from pyjpegdecoder_amd import _binding as B
    from tools import reduce_model
    rng = np.random.default_rng(29)
    for k, (w, h, fx, fy) in enumerate(_reduce_cases()):
        if k % 3 == 0 and k > 40 and fx * fy < 100:       # (a third of the small ones is enough for the twin)
            continue
        a = _image(rng, w, h, 3 if k % 2 else 1)
        if fx * fy > 65536:
            with pytest.raises(ValueError):
                B.reduce(a, fx, fy)
            continue
        assert np.array_equal(B.reduce(a, fx, fy), reduce_model.reduce(a, fx, fy)), (w, h, fx, fy)
        px, py = w % fx, h % fy
        assert np.array_equal(B.reduce(a, fx, fy, px, 0), reduce_model.reduce(a[:, ::-1], fx, fy)[:, ::-1]), (w, h, fx, fy)
        assert np.array_equal(B.reduce(a, fx, fy, 0, py), reduce_model.reduce(a[::-1], fx, fy)[::-1]), (w, h, fx, fy)
        both = B.reduce(a, fx, fy, px, py)
        assert np.array_equal(both, reduce_model.reduce(a[::-1, ::-1], fx, fy)[::-1, ::-1]), (w, h, fx, fy)
        assert np.array_equal(both, reduce_model.reduce(a, fx, fy, px, py)), (w, h, fx, fy)
    a = _image(rng, 10, 7, 3)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((7, 10, 3), dtype=np.uint8)
    for bad in ((10, 7, 2, 3, 2, 0, 0), (10, 7, 3, 0, 2, 0, 0), (10, 7, 3, 3, 2, 2, 0), (10, 7, 3, 3, 2, 0, 2), (10, 7, 3, 3, 2, -1, 0)):
        assert lib.mj_host_reduce(p(a), *bad, p(out)) == B.MJ_ERR_INVALID, bad
    assert lib.mj_host_reduce(None, 10, 7, 3, 3, 2, 0, 0, p(out)) == B.MJ_ERR_INVALID
    # a 1 x 1 cell is the identity
    assert np.array_equal(B.reduce(a, 1, 1), a)


@pytest.mark.parametrize("filter", FILTERS)
def test_library_boxed_tables_are_the_models(lib, filter):
    from pyjpegdecoder_amd import _binding as B
    from tools import reduce_model
    rng = np.random.default_rng(31)
    cases = [(480, 1920 / 4, 224), (540, 1080 / 2, 224), (18, 70 / 4, 8), (17, 50 / 3, 7), (10, 37 / 4, 5), (22, 64 / 3, 10), (4, 128 / 32, 4)]
    # (sizes at which the table from a box in doubles is another table, for one filter or another: found by search)
    for w, o, gap in ((88, 10, 1.5), (34, 5, 1.0), (146, 18, 1.5), (148, 32, 1.5), (370, 20, 1.0), (328, 5, 1.0), (184, 16, 3.0)):
        f = reduce_model.reduce_factors(w, 1, o, 1, gap)[0]
        cases.append((-(-w // f), w / f, o))
    for _ in range(60):
        w, f, o = int(rng.integers(2, 3000)), int(rng.integers(1, 40)), int(rng.integers(1, 300))
        cases.append((-(-w // f), w / f, o))
    parted = 0
    for in_size, in1, o in cases:
        got = B.resize_table_boxed(in_size, o, (0.0, in1), filter)
        want = reduce_model.axis_table(in_size, o, filter, (0.0, in1))
        for x, y in zip(got, want):
            assert x.shape == y.shape and np.array_equal(x, y), (in_size, in1, o)
        other = reduce_model.axis_table(in_size, o, filter, (0.0, in1), box32=False)
        parted += any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(got, other))
    assert parted >= 1          # (the function rounds the box to float32: a table from the doubles is another table somewhere)
    # a box that starts inside the axis, as Pillow's precompute_coeffs takes it
    for x, y in zip(B.resize_table_boxed(40, 9, (2.5, 31.25), filter), reduce_model.axis_table(40, 9, filter, (2.5, 31.25))):
        assert np.array_equal(x, y)
    ks = ctypes.c_int32()
    for bad in ((40, -1.0, 30.0, 9), (40, 0.0, 40.5, 9), (40, 5.0, 5.0, 9), (40, 0.0, float("nan"), 9), (0, 0.0, 1.0, 9), (40, 0.0, 30.0, 0)):
        assert lib.mj_host_resize_table_boxed(B.FILTERS[filter], bad[0], bad[1], bad[2], bad[3], None, None, None, 0, ctypes.byref(ks)) == B.MJ_ERR_INVALID, bad
    assert lib.mj_host_resize_table_boxed(9, 40, 0.0, 30.0, 9, None, None, None, 0, ctypes.byref(ks)) == B.MJ_ERR_INVALID


@pytest.mark.parametrize("filter", FILTERS)
def test_unboxed_tables_are_what_they_were(lib, filter):
    """tests/test_resample_host.py's pairs: the two table functions still give the model's table, and the whole axis as a box gives
    the identical one."""
    from pyjpegdecoder_amd import _binding as B
    from tools import resize_model
    for i, o in PAIRS:
        want = resize_model.axis_table(i, o, filter)
        for x, y in zip(B.resize_table(i, o, filter), want):
            assert np.array_equal(x, y), (i, o)
        for x, y in zip(B.resize_table_boxed(i, o, (0.0, float(i)), filter), want):
            assert np.array_equal(x, y), (i, o)
        if filter == "bilinear":
            for x, y in zip(B.resize_table(i, o), want):
                assert np.array_equal(x, y), (i, o)


def _batch(sizes):
    """an mj_batch that holds nothing but its images' sizes: what the request's checks look at"""
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
    r, keep = B.plan_request(batch.n_images if batch is not None else 0, **kw)
    out = B.PlanRequestC()
    rc = lib.mj_debug_normalise_request(ctypes.byref(batch) if batch is not None else None, ctypes.byref(r), ctypes.byref(out))
    return rc, out, lib.mj_last_error(None).decode()


def test_request_refusals_and_the_default_rule_need_no_gpu(lib):
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import normalize_reducing_gap
    # the field is an ordinary member (its place in the request: test_plan_request_host)
    assert B.PlanRequestC().reducing_gap == 0.0
    r = B.PlanRequestC()
    r.reducing_gap = 1.5
    assert r.reducing_gap == 1.5 and r.filter == 0 and not r.places and not r.fill
    batch, keep = _batch([(1920, 1080), (64, 64)])
    # the value, before anything else is looked at — no context, not even a batch
    for bad in (0.5, float("nan"), float("inf"), -2.0, 0.999999):
        rc, _, msg = _normal(lib, None, size=(8, 8), reducing_gap=bad)
        assert rc == B.MJ_ERR_INVALID and "reducing_gap must be 1.0 or greater" in msg, (bad, msg)
        h = ctypes.c_void_p()
        r, _ = B.plan_request(0, size=(8, 8), reducing_gap=bad)
        assert lib.mj_plan_create_with(None, None, ctypes.byref(r), ctypes.byref(h)) == B.MJ_ERR_INVALID
        assert "reducing_gap must be 1.0 or greater" in lib.mj_last_error(None).decode()
    # a gap without a size
    r = B.PlanRequestC()
    r.reducing_gap = 2.0
    out = B.PlanRequestC()
    assert lib.mj_debug_normalise_request(ctypes.byref(batch), ctypes.byref(r), ctypes.byref(out)) == B.MJ_ERR_INVALID
    assert "reducing_gap needs a size" in lib.mj_last_error(None).decode()
    with pytest.raises(ValueError, match="reducing_gap needs size"):
        B.plan_request(1, reducing_gap=2.0)
    # the default rule: a gap under which every factor is 1 yields the request without it
    rc, out, _ = _normal(lib, batch, size=(224, 224), reducing_gap=2.0)
    assert rc == B.MJ_OK and out.reducing_gap == 2.0
    rc, out, _ = _normal(lib, batch, size=(700, 400), reducing_gap=2.0)          # 1920 / 700 / 2 and 1080 / 400 / 2 are below 2
    assert rc == B.MJ_OK and out.reducing_gap == 0.0 and (out.out_width, out.out_height) == (700, 400)
    rc, out, _ = _normal(lib, batch, size=(700, 400), reducing_gap=1.0)          # 1920 / 700 = 2.74: a factor of 2
    assert rc == B.MJ_OK and out.reducing_gap == 1.0
    # ... from the window's size, the oriented size and the place's size where there are any
    rc, out, _ = _normal(lib, batch, size=(224, 224), reducing_gap=2.0, rois=[(0, 0, 500, 500), (0, 0, 64, 64)])
    assert rc == B.MJ_OK and out.reducing_gap == 0.0
    rc, out, _ = _normal(lib, batch, size=(600, 224), reducing_gap=2.0)          # 1080 / 224 / 2 = 2.4: the height reduces
    assert rc == B.MJ_OK and out.reducing_gap == 2.0
    rc, out, _ = _normal(lib, batch, size=(600, 300), reducing_gap=2.0, orientation=[6, 6])      # oriented 1080 x 1920: 1920 / 300 / 2 = 3.2
    assert rc == B.MJ_OK and out.reducing_gap == 2.0
    rc, out, _ = _normal(lib, batch, size=(600, 300), reducing_gap=2.0)          # upright: 1920 / 600 / 2 = 1.6, 1080 / 300 / 2 = 1.8
    assert rc == B.MJ_OK and out.reducing_gap == 0.0
    rc, out, _ = _normal(lib, batch, size=(600, 300), reducing_gap=2.0, places=[(100, 100, 0, 0), (600, 300, 0, 0)])
    assert rc == B.MJ_OK and out.reducing_gap == 2.0
    # the Python argument
    assert normalize_reducing_gap(None, None) is None and normalize_reducing_gap(2, (8, 8)) == 2.0
    with pytest.raises(ValueError, match="reducing_gap must be 1.0 or greater"):
        normalize_reducing_gap(0.5, (8, 8))
    with pytest.raises(ValueError, match="reducing_gap must be 1.0 or greater"):
        normalize_reducing_gap(float("nan"), (8, 8))
    with pytest.raises(ValueError, match="reducing_gap needs size"):
        normalize_reducing_gap(2.0, None)
    with pytest.raises(ValueError, match="must be None or a number"):
        normalize_reducing_gap("2", (8, 8))
    with pytest.raises(ValueError, match="not exact as a 32-bit float"):
        normalize_reducing_gap(1.1, (8, 8))
    assert normalize_reducing_gap(2.25, (8, 8)) == 2.25


def test_new_entry_points_are_exported_and_in_the_header(lib):
    from conftest import ROOT
    header = (ROOT / "include" / "mijpeg.h").read_text()
    for name in ("mj_host_reduce_factors", "mj_host_reduce", "mj_host_resize_table_boxed", "mj_debug_reduce_shape", "mj_debug_normalise_request",
                 "mj_plan_time_reduce"):
        assert hasattr(lib, name) and name + "(" in header, name
    assert "float reducing_gap;" in header
