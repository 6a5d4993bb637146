"""Aspect-preserving sizing on the MI355X (mj_plan_request.places / fill, BatchDecoder.decode / decode_device /
decode_device_iter(size=..., resize_to=..., place=..., fill=...)): every output is byte for byte tools/place_model.py — which
tests/test_place_host.py pins to Pillow and to the libraries' rules — applied to the oracle's pixels of the image or window, in
every layout.  Expected values never come from the library."""
import numpy as np
import pytest

from conftest import GOLDEN, oracle_rgb_all
from test_resize import as_layout, rowmajor_window
from test_roi import LAYOUTS, _fixture_files, mcu_size, window_kinds

pytestmark = pytest.mark.gpu

FILTERS = ("bilinear", "bicubic", "lanczos")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

_cache = {}


def places_for(resize_to, place, canvas, dims):
    """(width, height, x, y) per file from tools/place_model.py's rules (never the package's)."""
    from tools import place_model
    out = []
    for i, (w, h) in enumerate(dims):
        kind = resize_to[i] if isinstance(resize_to, list) else resize_to
        xy = place[i] if isinstance(place, list) else place
        r = place_model.resized_size(kind, w, h, canvas)
        out.append(tuple(r) + tuple(xy if xy is not None else place_model.centred(kind, r, canvas)))
    return out


def model(key, img_rm, pl, canvas, fill, filter):
    """tools/place_model.py of a row-major image, computed once per case and left unchanged: the layouts share it."""
    from tools import place_model
    k = (key, tuple(pl), tuple(canvas), tuple(np.atleast_1d(fill).tolist()), filter)
    if k not in _cache:
        _cache[k] = place_model.place(img_rm, pl[:2], pl[2:], canvas, fill, filter)
        _cache[k].setflags(write=False)
    return _cache[k]


def expect(key, full, win, pl, canvas, fill, filter, layout):
    return as_layout(model((key, tuple(win)), rowmajor_window(full, win), pl, canvas, fill, filter), layout)


def whole(full):
    return (0, 0, full.shape[0], full.shape[1])


@pytest.fixture(scope="module")
def fixtures():
    """The fixture files up to 128 x 128, by component count: (name, raw, oracle pixels, MCU size)."""
    files = _fixture_files()
    fulls = oracle_rgb_all([raw for _, raw in files])
    out = [(name, raw, full, mcu_size(raw)) for (name, raw), full in zip(files, fulls) if max(full.shape[:2]) <= 128]
    return {nc: [f for f in out if (f[2].ndim == 3) == (nc == 3)] for nc in (1, 3)}


@pytest.fixture(scope="module")
def big():
    raw = (GOLDEN / "files" / "c3_1920x1080_420_dri120.jpg").read_bytes()
    return raw, oracle_rgb_all([raw])[0]


def coverage(pl, canvas):
    """(cropped on x, cropped on y, padded on x, padded on y) of one placed image"""
    w, h, x, y = pl
    return (x < 0 or x + w > canvas[0], y < 0 or y + h > canvas[1], x > 0 or x + w < canvas[0], y > 0 or y + h < canvas[1])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("filter", FILTERS)
def test_every_fixture_every_layout(fixtures, filter, layout):
    """Every fixture file, colour and grey, whole and through an inner window: resize_to=40 and 20 into (32, 32), "contain" into
    (64, 64) with a three-byte fill, explicit (w, h) with per-file offsets, negative and mixed ones among them."""
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    crop_both = pad_both = mixed = 0
    try:
        for nc, group in fixtures.items():
            assert group
            raws = [f[1] for f in group]
            inner = [window_kinds(f[2].shape[0], f[2].shape[1], *f[3])["inner"] for f in group]
            offsets = [((-5, -3), (4, 6), (-7, 9), (11, -2))[i % 4] for i in range(len(group))]
            cases = ((40, None, (32, 32), 0), (20, None, (32, 32), 0),
                     ("contain", None, (64, 64), (114, 7, 200) if nc == 3 else 114),
                     ((45, 38) if nc == 3 else (21, 50), offsets, (32, 32), (9, 250, 77) if nc == 3 else 31))
            for resize_to, place, canvas, fill in cases:
                for wins in (None, inner):
                    dims = [(f[2].shape[0], f[2].shape[1]) if wins is None else wins[i][2:] for i, f in enumerate(group)]
                    pls = places_for(resize_to, place, canvas, dims)
                    if any(min(p[:2]) < 1 or p[2] >= canvas[0] or p[3] >= canvas[1] or p[2] + p[0] <= 0 or p[3] + p[1] <= 0 for p in pls):
                        continue        # (an inner window too thin for this kind: the package refuses it)
                    got = dec.decode(raws, rois=wins, size=canvas, resample=filter, resize_to=resize_to, place=place, fill=fill)
                    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
                    assert got.shape == (len(group),) + dec._shape(canvas[0], canvas[1], nc)
                    for i, (name, _, full, _) in enumerate(group):
                        win = whole(full) if wins is None else wins[i]
                        cx, cy, px, py = coverage(pls[i], canvas)
                        crop_both += cx and cy
                        pad_both += px and py and not cx and not cy
                        mixed += (cx and py and not cy) or (cy and px and not cx)
                        assert np.array_equal(got[i], expect(name, full, win, pls[i], canvas, fill, filter, layout)), (name, resize_to, win, pls[i])
        assert crop_both and pad_both and mixed, (crop_both, pad_both, mixed)
    finally:
        dec.close()


def _plan(dec, raw, canvas, pls, filter="bicubic", fill=None, **kw):
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    prep = prepare_batch([raw], dec.layout, 0)
    return B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 1}, size=canvas, filter=filter, places=pls, fill=fill, **kw)


def _run_into_sentinel(dec, plan, canvas, nc, sentinel):
    """execute into a device buffer pre-filled with `sentinel`: an element the launch does not write keeps it"""
    import torch
    out = torch.full((canvas[0] * canvas[1] * nc,), sentinel, dtype=torch.uint8, device=torch.device("cuda", dec.ctx.device))
    plan.execute(0, out.data_ptr())
    plan.sync()
    assert not plan.read(rgb=False)["status"].any()
    return out.cpu().numpy()


@pytest.mark.parametrize("layout", ["rowmajor", "xmajor"])
def test_evaluation_transform_of_1080p(big, layout):
    """1920 x 1080 -> Resize(256) = 455 x 256 -> centre 224 x 224, bicubic: several tiles on both axes, every one of them cropped."""
    from pyjpegdecoder_amd import BatchDecoder
    raw, full = big
    canvas = (224, 224)
    pls = places_for(256, None, canvas, [(1920, 1080)])
    assert pls == [(455, 256, -116, -16)]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        plan = _plan(dec, raw, canvas, pls)
        try:
            shape = plan.resize_shape()
            assert shape["tiles_x"] > 1 and shape["tiles_y"] > 1 and shape["signed"], shape
            got = _run_into_sentinel(dec, plan, canvas, 3, 0xA5)
        finally:
            plan.close()
        want = expect("c3", full, whole(full), pls[0], canvas, 0, "bicubic", layout)
        assert np.array_equal(got.reshape(want.shape), want)
        assert np.array_equal(dec.decode([raw], size=canvas, resample="bicubic", resize_to=256)[0], want)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["rowmajor", "xmajor"])
def test_tiles_of_fill_and_tiles_that_straddle_the_image(big, layout):
    """An explicit size placed from the plan's own tile shape so that on each axis at least one tile is wholly fill, one straddles
    the image's leading edge and one its trailing edge — asserted from the reported shape.  The output buffer holds a sentinel
    that differs from the fill, so a fill element nobody wrote shows."""
    from pyjpegdecoder_amd import BatchDecoder
    raw, full = big
    canvas, rw, rh, fill = (448, 448), 150, 150, (200, 100, 50)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        probe = _plan(dec, raw, canvas, [(rw, rh, 0, 0)], fill=fill)
        tr, tc = probe.resize_shape()["tile_rows"], probe.resize_shape()["tile_cols"]
        probe.close()
        pl = (rw, rh, tc + tc // 2, tr + tr // 2 + 1)
        plan = _plan(dec, raw, canvas, [pl], fill=fill)
        try:
            shape = plan.resize_shape()
            assert shape["tiles_x"] > 1 and shape["tiles_y"] > 1, shape
            for lo, size, tile, total in ((pl[2], rw, shape["tile_cols"], canvas[0]), (pl[3], rh, shape["tile_rows"], canvas[1])):
                assert lo >= tile, "the first tile is wholly fill"
                assert lo % tile != 0, "a tile straddles the leading edge"
                assert (lo + size) % tile != 0 and lo + size < total, "a tile straddles the trailing edge"
                assert total - (lo + size) > tile, "a tile behind the image is wholly fill"
            got = _run_into_sentinel(dec, plan, canvas, 3, 0xA5)
        finally:
            plan.close()
        want = expect("c3", full, whole(full), pl, canvas, fill, "bicubic", layout)
        assert np.array_equal(got.reshape(want.shape), want)
    finally:
        dec.close()


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_float16_normalize_and_mirror_include_the_padding(fixtures, layout):
    """fill pixels are the table's entry for the fill byte, and a mirrored file's canvas is flipped with its padding."""
    from tools import normalize_model
    from pyjpegdecoder_amd import BatchDecoder
    group = fixtures[3][:6]
    canvas, fill = (48, 40), (114, 7, 200)
    flags = [i % 2 == 1 for i in range(len(group))]
    offs = [(9, -4) if i % 3 else (-6, 7) for i in range(len(group))]
    pls = places_for((36, 30), offs, canvas, [f[2].shape[:2] for f in group])
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode([f[1] for f in group], size=canvas, resample="bicubic", resize_to=(36, 30), place=offs, fill=fill,
                         dtype="float16", normalize=(MEAN, STD), mirror=flags)
        assert got.dtype == np.float16
        for i, (name, _, full, _) in enumerate(group):
            rm = model((name, whole(full)), rowmajor_window(full, whole(full)), pls[i], canvas, fill, "bicubic")
            assert (rm[0, -1] == fill).all() or (rm[-1, 0] == fill).all()            # (padding is there to be flipped)
            if flags[i]:
                rm = rm[:, ::-1]
            want = as_layout(normalize_model.normalize(rm, "float16", MEAN, STD), layout)
            assert np.array_equal(_bits(got[i]), want), (name, layout)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["rowmajor", "xmajor"])
def test_orientations_with_contain(fixtures, layout):
    """orientation 3, 6 and 8 (and 1) with "contain": transposing and not are separate plans into one array; the geometry is the
    oriented image's."""
    from tools import orient_model
    from pyjpegdecoder_amd import BatchDecoder
    group = fixtures[3][:8]
    turns = [(3, 6, 8, 1)[i % 4] for i in range(len(group))]
    canvas, fill = (64, 64), (1, 2, 3)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode([f[1] for f in group], size=canvas, resize_to="contain", fill=fill, orientation=turns, resample="bicubic")
        for i, (name, _, full, _) in enumerate(group):
            rm = orient_model.orient(rowmajor_window(full, whole(full)), turns[i])
            pl = places_for("contain", None, canvas, [(rm.shape[1], rm.shape[0])])[0]
            want = as_layout(model((name, "o", turns[i]), rm, pl, canvas, fill, "bicubic"), layout)
            assert np.array_equal(got[i], want), (name, turns[i])
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_modes_over_grey_and_colour(fixtures, mode, layout):
    from tools import mode_model
    from pyjpegdecoder_amd import BatchDecoder
    group = fixtures[1][:3] + fixtures[3][:4]
    canvas = (32, 32)
    fill = (114, 7, 200) if mode == "RGB" else 99
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for resize_to, filter in ((20, "bilinear"), ("contain", "lanczos")):
            got = dec.decode([f[1] for f in group], size=canvas, resize_to=resize_to, fill=fill, mode=mode, resample=filter)
            for i, (name, _, full, _) in enumerate(group):
                rm = mode_model.convert(rowmajor_window(full, whole(full)), mode)
                pl = places_for(resize_to, None, canvas, [full.shape[:2]])[0]
                want = as_layout(model((name, mode), rm, pl, canvas, fill, filter), layout)
                assert np.array_equal(got[i], want), (name, mode, resize_to)
    finally:
        dec.close()


@pytest.mark.parametrize("segment", ["gpu", "host"])
def test_device_calls_equal_decode(fixtures, segment):
    """decode_device and decode_device_iter against decode (which the tests above hold to the model), with the markers found on
    the GPU and on the host."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    raws = [f[1] for f in fixtures[3]]
    kw = dict(size=(32, 32), resize_to=20, fill=(5, 6, 7), resample="bicubic", dtype="float32", normalize=(MEAN, STD))
    dec = BatchDecoder(device=0, layout="planar_rowmajor", segment=segment, gpu_segment_min_files=2)
    try:
        want = dec.decode(raws, **kw)
        got = dec.decode_device(raws, **kw)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        cut = len(raws) // 2
        parts = list(dec.decode_device_iter([raws[:cut], raws[cut:]], **kw))
        assert np.array_equal(torch.cat(parts).cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["rowmajor", "xmajor"])
def test_derived_window_decodes_less_and_reads_nothing_else(big, layout, tune):
    """1080p with resize_to=256 into (224, 224): the plan decodes a window of the source — its source_bytes is smaller than the
    whole-image plan's — and the output is the same with the intermediate buffer poisoned first."""
    from pyjpegdecoder_amd import BatchDecoder
    raw, full = big
    canvas = (224, 224)
    pls = [(455, 256, -116, -16)]
    want = expect("c3", full, whole(full), pls[0], canvas, 0, "bicubic", layout)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        nbytes = {}
        for route in ("1", "0"):
            tune("MJ_PLACE_WINDOW", route)
            plan = _plan(dec, raw, canvas, pls)
            try:
                plan.fill_source(0xCD)
                plan.execute()
                plan.sync()
                out = plan.read(rgb=True)
                assert not out["status"].any()
                assert np.array_equal(out["rgb"].reshape(want.shape), want), route
                nbytes[route] = plan.time_resize(1)[1]
            finally:
                plan.close()
        assert 0 < nbytes["1"] < nbytes["0"], nbytes
    finally:
        dec.close()


def test_nothing_moved_and_refusals(fixtures):
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    group = fixtures[3][:4]
    raws = [f[1] for f in group]
    size = (33, 21)
    dec = BatchDecoder(device=0, layout="rowmajor")
    try:
        plain = dec.decode(raws, size=size, resample="bicubic")
        assert np.array_equal(dec.decode(raws, size=size, resample="bicubic", resize_to=size), plain)
        prep = prepare_batch([raws[0]] * len(raws), dec.layout, 0)       # (one plan: one kind of file)
        keep = {"prep": prep, "n_images": len(raws)}
        shapes = []
        for kw in ({}, {"places": [size + (0, 0)] * len(raws)}):
            plan = B.Plan(dec.ctx, prep.to_c(), keep, size=size, filter="bicubic", **kw)
            shapes.append(plan.resize_shape())
            plan.close()
        # places=NULL through the C ABI
        import ctypes

        from routes_common import create_with
        h = ctypes.c_void_p()
        dec.ctx.check(create_with(dec.ctx.lib, dec.ctx.handle, prep.to_c(), h, out_width=size[0], out_height=size[1], filter=B.MJ_FILTER_BICUBIC,
                                  mode=B.MJ_MODE_NATIVE, places=None, fill=None))
        out = (ctypes.c_int32 * 8)()
        dec.ctx.check(dec.ctx.lib.mj_debug_resize_shape(h, out))
        dec.ctx.lib.mj_plan_destroy(h)
        assert shapes[0] == shapes[1] and [int(v) for v in out][:5] == [shapes[0][k] for k in ("tile_rows", "tile_cols", "tiles_x", "tiles_y", "lds_bytes")]
        with pytest.raises(B.BackendError, match="image 2: .*does not meet"):
            B.Plan(dec.ctx, prep.to_c(), keep, size=size, places=[(8, 8, 0, 0), (8, 8, 1, 1), (8, 8, 33, 0), (8, 8, 0, 0)])
        with pytest.raises(ValueError, match="file 1: .*does not meet"):
            dec.decode(raws, size=size, resize_to=(8, 8), place=[None, (0, -8), None, None])
    finally:
        dec.close()


@pytest.fixture(scope="module")
def squares():
    """One 64 x 64 grey and one 64 x 64 colour golden file: (raw, oracle pixels)."""
    raws = [(GOLDEN / "files" / name).read_bytes() for name in ("64x64_grey_pil.jpg", "64x64_420_pil.jpg")]
    fulls = oracle_rgb_all(raws)
    assert fulls[0].shape == (64, 64) and fulls[1].shape == (64, 64, 3)
    return list(zip(("grey", "colour"), raws, fulls))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
@pytest.mark.parametrize("dtype", ["uint8", "float16", "float32"])
@pytest.mark.parametrize("kind", ["native", "mode"])
def test_every_placed_instance_once(squares, kind, dtype, filter, layout):
    """Every placed instance of the four resize kernels — {native, converting} x {1-, 2-, 4-byte elements} x {unsigned, signed taps}
    x {grey, colour source} x both source orders, planar or not — on one small plan each: two copies of a 64 x 64 file resized to
    28 x 28 at (-3, 5) of a 40 x 24 canvas, the second one mirrored, float outputs normalised.  Asserted from the plan's reported
    shape: along the height there is a tile that is wholly fill (rows above 5), one that straddles the image's edge, and tiles
    wholly inside its rows; a tile is as wide as the 40-column canvas, so every tile that meets the image also straddles its right
    edge (columns 25..39 are fill).  Bit-exact against tools/place_model.py over the oracle's pixels, flipped with the padding for
    the mirrored copy, then tools/normalize_model.py; the output buffer holds a sentinel first."""
    import torch
    from tools import mode_model, normalize_model
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    canvas, pl, flags = (40, 24), (28, 28, -3, 5), [0, 1]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for name, raw, full in squares:
            mode = None if kind == "native" else "RGB" if name == "grey" else "L"
            rm = mode_model.convert(rowmajor_window(full, whole(full)), mode)
            nc = 3 if rm.ndim == 3 else 1
            fill = (114, 7, 200) if nc == 3 else (99,)
            mean, std = (MEAN, STD) if nc == 3 else (MEAN[:1], STD[:1])
            prep = prepare_batch([raw, raw], dec.layout, 0)
            plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 2}, size=canvas, filter=filter, mode=mode, places=[pl, pl], fill=fill,
                          output=("uint8", None, None, flags) if dtype == "uint8" else (dtype, mean, std, flags))
            try:
                shape = plan.resize_shape()
                tr = shape["tile_rows"]
                assert shape["signed"] == (filter == "bicubic") and shape["tiles_y"] > 2, shape
                assert tr <= pl[3], "the first tile is wholly fill"
                assert pl[3] % tr != 0, "a tile straddles the image's upper edge"
                assert (pl[3] + tr - 1) // tr * tr + tr <= canvas[1], "a tile lies wholly inside the image's rows"
                out = torch.full((int(plan.info.rgb_bytes),), 0xA5, dtype=torch.uint8, device=torch.device("cuda", dec.ctx.device))
                plan.execute(0, out.data_ptr())
                plan.sync()
                assert not plan.read(rgb=False)["status"].any()
                got = out.cpu().numpy()
            finally:
                plan.close()
            placed = model((name, mode), rm, pl, canvas, fill if nc == 3 else fill[0], filter)
            for i in range(2):
                img = placed[:, ::-1] if flags[i] else placed
                want = as_layout(img if dtype == "uint8" else normalize_model.normalize(img, dtype, mean if nc == 3 else mean[0], std if nc == 3 else std[0]), layout)
                per = want.size * want.dtype.itemsize
                assert np.array_equal(got[i * per:(i + 1) * per].view(want.dtype).reshape(want.shape), want), (name, mode, i)
    finally:
        dec.close()
