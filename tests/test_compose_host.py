"""compose= without a GPU: tools/compose_model.py against Pillow's Image.paste of crops, mj_host_compose — the compose launch's own
resolve and job list — against the model on exactly sized arrays of random bits, mj_host_compose_resolve's rectangles (disjoint, a
partition of the canvas, painting them is the model), normalize_compose's and the C ABI's refusals by message, and mosaic_tiles
against the four-line formula."""
import numpy as np
import pytest

from compose_cases import (BITS, DTYPES, GEOMETRIES, LAYOUTS, N_SOURCES, all_cases, fill_for, grid64, model_compose, random_bits,
                           same_bits, shape_of)

CASES = all_cases()


def test_the_case_list_is_what_it_says():
    """source 4 is never named, the grid has 64 tiles in one output, and the random bits hold NaN patterns"""
    for name, (SW, SH), (W, H), outputs, _ in CASES:
        assert all(0 <= t[0] < N_SOURCES - 1 for tiles in outputs for t in tiles), name
    assert [len(o) for o in grid64(13, 9)[1]] == [64]
    for dtype, exp_mask, mant in (("float16", 0x7C00, 0x3FF), ("bfloat16", 0x7F80, 0x7F), ("float32", 0x7F800000, 0x7FFFFF)):
        a = random_bits(dtype, "rowmajor", 13, 9, 3)
        assert (((a & exp_mask) == exp_mask) & ((a & mant) != 0)).any(), dtype


@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_the_model_is_pillows_paste(mode):
    """canvas = Image.new(mode, (W, H), fill); canvas.paste(tile.crop((sx, sy, sx + w, sy + h)), (dx, dy)), in order"""
    from PIL import Image
    C = 3 if mode == "RGB" else 1
    for name, (SW, SH), (W, H), outputs, three in CASES:
        pre = random_bits("uint8", "rowmajor", SW, SH, C)
        fill = fill_for(1, C, three)
        got = model_compose(pre, outputs, (W, H), "rowmajor", fill)
        tiles = [Image.fromarray(pre[s], mode) for s in range(len(pre))]
        for m, entry in enumerate(outputs):
            canvas = Image.new(mode, (W, H), tuple(fill) if C == 3 else fill[0])
            for s, (dx, dy), (sx, sy, w, h) in entry:
                canvas.paste(tiles[s].crop((sx, sy, sx + w, sy + h)), (dx, dy))
            assert np.array_equal(np.asarray(canvas), got[m]), (name, (W, H), m)


def test_the_model_in_the_four_layouts_is_one_model():
    """the same (C, H, W) content in every layout gives the same (C, H, W) result"""
    from tools.erase_model import chw_view
    for name, (SW, SH), (W, H), outputs, three in CASES:
        for C in (1, 3):
            fill = fill_for(2, C, three)
            base = random_bits("float16", "planar_rowmajor", SW, SH, C)
            want = model_compose(base, outputs, (W, H), "planar_rowmajor", fill)
            for layout in LAYOUTS:
                pre = np.empty((len(base),) + shape_of(layout, SW, SH, C), dtype=base.dtype)
                for k in range(len(base)):
                    chw_view(pre[k], layout)[...] = chw_view(base[k], "planar_rowmajor")
                got = model_compose(pre, outputs, (W, H), layout, fill)
                assert got.shape == (len(outputs),) + shape_of(layout, W, H, C)
                for m in range(len(outputs)):
                    assert np.array_equal(chw_view(got[m], layout), chw_view(want[m], "planar_rowmajor")), (name, layout, C, m)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_host_twin_against_the_model(layout, C, dtype):
    """mj_host_compose on exactly sized arrays of random bits, NaN patterns among them: every case"""
    from pyjpegdecoder_amd import _binding as B
    es = np.dtype(BITS[dtype]).itemsize
    for name, (SW, SH), (W, H), outputs, three in CASES:
        pre = random_bits(dtype, layout, SW, SH, C)
        fill = fill_for(es, C, three)
        want = model_compose(pre, outputs, (W, H), layout, fill)
        got = B.host_compose(np.array(pre), LAYOUTS.index(layout), dtype, C, (SW, SH), (W, H), fill, outputs)
        assert same_bits(got.reshape(want.shape), want), (name, layout, C, dtype, (W, H))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_resolved_rectangles_partition_every_canvas(layout):
    """per output: pairwise disjoint, areas that sum to W x H, and painting them — source pixels or fill — is the model; an output
    with 64 tiles stays below the capacity the function reports"""
    from pyjpegdecoder_amd import _binding as B
    from tools.erase_model import chw_view
    C = 3
    for name, (SW, SH), (W, H), outputs, three in CASES:
        pre = random_bits("uint8", layout, SW, SH, C)
        fill = fill_for(1, C, three)
        want = model_compose(pre, outputs, (W, H), layout, fill)
        rects, cap = B.host_compose_resolve(LAYOUTS.index(layout), C, (SW, SH), N_SOURCES, (W, H), outputs)
        assert cap == sum((2 * len(t) + 1) ** 2 for t in outputs) and len(rects) < cap, (name, len(rects), cap)
        assert len(rects) >= len(outputs)
        painted = np.zeros_like(want)
        count = np.zeros((len(outputs), H, W), dtype=np.int32)
        for r in rects:
            m, x, y, w, h, s, sx, sy = (int(r[k]) for k in ("output", "x", "y", "width", "height", "source", "sx", "sy"))
            assert w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= W and y + h <= H, (name, r)
            count[m, y:y + h, x:x + w] += 1
            view = chw_view(painted[m], layout)
            if s < 0:
                view[:, y:y + h, x:x + w] = np.asarray(fill, dtype=np.uint8).reshape(C, 1, 1)
            else:
                assert 0 <= sx and 0 <= sy and sx + w <= SW and sy + h <= SH, (name, r)
                view[:, y:y + h, x:x + w] = chw_view(pre[s], layout)[:, sy:sy + h, sx:sx + w]
        assert (count == 1).all(), (name, layout, "the rectangles overlap or leave a hole")
        assert sum(int(r["width"]) * int(r["height"]) for r in rects) == len(outputs) * W * H
        assert np.array_equal(painted, want), (name, layout)
        if name == "grid64":
            assert len(outputs[0]) == 64 and len(rects) < cap == 129 * 129


def test_later_wins_and_order_matters():
    (SW, SH), (W, H) = GEOMETRIES[0]
    by_name = {c[0]: c for c in CASES if c[1] == (SW, SH) and c[2] == (W, H)}
    pre = random_bits("uint8", "rowmajor", SW, SH, 3)
    a = model_compose(pre, by_name["chain"][3], (W, H), "rowmajor", 0)
    b = model_compose(pre, by_name["chain_reversed"][3], (W, H), "rowmajor", 0)
    assert not np.array_equal(a, b)
    assert np.array_equal(a[0, 7:13, 9:18], pre[2][3:9, 4:13]) and np.array_equal(b[0, 1:7, 1:10], pre[0][0:6, 0:9])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
OK = dict(size=(21, 14), outputs=[[(0, (1, 1))], [(1, (0, 0), (0, 0, 4, 4))]])


def test_the_two_tile_forms():
    from pyjpegdecoder_amd import normalize_compose
    got = normalize_compose(dict(size=[21, 14], fill=7, outputs=[[(0, (-3, 2)), [1, [4, 5], [1, 2, 3, 4]]], []]), (13, 9), 2, 3)
    assert got == {"size": (21, 14), "fill": (7, 7, 7), "outputs": [[(0, (-3, 2), (0, 0, 13, 9)), (1, (4, 5), (1, 2, 3, 4))], []]}
    assert normalize_compose(None, None) is None and normalize_compose(None, (13, 9), 2, 3, mix=[None]) is None
    assert normalize_compose(dict(size=(5, 5), outputs=[[]], fill=(1, 2, 3)), (13, 9))["fill"] == (1, 2, 3)
    assert normalize_compose(dict(size=(5, 5), outputs=[[(np.int64(1), (np.int32(-2), 0))]]), (13, 9), 2, 1)["outputs"] == [[(1, (-2, 0), (0, 0, 13, 9))]]


REFUSALS = [
    (dict(compose=OK, size=None), "compose needs size"),
    (dict(compose=OK, return_seams=True), "compose and return_seams do not go together"),
    (dict(compose=OK, mix=[("cutmix", 1, (0, 0, 1, 1)), None]), "compose and mix do not go together"),
    (dict(compose=[OK]), "compose must be None or a dict"),
    (dict(compose=dict(OK, tiles=[])), "compose: unknown key 'tiles'"),
    (dict(compose=dict(outputs=OK["outputs"])), "compose: size is required"),
    (dict(compose=dict(OK, size=(21, 0))), "compose: size is required"),
    (dict(compose=dict(OK, size=(21, 65536))), "compose: size is required"),
    (dict(compose=dict(OK, size=21)), "compose: size is required"),
    (dict(compose=dict(size=(21, 14))), "compose: outputs must be a list"),
    (dict(compose=dict(OK, outputs=[])), "compose: outputs must be a list"),
    (dict(compose=dict(OK, outputs=((),))), "compose: outputs must be a list"),
    (dict(compose=dict(OK, outputs=[[], [(0, (0, 0))] * 65])), "compose: output 1: 65 tiles, more than 64"),
    (dict(compose=dict(OK, outputs=[[(0,)]])), r"compose: output 0, tile 0: a tile is \(source, \(dx, dy\)\)"),
    (dict(compose=dict(OK, outputs=[[], [(0, (0, 0)), (0, (0, 0), (0, 0, 1, 1), 3)]])), "compose: output 1, tile 1: a tile is"),
    (dict(compose=dict(OK, outputs=[[(2, (0, 0))]])), "compose: output 0, tile 0: source 2 is not the index of an output, an integer 0..1"),
    (dict(compose=dict(OK, outputs=[[(-1, (0, 0))]])), "compose: output 0, tile 0: source -1 is not"),
    (dict(compose=dict(OK, outputs=[[(0.0, (0, 0))]])), "compose: output 0, tile 0: source 0.0 is not"),
    (dict(compose=dict(OK, outputs=[[(0, (0.5, 0))]])), "compose: output 0, tile 0: the offset is two integers"),
    (dict(compose=dict(OK, outputs=[[(0, (0, 0, 0))]])), "compose: output 0, tile 0: the offset is two integers"),
    (dict(compose=dict(OK, outputs=[[(0, (0, 0), (0, 0, 1.0, 1))]])), "compose: output 0, tile 0: the window is four integers"),
    (dict(compose=dict(OK, outputs=[[(0, (0, 0), (0, 0, 1))]])), "compose: output 0, tile 0: the window is four integers"),
    (dict(compose=dict(OK, outputs=[[(0, (1 << 20, 0))]])), r"compose: output 0, tile 0: offset \(1048576, 0\) is 2\*\*20 or more"),
    (dict(compose=dict(OK, outputs=[[(0, (0, 0)), (0, (0, -(1 << 20)))]])), "compose: output 0, tile 1: offset"),
    (dict(compose=dict(OK, outputs=[[(0, (0, 0), (0, 0, 0, 1))]])), "compose: output 0, tile 0: the window's width and height must be at least 1"),
    (dict(compose=dict(OK, outputs=[[(0, (0, 0), (1, 0, 13, 9))]])), r"compose: output 0, tile 0: window \(1, 0, 13, 9\) is not inside the 13 x 9 tile canvas"),
    (dict(compose=dict(OK, outputs=[[(0, (0, 0), (0, -1, 2, 2))]])), "compose: output 0, tile 0: window .* is not inside"),
    (dict(compose=dict(OK, fill=(1, 2))), "compose: fill must be None, one byte or one per output component"),
    (dict(compose=dict(OK, fill=256)), "compose: fill must be 0..255"),
    (dict(compose=dict(OK, fill=(0, -1, 0))), "compose: fill must be 0..255"),
    (dict(compose=dict(OK, fill="grey")), "compose: fill must be None"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_what_normalize_compose_refuses(kw, msg):
    from pyjpegdecoder_amd import normalize_compose
    kw = dict(dict(size=(13, 9), return_seams=False, mix=None), **kw)
    with pytest.raises(ValueError, match=msg):
        normalize_compose(kw["compose"], kw["size"], 2, 3, kw["return_seams"], kw["mix"])


def test_an_also_entry_is_checked_with_its_own_keys():
    from pyjpegdecoder_amd.batch import normalize_also
    call = dict(size=(13, 9))
    groups = normalize_also([dict(size=(8, 8), compose=dict(size=(20, 20), outputs=[[(0, (1, 1))]]))], call, (13, 9))
    assert groups[0]["compose"]["size"] == (20, 20)
    with pytest.raises(ValueError, match=r"also\[0\]: compose: output 0, tile 0: window \(0, 0, 9, 9\) is not inside the 8 x 8 tile canvas"):
        normalize_also([dict(size=(8, 8), compose=dict(size=(20, 20), outputs=[[(0, (1, 1), (0, 0, 9, 9))]]))], call, (13, 9))
    with pytest.raises(ValueError, match=r"also\[0\]: compose and mix do not go together"):
        normalize_also([dict(size=(8, 8), mix=[("cutmix", 0, (0, 0, 1, 1))], compose=dict(size=(20, 20), outputs=[[]]))], call, (13, 9))


def _tiles(*rows):
    from pyjpegdecoder_amd import _binding as B
    a = np.zeros(len(rows), dtype=B.COMPOSE_TILE_DTYPE)
    for k, row in enumerate(rows):
        a[k] = row
    return a


def test_what_the_c_abi_refuses():
    """mj_host_compose: MJ_ERR_INVALID with a message that names the tile — and nothing is written"""
    import ctypes
    from pyjpegdecoder_amd import _binding as B
    src = np.array(random_bits("uint8", "rowmajor", 13, 9, 3))

    def call(tiles, n_outputs=2, layout=1, dtype="uint8", C=3, ssize=(13, 9), dsize=(21, 14), s=None):
        return B.host_compose(src if s is None else s, layout, dtype, C, ssize, dsize, (1, 2, 3), tiles, n_outputs=n_outputs)
    good = (1, 0, 0, 0, 13, 9, 2, 2)        # (output, source, sx, sy, width, height, dx, dy)
    assert call(_tiles(good)).shape == (2, 21 * 14 * 3)
    for tiles, msg in [(_tiles(good, (2, 0, 0, 0, 1, 1, 0, 0)), "mj_host_compose: tile 1 .output 2, source 0.*no such output"),
                       (_tiles((-1, 0, 0, 0, 1, 1, 0, 0)), "tile 0 .*no such output"),
                       (_tiles(good, (0, 5, 0, 0, 1, 1, 0, 0)), "tile 1 .*no such source"),
                       (_tiles((0, -1, 0, 0, 1, 1, 0, 0)), "tile 0 .*no such source"),
                       (_tiles((0, 0, 0, 0, 0, 1, 0, 0)), "tile 0 .*a width or height below 1"),
                       (_tiles((0, 0, 1, 0, 13, 9, 0, 0)), "tile 0 .*the window is not inside the source canvas"),
                       (_tiles((0, 0, 0, -1, 2, 2, 0, 0)), "tile 0 .*the window is not inside the source canvas"),
                       (_tiles((0, 0, 0, 0, 2, 2, 1 << 20, 0)), "tile 0 .*an offset of 2.20 or more"),
                       (_tiles((0, 0, 0, 0, 2, 2, 0, -(1 << 20))), "tile 0 .*an offset of 2.20 or more"),
                       (_tiles(*([good] * 65)), "tile 64 .*more than 64 tiles in one output")]:
        with pytest.raises(ValueError, match=msg):
            call(tiles)
    ok = _tiles(good)
    for kw, msg in [(dict(layout=4), "layout 4"), (dict(C=2), "2 components"), (dict(ssize=(0, 9)), "sources of 0 x 9"), (dict(dsize=(21, 65536)), "outputs of 21 x 65536"),
                    (dict(n_outputs=0), "0 outputs"), (dict(s=src[:0]), "0 sources")]:
        with pytest.raises(ValueError, match=msg):
            call(ok, **kw)
    L = B.load_library()
    dst = np.full((2, 21 * 14 * 3), 0x5A, dtype=np.uint8)
    tiles, n, _keep = B.compose_tiles(ok)
    fill = (ctypes.c_uint32 * 3)(1, 2, 3)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    u8 = B.DTYPES["uint8"]
    assert L.mj_host_compose(None, p(dst), 1, u8, 3, 13, 9, 5, 21, 14, 2, fill, n, tiles) == B.MJ_ERR_INVALID and b"NULL" in L.mj_last_error(None)
    assert L.mj_host_compose(p(src), p(dst), 1, u8, 3, 13, 9, 5, 21, 14, 2, None, n, tiles) == B.MJ_ERR_INVALID and b"NULL" in L.mj_last_error(None)
    assert L.mj_host_compose(p(src), p(dst), 1, u8, 3, 13, 9, 5, 21, 14, 2, fill, 1, None) == B.MJ_ERR_INVALID and b"NULL" in L.mj_last_error(None)
    assert L.mj_host_compose(p(src), p(dst), 1, 9, 3, 13, 9, 5, 21, 14, 2, fill, n, tiles) == B.MJ_ERR_INVALID and b"dtype 9" in L.mj_last_error(None)
    assert L.mj_host_compose(p(src), p(dst), 1, u8, 3, 13, 9, 5, 21, 14, 2, fill, -1, tiles) == B.MJ_ERR_INVALID and b"-1 tiles" in L.mj_last_error(None)
    both = np.zeros(5 * 13 * 9 * 3 + 2 * 21 * 14 * 3, dtype=np.uint8)
    assert L.mj_host_compose(p(both), ctypes.c_void_p(both.ctypes.data + 100), 1, u8, 3, 13, 9, 5, 21, 14, 2, fill, n, tiles) == B.MJ_ERR_INVALID
    assert b"overlap" in L.mj_last_error(None)
    f32 = np.zeros(5 * 13 * 9 * 3 + 1, dtype=np.float32)
    out32 = np.zeros(2 * 21 * 14 * 3 + 1, dtype=np.float32)
    assert L.mj_host_compose(ctypes.c_void_p(f32.ctypes.data + 2), p(out32), 1, B.DTYPES["float32"], 3, 13, 9, 5, 21, 14, 2, fill, n, tiles) == B.MJ_ERR_INVALID
    assert b"not aligned to its 4-byte elements" in L.mj_last_error(None)
    assert (dst == 0x5A).all()              # a refused call wrote nothing
    # no tiles at all: every canvas is fill
    got = B.host_compose(src, 1, "uint8", 3, (13, 9), (21, 14), (1, 2, 3), [[], []])
    assert np.array_equal(got.reshape(2, 14, 21, 3), np.broadcast_to(np.array([1, 2, 3], dtype=np.uint8), (2, 14, 21, 3)))


def test_the_library_exports_the_calls():
    from pyjpegdecoder_amd import _binding as B
    L = B.load_library()
    for name in ("mj_compose", "mj_compose_time", "mj_host_compose", "mj_host_compose_resolve"):
        assert name in B.EXPORTS and hasattr(L, name)


# ---- mosaic_tiles -----------------------------------------------------------------------------------------------------------
def _mosaic4(size, centre, tile_sizes):
    """Ultralytics' Mosaic._mosaic4, its four lines written out for a W x H canvas (2 s x 2 s there): (x1a, y1a, x2a, y2a) on the
    canvas and (x1b, y1b, x2b, y2b) in the image; canvas[y1a:y2a, x1a:x2a] = img[y1b:y2b, x1b:x2b]"""
    (W, H), (xc, yc) = size, centre
    out = []
    for i, (w, h) in enumerate(tile_sizes):
        if i == 0:
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
        elif i == 1:
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, W), yc
            x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
        elif i == 2:
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(H, yc + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, min(y2a - y1a, h)
        else:
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, W), min(H, yc + h)
            x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
        out.append(((x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b)))
    return out


@pytest.mark.parametrize("size,centre,tile_sizes,n", [
    ((640, 640), (300, 350), [(320, 240), (200, 320), (320, 213), (240, 320)], 4),
    ((640, 640), (160, 480), [(320, 320)] * 4, 4),                      # images larger than their quadrant
    ((64, 48), (10, 40), [(30, 44), (64, 48), (33, 9), (100, 100)], 4),
    ((640, 640), (0, 0), [(320, 240)] * 4, 1),                          # the centre at a corner: three images drop out
    ((640, 640), (640, 640), [(320, 240)] * 4, 1),
    ((640, 640), (640, 0), [(320, 240)] * 4, 1),
    ((640, 640), (0, 300), [(320, 240)] * 4, 2),
])
def test_mosaic_tiles_against_the_formula(size, centre, tile_sizes, n):
    from pyjpegdecoder_amd import mosaic_tiles, normalize_compose
    tiles = mosaic_tiles(size, centre, tile_sizes)
    assert len(tiles) == n
    want = _mosaic4(size, centre, tile_sizes)
    seen = set()
    for i, (dx, dy), (sx, sy, w, h) in tiles:
        (x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b) = want[i]
        assert (dx, dy, dx + w, dy + h) == (x1a, y1a, x2a, y2a) and (sx, sy, sx + w, sy + h) == (x1b, y1b, x2b, y2b), i
        assert 0 <= sx and 0 <= sy and sx + w <= tile_sizes[i][0] and sy + h <= tile_sizes[i][1]
        seen.add(i)
    for i, ((x1a, y1a, x2a, y2a), _) in enumerate(want):
        assert (i in seen) == (x2a > x1a and y2a > y1a)
    # what it returns is what compose= takes, on tile canvases that hold the images
    tw, th = max(w for w, _ in tile_sizes), max(h for _, h in tile_sizes)
    assert normalize_compose(dict(size=size, outputs=[tiles]), (tw, th), 4, 3)["outputs"] == [tiles]
