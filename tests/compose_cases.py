"""What the compose tests share (tests/test_compose_host.py on the CPU, tests/test_compose.py and tests/test_compose_routes.py on the
MI355X): the geometries, the tile lists, the fills, arrays of random bits, and the model by import.

Tile canvases are 13 x 9 and 24 x 16, composed canvases 21 x 14 and 37 x 23, and an 8 x 8 grid of 64 tiles of 4 x 3 goes on a 41 x 33
canvas.  Every case has N_SOURCES = 5 sources and names at most the first four: source 4 is the one no one names."""
import numpy as np

from erase_cases import LAYOUTS, same_bits, storage  # noqa: F401

# (tile canvas, composed canvas)
GEOMETRIES = (((13, 9), (21, 14)), ((24, 16), (37, 23)))
N_SOURCES = 5
DTYPES = ("uint8", "float16", "bfloat16", "float32")
BITS = {"uint8": np.uint8, "float16": np.uint16, "bfloat16": np.uint16, "float32": np.uint32}
# element bit patterns per component, by element size: all different, a NaN pattern among them
FILL_BITS = {1: (0xA5, 0x3C, 0x7F), 2: (0x7E01, 0x3C00, 0xFBFF), 4: (0x7FC00001, 0x3F800000, 0xFF7FFFFF)}


def full_form(outputs, SW, SH):
    """every tile as (source, (dx, dy), (sx, sy, w, h))"""
    return [[(t[0], tuple(t[1]), tuple(t[2]) if len(t) > 2 else (0, 0, SW, SH)) for t in tiles] for tiles in outputs]


def grid64(SW, SH):
    """((W, H), outputs): ONE output of 64 tiles of 4 x 3 — windows at different places of the sources — with one-pixel gutters"""
    tiles = [(k % 4, (1 + 5 * (k % 8), 1 + 4 * (k // 8)), (k % (SW - 3), k % (SH - 2), 4, 3)) for k in range(64)]
    return (41, 33), [tiles]


def cases(SW, SH, W, H):
    """{name: (outputs, three_fills)} on W x H canvases from SW x SH tiles; ``three_fills``: the fill has three different components
    (else one element for all)"""
    chain = [(0, (1, 1), (0, 0, 9, 6)), (1, (5, 4), (2, 1, 9, 6)), (2, (9, 7), (4, 3, 9, 6))]
    out = {
        "whole": ([[(0, (3, 2))]], False),
        "corner_pixels": ([[(0, (0, 0), (0, 0, 1, 1)), (1, (W - 1, 0), (SW - 1, 0, 1, 1)), (2, (0, H - 1), (0, SH - 1, 1, 1)),
                            (3, (W - 1, H - 1), (SW - 1, SH - 1, 1, 1))]], True),
        "odd_window": ([[(1, (5, 3), (3, 1, 7, 5))]], False),
        "clipped": ([[(0, (-4, 2))], [(1, (W - 5, 2))], [(2, (3, -3))], [(3, (3, H - 4))], [(0, (-6, -5))], [(1, (W - 3, H - 2))]], True),
        "outside_and_empty": ([[(0, (W, 0))], [(1, (-SW, 3))], [(2, (3, H + 5))], [(3, (3, -SH))], []], True),
        "exact_cover": ([[(0, (0, 0)), (1, (SW, 0), (0, 0, W - SW, SH)), (2, (0, SH), (0, 0, SW, H - SH)), (3, (SW, SH), (2, 1, W - SW, H - SH))]], True),
        "chain": ([chain], False),
        "chain_reversed": ([chain[::-1]], False),
        "twice_in_one": ([[(0, (0, 0), (0, 0, 6, 5)), (0, (8, 6), (3, 2, 7, 6))]], True),
        "twice_in_two": ([[(1, (2, 2))], [(1, (4, 1), (1, 1, 5, 5))]], False),
        "three_fills": ([[(2, (6, 4), (1, 2, 5, 3))], []], True),
    }
    return {name: (full_form(outputs, SW, SH), three) for name, (outputs, three) in out.items()}


def all_cases():
    """[(name, (SW, SH), (W, H), outputs, three_fills)]: every case on both geometries, and the grid"""
    out = []
    for (SW, SH), (W, H) in GEOMETRIES:
        out += [(name, (SW, SH), (W, H), outputs, three) for name, (outputs, three) in cases(SW, SH, W, H).items()]
    size, outputs = grid64(13, 9)
    out.append(("grid64", (13, 9), size, outputs, True))
    return out


def fill_for(esize: int, C: int, three: bool):
    """the fill's element bit patterns, one per component"""
    f = FILL_BITS[esize]
    return list(f[:C]) if three else [f[1]] * C


def shape_of(layout: str, W: int, H: int, C: int):
    wh = (W, H) if layout in ("xmajor", "planar") else (H, W)
    if C == 1:
        return wh
    return (C,) + wh if layout.startswith("planar") else wh + (C,)


_bits = {}


def random_bits(dtype: str, layout: str, SW: int, SH: int, C: int, n: int = N_SOURCES):
    """``n`` tile canvases of random bit patterns (NaN patterns among the float ones), as unsigned integers of the element size"""
    key = (dtype, layout, SW, SH, C, n)
    if key not in _bits:
        t = BITS[dtype]
        rng = np.random.default_rng(SW * 1000 + SH * 10 + C + np.dtype(t).itemsize)
        a = rng.integers(0, 1 << (8 * np.dtype(t).itemsize), size=(n,) + shape_of(layout, SW, SH, C), dtype=np.uint64).astype(t)
        a.setflags(write=False)
        _bits[key] = a
    return _bits[key]


def model_compose(pre: np.ndarray, outputs, size, layout: str, fill) -> np.ndarray:
    from tools import compose_model
    return compose_model.compose(pre, outputs, size, layout, fill=np.asarray(fill, dtype=pre.dtype) if not np.isscalar(fill) else fill)
