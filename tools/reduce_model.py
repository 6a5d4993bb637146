"""The two-step resize `decode(..., size=..., reducing_gap=g)` computes, as a small NumPy model: what Pillow's
`Image.resize(size, filter, reducing_gap=g)` does to 8-bit images.  First `Image.reduce((fx, fy))` — a box average over integer
cells, one rounding — then the resample of the reduced image over the fractional box (0, 0, w / fx, h / fy), which Pillow
carries as 32-bit floats.  Tests hold the library's host twins and the GPU's pixels to this model, and the model to Pillow itself
(tests/test_reduce_host.py).

`reduce` takes phases: the library reduces images in stored order, and for an axis the orientation reverses the cell
boundaries lie at phase + k * f with phase = size mod f — the partial cell comes first — so that the reduced stored-order image
is the stored-order counterpart of Pillow's reduced oriented image."""
import math

import numpy as np

from tools import resize_model

PRECISION_BITS = resize_model.PRECISION_BITS
FILTERS = resize_model.FILTERS
MAX_CELL = 65536        # pixels per cell the library takes: every sum and product stays inside 32 bits, as Pillow's are


def reduce_factors(src_w: int, src_h: int, dst_w: int, dst_h: int, gap: float):
    """(fx, fy) of Image.resize((dst_w, dst_h), reducing_gap=gap) on a src_w x src_h image: doubles, divided in this order."""
    if not gap >= 1.0:
        raise ValueError("reducing_gap must be 1.0 or greater")
    return int(src_w / dst_w / gap) or 1, int(src_h / dst_h / gap) or 1


def multiplier(n: int) -> int:
    """m(n) = (uint32)(float32(2^32) / float32(256 n)): a float32 division, truncated"""
    return int(np.float32(4294967296.0) / np.float32(256 * n))


def cells(size: int, f: int, phase: int = 0):
    """[(start, end)] of the ceil(size / f) cells of an axis: boundaries at phase + k * f (phase 0: at k * f)"""
    off = (f - phase) if phase else 0
    n = -(-size // f)
    return [(max(0, k * f - off), min(size, (k + 1) * f - off)) for k in range(n)]


def reduce(img: np.ndarray, fx: int, fy: int, phase_x: int = 0, phase_y: int = 0) -> np.ndarray:
    """img: uint8 (H, W) or (H, W, C).  Returns (ceil(H / fy), ceil(W / fx)[, C]): every cell's
    ((sum + n // 2) * m(n)) >> 24 in 32-bit unsigned arithmetic, n the cell's own pixel count."""
    img = np.asarray(img, dtype=np.uint8)
    cx, cy = cells(img.shape[1], fx, phase_x), cells(img.shape[0], fy, phase_y)
    # (sums along the height, then along the width: integer sums, any order)
    s = np.add.reduceat(img.astype(np.uint64), [a for a, _ in cy], axis=0)
    s = np.add.reduceat(s, [a for a, _ in cx], axis=1)
    n = np.outer([b - a for a, b in cy], [b - a for a, b in cx]).astype(np.uint64)
    m = np.zeros(n.shape, dtype=np.uint64)
    for v in np.unique(n):
        m[n == v] = multiplier(int(v))
    if img.ndim == 3:
        n, m = n[:, :, None], m[:, :, None]
    return ((((s + n // 2) * m) & 0xFFFFFFFF) >> 24).astype(np.uint8)


def axis_table(in_size: int, out_size: int, filter: str = "bilinear", box=None, box32: bool = True):
    """resize_model.axis_table over the part [box[0], box[1]) of the axis (None: the whole axis, the identical table).  The box is
    rounded to float32 (``box32`` False: kept in doubles — not what Pillow does; the tests show the difference)."""
    if box is None:
        return resize_model.axis_table(in_size, out_size, filter)
    if box32:
        in0, in1 = np.float32(box[0]), np.float32(box[1])
        span = float(in1 - in0)                   # (a float32 subtraction)
        in0 = float(in0)
    else:
        in0, span = float(box[0]), float(box[1]) - float(box[0])
    fsupport, weight = FILTERS[filter]
    scale = span / out_size
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ss = 1.0 / filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, dtype=np.int32)
    count = np.zeros(out_size, dtype=np.int32)
    taps = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        lo = max(0, int(center - support + 0.5))
        hi = min(in_size, int(center + support + 0.5))
        w = []
        ww = 0.0
        for x in range(hi - lo):
            v = weight((x + lo - center + 0.5) * ss)
            w.append(v)
            ww += v
        xmin[xx], count[xx] = lo, hi - lo
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            taps[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
    return xmin, count, taps


def tall(width: int, height: int, out_height: int) -> bool:
    """Pillow resamples such an image along the height first — a pass order this model (and the library) does not have"""
    return height > 100 * width and out_height < height


def resize(img: np.ndarray, size, filter: str = "bilinear", reducing_gap=None, box32: bool = True) -> np.ndarray:
    """img: uint8 (H, W) or (H, W, C), row-major; size = (width, height).  Image.resize(size, filter, reducing_gap=...):
    without a gap, or with both factors 1, resize_model.resize; else the reduce, then the two passes over the float32 box —
    a pass runs when the size changes or the box is not the whole axis."""
    width, height = int(size[0]), int(size[1])
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    if reducing_gap is None:
        return resize_model.resize(img, size, filter)
    fx, fy = reduce_factors(w, h, width, height, reducing_gap)
    if fx == 1 and fy == 1:
        return resize_model.resize(img, size, filter)
    img = reduce(img, fx, fy)
    bx, by = (0.0, w / fx), (0.0, h / fy)
    cast = (lambda v: float(np.float32(v))) if box32 else float
    if img.shape[1] != width or cast(bx[1]) != width:
        img = resize_model.resample_axis(img, width, 1, table=axis_table(img.shape[1], width, filter, bx, box32))
    if img.shape[0] != height or cast(by[1]) != height:
        img = resize_model.resample_axis(img, height, 0, table=axis_table(img.shape[0], height, filter, by, box32))
    return np.ascontiguousarray(img)
