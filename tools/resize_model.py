"""The resize `decode(..., size=(width, height), resample=...)` computes, as a small NumPy model: what Pillow's
`Image.resize(size, filter)` does to 8-bit images, for its convolution filters — BILINEAR (the default), BOX, HAMMING, BICUBIC
and LANCZOS.  Tests hold the library's tap tables and the GPU's pixels to this model, and the model to Pillow itself
(tests/test_resize_host.py, tests/test_resample_host.py).

Per axis: double-precision filter weights whose support grows with the scale when shrinking (antialiasing), normalised,
rounded away from zero to 22-bit integers; the pixels are integer sums of those taps, rounded and clipped to 8 bits at both
ends (the taps of BICUBIC and LANCZOS are negative in their side lobes).  Two passes with a uint8 intermediate image: along the
width first (if it changes), then along the height (if it changes)."""
import math

import numpy as np

PRECISION_BITS = 22

_F054, _F046 = float(np.float32(0.54)), float(np.float32(0.46))      # Pillow writes these two as float literals


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _box(x: float) -> float:
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _hamming(x: float) -> float:
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_F054 + _F046 * math.cos(x))


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# name -> (support, weight function); the order is the library's MJ_FILTER_* numbering
FILTERS = {"bilinear": (1.0, _bilinear), "box": (0.5, _box), "hamming": (1.0, _hamming), "bicubic": (2.0, _bicubic),
           "lanczos": (3.0, _lanczos)}


def axis_table(in_size: int, out_size: int, filter: str = "bilinear"):
    """(xmin[out_size], count[out_size], taps[out_size, ksize]) int32: output index xx is
    clip8((2^21 + sum_t taps[xx, t] * in[xmin[xx] + t]) >> 22) over t < count[xx]; taps behind count are zero."""
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be positive")
    fsupport, weight = FILTERS[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ss = 1.0 / filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, dtype=np.int32)
    count = np.zeros(out_size, dtype=np.int32)
    taps = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(0, int(center - support + 0.5))
        hi = min(in_size, int(center + support + 0.5))
        w = []
        ww = 0.0
        for x in range(hi - lo):
            v = weight((x + lo - center + 0.5) * ss)
            w.append(v)
            ww += v                               # left to right
        xmin[xx], count[xx] = lo, hi - lo
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            taps[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)   # away from zero
    return xmin, count, taps


def resample_axis(a: np.ndarray, out_size: int, axis: int, table=None, filter: str = "bilinear", clipped=None) -> np.ndarray:
    """One pass: uint8 array `a` resampled along `axis` to out_size entries.  ``clipped``: None, or a list that receives
    (sums whose shifted value lay below 0, sums whose shifted value lay above 255) — how often the pass reached either clamp."""
    a = np.moveaxis(np.asarray(a, dtype=np.uint8), axis, 0)
    xmin, count, taps = table if table is not None else axis_table(a.shape[0], out_size, filter)
    out = np.empty((out_size,) + a.shape[1:], dtype=np.uint8)
    wide = a.astype(np.int64)
    below = above = 0
    for xx in range(out_size):
        n, lo = int(count[xx]), int(xmin[xx])
        k = taps[xx, :n].astype(np.int64).reshape((n,) + (1,) * (a.ndim - 1))
        acc = ((1 << (PRECISION_BITS - 1)) + (k * wide[lo:lo + n]).sum(axis=0)) >> PRECISION_BITS      # (arithmetic shift)
        below += int((acc < 0).sum())
        above += int((acc > 255).sum())
        out[xx] = np.clip(acc, 0, 255)
    if clipped is not None:
        clipped.append((below, above))
    return np.moveaxis(out, 0, axis)


def resize(img: np.ndarray, size, filter: str = "bilinear", clipped=None) -> np.ndarray:
    """img: uint8 (H, W) or (H, W, C), row-major; size = (width, height).  Returns (height, width[, C]).  ``clipped``: as
    :func:`resample_axis`, one entry per pass that ran (width first)."""
    width, height = int(size[0]), int(size[1])
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.shape[1] != width:
        img = resample_axis(img, width, 1, filter=filter, clipped=clipped)
    if img.shape[0] != height:
        img = resample_axis(img, height, 0, filter=filter, clipped=clipped)
    return np.ascontiguousarray(img)
