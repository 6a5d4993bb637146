"""The resize `decode(..., size=(width, height))` computes, as a small NumPy model: what Pillow's
`Image.resize(size, Image.BILINEAR)` does to 8-bit images.  Tests hold the library's tap tables and the GPU's pixels to this
model, and the model to Pillow itself (tests/test_resize_host.py).

Per axis: double-precision triangle-filter weights whose support grows with the scale when shrinking (antialiasing), normalised,
rounded to 22-bit integers; the pixels are integer sums of those taps, rounded and clipped to 8 bits.  Two passes with a uint8
intermediate image: along the width first (if it changes), then along the height (if it changes)."""
import math

import numpy as np

PRECISION_BITS = 22


def axis_table(in_size: int, out_size: int):
    """(xmin[out_size], count[out_size], taps[out_size, ksize]) int32: output index xx is
    clip8((2^21 + sum_t taps[xx, t] * in[xmin[xx] + t]) >> 22) over t < count[xx]; taps behind count are zero."""
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be positive")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
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
            a = abs((x + lo - center + 0.5) * ss)
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v                               # left to right
        xmin[xx], count[xx] = lo, hi - lo
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            taps[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5)
    return xmin, count, taps


def resample_axis(a: np.ndarray, out_size: int, axis: int, table=None) -> np.ndarray:
    """One pass: uint8 array `a` resampled along `axis` to out_size entries."""
    a = np.moveaxis(np.asarray(a, dtype=np.uint8), axis, 0)
    xmin, count, taps = table if table is not None else axis_table(a.shape[0], out_size)
    out = np.empty((out_size,) + a.shape[1:], dtype=np.uint8)
    wide = a.astype(np.int64)
    for xx in range(out_size):
        n, lo = int(count[xx]), int(xmin[xx])
        k = taps[xx, :n].astype(np.int64).reshape((n,) + (1,) * (a.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (k * wide[lo:lo + n]).sum(axis=0)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img: np.ndarray, size) -> np.ndarray:
    """img: uint8 (H, W) or (H, W, C), row-major; size = (width, height).  Returns (height, width[, C])."""
    width, height = int(size[0]), int(size[1])
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.shape[1] != width:
        img = resample_axis(img, width, 1)
    if img.shape[0] != height:
        img = resample_axis(img, height, 0)
    return np.ascontiguousarray(img)
