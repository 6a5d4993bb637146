"""The colour operations of `decode(..., size=, color_ops=)`, restated in NumPy: what one call of Pillow's ``ImageEnhance.*`` or
``ImageOps.*`` does to the bytes of an 8-bit "RGB" or "L" image.  The GPU path (csrc/colour.hip) and its host twin
(mj_host_colour_ops) are held to this model, and the model to Pillow itself (tests/test_colour_host.py) — bytes, not tolerances.

A chain is a sequence of ops applied in order to the finished uint8 canvas of an output, in front of the mirror and the output's
element type (tools/normalize_model.py).  An op is a tuple whose first element is its name:

    ("brightness", f)  ("color", f)  ("contrast", f)  ("sharpness", f)      ImageEnhance.<Name>(im).enhance(f)
    ("posterize", bits)  ("solarize", t)  ("autocontrast",)  ("equalize",)  ("invert",)      ImageOps.<name>(im[, value])

Images are row-major: (H, W, 3) for "RGB", (H, W) for "L".

The four enhancers are ``Image.blend(degenerate, image, f)`` with their own degenerate image (blend).  Everything else is a
look-up table per band; three of them — contrast's mean, autocontrast and equalize — are made from the image's histogram.
"""
import math

import numpy as np

from tools import mode_model

MAX_OPS = 4
OPS = ("brightness", "color", "contrast", "sharpness", "posterize", "solarize", "autocontrast", "equalize", "invert")
VALUED = ("brightness", "color", "contrast", "sharpness", "posterize", "solarize")       # ops that take a value


def blend(d: np.ndarray, v: np.ndarray, f: float) -> np.ndarray:
    """Image.blend(d, v, f) of uint8 arrays: t = fl32(fl32(d) + fl32(alpha * fl32(v - d))) with alpha = float32(f) and v - d an
    int; for 0 <= alpha <= 1 the byte is t truncated, otherwise 0 where t <= 0, 255 where t >= 255, else t truncated."""
    alpha = np.float32(f)
    diff = (v.astype(np.int32) - d.astype(np.int32)).astype(np.float32)
    t = d.astype(np.float32) + alpha * diff           # (float32 arrays: every operation rounds to float32)
    if 0.0 <= alpha <= 1.0:
        return t.astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.uint8))).astype(np.uint8)


def grey(a: np.ndarray) -> np.ndarray:
    """the image's L: Pillow's convert("L") of a colour image, the image itself for "L" """
    return mode_model.luma(a[..., 0], a[..., 1], a[..., 2]) if a.ndim == 3 else a


def contrast_mean(a: np.ndarray) -> int:
    """ImageEnhance.Contrast's grey level: int(mean of the image's L + 0.5), the mean a double division of exact integers"""
    h = np.bincount(grey(a).ravel(), minlength=256)
    total = sum(i * int(h[i]) for i in range(256))
    return int(total / int(h.sum()) + 0.5)


def smooth(a: np.ndarray) -> np.ndarray:
    """im.filter(ImageFilter.SMOOTH): the 3 x 3 kernel (1,1,1, 1,5,1, 1,1,1) / 13 in float32, rows added bottom-up onto 0.5, every
    product and sum rounded on its own; the first and last row and column are copied; bands separately."""
    out = a.copy()
    h, w = a.shape[:2]
    if h < 3 or w < 3:
        return out
    k1, k5 = np.float32(1 / 13.0), np.float32(5 / 13.0)
    p = a.astype(np.float32)

    def row(r, km):
        return (r[:, :-2] * k1 + r[:, 1:-1] * km) + r[:, 2:] * k1
    ss = np.full(p[1:-1, 1:-1].shape, np.float32(0.5), dtype=np.float32)
    ss = ss + row(p[2:], k1)
    ss = ss + row(p[1:-1], k5)
    ss = ss + row(p[:-2], k1)
    out[1:-1, 1:-1] = np.where(ss <= 0, 0, np.where(ss >= 255, 255, np.clip(ss, 0, 255).astype(np.uint8)))
    return out


def autocontrast_table(h) -> np.ndarray:
    """ImageOps.autocontrast's table of one band with histogram ``h`` (cutoff 0): identity, or the stretch of [lo, hi] to [0, 255]"""
    nz = [i for i in range(256) if h[i]]
    lut = np.arange(256, dtype=np.uint8)
    if not nz or nz[-1] <= nz[0]:
        return lut
    lo, hi = nz[0], nz[-1]
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    for i in range(256):
        lut[i] = min(max(int(i * scale + offset), 0), 255)
    return lut


def equalize_table(h) -> np.ndarray:
    """ImageOps.equalize's table of one band with histogram ``h``; the clip at 255 is Pillow's conversion of the table to bytes"""
    nz = [int(v) for v in h if v]
    lut = np.arange(256, dtype=np.uint8)
    if len(nz) <= 1:
        return lut
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return lut
    n = step // 2
    for i in range(256):
        lut[i] = min(255, n // step)
        n += int(h[i])
    return lut


def solarize_threshold(t: float) -> int:
    """what the layer compares with: v stays where v < t, i.e. v < ceil(t) for a byte; clamped to 0..256"""
    return min(max(math.ceil(t), 0), 256)


def _per_band(a: np.ndarray, table_of) -> np.ndarray:
    if a.ndim == 2:
        return table_of(np.bincount(a.ravel(), minlength=256))[a]
    return np.stack([table_of(np.bincount(a[..., c].ravel(), minlength=256))[a[..., c]] for c in range(a.shape[2])], axis=-1)


def apply_op(a: np.ndarray, op) -> np.ndarray:
    """one op on a uint8 (H, W, 3) or (H, W) image"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    name = op[0]
    if name not in OPS or len(op) != (2 if name in VALUED else 1):
        raise ValueError(f"no colour op {op!r}")
    if name == "brightness":
        return blend(np.zeros_like(a), a, op[1])
    if name == "color":
        return a if a.ndim == 2 else blend(np.repeat(grey(a)[..., None], 3, axis=-1), a, op[1])
    if name == "contrast":
        return blend(np.full_like(a, contrast_mean(a)), a, op[1])
    if name == "sharpness":
        return blend(smooth(a), a, op[1])
    if name == "posterize":
        bits = int(op[1])
        if not 1 <= bits <= 8:
            raise ValueError(f"posterize takes 1..8 bits, not {op[1]!r}")
        return a & np.uint8(~((1 << (8 - bits)) - 1) & 0xFF)
    if name == "solarize":
        return np.where(a < solarize_threshold(op[1]), a, 255 - a).astype(np.uint8)
    if name == "invert":
        return (255 - a).astype(np.uint8)
    return _per_band(a, autocontrast_table if name == "autocontrast" else equalize_table)


def apply_chain(a: np.ndarray, chain) -> np.ndarray:
    """``chain`` (None or a sequence of at most MAX_OPS ops) on a uint8 (H, W, 3) or (H, W) image"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if chain is None:
        return a
    if len(chain) > MAX_OPS:
        raise ValueError(f"a chain has at most {MAX_OPS} ops, not {len(chain)}")
    for op in chain:
        a = apply_op(a, op)
    return a
