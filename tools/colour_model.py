"""The colour operations of `decode(..., size=, color_ops=)`, restated in NumPy: what one call of Pillow's ``ImageEnhance.*`` or
``ImageOps.*`` does to the bytes of an 8-bit "RGB" or "L" image.  The GPU path (csrc/colour.hip) and its host twin
(mj_host_colour_ops) are held to this model, and the model to Pillow itself (tests/test_colour_host.py) — bytes, not tolerances.

A chain is a sequence of ops applied in order to the finished uint8 canvas of an output, in front of the mirror and the output's
element type (tools/normalize_model.py).  An op is a tuple whose first element is its name:

    ("brightness", f)  ("color", f)  ("contrast", f)  ("sharpness", f)      ImageEnhance.<Name>(im).enhance(f)
    ("posterize", bits)  ("solarize", t)  ("autocontrast",)  ("equalize",)  ("invert",)      ImageOps.<name>(im[, value])
    ("gaussian_blur", radius)  ("box_blur", radius)      im.filter(ImageFilter.GaussianBlur(radius) / BoxBlur(radius)), 0 <= radius <= 1024
    ("adjust_hue", f)      torchvision's F.adjust_hue(im, f), -0.5 <= f <= 0.5: the H of im.convert("HSV") plus hue_shift(f), and back

Images are row-major: (H, W, 3) for "RGB", (H, W) for "L".

The four enhancers are ``Image.blend(degenerate, image, f)`` with their own degenerate image (blend).  Everything else is a
look-up table per band; three of them — contrast's mean, autocontrast and equalize — are made from the image's histogram.

The two blurs are Pillow's BoxBlur.c: passes of one box filter with a fractional radius along the width, then along the height
(box_pass) — one pass each for box_blur, three each for gaussian_blur with the box radius gaussian_box_radius gives.  Every pass
stores bytes, and the next pass reads those bytes.

adjust_hue is Pillow's Convert.c both ways (rgb_to_hsv, hsv_to_rgb) around a byte addition that wraps.  The round trip alone — factor
0 — changes most colours: torchvision takes it whenever the op is called, and so does this model.  An "L" image is returned as it is.
"""
import math

import numpy as np

from tools import mode_model

MAX_OPS = 4
OPS = ("brightness", "color", "contrast", "sharpness", "posterize", "solarize", "autocontrast", "equalize", "invert", "gaussian_blur", "box_blur")
VALUED = ("brightness", "color", "contrast", "sharpness", "posterize", "solarize", "gaussian_blur", "box_blur")       # ops that take a value
TORCHVISION_OPS = ("adjust_hue",)       # the op that is torchvision's and not Pillow's (OPS stays Pillow's own; it takes a value too)
MAX_RADIUS = 1024


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


def gaussian_box_radius(radius: float) -> np.float32:
    """the radius of the box filter whose three passes stand for a Gaussian of this radius (BoxBlur.c: _gaussian_blur_radius with
    passes = 3): float32 throughout, except that the square root and the floor are taken in double"""
    f = np.float32
    sigma2 = f(f(radius) * f(radius)) / f(3)
    L = f(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * sigma2)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = a / (f(6) * (sigma2 - (l + f(1)) * (l + f(1))))
    return f(l + a)


def box_weights(fr) -> tuple:
    """(r, ww, fw) of one pass with box radius ``fr``: its whole part, the 8.24 weight of a pixel inside it and that of the two
    pixels just outside — ww = (uint32)(fl32(1 << 24) / fl32(fr * 2 + 1)), fw = ((1 << 24) - (2 r + 1) ww) / 2 in 32-bit unsigned"""
    fr = np.float32(fr)
    r = int(fr)
    ww = int(np.float32(1 << 24) / (fr * np.float32(2) + np.float32(1))) & 0xFFFFFFFF
    fw = (((1 << 24) - (2 * r + 1) * ww) & 0xFFFFFFFF) // 2
    return r, ww, fw


def box_pass(a: np.ndarray, fr, axis: int) -> np.ndarray:
    """one pass along ``axis`` (of length n) of a uint8 array: out[x] = (ww * sum(in[clamp(x + d)], d = -r .. r) + fw * (in[clamp(x - r
    - 1)] + in[clamp(x + r + 1)]) + (1 << 23)) >> 24, clamp to 0 .. n - 1, in 32-bit unsigned arithmetic.  (Pillow keeps a running
    sum; the sums are exact integers, so this direct form gives its bytes.)"""
    r, ww, fw = box_weights(fr)
    v = np.moveaxis(a, axis, 0).astype(np.uint64)
    n = v.shape[0]
    idx = np.clip(np.arange(-r - 1, n + r + 1), 0, n - 1)
    p = v[idx]                                          # (entry j is in[clamp(j - r - 1)])
    cs = np.concatenate([np.zeros((1,) + p.shape[1:], dtype=np.uint64), np.cumsum(p, axis=0, dtype=np.uint64)])
    inner = cs[2 * r + 2:2 * r + 2 + n] - cs[1:1 + n]                # sum of p[x + 1 .. x + 2 r + 1]
    far = p[:n] + p[2 * r + 2:2 * r + 2 + n]
    out = (((np.uint64(ww) * inner + np.uint64(fw) * far + np.uint64(1 << 23)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)) & np.uint64(0xFF)
    return np.ascontiguousarray(np.moveaxis(out.astype(np.uint8), 0, axis))


def blur(a: np.ndarray, fr, passes: int) -> np.ndarray:
    """``passes`` passes along the width, then as many along the height (axes 1 and 0 of (H, W[, 3])), all with box radius ``fr``"""
    for axis in (1, 0):
        for _ in range(passes):
            a = box_pass(a, fr, axis)
    return a


def rgb_to_hsv(a: np.ndarray) -> np.ndarray:
    """im.convert("HSV") of uint8 (..., 3) (Convert.c: rgb2hsv_row).  V = max; max == min: H = S = 0.  Else, in float32 unless said
    otherwise, cr = max - min, s = cr / max, rc = (max - r) / cr (gc, bc alike); h = bc - gc where r is the max, else 2.0 + rc - bc
    where g is, else 4.0 + gc - rc — evaluated in double and rounded to float32 —; h = fl32(fmod(h / 6.0 + 1.0, 1.0)) in double;
    H = (int)(h * 255.0), S = (int)(s * 255.0) in double, clipped to a byte."""
    f, d = np.float32, np.float64
    a = np.asarray(a, dtype=np.uint8)
    r, g, b = (a[..., c].astype(np.int32) for c in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    flat = maxc == minc
    cr = np.where(flat, 1, maxc - minc).astype(f)
    s = cr / np.where(flat, 1, maxc).astype(f)
    rc, gc, bc = ((maxc - v).astype(f) / cr for v in (r, g, b))
    rc, gc, bc = rc.astype(d), gc.astype(d), bc.astype(d)
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc)).astype(f)
    h = np.fmod(h.astype(d) / 6.0 + 1.0, 1.0).astype(f)
    H = np.clip((h.astype(d) * 255.0).astype(np.int32), 0, 255)
    S = np.clip((s.astype(d) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(flat, 0, H), np.where(flat, 0, S), maxc], axis=-1).astype(np.uint8)


def hsv_to_rgb(a: np.ndarray) -> np.ndarray:
    """Image.merge("HSV", ...).convert("RGB") of uint8 (..., 3) (Convert.c: hsv2rgb).  S == 0: R = G = B = V.  Else hf = fl32(H) * 6.0
    / 255.0 in double, i = floor(hf), f = fl32(hf - i), fs = fl32(S / 255.0); p = round(V * (1.0 - fs)), q = round(V * (1.0 - fs * f))
    — the product fs * f a float32 one —, t = round(V * (1.0 - fs * (1.0 - f))), otherwise in double, round half away from zero, clipped
    to a byte; i % 6 picks (V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)."""
    f32, d = np.float32, np.float64
    a = np.asarray(a, dtype=np.uint8)
    H, S, V = a[..., 0], a[..., 1], a[..., 2]
    hf = H.astype(f32).astype(d) * 6.0 / 255.0
    i = np.floor(hf)
    f = (hf - i).astype(f32)
    fs = (S.astype(d) / 255.0).astype(f32)
    v = V.astype(d)

    def rnd(x):         # (C's round on values that are not negative: x - trunc(x) is exact)
        t = np.trunc(x)
        return np.clip(np.where(x - t >= 0.5, t + 1, t), 0, 255).astype(np.uint8)
    p = rnd(v * (1.0 - fs.astype(d)))
    q = rnd(v * (1.0 - (fs * f).astype(d)))
    t = rnd(v * (1.0 - fs.astype(d) * (1.0 - f.astype(d))))
    k = i.astype(np.int32) % 6
    pick = lambda c0, c1, c2, c3, c4, c5: np.choose(k, [c0, c1, c2, c3, c4, c5])       # noqa: E731
    out = np.stack([pick(V, q, p, p, t, V), pick(t, V, V, q, p, p), pick(p, p, t, V, V, q)], axis=-1)
    return np.where((S == 0)[..., None], V[..., None], out).astype(np.uint8)


def hue_shift(f: float) -> int:
    """what adjust_hue adds to the H byte: int(f * 255) & 255 — the product a double's, truncated toward zero, then wrapped (what
    torchvision's np.array(f * 255).astype(np.uint8) gives on x86-64)"""
    return int(float(f) * 255) & 255


def adjust_hue(a: np.ndarray, f: float) -> np.ndarray:
    """torchvision's F.adjust_hue on a PIL image: "L" as it is; "RGB" to HSV, H + hue_shift(f) mod 256, and back — also for f = 0"""
    if not -0.5 <= f <= 0.5:
        raise ValueError(f"adjust_hue takes a factor of -0.5..0.5, not {f!r}")
    if a.ndim == 2:
        return a
    hsv = rgb_to_hsv(a)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift(f)) & 255
    return hsv_to_rgb(hsv)


def _per_band(a: np.ndarray, table_of) -> np.ndarray:
    if a.ndim == 2:
        return table_of(np.bincount(a.ravel(), minlength=256))[a]
    return np.stack([table_of(np.bincount(a[..., c].ravel(), minlength=256))[a[..., c]] for c in range(a.shape[2])], axis=-1)


def apply_op(a: np.ndarray, op) -> np.ndarray:
    """one op on a uint8 (H, W, 3) or (H, W) image"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    name = op[0]
    if name not in OPS + TORCHVISION_OPS or len(op) != (2 if name in VALUED + TORCHVISION_OPS else 1):
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
    if name in ("gaussian_blur", "box_blur"):
        if not 0 <= op[1] <= MAX_RADIUS:
            raise ValueError(f"{name} takes a radius of 0..{MAX_RADIUS}, not {op[1]!r}")
        return blur(a, gaussian_box_radius(op[1]), 3) if name == "gaussian_blur" else blur(a, np.float32(op[1]), 1)
    if name == "adjust_hue":
        return adjust_hue(a, op[1])
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
