"""What `decode(..., size=..., affine=...)` puts in front of the window and the resize, restated in NumPy: Pillow's

    img.transform(img.size, Image.AFFINE, a, resample, fillcolor=fill)

for 8-bit images of one or three components (tests/test_affine_host.py holds `transform` to Pillow itself, bit for bit, and the
library's host twin mj_host_affine and its kernel to `transform`).  The matrix a = (a0 .. a5) maps OUTPUT pixels to source
coordinates.  Output pixel (x, y) of a source of w x h pixels:

bilinear, bicubic   xin = a0 (x + 0.5) + a1 (y + 0.5) + a2, yin = a3 (x + 0.5) + a4 (y + 0.5) + a5 in doubles, every operation
    rounded on its own, in that order.  fill where xin < 0, xin >= w, yin < 0 or yin >= h.  Else both minus 0.5, ix = floor(xin),
    dx = xin - ix (rows likewise), and
      bilinear  columns clip(ix), clip(ix + 1); row clip(iy) gives v1 = p0 + (p1 - p0) dx, row iy + 1 gives v2 likewise if it
                lies inside the image, else v2 = v1; the byte is v1 + (v2 - v1) dy, truncated
      bicubic   columns clip(ix - 1 .. ix + 2); cubic(v1, v2, v3, v4, d) = v2 + d ((-v1 + v3) + d ((2 (v1 - v2) + v3 - v4)
                + d (-v1 + v2 - v3 + v4))); row clip(iy - 1) is always read, rows iy, iy + 1, iy + 2 are read where they lie
                inside the image and else repeat the value of the row before; 0 for a value <= 0, 255 for one >= 255, else truncated
nearest, a1 == a3 == 0   Pillow's ImagingScaleAffine: the source column of column x by ACCUMULATION — xo = a2 + a0 * 0.5, then
    per column (xo < 0 ? -1 : (int)xo) and xo += a0 —, rows likewise with a5 + a4 * 0.5 and a4 (`scale_table`)
nearest otherwise   16.16 fixed point: FIX(v) = floor(v * 65536 + 0.5) (`fix`), A2 = FIX(a2 + a0 * 0.5 + a1 * 0.5),
    A5 = FIX(a5 + a3 * 0.5 + a4 * 0.5), xi = (int32)(A2 + x A0 + y A1) >> 16 in wrapping 32-bit arithmetic; yi likewise
A pixel whose source lies outside the image is fill.

A WINDOW of the transform is the transform evaluated at the window's absolute coordinates (`transform(.., window=)`): folding
the window's origin into a2 / a5 gives other bits.

`rotation_matrix` is the matrix Image.rotate builds (expand=False); `fault` is what the library refuses of a matrix."""
import math

import numpy as np

FILTERS = ("nearest", "bilinear", "bicubic")


def fix(v: float) -> int:
    """Pillow's FIX: v in 16.16 fixed point, rounded to nearest (ties up)"""
    return int(math.floor(v * 65536.0 + 0.5))


def scale_table(scale: float, offset: float, size: int, n: int) -> np.ndarray:
    """the source index of each of n output indices of the nearest scale path, -1 outside [0, size): accumulated, not multiplied"""
    out = np.empty(n, dtype=np.int64)
    o = offset + scale * 0.5
    for j in range(n):
        idx = -1 if o < 0.0 else int(o)
        out[j] = idx if 0 <= idx < size else -1
        o += scale
    return out


def _cubic(v1, v2, v3, v4, d):
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return v2 + d * (p2 + d * (p3 + d * p4))


def transform(img: np.ndarray, a, resample: str = "nearest", fill=0, window=None) -> np.ndarray:
    """img: uint8 (h, w) or (h, w, C), row-major.  The window (x, y, width, height) (None: all) of its transform, same components."""
    src = img.reshape(img.shape[0], img.shape[1], -1)
    h, w, C = src.shape
    x0, y0, ww, wh = window if window is not None else (0, 0, w, h)
    a = [float(v) for v in a]
    fillv = np.broadcast_to(np.asarray(fill, dtype=np.uint8), (C,))
    out = np.empty((wh, ww, C), dtype=np.uint8)
    out[:] = fillv
    X, Y = np.meshgrid(np.arange(x0, x0 + ww, dtype=np.int64), np.arange(y0, y0 + wh, dtype=np.int64))
    if resample == "nearest":
        if a[1] == 0 and a[3] == 0:
            sx = scale_table(a[0], a[2], w, x0 + ww)[x0:][None, :].repeat(wh, 0)
            sy = scale_table(a[4], a[5], h, y0 + wh)[y0:][:, None].repeat(ww, 1)
        else:
            A = [fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]
            wrap = lambda v: ((v + (1 << 31)) % (1 << 32)) - (1 << 31)          # noqa: E731 (int32 wrap-around of exact integers)
            sx = wrap(A[2] + X * A[0] + Y * A[1]) >> 16
            sy = wrap(A[5] + X * A[3] + Y * A[4]) >> 16
        ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        out[ok] = src[sy[ok], sx[ok]]
        return out.reshape((wh, ww) + img.shape[2:])
    xc, yc = X + 0.5, Y + 0.5
    xin = a[0] * xc + a[1] * yc + a[2]
    yin = a[3] * xc + a[4] * yc + a[5]
    ok = ~((xin < 0.0) | (xin >= w) | (yin < 0.0) | (yin >= h))
    out[ok] = taps(src, xin[ok], yin[ok], resample)
    return out.reshape((wh, ww) + img.shape[2:])


def taps(src: np.ndarray, xin: np.ndarray, yin: np.ndarray, resample: str) -> np.ndarray:
    """The bilinear / bicubic bytes (n, C) of source coordinates (xin, yin) — n doubles each, all INSIDE the image src (h, w, C) —:
    the 2 x 2 / 4 x 4 taps around (xin - 0.5, yin - 0.5) as the module's head describes them.  tools/perspective_model.py shares it."""
    h, w = src.shape[:2]
    xin, yin = xin - 0.5, yin - 0.5
    ix, iy = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - ix)[:, None], (yin - iy)[:, None]
    s = src.astype(np.float64)
    cx = lambda v: np.clip(v, 0, w - 1)         # noqa: E731
    cy = lambda v: np.clip(v, 0, h - 1)         # noqa: E731
    if resample == "bilinear":
        c0, c1 = cx(ix), cx(ix + 1)

        def row(r):
            p0, p1 = s[r, c0], s[r, c1]
            return p0 + (p1 - p0) * dx
        v1 = row(cy(iy))
        inside = ((iy + 1 >= 0) & (iy + 1 < h))[:, None]
        v2 = np.where(inside, row(cy(iy + 1)), v1)
        return (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)
    if resample == "bicubic":
        c = [cx(ix - 1), cx(ix), cx(ix + 1), cx(ix + 2)]

        def row(r):
            return _cubic(s[r, c[0]], s[r, c[1]], s[r, c[2]], s[r, c[3]], dx)
        v = [row(cy(iy - 1))]
        for k in (0, 1, 2):
            inside = ((iy + k >= 0) & (iy + k < h))[:, None]
            v.append(np.where(inside, row(cy(iy + k)), v[-1]))
        t = _cubic(v[0], v[1], v[2], v[3], dy)
        return np.where(t <= 0.0, 0, np.where(t >= 255.0, 255, np.trunc(np.clip(t, 0.0, 255.0)))).astype(np.uint8)
    raise ValueError(f"resample must be one of {FILTERS}, not {resample!r}")


def rotation_matrix(angle: float, size, center=None, translate=None):
    """Image.rotate's matrix for expand=False (its round(.., 15) included); pyjpegdecoder_amd.rotation_matrix is held to this"""
    w, h = size
    angle = angle % 360.0
    tx, ty = translate if translate is not None else (0, 0)
    cx, cy = center if center is not None else (w / 2.0, h / 2.0)
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    x, y = -cx - tx, -cy - ty
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def fault(a, resample: str, w: int, h: int):
    """what the library refuses of matrix a for a w x h image: None, or the reason (csrc/affine.hip: affine_fault)"""
    if not all(math.isfinite(v) for v in a):
        return "a matrix entry is not finite"
    if w >= 32768 or h >= 32768:
        return "an image with a side of 32768 or more"
    corners = [(x, y) for y in (0.5, h - 0.5) for x in (0.5, w - 0.5)]
    if resample == "nearest":
        corners += [(float(x), float(y)) for y in (0, h) for x in (0, w)]
    for x, y in corners:
        if not (abs(a[0] * x + a[1] * y + a[2]) < 32768.0 and abs(a[3] * x + a[4] * y + a[5]) < 32768.0):
            return "a corner of the output has a source coordinate of magnitude 32768 or more"
    if resample == "nearest" and not (a[1] == 0 and a[3] == 0):
        fixed = (a[0], a[1], a[2] + a[0] * 0.5 + a[1] * 0.5, a[3], a[4], a[5] + a[3] * 0.5 + a[4] * 0.5)
        if not all(abs(v) < 32767.0 for v in fixed):
            return "a matrix entry of magnitude 32767 or more does not fit NEAREST's 16.16 fixed point"
    return None


def expected(pixels_rm: np.ndarray, a, window, size, resample: str = "nearest", affine_fill=0, filter: str = "bilinear", orientation: int = 1,
             mode=None, mirror: bool = False, resized=None, xy=(0, 0), fill=0) -> np.ndarray:
    """One output's bytes, row-major (height, width[, C]): `pixels_rm` are the file's pixels as a plain decode gives them (stored
    order, the file's own components).  mode -> orientation -> transform with matrix a (None: none) -> window (None: the whole
    transformed image) -> resize to `size` (or to `resized` at `xy` on the canvas `size`, `fill` elsewhere) -> mirror: the order
    of include/mijpeg.h, with tools/mode_model.py, orient_model.py and views_model.py (place_model.py, resize_model.py) for the rest."""
    from tools import mode_model, orient_model, views_model
    img = orient_model.orient(mode_model.convert(pixels_rm, mode), orientation)
    if a is not None:
        img = transform(img, a, resample, affine_fill)
    return views_model.expected(img, window, size, filter, mirror=mirror, resized=resized, xy=xy, fill=fill)
