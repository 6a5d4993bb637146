"""What `decode(..., size=..., perspective=...)` puts in front of the window and the resize, restated in NumPy: Pillow's

    img.transform(img.size, Image.PERSPECTIVE, c, resample, fillcolor=fill)

for 8-bit images of one or three components (Pillow 12.2's Geometry.c: perspective_transform, ImagingGenericTransform;
tests/test_perspective_host.py holds `transform` to Pillow itself, bit for bit, and the library's host twin mj_host_perspective and
its kernel to `transform`).  The coefficients c = (c0 .. c7) map OUTPUT pixels to source coordinates.  Output pixel (X, Y) — in
ABSOLUTE coordinates of the transformed image: a WINDOW of the transform is the transform evaluated at the window's coordinates
(`transform(.., window=)`) — of a source of w x h pixels, every double operation rounded on its own, in this order:

    xc = X + 0.5;  yc = Y + 0.5
    d   = c6 * xc + c7 * yc + 1
    xin = (c0 * xc + c1 * yc + c2) / d
    yin = (c3 * xc + c4 * yc + c5) / d

The divisions are IEEE double divisions (never a reciprocal and a multiply).  Pillow evaluates d twice; it is the same value.

inside    xin >= 0 and xin < w and yin >= 0 and yin < h.  Written this way round, NaN and +-inf are outside.  An outside pixel is fill.
nearest   the source pixel is ((int)xin, (int)yin), converted only after the inside test: no 0.5 shift, no fixed point, no tables
          (Pillow's COORD and its range test give the same bytes on x86-64).
bilinear, bicubic   inside as above, then both minus 0.5, ix = floor(xin), dx = xin - ix (rows likewise), and the 2 x 2 / 4 x 4
          taps of tools/affine_model.py (`taps`): clipped columns, a row outside the image repeats the row before it, bilinear
          truncates, bicubic clips to 0..255 and truncates.

The pole — the line d = 0 — may cross the frame, and is ordinary: next to it the coordinates are huge or infinite, hence outside,
hence fill; beyond it the source is sampled where the formula says.  The one spot where Pillow's C is undefined is 0 / 0: NaN
passes its bilinear range test, and it converts NaN to an int.  The library defines that pixel as FILL, and so does this model
(NaN fails the inside test); the tests against Pillow stay away from it.

`coeffs` solves for the coefficients from four corners (pyjpegdecoder_amd.perspective_coeffs is held to it); `get_params` draws
corners by the rule of torchvision's RandomPerspective.get_params."""
import math

import numpy as np

from tools import affine_model

FILTERS = affine_model.FILTERS
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def source_coords(c, X, Y):
    """(xin, yin) of the output pixels (X, Y) (integer arrays, absolute coordinates): doubles, inf and NaN where the rule gives them"""
    c = [np.float64(v) for v in c]
    xc, yc = X + 0.5, Y + 0.5
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = c[6] * xc + c[7] * yc + 1
        xin = (c[0] * xc + c[1] * yc + c[2]) / d
        yin = (c[3] * xc + c[4] * yc + c[5]) / d
    return xin, yin


def transform(img: np.ndarray, c, resample: str = "nearest", fill=0, window=None) -> np.ndarray:
    """img: uint8 (h, w) or (h, w, C), row-major.  The window (x, y, width, height) (None: all) of its transform, same components."""
    if resample not in FILTERS:
        raise ValueError(f"resample must be one of {FILTERS}, not {resample!r}")
    src = img.reshape(img.shape[0], img.shape[1], -1)
    h, w, C = src.shape
    x0, y0, ww, wh = window if window is not None else (0, 0, w, h)
    out = np.empty((wh, ww, C), dtype=np.uint8)
    out[:] = np.broadcast_to(np.asarray(fill, dtype=np.uint8), (C,))
    X, Y = np.meshgrid(np.arange(x0, x0 + ww, dtype=np.int64), np.arange(y0, y0 + wh, dtype=np.int64))
    xin, yin = source_coords(c, X, Y)
    with np.errstate(invalid="ignore"):
        ok = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    if resample == "nearest":
        out[ok] = src[yin[ok].astype(np.int64), xin[ok].astype(np.int64)]
    else:
        out[ok] = affine_model.taps(src, xin[ok], yin[ok], resample)
    return out.reshape((wh, ww) + img.shape[2:])


def fill_share(img: np.ndarray, c, window=None) -> float:
    """the share of the window's pixels that are fill (the rule's, whatever the filter)"""
    h, w = img.shape[:2]
    x0, y0, ww, wh = window if window is not None else (0, 0, w, h)
    X, Y = np.meshgrid(np.arange(x0, x0 + ww, dtype=np.int64), np.arange(y0, y0 + wh, dtype=np.int64))
    xin, yin = source_coords(c, X, Y)
    with np.errstate(invalid="ignore"):
        ok = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    return 1.0 - float(ok.mean())


def coeffs(startpoints, endpoints):
    """the eight coefficients that take the output's `endpoints` to the source's `startpoints` (four (x, y) pairs each): the 8 x 8
    system torchvision's _get_perspective_coeffs sets up, in float64, solved with NumPy"""
    a = np.zeros((8, 8), dtype=np.float64)
    b = np.zeros(8, dtype=np.float64)
    for i, ((sx, sy), (ex, ey)) in enumerate(zip(startpoints, endpoints)):
        a[2 * i] = [ex, ey, 1, 0, 0, 0, -sx * ex, -sx * ey]
        a[2 * i + 1] = [0, 0, 0, ex, ey, 1, -sy * ex, -sy * ey]
        b[2 * i], b[2 * i + 1] = sx, sy
    return tuple(float(v) for v in np.linalg.solve(a, b))


def corners(w: int, h: int):
    """the start points of torchvision's rule: the image's corners, top-left, top-right, bottom-right, bottom-left"""
    return [(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)]


def get_params(w: int, h: int, distortion_scale: float, rng: np.random.Generator):
    """(startpoints, endpoints) by the rule of torchvision's RandomPerspective.get_params (its integer ranges; this generator's draws)"""
    half_h, half_w = h // 2, w // 2
    dw, dh = int(distortion_scale * half_w), int(distortion_scale * half_h)
    tl = (int(rng.integers(0, dw + 1)), int(rng.integers(0, dh + 1)))
    tr = (int(rng.integers(w - dw - 1, w)), int(rng.integers(0, dh + 1)))
    br = (int(rng.integers(w - dw - 1, w)), int(rng.integers(h - dh - 1, h)))
    bl = (int(rng.integers(0, dw + 1)), int(rng.integers(h - dh - 1, h)))
    return corners(w, h), [tl, tr, br, bl]


def fault(c, w: int, h: int):
    """what the library refuses of coefficients c for a w x h image: None, or the reason (csrc/affine.hip: perspective_fault)"""
    if not all(math.isfinite(v) for v in c):
        return "a coefficient is not finite"
    if w >= 32768 or h >= 32768:
        return "an image with a side of 32768 or more"
    return None


def expected(pixels_rm: np.ndarray, c, window, size, resample: str = "nearest", affine_fill=0, filter: str = "bilinear", orientation: int = 1,
             mode=None, mirror: bool = False, resized=None, xy=(0, 0), fill=0) -> np.ndarray:
    """One output's bytes, row-major (height, width[, C]), as tools/affine_model.py's `expected` gives them for a matrix: mode ->
    orientation -> transform with coefficients c (None: none) -> window -> resize / place -> mirror."""
    from tools import mode_model, orient_model, views_model
    img = orient_model.orient(mode_model.convert(pixels_rm, mode), orientation)
    if c is not None:
        img = transform(img, c, resample, affine_fill)
    return views_model.expected(img, window, size, filter, mirror=mirror, resized=resized, xy=xy, fill=fill)
