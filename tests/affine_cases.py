"""What tests/test_affine_paths_host.py (no GPU) and tests/test_affine_paths.py (MI355X) share: the calls that take k_affine
(csrc/affine.hip) down the paths tests/test_affine.py does not reach — NEAREST by index tables, the bicubic clamp, every
orientation through StoredFetch, windows of many tiles and every row tail — and `census`, which counts, for one matrix on one
image, how often each branch of tools/affine_model.transform is taken.  The host file holds every case to the census (a case
that claims the clamp clamps) and to the wrong variants of the model it must tell apart; the GPU file runs the same cases.

A case is one OUTPUT of a call: a file, the mode and orientation it is shown in, a matrix (None: untransformed), the filter of
the transform and a window of the transformed image.  `source` is the image the transform reads (convert, then orient) and
`buffer` the bytes the affine launch writes for the case — tools/affine_model.transform of the source at the window.  Neither a
test file nor a conftest: nothing here is collected."""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from conftest import GOLDEN

FILL3, FILL1 = (7, 99, 200), 55
NOISE, Q98, ODD, GREY, BIG = "96x64_420_q100_noise", "64x64_444_q98_pil", "70x50_420_pil_opt", "50x70_grey_dri4", "c2_512x512_420"
CHECK3, CHECK1 = "checker_48x40_444", "checker_48x40_grey"           # tests/golden/affine (tools/make_affine_fixtures.py)
DIMS = {NOISE: (96, 64), Q98: (64, 64), ODD: (70, 50), GREY: (50, 70), BIG: (512, 512), CHECK3: (48, 40), CHECK1: (48, 40)}
COMPS = {NOISE: 3, Q98: 3, ODD: 3, GREY: 1, BIG: 3, CHECK3: 3, CHECK1: 1}
FILTERS = ("nearest", "bilinear", "bicubic")
_pixels = {}


def path(name: str):
    return GOLDEN / ("affine" if name.startswith("checker_") else "files") / f"{name}.jpg"


def raw(name: str) -> bytes:
    return path(name).read_bytes()


def pixels(name: str) -> np.ndarray:
    """the file's pixels without the library, row-major (h, w[, 3]): the golden .npz, the oracle's decode for the fixtures"""
    if name not in _pixels:
        if name.startswith("checker_"):
            from oracle import oracle
            full = oracle.decode(raw(name))["rgb"]
        else:
            full = np.load(GOLDEN / "files" / f"{name}.npz")["rgb"]
        a = np.ascontiguousarray(full.swapaxes(0, 1))
        a.setflags(write=False)
        _pixels[name] = a
    return _pixels[name]


def rotate_shear(size, degrees=30.0, shear=0.2, shift=(0.0, 0.0)):
    """output -> input: a rotation by `degrees` about the centre with a shear along x, then a shift (tests/test_affine.py's)"""
    w, h = size
    t = math.radians(degrees)
    a0, a1, a3, a4 = math.cos(t), math.sin(t) + shear, -math.sin(t), math.cos(t)
    cx, cy = w / 2.0, h / 2.0
    return (a0, a1, cx - a0 * cx - a1 * cy + shift[0], a3, a4, cy - a3 * cx - a4 * cy + shift[1])


def tenths(size, frac=0.2):
    """The rotation (0.8, 0.6; -0.6, 0.8) about the centre with offsets that are whole numbers plus `frac`.  None of 0.8, 0.6 and
    0.2 is a binary fraction, and the exact source coordinate of every pixel is a multiple of 0.1: for a fifth of the pixels it
    is a whole number (bilinear, bicubic: frac 0.2; NEAREST's fixed point: frac 0.3), so the LAST bit of the evaluation decides
    floor() there — a fused multiply-add, an origin folded into the offset or a FIX that truncates shows in whole pixels."""
    w, h = size
    cx, cy = w / 2.0, h / 2.0
    return (0.8, 0.6, round(cx - 0.8 * cx - 0.6 * cy) + frac, -0.6, 0.8, round(cy + 0.6 * cx - 0.8 * cy) + frac)


def oriented(size, o: int):
    return (size[1], size[0]) if o >= 5 else tuple(size)


@dataclass(frozen=True)
class Case:
    name: str
    file: str
    a: Optional[Tuple[float, ...]]
    resample: str
    window: Tuple[int, int, int, int]
    orientation: int = 1
    mode: Optional[str] = None

    @property
    def ncomp(self) -> int:
        return {None: COMPS[self.file], "RGB": 3, "L": 1}[self.mode]

    @property
    def fill(self):
        return FILL3 if self.ncomp == 3 else FILL1

    @property
    def size(self):
        return self.window[2:]


def source(c: Case, px: Optional[np.ndarray] = None, orientation: Optional[int] = None) -> np.ndarray:
    """the image the transform of case c reads: the file's pixels (`px`; None: `pixels`) converted, then oriented"""
    from tools import mode_model, orient_model
    return orient_model.orient(mode_model.convert(pixels(c.file) if px is None else px, c.mode), c.orientation if orientation is None else orientation)


def buffer(c: Case, px: Optional[np.ndarray] = None) -> np.ndarray:
    """what the affine launch writes for case c, row-major — for a call whose size is the window's, the output itself"""
    from tools import affine_model
    src = source(c, px)
    x, y, w, h = c.window
    if c.a is None:
        return np.ascontiguousarray(src[y:y + h, x:x + w])
    return affine_model.transform(src, c.a, c.resample, c.fill, c.window)


# ---- the census -------------------------------------------------------------------------------------------------------------------
def _runs(t: np.ndarray):
    ins = np.flatnonzero(t >= 0)
    if not ins.size:
        return len(t), 0, 0
    return int(ins[0]), int(len(t) - 1 - ins[-1]), int((t >= 0).sum())


def census(pixels_rm: np.ndarray, a, resample: str, window=None) -> dict:
    """How often each branch of tools/affine_model.transform(pixels_rm, a, resample, window=window) is taken: counts.

    all filters         pixels, inside, fill
    nearest, tables     x_lead, x_trail, x_inside, y_lead, y_trail, y_inside — the -1 entries in front of and behind the inside
                        entries of each axis' table over the window, and the inside entries
    nearest, fixed      negative — pixels whose 32-bit sum of x or of y is negative (its >> 16 is an arithmetic shift)
    bilinear, bicubic   ix_m1 (ix == -1), ix_hi (ix + 1 >= w), iy_m1 (iy == -1), iy_hi (iy + 1 >= h), of the inside pixels
    bicubic             iy_hi2 (iy + 2 >= h), values (inside component values), below (t < 0), above (t > 255)"""
    from tools.affine_model import _cubic, fix, scale_table
    src = pixels_rm.reshape(pixels_rm.shape[0], pixels_rm.shape[1], -1)
    h, w, C = src.shape
    x0, y0, ww, wh = window if window is not None else (0, 0, w, h)
    a = [float(v) for v in a]
    out = {"pixels": ww * wh}
    X, Y = np.meshgrid(np.arange(x0, x0 + ww, dtype=np.int64), np.arange(y0, y0 + wh, dtype=np.int64))
    if resample == "nearest" and a[1] == 0 and a[3] == 0:
        tx, ty = scale_table(a[0], a[2], w, x0 + ww)[x0:], scale_table(a[4], a[5], h, y0 + wh)[y0:]
        out["x_lead"], out["x_trail"], out["x_inside"] = _runs(tx)
        out["y_lead"], out["y_trail"], out["y_inside"] = _runs(ty)
        out["inside"] = out["x_inside"] * out["y_inside"]
    elif resample == "nearest":
        A = [fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]
        wrap = lambda v: ((v + (1 << 31)) % (1 << 32)) - (1 << 31)          # noqa: E731
        ux, uy = wrap(A[2] + X * A[0] + Y * A[1]), wrap(A[5] + X * A[3] + Y * A[4])
        sx, sy = ux >> 16, uy >> 16
        out["inside"] = int(((sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)).sum())
        out["negative"] = int(((ux < 0) | (uy < 0)).sum())
    else:
        xc, yc = X + 0.5, Y + 0.5
        xin = a[0] * xc + a[1] * yc + a[2]
        yin = a[3] * xc + a[4] * yc + a[5]
        ok = ~((xin < 0.0) | (xin >= w) | (yin < 0.0) | (yin >= h))
        xin, yin = xin[ok] - 0.5, yin[ok] - 0.5
        ix, iy = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
        out["inside"] = int(ok.sum())
        out.update(ix_m1=int((ix == -1).sum()), ix_hi=int((ix + 1 >= w).sum()), iy_m1=int((iy == -1).sum()), iy_hi=int((iy + 1 >= h).sum()))
        if resample == "bicubic":
            out["iy_hi2"] = int((iy + 2 >= h).sum())
            dx, dy = (xin - ix)[:, None], (yin - iy)[:, None]
            s = src.astype(np.float64)
            cols = [np.clip(ix + k, 0, w - 1) for k in (-1, 0, 1, 2)]

            def row(r):
                return _cubic(s[r, cols[0]], s[r, cols[1]], s[r, cols[2]], s[r, cols[3]], dx)
            v = [row(np.clip(iy - 1, 0, h - 1))]
            for k in (0, 1, 2):
                v.append(np.where(((iy + k >= 0) & (iy + k < h))[:, None], row(np.clip(iy + k, 0, h - 1)), v[-1]))
            t = _cubic(v[0], v[1], v[2], v[3], dy)
            out.update(values=int(t.size), below=int((t < 0.0).sum()), above=int((t > 255.0).sum()))
    out["fill"] = out["pixels"] - out["inside"]
    return out


_census = {}


def case_census(c: Case) -> dict:
    key = (c.file, c.a, c.resample, c.window, c.orientation, c.mode)
    if key not in _census:
        _census[key] = census(source(c), c.a, c.resample, c.window)
    return _census[key]


# ---- tables: one plan of nine views of one file, NEAREST ----------------------------------------------------------------------------
TW, TH = 40, 24
S1, S2 = (1.7, 0, -20.3, 0, 0.6, -7.9), (0.5, 0, 10.25, 0, 2.0, -30.0)
S3 = (3.1, 0, -40.0, 0, 3.3, -20.0)           # a strong shrink: ONE 40 x 24 window holds -1 runs at both ends of both axes
FLIP, SHIFT = (-1, 0, 96, 0, 1, 0), (1, 0, 0.37, 0, 1, -2.61)
SCALES = {"s1": S1, "s2": S2, "s3": S3}


def table_cases():
    """(matrix, origin) of every view — all windows TW x TH: the scale matrices on windows that hang over the leading runs of -1
    (near the origin), over the trailing ones (s1 and s2 again, far from it) and over both (s3); the flip; the sub-pixel shift,
    whose rows begin with -1; a rotation (fixed point, kind 2) and the `tenths` one; an untransformed view."""
    rows = [("s1_lead", S1, (2, 1)), ("s2_lead", S2, (3, 2)), ("flip", FLIP, (56, 40)), ("shift", SHIFT, (17, 0)),
            ("rotation", rotate_shear(DIMS[NOISE], 30.0, 0.2, (1.5, -2.0)), (56, 3)), ("none", None, (11, 7)), ("s1_trail", S1, (52, 40)),
            ("s2_trail", S2, (50, 36)), ("s3_both", S3, (5, 2)), ("tenths", tenths(DIMS[NOISE], 0.3), (2, 36))]
    return [Case(n, NOISE, m, "nearest", o + (TW, TH)) for n, m, o in rows]


# ---- the clamp: bicubic ------------------------------------------------------------------------------------------------------------
CLAMP_A = (0.37, 0.11, 20, -0.09, 0.41, 15)


def clamp_cases():
    """bicubic on the RGB noise files at their own size (two matrices) and on the checker fixtures as colour, as mode="L", as grey
    and as grey to RGB — each once with the window the whole image and once with a corner window"""
    out = []
    for f in (Q98, NOISE):
        w, h = DIMS[f]
        for tag, m in (("zoom", CLAMP_A), ("turn", rotate_shear(DIMS[f], -25.0, 0.15, (1.5, -2.0)))):
            out.append(Case(f"{f}_{tag}", f, m, "bicubic", (0, 0, w, h)))
    out.append(Case(f"{Q98}_zoom_corner", Q98, CLAMP_A, "bicubic", (64 - 37, 64 - 29, 37, 29)))
    out.append(Case(f"{NOISE}_turn_corner", NOISE, rotate_shear(DIMS[NOISE], -25.0, 0.15, (1.5, -2.0)), "bicubic", (0, 0, 37, 29)))
    w, h = DIMS[CHECK3]
    zoom, turn = (0.31, 0.07, 9.2, -0.05, 0.29, 11.4), rotate_shear((w, h), 18.0, 0.1, (0.5, -1.0))
    for tag, f, mode in (("colour", CHECK3, None), ("colour_as_L", CHECK3, "L"), ("grey", CHECK1, None), ("grey_as_RGB", CHECK1, "RGB")):
        out.append(Case(f"checker_{tag}_zoom", f, zoom, "bicubic", (0, 0, w, h), mode=mode))
        out.append(Case(f"checker_{tag}_turn_corner", f, turn, "bicubic", (w - 29, 0, 29, 23), mode=mode))
    return out


# ---- orientations: eight copies of a file, orientation 1..8, a window off the origin, a matrix per output --------------------------
ANGLES = (25.0, -33.0, 40.0, None, 28.0, -36.0, 44.0, 33.0)          # (orientation 4 has the `tenths` matrix)


OW, OH = 31, 33                      # one size for the windows of all eight: it is the call's size


def orientation_cases(file: str, resample: str, mode=None):
    out = []
    for o in range(1, 9):
        ow, oh = oriented(DIMS[file], o)
        if o == 4:
            m = tenths((ow, oh), 0.3 if resample == "nearest" else 0.2)
        else:
            m = rotate_shear((ow, oh), ANGLES[o - 1], 0.05 * (o - 4), (0.5 * (o - 4), 0.4 * (4 - o)))
        d = 1 + o % 3
        x, y = (d if o & 1 else ow - OW - d), (d + 1 if o & 2 else oh - OH - d - 1)       # off the origin, towards a corner in turn
        if o == 4:                  # (where the `tenths` matrix tells a folded origin apart under every filter)
            x, y = 3, oh - OH - 4
        out.append(Case(f"{file}_{mode or 'own'}_{resample}_o{o}", file, m, resample, (x, y, OW, OH), o, mode))
    return out


def edge_cases(file: str, resample: str):
    """Two calls, each at its windows' own size: orientations 1..4 and orientations 5..8 of the file, every output the WHOLE
    oriented image under a rotation with shear, so that the frame of the source crosses the output on all four sides — pixels with
    ix == -1, ix + 1 >= w, iy == -1 and iy + 1 >= h in every output, each of them a byte of the result."""
    groups = []
    for turned in (range(1, 5), range(5, 9)):
        cases = []
        for o in turned:
            ow, oh = oriented(DIMS[file], o)
            m = rotate_shear((ow, oh), EDGE_ANGLES[o - 1], 0.05 * (o - 4), (0.5 * (o - 4), 0.4 * (4 - o)))
            cases.append(Case(f"edge_{file}_{resample}_o{o}", file, m, resample, (0, 0, ow, oh), o))
        groups.append(cases)
    return groups


EDGE_ANGLES = (25.0, -33.0, 40.0, -18.0, 28.0, -36.0, 44.0, 33.0)


def ideal_checker(name: str) -> np.ndarray:
    """the board the checker fixtures were encoded from (tools/make_affine_fixtures.py), row-major, in the fixture's components"""
    y, x = np.mgrid[0:40, 0:48]
    board = (((x // 8 + y // 8) & 1) * 255).astype(np.uint8)
    return np.stack([board] * 3, axis=-1) if name == CHECK3 else board


def other_mode(file: str) -> str:
    return "L" if COMPS[file] == 3 else "RGB"


# ---- tiles ----------------------------------------------------------------------------------------------------------------------------
TILE_SIZE = (48, 32)


def tile_cases(resample: str, layout: str):
    """One plan: the whole 512 x 512 image (8 x 32 tiles), a 1 x 1 window, a window of exactly one tile, one a pixel more than a
    tile along each axis, and a 300 x 20 window — the tile is 64 along the layout's contiguous axis and 16 along the other."""
    fast_is_x = layout in ("rowmajor", "planar_rowmajor")
    tile = (64, 16) if fast_is_x else (16, 64)
    wins = [(0, 0, 512, 512), (377, 201, 1, 1), (129, 300) + tile, (40, 77, tile[0] + 1, tile[1] + 1), (150, 411, 300, 20)]
    mats = [rotate_shear((512, 512), 17.0, 0.1, (3.0, -5.0)), rotate_shear((512, 512), -40.0, 0.0), tenths((512, 512)),
            rotate_shear((512, 512), 75.0, -0.2, (20.0, 9.0)), rotate_shear((512, 512), 5.0, 0.3, (-7.5, 2.25))]
    return [Case(f"tile_{resample}_{k}", BIG, m, resample, w) for k, (w, m) in enumerate(zip(wins, mats))]


def row_tail_cases(r: int, layout: str, mode=None):
    """three windows of (64 + r) x 19 — 19 x (64 + r) where columns are contiguous — at origins of every parity"""
    fast_is_x = layout in ("rowmajor", "planar_rowmajor")
    w, h = (64 + r, 19) if fast_is_x else (19, 64 + r)
    origins = [(1, 2), (222, 333), (512 - w, 512 - h)]
    mats = [rotate_shear((512, 512), 8.0 + r, 0.05, (200.0, 190.0)), tenths((512, 512)), rotate_shear((512, 512), -12.0 * r, 0.1, (-180.0, -170.0))]
    return [Case(f"tail{r}_{mode or 'own'}_{k}", BIG, m, "bilinear", o + (w, h), mode=mode) for k, (o, m) in enumerate(zip(origins, mats))]
