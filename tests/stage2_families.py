"""Input families for the fast stage 2's rare pixel paths, and a census that says which of them an image reaches.

The strip worker (csrc/reconstruct_fast_strips.h, phase B) is exact in fp32 only because a chain of rare-case decisions
sends the right lanes elsewhere: the B tie at |Cb - 128| = 125, the R tie and the fp32 range at |c| >= 250, the green
quotient next to a remainder of +-25000, and the demotion of a whole strip from the staged stores to the per-lane ones.
Each family below builds the coefficient blocks of small images that land on one of these decisions, in every sampling
layout; `census` counts, from the ORACLE's output alone (never the library's), the pixels and MCUs that meet each
condition — so "the rare path was reached" is an assertion of tests/test_stage2_families_host.py, not a hope, and
tests/test_stage2_rare_paths.py drives the same files through the kernel's routes.

Plain helper module (no fixtures, no hooks).  Files come from tools/craft_jpeg.craft_baseline(blocks=, qts=), with a restart
interval of one MCU row: the DC predictors start at 0 in every row, so a row's chroma may sit at +1000 and the next at
-1000 without a DC difference the Annex-K tables cannot code."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

LAYOUTS = {
    "grey": ((1, 1),),
    "444": ((1, 1), (1, 1), (1, 1)),
    "422": ((2, 1), (1, 1), (1, 1)),
    "440": ((1, 2), (1, 1), (1, 1)),
    "420": ((2, 2), (1, 1), (1, 1)),
    "411": ((4, 1), (1, 1), (1, 1)),
}
COLOUR = [k for k in LAYOUTS if k != "grey"]
SUBSAMPLED = [k for k in COLOUR if k != "444"]
FAMILIES = ("tie", "green", "range", "clamp", "wild", "planted")

# zig-zag index of coefficient (row, column) of the 3x3 low-frequency corner, DC left out
CORNER = (1, 2, 3, 4, 5, 7, 8, 12)
INT16_SUM = 4 * (32767 - 128)          # sum |dequantised coefficient| / 4 + 128 <= 32767: every IDCT sample inside int16


def families_of(layout: str):
    """Greyscale has no chroma: only the families about luma, the output clamp and the stores apply."""
    return ("clamp", "wild", "planted") if layout == "grey" else FAMILIES


# ---- the strip worker's geometry (FGeo, strip_sv), restated ------------------------------------------------------------------
@dataclass(frozen=True)
class Geo:
    mw: int          # MCU size along the kernel's x (one lane per pixel column) ...
    mh: int          # ... and along its y (the direction of a lane's byte run)
    tml: int         # MCUs the 64 lanes cover in one turn
    sv: int          # turns per lane
    @property
    def tmw(self):   # MCUs of a strip
        return self.tml * self.sv
    @property
    def strip(self):  # pixel rows of a strip
        return self.tmw * self.mh


def kernel_geo(layout: str, transposed: bool) -> Geo:
    """x-major output: the kernel's (x, y) is the image's; row-major: the worker runs on the transposed image."""
    f = LAYOUTS[layout]
    nc = len(f)
    hs, vs = f[0] if nc == 3 else (1, 1)
    if transposed:
        hs, vs = vs, hs
    mw, mh = 8 * hs, 8 * vs
    tml = 64 // mw
    run = tml * 8 * nc
    sv = 1 if mh != 8 else (1 if run >= 192 else (4 if run == 64 else 2))
    return Geo(mw, mh, tml, sv)


def mcu_px(layout: str) -> Tuple[int, int]:
    f = LAYOUTS[layout]
    return (8 * f[0][0], 8 * f[0][1]) if len(f) == 3 else (8, 8)


@dataclass
class Image:
    layout: str
    family: str
    name: str
    width: int
    height: int
    blocks: np.ndarray                      # int16 [n_blocks, 64], zig-zag, MCU order, absolute DC
    qts: Tuple[np.ndarray, np.ndarray]
    planted: List[Tuple[int, int]] = field(default_factory=list)     # (MCU column, MCU row) of the planted MCUs
    _raw: Optional[bytes] = None

    @property
    def factors(self):
        return LAYOUTS[self.layout]

    @property
    def mcus(self) -> Tuple[int, int]:
        mw, mh = mcu_px(self.layout)
        return -(-self.width // mw), -(-self.height // mh)

    def file(self) -> bytes:
        """The baseline file of these blocks, one restart interval per MCU row."""
        if self._raw is None:
            from tools import craft_jpeg
            self._raw = craft_jpeg.craft_baseline(self.width, self.height, self.factors, restart_interval=self.mcus[0],
                                                  blocks=self.blocks, qts=self.qts)
        return self._raw


def _qt(v: int) -> np.ndarray:
    return np.full(64, v, dtype=np.uint8)


class _Grid:
    """Blocks of an image on its MCU grid: y[row, col, block of the MCU, 64], cb / cr[row, col, 64]."""

    def __init__(self, layout, width, height):
        self.layout, self.width, self.height = layout, width, height
        mw, mh = mcu_px(layout)
        self.mcw, self.mch = -(-width // mw), -(-height // mh)
        f = LAYOUTS[layout]
        self.nby = f[0][0] * f[0][1] if len(f) == 3 else 1
        self.y = np.zeros((self.mch, self.mcw, self.nby, 64), dtype=np.int64)
        self.cb = np.zeros((self.mch, self.mcw, 64), dtype=np.int64)
        self.cr = np.zeros((self.mch, self.mcw, 64), dtype=np.int64)

    def image(self, family, name, qts, planted=()):
        if len(LAYOUTS[self.layout]) == 1:
            blocks = self.y.reshape(-1, 64)
        else:
            blocks = np.concatenate([self.y, self.cb[:, :, None], self.cr[:, :, None]], axis=2).reshape(-1, 64)
        assert np.abs(blocks).max() <= 32767
        return Image(self.layout, family, name, self.width, self.height, blocks.astype(np.int16), qts, list(planted))


def _sizes(layout: str) -> Dict[str, Tuple[int, int]]:
    """Image sizes in units of the strips of BOTH output orders (x-major strips run down the height, row-major strips along
    the width): A odd x odd with 3 columns / 5 rows behind the last full strip (a bottom strip of fewer than 16 bytes per
    column, a partial MCU at the right edge, H * 3 no multiple of 4); B multiples of 4 with a last strip of one MCU and 4
    pixels; C odd x odd, one strip plus one MCU plus a few pixels; D multiples of 4 with a last strip of 4 pixels alone."""
    sx, sy = kernel_geo(layout, True).strip, kernel_geo(layout, False).strip
    mw, mh = mcu_px(layout)
    return {"A": (2 * sx + 3, 2 * sy + 5), "B": (2 * sx + mw + 4, 2 * sy + mh + 4), "C": (sx + 2 * mw + 1, sy + mh + 3),
            "D": (2 * sx + 4, 2 * sy + 4)}


def _rng(layout: str, family: str):
    return np.random.default_rng([20261017, list(LAYOUTS).index(layout), FAMILIES.index(family)])


def _benign_luma(g: _Grid, rng, lo=-100, hi=100):
    """Luma table all 8: DC = Y - 128.  A different level in every MCU (a misplaced run shows), one small AC in half the blocks."""
    g.y[..., 0] = rng.integers(lo, hi + 1, size=g.y.shape[:-1])
    k = rng.integers(1, 6, size=g.y.shape[:-1])
    v = rng.integers(-6, 7, size=g.y.shape[:-1]) * (rng.random(g.y.shape[:-1]) < 0.5)
    np.put_along_axis(g.y, k[..., None], v[..., None], axis=-1)


# (chroma blocks per layout for the B-tie family: what its floors need at the rates a CPU run of this recipe gave)
_TIE_MCUS = {"444": (20, 20), "422": (48, 72), "440": (64, 34), "420": (30, 32), "411": (24, 72)}


def _tie(layout):
    """Chroma table all 1.  Cb: DC = 8 * (+-125) + [-24, 24] and up to three coefficients of the 3x3 corner in [-12, 12]: about
    half of such blocks have samples on both sides of +-125, and with subsampled chroma an interpolated value can be 125
    where no source sample is.  One sign per MCU row (see the module's note on DC differences)."""
    rng = _rng(layout, "tie")
    mw, mh = mcu_px(layout)
    mcw, mch = _TIE_MCUS[layout]
    g = _Grid(layout, mcw * mw - 4, mch * mh - 4)
    _benign_luma(g, rng)
    sign = np.where(np.arange(g.mch) % 2 == 0, 1, -1)[:, None]
    g.cb[..., 0] = sign * 1000 + rng.integers(-24, 25, size=(g.mch, g.mcw))
    for _ in range(3):
        on = rng.random((g.mch, g.mcw)) < 0.6
        k = rng.choice(CORNER, size=(g.mch, g.mcw))
        v = rng.integers(-12, 13, size=(g.mch, g.mcw)) * on
        np.put_along_axis(g.cb, k[..., None], v[..., None], axis=-1)
    g.cr[..., 0] = rng.integers(-400, 401, size=(g.mch, g.mcw))
    return [g.image("tie", "brackets", (_qt(8), _qt(1)))]


def green_pairs():
    """The (cb, cr) of the colour lattice test: |c| < 250, remainder of 17207 cb + 35707 cr within 2 of +-25000."""
    cb, cr = np.meshgrid(np.arange(-249, 250), np.arange(-249, 250), indexing="ij")
    near = green_remainder(cb, cr) >= 24998
    return np.stack([cb[near], cr[near]], axis=1)


def green_remainder(cb, cr):
    """|remainder| of the green numerator N = 17207 cb + 35707 cr against 50000 (0 ... 25000)."""
    n = 17207 * np.asarray(cb, dtype=np.int64) + 35707 * np.asarray(cr, dtype=np.int64)
    return np.abs(((n + 25000) % 50000) - 25000)


def _green(layout):
    """Chroma table 8 for the DC and 1 for the rest, DC-only chroma at the lattice pairs (every sample of the MCU = the pair, through the subsampled
    chroma_of as well), with three Y each; then the same pairs with one small AC coefficient, so that hits land behind an
    upsample.  Every other MCU is benign.  Sizes are multiples of 4: the strips are staged and the patch happens in LDS."""
    rng = _rng(layout, "green")
    pairs = green_pairs()
    ys = (17, 128, 254)
    entries = [(cb, cr, y, grad) for grad in (0, 1) for y in ys for cb, cr in pairs]
    mw, mh = mcu_px(layout)
    mcw = 17
    mch = -(-2 * len(entries) // mcw) + 1
    g = _Grid(layout, mcw * mw - 4, mch * mh - 4)
    _benign_luma(g, rng)
    g.cb[..., 0] = rng.integers(-90, 91, size=(g.mch, g.mcw))
    g.cr[..., 0] = rng.integers(-90, 91, size=(g.mch, g.mcw))
    for i, (cb, cr, y, grad) in enumerate(entries):
        r, c = divmod(2 * i, mcw)
        g.y[r, c] = 0
        g.y[r, c, :, 0] = y - 128
        g.cb[r, c, 0], g.cr[r, c, 0] = cb, cr
        if grad:
            g.cb[r, c, int(rng.choice((1, 2)))] = int(rng.choice((-9, -6, -4, 4, 6, 9)))
            g.cr[r, c, int(rng.choice((1, 2)))] = int(rng.choice((-9, -6, -4, 4, 6, 9)))
    qc = _qt(1)
    qc[0] = 8
    return [g.image("green", "lattice", (_qt(8), qc))]


def _range(layout):
    """Chroma table all 8 (DC = the sample).  Flat MCUs at |c| = 249, 250, 251 for either component and sign, MCUs at 248 with a
    small gradient, and MCUs far outside (DC to +-1000 plus one large AC coefficient: |c| to a few thousand) — every
    other MCU benign.  The MCUs at the edge carry a luma gradient around 128 - 1.402 cr (128 - 1.772 cb): their R (B) is unclamped."""
    rng = _rng(layout, "range")
    w, h = _sizes(layout)["A"]
    g = _Grid(layout, w, h)
    _benign_luma(g, rng)
    g.cb[..., 0] = rng.integers(-100, 101, size=(g.mch, g.mcw))
    g.cr[..., 0] = rng.integers(-100, 101, size=(g.mch, g.mcw))
    special = []
    for comp in (0, 1):
        for sgn in (1, -1):
            special += [(comp, sgn * m, 0, 0) for m in (249, 250, 251)]
            special += [(comp, sgn * 248, int(rng.choice((1, 2))), int(rng.choice((-3, -2, 2, 3)))) for _ in range(3)]
            special += [(comp, sgn * int(rng.integers(300, 1001)), int(rng.choice((1, 2, 4))), int(rng.choice((-1, 1)) * rng.integers(200, 1001)))
                        for _ in range(3)]
    cells = [(r, c) for r in range(g.mch) for c in range(g.mcw) if (r + c) % 2 == 0]
    assert len(cells) >= len(special), (layout, len(cells), len(special))
    for i, (r, c) in enumerate(cells):
        comp, dc, k, v = special[i % len(special)]
        blk = g.cb if comp == 0 else g.cr
        blk[r, c, 0] = dc
        if k:
            blk[r, c, k] = v
        if abs(dc) <= 251:
            # luma that keeps this MCU's R (B) INSIDE 0..255, odd and even: 1.402 * 250 is the exact .5 the range decision guards,
            # and a saturated R would hide what the fp32 expression makes of it
            g.y[r, c, :, 0] = -int(round((1.772 if comp == 0 else 1.402) * dc)) + rng.integers(-100, 101, size=g.nby)
            g.y[r, c, :, 1:] = 0
            g.y[r, c, :, 1], g.y[r, c, :, 2] = rng.choice((-5, -3, 3, 5), size=g.nby), rng.choice((-5, -3, 3, 5), size=g.nby)
    return [g.image("range", "edges", (_qt(8), _qt(8)))]


def _clamp(layout):
    """Luma table all 8: Y from far below 0 to far above 255, flat and with a gradient; chroma (table all 8) at 0, +-100, +-127 and
    +-200, so that R, G and B saturate at both ends and also pass through the range unclamped."""
    rng = _rng(layout, "clamp")
    w, h = _sizes(layout)["B"]
    g = _Grid(layout, w, h)
    levels = np.array([-1000, -600, -300, -160, -129, -128, -127, -60, 0, 60, 126, 127, 128, 200, 300, 600, 900])
    g.y[..., 0] = rng.choice(levels, size=g.y.shape[:-1])
    k = rng.integers(1, 6, size=g.y.shape[:-1])
    v = rng.integers(-40, 41, size=g.y.shape[:-1]) * (rng.random(g.y.shape[:-1]) < 0.4)
    np.put_along_axis(g.y, k[..., None], v[..., None], axis=-1)
    cl = np.array([0, 0, 100, -100, 127, -127, 200, -200])
    g.cb[..., 0] = rng.choice(cl, size=(g.mch, g.mcw))
    g.cr[..., 0] = rng.choice(cl, size=(g.mch, g.mcw))
    return [g.image("clamp", "levels", (_qt(8), _qt(8)))]


def _heavy(rng, shape, scale, tail, factor, top):
    v = rng.laplace(0.0, scale, size=shape + (64,)) * np.exp(-np.arange(64) / 16.0)
    big = rng.random(shape + (64,)) < tail
    v[big] *= factor
    return np.clip(np.rint(v), -top, top).astype(np.int64)


def bound_blocks(blocks: np.ndarray, q: int) -> np.ndarray:
    """Zero a block's highest coefficients until sum |coefficient * q| <= INT16_SUM (the reference's cast is undefined beyond)."""
    a = np.abs(blocks) * q
    keep = np.cumsum(a, axis=-1) <= INT16_SUM
    return blocks * keep


def _wild(layout):
    """Heavy-tailed blocks in every component (luma table 12, chroma table 8 for the DC and 14 for the rest, AC values to +-1023,
    the int16 bound enforced per block): chroma wild in a third of the MCUs (slow lanes), moderate in the others (plain lanes),
    and a quarter of the moderate ones flat at a pair of the green lattice (patched lanes) — so that all three kinds share strips."""
    rng = _rng(layout, "wild")
    w, h = _sizes(layout)["C"]
    g = _Grid(layout, w, h)
    g.y[:] = _heavy(rng, g.y.shape[:-1], 10.0, 0.03, 40.0, 1023)
    g.y[..., 0] = rng.integers(-60, 61, size=g.y.shape[:-1])
    wild = rng.random((g.mch, g.mcw)) < 0.33
    for blk in (g.cb, g.cr):
        calm = _heavy(rng, (g.mch, g.mcw), 1.5, 0.0, 1.0, 1023)
        mad = _heavy(rng, (g.mch, g.mcw), 10.0, 0.04, 40.0, 1023)
        blk[:] = np.where(wild[..., None], mad, calm)
        blk[..., 0] = rng.integers(-100, 101, size=(g.mch, g.mcw))
    pr = green_pairs()
    pr = pr[(green_remainder(pr[:, 0], pr[:, 1]) >= 24999) & (np.abs(pr[:, 0]) != 125)]
    seeded = ~wild & (rng.random((g.mch, g.mcw)) < 0.25)
    for r, c in np.argwhere(seeded):
        cb, cr = pr[int(rng.integers(0, len(pr)))]
        g.cb[r, c], g.cr[r, c] = 0, 0
        g.cb[r, c, 0], g.cr[r, c, 0] = cb, cr
    qc = _qt(14)
    qc[0] = 8
    g.y[:] = bound_blocks(g.y, 12)
    g.cb[:] = bound_blocks(g.cb, 14)
    g.cr[:] = bound_blocks(g.cr, 14)
    return [g.image("wild", "heavy", (_qt(12), qc))]


def _planted(layout):
    """Flat MCUs of differing grey levels everywhere, and single planted rare MCUs: never two in one strip of either output order,
    at the first and the last MCU of strips, in the first and last MCU column / row, and in the short last strips.  Two sizes:
    D (multiples of 4: the strip would be staged, the planted lane demotes it to the per-lane stores with their 16 / 8 / 4-byte
    branches; last strip of 4 pixels) and A (odd: no staging at all, the last strip holds 15 bytes of a column)."""
    out = []
    for key in ("D", "A"):
        rng = _rng(layout, "planted")
        w, h = _sizes(layout)[key]
        g = _Grid(layout, w, h)
        g.y[..., 0] = rng.integers(-100, 101, size=g.y.shape[:-1])
        tx, ty = kernel_geo(layout, True).tmw, kernel_geo(layout, False).tmw
        xs = sorted({0, tx - 1, tx, 2 * tx - 1, g.mcw - 1} & set(range(g.mcw)))
        ys = sorted({0, ty - 1, ty, 2 * ty - 1, g.mch - 1} & set(range(g.mch)))
        planted, used_col, used_row = [], set(), set()
        for i, y in enumerate(ys):                      # a diagonal through the candidates, then whatever still fits
            for x in xs[i % len(xs):] + xs[:i % len(xs)]:
                if (x, y // ty) in used_col or (y, x // tx) in used_row:
                    continue
                planted.append((x, y)); used_col.add((x, y // ty)); used_row.add((y, x // tx))
        if layout == "grey":
            kinds = [(900, 0, 0), (-900, 0, 0)]
        else:
            pr = green_pairs()
            pr = pr[(green_remainder(pr[:, 0], pr[:, 1]) >= 24999) & (np.abs(pr[:, 0]) != 125)]
            kinds = [(0, 125, 30), (0, -125, -30), (0, 40, 250), (0, -40, -251), (0, 700, 0)] + [(0, int(a), int(b)) for a, b in pr[:3]]
        for i, (x, y) in enumerate(planted):
            dy, cb, cr = kinds[i % len(kinds)]
            if dy:
                g.y[y, x, :, 0] = dy
            g.cb[y, x, 0], g.cr[y, x, 0] = cb, cr
        out.append(g.image("planted", "one_per_strip_" + key, (_qt(8), _qt(8)), planted))
    return out


_BUILD = {"tie": _tie, "green": _green, "range": _range, "clamp": _clamp, "wild": _wild, "planted": _planted}


@functools.lru_cache(maxsize=None)
def images(layout: str, family: str) -> Tuple[Image, ...]:
    """The images of one family in one layout (built once per process: tests share them and must not change them)."""
    assert family in families_of(layout), (layout, family)
    return tuple(_BUILD[family](layout))


def batch_pair(layout: str) -> List[Image]:
    """Two images of different odd sizes: in one plan the second's output starts at an odd byte."""
    a, b = (images(layout, "range")[0] if layout != "grey" else images(layout, "planted")[1]), images(layout, "wild")[0]
    assert a.width % 2 and a.height % 2 and b.width % 2 and b.height % 2 and (a.width, a.height) != (b.width, b.height)
    return [a, b]


# ---- the census ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_of(layout: str, family: str, k: int) -> dict:
    """oracle.decode of image k's file, with the IDCT seam (shared by every test; read-only)."""
    from oracle import oracle
    out = oracle.decode(images(layout, family)[k].file(), want_idct=True)
    for a in ("rgb", "planes", "idct", "coef"):
        out[a].setflags(write=False)
    return out


def census(img: Image, ref: dict, transposed: bool = False) -> dict:
    """Counts over one image, from the oracle's planes (upsampled, cropped Y / Cb / Cr), its IDCT seam (the chroma SOURCE
    samples of every MCU) and its RGB.

    MCU-level flags, each a superset of what any lane of that MCU can see in either output order (a lane looks at one or two
    source rows of its MCU): `tie` = the Cb source samples are not all inside (-125, 125), all above 125 or all below
    -125; `far` = some chroma source sample has |c| >= 250; `slow` = tie or far.  A green hit is a pixel whose remainder is
    within 1.5 of +-25000 in an MCU that is NOT slow: its lane keeps the fp32 bytes and only the patch makes them right.

    Which turn: a lane's run goes along the kernel's y — the image's y in x-major output, its x in row-major (`transposed`).
    With m = (that coordinate) // (MCU size along it), the MCU is number m % TMW of its strip (strips start at the image's
    edge and hold TMW = TML * SV MCUs) and is done in turn (m % TMW) // TML; its 8-row part is (coordinate % MCU size) // 8."""
    W, H = img.width, img.height
    out = {"pixels": W * H, "transposed": transposed}
    planes, rgb = ref["planes"], ref["rgb"]
    yp = planes[..., 0].astype(np.int64) if planes.ndim == 3 else planes.astype(np.int64)
    out["y_below_0"], out["y_above_255"] = int((yp < 0).sum()), int((yp > 255).sum())
    out["y_min"], out["y_max"] = int(yp.min()), int(yp.max())
    chans = rgb.reshape(W, H, -1)
    out["sat_0"] = [int((chans[..., c] == 0).sum()) for c in range(chans.shape[-1])]
    out["sat_255"] = [int((chans[..., c] == 255).sum()) for c in range(chans.shape[-1])]
    out["unclamped"] = [int(((chans[..., c] > 0) & (chans[..., c] < 255)).sum()) for c in range(chans.shape[-1])]
    mcw, mch = img.mcus
    geo = kernel_geo(img.layout, transposed)
    out["geo"] = geo
    if len(img.factors) == 1:
        return out
    nby = img.factors[0][0] * img.factors[0][1]
    per = nby + 2
    seam = ref["idct"].reshape(mch, mcw, per, 8, 8).astype(np.int64) - 128
    scb, scr = seam[:, :, nby], seam[:, :, nby + 1]                        # [MCU row, MCU column, x, y] source samples
    mn, mx = scb.min(axis=(2, 3)), scb.max(axis=(2, 3))
    tie = ~(((mx < 125) & (mn > -125)) | (mn > 125) | (mx < -125))
    brackets = ((mn < 125) & (mx > 125)) | ((mn < -125) & (mx > -125))
    has125 = (np.abs(scb) == 125).any(axis=(2, 3))
    far = np.maximum(np.abs(scb).max(axis=(2, 3)), np.abs(scr).max(axis=(2, 3))) >= 250
    slow = tie | far
    mwp, mhp = mcu_px(img.layout)
    X, Y = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    mcx, mcy = X // mwp, Y // mhp
    cb, cr = planes[..., 1].astype(np.int64) - 128, planes[..., 2].astype(np.int64) - 128
    is125 = np.abs(cb) == 125
    out["cb125"] = int(is125.sum())
    out["cb125_interp_only"] = int((is125 & ~has125[mcy, mcx]).sum())
    out["mcus"] = mcw * mch
    out["mcus_bracket"], out["mcus_tie"], out["mcus_far"], out["mcus_slow"] = int(brackets.sum()), int(tie.sum()), int(far.sum()), int(slow.sum())
    out["src_mag"] = {name: {m: int((np.abs(s) == m).sum()) for m in (249, 250, 251)} for name, s in (("cb", scb), ("cr", scr))}
    out["src_abs_max"] = int(max(np.abs(scb).max(), np.abs(scr).max()))
    hit = (green_remainder(cb, cr) >= 24999) & ~slow[mcy, mcx]
    out["green_hits"] = int(hit.sum())
    out["mcus_green"] = int(np.unique((mcy * mcw + mcx)[hit]).size)
    run = X if transposed else Y
    part = (run % geo.mh) // 8
    turn = ((run // geo.mh) % geo.tmw) // geo.tml
    out["green_by_part"] = [int((hit & (part == p)).sum()) for p in range(geo.mh // 8)]
    out["green_by_turn"] = [int((hit & (turn == t)).sum()) for t in range(geo.sv)]
    # strips (of this output order) by what their MCUs are: a strip is TMW MCUs along the run direction in one MCU column of it
    m_run, m_col = (mcx, mcy) if transposed else (mcy, mcx)
    sid = (m_col * (max(mcw, mch) // geo.tmw + 2) + m_run // geo.tmw)
    green_mcu = np.zeros_like(slow)
    green_mcu[mcy[hit], mcx[hit]] = True
    k_slow, k_green = slow[mcy, mcx], green_mcu[mcy, mcx] & ~slow[mcy, mcx]
    s_slow, s_green = set(np.unique(sid[k_slow])), set(np.unique(sid[k_green]))
    s_plain = set(np.unique(sid[~k_slow & ~k_green]))
    out["strips"] = int(np.unique(sid).size)
    # ... and the hits whose STRIP has no slow MCU: with a run of whole dwords (`stageable`) that strip keeps the staged stores and
    # the patch happens in LDS (green_fix_lds); in a strip a slow lane demotes, the hit goes through the exact routine instead
    clean = hit & ~np.isin(sid, sorted(s_slow))
    out["stageable"] = ((W if transposed else H) * 3) % 4 == 0
    out["green_staged_hits"] = int(clean.sum())
    out["green_staged_by_part"] = [int((clean & (part == p)).sum()) for p in range(geo.mh // 8)]
    out["green_staged_by_turn"] = [int((clean & (turn == t)).sum()) for t in range(geo.sv)]
    out["strips_slow_and_plain"] = len(s_slow & s_plain)
    out["strips_green_and_plain"] = len((s_green - s_slow) & s_plain)
    out["strips_all_three"] = len(s_slow & s_green & s_plain)
    return out


def planted_census(img: Image, ref: dict, transposed: bool) -> dict:
    """Where the planted MCUs of a `planted` image sit in the strips of one output order: every strip with a planted MCU has exactly
    one, and these are its position (first / last MCU of a full strip), its MCU column's position and whether the strip is
    the short last one.  (That the planted MCUs ARE rare and the others are not is `census`' mcus_slow / mcus_green.)"""
    geo = kernel_geo(img.layout, transposed)
    mcw, mch = img.mcus
    n_run, n_col = (mcw, mch) if transposed else (mch, mcw)
    size_run = img.width if transposed else img.height
    seen = {}
    for (x, y) in img.planted:
        m, c = (x, y) if transposed else (y, x)
        seen.setdefault((c, m // geo.tmw), []).append(m % geo.tmw)
    last_strip = (n_run - 1) // geo.tmw
    return {
        "strips_with_one": sum(len(v) == 1 for v in seen.values()), "strips_with_more": sum(len(v) > 1 for v in seen.values()),
        "first_of_strip": sum(v == [0] for v in seen.values()),
        "last_of_full_strip": sum(v == [geo.tmw - 1] for v in seen.values()),
        "first_column": sum(c == 0 for c, _ in seen), "last_column": sum(c == n_col - 1 for c, _ in seen),
        "in_last_strip": sum(s == last_strip for _, s in seen),
        "last_strip_rows": size_run - last_strip * geo.strip,
    }


def staged_windows(img: Image) -> Dict[str, Tuple[int, int, int, int]]:
    """Windows (x, y, width, height) whose strips the WIN instance can stage in BOTH output orders: origin and extent multiples of
    4 along either axis (window bytes per column / row and the top row's offset are whole dwords), starting and ending 4 pixels
    inside MCUs (bytes cut from the first strip's runs, rlo > 0, and from the last's, rhi < RUN).  `staged` covers nearly the whole
    image; `staged_shifted` starts one MCU further in, so the window's strips — which begin at the window's first MCU row —
    do not coincide with the image's."""
    W, H = img.width, img.height
    mw, mh = mcu_px(img.layout)
    out = {}
    def extent(size, o, m, strip):
        # the largest multiple of 8 that ends short of the edge, 4 pixels inside an MCU and at least 12 rows (36 bytes) into the
        # window's last strip (strips start at the window's first MCU row): 4 rows alone would be 12 bytes, too few to stage
        e = ((size - o - 1) // 8) * 8
        while e >= 8 and (o + e - (o // m) * m) % strip == 4:
            e -= 8
        return e

    for name, (x0, y0) in (("staged", (4, 4)), ("staged_shifted", (mw + 4, mh + 4))):
        w, h = extent(W, x0, mw, kernel_geo(img.layout, True).strip), extent(H, y0, mh, kernel_geo(img.layout, False).strip)
        if w >= 8 and h >= 8:
            out[name] = (x0, y0, w, h)
    return out


def window_census(img: Image, ref: dict, win, transposed: bool) -> dict:
    """What a window plan of ONE image (its output starts at byte 0) meets in one output order.  The WIN instance cuts the window's
    MCU rectangle into strips that start at the window's FIRST MCU row (along the run direction): MCU m of the run is number
    (m - m0) % TMW of its strip and is done in turn ((m - m0) % TMW) // TML, m0 = (window origin) // (MCU size).  A strip is
    staged iff the window's run bytes and its origin's offset are whole dwords (`eligible`), it holds 16 bytes or more of the
    run, and no lane of it is slow — here: none of its MCUs is (the MCU-level flags of `census`, a superset)."""
    x0, y0, w, h = win
    geo = kernel_geo(img.layout, transposed)
    mcw, mch = img.mcus
    r0, rn, a0, an = (x0, w, y0, h) if transposed else (y0, h, x0, w)          # run axis / across axis
    out = {"eligible": (rn * 3) % 4 == 0 and (r0 * 3) % 4 == 0, "geo": geo}
    nby = img.factors[0][0] * img.factors[0][1]
    seam = ref["idct"].reshape(mch, mcw, nby + 2, 8, 8).astype(np.int64) - 128
    scb, scr = seam[:, :, nby], seam[:, :, nby + 1]
    mn, mx = scb.min(axis=(2, 3)), scb.max(axis=(2, 3))
    slow = ~(((mx < 125) & (mn > -125)) | (mn > 125) | (mx < -125)) | (np.maximum(np.abs(scb).max(axis=(2, 3)), np.abs(scr).max(axis=(2, 3))) >= 250)
    mwp, mhp = mcu_px(img.layout)
    X, Y = np.meshgrid(np.arange(x0, x0 + w), np.arange(y0, y0 + h), indexing="ij")
    mcx, mcy = X // mwp, Y // mhp
    planes = ref["planes"][x0:x0 + w, y0:y0 + h]
    cb, cr = planes[..., 1].astype(np.int64) - 128, planes[..., 2].astype(np.int64) - 128
    run, m_run, m_col = (X, mcx, mcy) if transposed else (Y, mcy, mcx)
    m0 = r0 // geo.mh
    strip = (m_run - m0) // geo.tmw
    sid = m_col * 4096 + strip
    slow_strips = np.unique(sid[slow[mcy, mcx]])
    # bytes of the strip's run inside the window: [rlo, rhi) of RUN = TMW * MH * 3
    first = (m0 + strip * geo.tmw) * geo.mh
    rlo, rhi = np.maximum(0, r0 - first) * 3, np.minimum(geo.strip, r0 + rn - first) * 3
    staged = out["eligible"] & (rhi - rlo >= 16) & ~np.isin(sid, slow_strips)
    hit = (green_remainder(cb, cr) >= 24999) & ~slow[mcy, mcx] & staged
    part = (run % geo.mh) // 8
    turn = ((m_run - m0) % geo.tmw) // geo.tml
    out["staged_strips"] = int(np.unique(sid[staged]).size)
    out["staged_strips_cut_at_the_top"] = int(np.unique(sid[staged & (rlo > 0)]).size)
    out["staged_strips_cut_at_the_bottom"] = int(np.unique(sid[staged & (rhi < geo.strip * 3)]).size)
    out["green_staged_hits"] = int(hit.sum())
    out["green_staged_by_part"] = [int((hit & (part == p)).sum()) for p in range(geo.mh // 8)]
    out["green_staged_by_turn"] = [int((hit & (turn == t)).sum()) for t in range(geo.sv)]
    out["green_staged_in_cut_strips"] = int((hit & ((rlo > 0) | (rhi < geo.strip * 3))).sum())
    return out
