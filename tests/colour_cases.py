"""What tests/test_colour_paths_host.py (no GPU) and tests/test_colour_paths.py (MI355X) share: the canvases that take the colour
launches (csrc/colour.hip) down the paths tests/test_colour.py and tests/test_blur.py do not reach on purpose — the data-dependent
branches of the tables (a flat band, a zero step, quotients above 255, the .5 tie of contrast's mean), every entry of every table,
the histogram launch's chunks and runs, the blurs' dword forms at row ends and clamps, and index lists over many outputs.

The crafted files are written with tools/craft_jpeg.craft_baseline: quantisation tables that are all 8, DC-only blocks, a restart
interval of one MCU row — every 8 x 8 block is flat at level DC + 128.  The call's size is the file's size, where the default
bilinear resize is the identity, so the canvas IS the block pattern.  Grey files have a 4:4:4 twin with neutral chroma (R = G = B);
COLOUR is a 4:4:4 file whose chroma DCs are not zero.  The host file holds every file to its levels, every case to what it is meant
to reach and to the wrong variants it must tell apart; the GPU file runs the same cases.  Neither a test file nor a conftest:
nothing here is collected."""
import numpy as np

Q8 = [[8] * 64] * 2
HIST_PIXELS, LANE_PIXELS = 4096, 16           # csrc/mijpeg_internal.h: kColourHistPixels, and a lane's share of a chunk
_files, _pixels = {}, {}


def _blocks(levels, chroma=None):
    """DC-only blocks in MCU order for a grid of block levels (rows of block rows); chroma: per block (Cb, Cr) levels, or None"""
    flat = [int(v) for row in levels for v in row]
    per = 1 if chroma is None else 3
    out = np.zeros((len(flat) * per, 64), dtype=np.int16)
    for k, v in enumerate(flat):
        out[k * per, 0] = v - 128
        if chroma is not None:
            out[k * per + 1, 0], out[k * per + 2, 0] = chroma[k][0] - 128, chroma[k][1] - 128
    return out


def craft(levels, colour: bool = False, chroma=None) -> bytes:
    """the file whose 8 x 8 blocks have these levels: greyscale, or 4:4:4 with neutral chroma (or with the chroma levels given)"""
    from tools import craft_jpeg
    levels = np.asarray(levels)
    bh, bw = levels.shape
    if colour and chroma is None:
        chroma = [(128, 128)] * (bw * bh)
    return craft_jpeg.craft_baseline(bw * 8, bh * 8, ((1, 1),) * (3 if colour else 1), restart_interval=bw, blocks=_blocks(levels, chroma if colour else None),
                                     qts=Q8)


def _grid(bw, bh, rest, first=()):
    g = np.full(bw * bh, rest, dtype=np.int64)
    g[:len(first)] = first
    return g.reshape(bh, bw)


PERMUTED = (np.arange(256) * 37 + 11) % 256          # every level once, neighbours far apart

# name -> the levels of its blocks, row by row (the table of the cases: what each reaches is asserted in the host file)
LEVELS = {
    "all_levels": PERMUTED.reshape(16, 16),                               # 128 x 128: every entry of every table is compared
    "one_level_77": _grid(4, 4, 77),                                      # hi <= lo, nz <= 1, contrast's mean = the level; one run per lane
    "one_level_255": _grid(4, 4, 255),                                    # ... and a blur of 255 stays 255
    "two_levels": _grid(4, 4, 10, [200] * 8),                             # autocontrast to {0, 255}
    "zero_step": _grid(4, 4, 240, [3, 50, 100]),                          # equalize: step == 0
    "clips": _grid(4, 4, 240, [3, 50, 100, 150, 200]),                    # equalize: step == 1, quotients 256 and 320 clipped to 255
    "mean_tie": _grid(4, 4, 10, [11] * 8),                           # colour_mean: 10.5 + 0.5 -> 11
    "board": (np.add.outer(np.arange(3), np.arange(5)) & 1) * 255,        # 40 x 24: a blur at full contrast, both directions
}
# COLOUR: 32 x 32, 4:4:4, sixteen blocks of their own (Y, Cb, Cr): the three components and L have histograms of their own
COLOUR = "colour"
_COLOUR_Y = _grid(4, 4, 0, [40 + 11 * k for k in range(16)])
_COLOUR_CHROMA = [(128 + ((k * 5) % 16 - 8) * 6, 128 + ((k * 11) % 16 - 7) * 7) for k in range(16)]
NAMES = list(LEVELS) + [COLOUR]


def size_of(name: str):
    bh, bw = (_COLOUR_Y if name == COLOUR else np.asarray(LEVELS[name])).shape
    return (bw * 8, bh * 8)


def raw(name: str, colour: bool = False) -> bytes:
    """the crafted file: grey, or (colour) its 4:4:4 twin; COLOUR is a colour file only"""
    key = (name, colour or name == COLOUR)
    if key not in _files:
        _files[key] = craft(_COLOUR_Y, True, _COLOUR_CHROMA) if name == COLOUR else craft(LEVELS[name], colour)
    return _files[key]


def intended(name: str, colour: bool = False) -> np.ndarray:
    """the canvas a grey crafted file (or its twin) is meant to be, row-major (H, W) or (H, W, 3)"""
    a = np.kron(np.asarray(LEVELS[name]), np.ones((8, 8), dtype=np.int64)).astype(np.uint8)
    return np.stack([a] * 3, axis=-1) if colour else a


def pixels(name: str, colour: bool = False) -> np.ndarray:
    """the file's pixels by the oracle, row-major (H, W) or (H, W, 3); never the library's"""
    key = (name, colour or name == COLOUR)
    if key not in _pixels:
        from oracle import oracle
        full = oracle.decode(raw(*key))["rgb"]
        a = np.ascontiguousarray(full.swapaxes(0, 1))
        a = a[..., 0] if a.ndim == 3 and a.shape[2] == 1 else a
        a.setflags(write=False)
        _pixels[key] = a
    return _pixels[key]


def canvas(name: str, colour: bool = False, mode=None) -> np.ndarray:
    """the canvas of the call at the file's own size in this mode, from the oracle's pixels"""
    from tools import mode_model
    return mode_model.convert(pixels(name, colour), mode)


# ---- the ops every canvas is meant for -------------------------------------------------------------------------------------------
FACTORS = (0, 0.3, 1, 1.9, -0.5)
TABLE_OPS = ([("brightness", f) for f in FACTORS] + [("contrast", f) for f in FACTORS] +
             [("posterize", 1), ("posterize", 8), ("solarize", 0), ("solarize", 256), ("invert",), ("autocontrast",), ("equalize",)])
STATISTICS = [("autocontrast",), ("equalize",), ("contrast", 1.9), ("contrast", 0.3), ("contrast", 0)]
BLURS = [("gaussian_blur", 2.0), ("box_blur", 1.5)]
OPS_OF = {"all_levels": TABLE_OPS, "one_level_77": STATISTICS, "one_level_255": STATISTICS + BLURS, "two_levels": STATISTICS, "zero_step": STATISTICS,
          "clips": STATISTICS, "mean_tie": STATISTICS, "board": BLURS + [("contrast", 0.3)], COLOUR: TABLE_OPS}
IDENTITY_FIRST = ("posterize", 8)             # in front of an op it makes the op read canvas 1, whose bytes are canvas 0's


def chains_of(name: str):
    """every op of the canvas alone, behind an op that changes nothing, and behind one that does"""
    ops = OPS_OF[name]
    return [(op,) for op in ops] + [(IDENTITY_FIRST, op) for op in ops] + [(("invert",), op) for op in ops if op in STATISTICS + BLURS]


# ---- canvas geometries, on natural files --------------------------------------------------------------------------------------------
HIST_SIZES = ((64, 64), (17, 241), (241, 17), (23, 7))          # one chunk exactly; 4097 pixels both ways; fewer pixels than lanes x 16
HIST_CHAINS = [(("equalize",),), (("autocontrast",), ("contrast", 1.6)), (("invert",), ("contrast", 0.4), ("equalize",))]
BLUR_SIZES = ((2, 5), (6, 5), (34, 3), (7, 1))                  # ow % 4 == 2 three times; oh == 1
BLUR_CHAINS = [(("gaussian_blur", 2.0),), (("box_blur", 1.5),), (("invert",), ("gaussian_blur", 0.8), ("box_blur", 0.25))]
BOX_RADII = (3, 4, 5, 6)                                        # on 6 x 5: r = n - 2, n - 1, n and beyond, for both sides

MANY, MANY_SIZE = 70, (16, 12)


def many_views(w: int, h: int):
    """70 windows of a w x h image, all different"""
    return [(0, (k % 9, (2 * k) % 7, w // 2 + k % 5, h // 2 + k % 3)) for k in range(MANY)]


def many_chains():
    """view k's chain from a cycle of seven, its factor or radius from k: histogram ops at steps 0, 1 and 2, blurs at steps 0 (two in
    seven), 1 (one in seven) and 3, per-pixel ops, an ended chain beside running ones, and None"""
    out = []
    for k in range(MANY):
        out.append([(("contrast", 0.5 + 0.02 * k), ("gaussian_blur", 0.3 + 0.03 * k)),
                    (("box_blur", 0.2 + 0.05 * k),),
                    (("brightness", 0.6 + 0.01 * k), ("equalize",)),
                    None,
                    (("gaussian_blur", 0.2 + 0.02 * k), ("autocontrast",), ("sharpness", 0.5 + 0.03 * k)),
                    (("solarize", 60 + 2 * k), ("color", 0.3 + 0.02 * k)),
                    (("autocontrast",), ("invert",), ("posterize", 1 + k % 8), ("box_blur", 0.5 + 0.04 * k))][k % 7])
    return out


# ---- the model with its parts exposed: what the wrong variants change ---------------------------------------------------------------
def memory_order(a: np.ndarray, layout: str) -> np.ndarray:
    """the canvas's pixels (npix, C) in the order the histogram launch walks them: rows in the row-major layouts, columns in the others"""
    b = a.reshape(a.shape[0], a.shape[1], -1)
    if layout in ("xmajor", "planar"):
        b = b.swapaxes(0, 1)
    return np.ascontiguousarray(b).reshape(-1, b.shape[2])


def histograms(a: np.ndarray, layout: str = "rowmajor", whole_chunks_only: bool = False, without_last_runs: bool = False) -> dict:
    """{component: 256 counts, "L": those of the canvas's L} as k_colour_hist counts them — chunks of HIST_PIXELS pixels, a lane
    LANE_PIXELS consecutive ones, one add per run of a value.  whole_chunks_only: a launch that loses the pixels beyond the last
    whole chunk; without_last_runs: one that never adds the run a lane ends with."""
    from tools import colour_model
    p = memory_order(a, layout)
    bands = {c: p[:, c].astype(np.int64) for c in range(p.shape[1])}
    bands["L"] = colour_model.grey(p[None, :, :] if p.shape[1] == 3 else p[None, :, 0]).ravel().astype(np.int64)
    n = len(p) // HIST_PIXELS * HIST_PIXELS if whole_chunks_only else len(p)
    out = {}
    for b, v in bands.items():
        h = np.zeros(256, dtype=np.int64)
        for s in range(0, n, LANE_PIXELS):
            lane = v[s:s + LANE_PIXELS]
            if without_last_runs:
                lane = lane[:len(lane) - int(np.argmax(lane[::-1] != lane[-1]) if (lane != lane[-1]).any() else len(lane))]
            h += np.bincount(lane, minlength=256)
        out[b] = h
    return out


def mean_of(h, round_half_up: bool = True) -> int:
    total = int(h.sum())
    if not total:
        return 0
    m = sum(i * int(h[i]) for i in range(256)) / total
    return int(m + 0.5) if round_half_up else int(m)


def table_op(a: np.ndarray, op, hists: dict, mean_band="L", round_half_up: bool = True, autocontrast=None, equalize=None) -> np.ndarray:
    """contrast, autocontrast or equalize on canvas ``a`` from the histograms given; the defaults are tools/colour_model.py's op"""
    from tools import colour_model as M
    if op[0] == "contrast":
        return M.blend(np.full_like(a, mean_of(hists[mean_band], round_half_up)), a, op[1])
    table_of = (autocontrast or M.autocontrast_table) if op[0] == "autocontrast" else (equalize or M.equalize_table)
    if a.ndim == 2:
        return table_of(hists[0])[a]
    return np.stack([table_of(hists[c])[a[..., c]] for c in range(3)], axis=-1)


def equalize_quantities(h):
    """(step, the UNCLIPPED quotient n // step at every level the band has) — step 0: no quotients"""
    nz = [int(v) for v in h if v]
    step = (sum(nz) - nz[-1]) // 255 if nz else 0
    return step, ([(step // 2 + int(h[:v].sum())) // step for v in np.flatnonzero(h)] if step else [])


def equalize_from_zero(h):
    step, _ = equalize_quantities(h)
    if len([v for v in h if v]) <= 1 or not step:
        return np.arange(256, dtype=np.uint8)
    return np.array([min(255, int(h[:v].sum()) // step) for v in range(256)], dtype=np.uint8)


def equalize_wrapping(h):
    step, _ = equalize_quantities(h)
    if len([v for v in h if v]) <= 1 or not step:
        return np.arange(256, dtype=np.uint8)
    return np.array([((step // 2 + int(h[:v].sum())) // step) & 255 for v in range(256)], dtype=np.uint8)


def autocontrast_always_stretching(h):
    """the stretch of [lo, hi] without the branch for hi <= lo (the span taken as at least one level)"""
    nz = np.flatnonzero(h)
    if not len(nz):
        return np.arange(256, dtype=np.uint8)
    lo, hi = int(nz[0]), int(nz[-1])
    scale = 255.0 / max(hi - lo, 1)
    return np.array([min(max(int(i * scale - lo * scale), 0), 255) for i in range(256)], dtype=np.uint8)


def blur_variant(a: np.ndarray, op, padded: bool = False, height_first: bool = False) -> np.ndarray:
    """a blur as tools/colour_model.blur does it, or: with the rows padded with zeros to a multiple of four pixels and the taps
    clamped at the padded width; with the passes along the height first"""
    from tools import colour_model as M
    fr, passes = (M.gaussian_box_radius(op[1]), 3) if op[0] == "gaussian_blur" else (np.float32(op[1]), 1)
    w = a.shape[1]
    for axis in ((0, 1) if height_first else (1, 0)):
        for _ in range(passes):
            if padded and axis == 1:
                wide = np.zeros(a.shape[:1] + ((w + 3) & ~3,) + a.shape[2:], dtype=np.uint8)
                wide[:, :w] = a
                a = np.ascontiguousarray(M.box_pass(wide, fr, 1)[:, :w])
            else:
                a = M.box_pass(a, fr, axis)
    return a
