"""What tests/test_reduce_paths_host.py (no GPU) and tests/test_reduce_paths.py (MI355X) share: the calls that take k_reduce
(csrc/reduce.hip) down the paths tests/test_reduce.py does not reach — row segments staged in pieces with cells that straddle a
piece boundary, several tiles along the contiguous axis together with a phase, full lanes with a tail store, the LUMA instance and
views' pitches on long rows, the early return along the contiguous axis, the largest cell — and `census`, which restates how the
launch is cut (csrc/resize_plan.hip: reduce_stage) and says, for every output of a plan, what each tile of it does.  The host file
holds every case to the census and to the wrong variants of the kernel's loop (`kernel`) it must tell apart; the GPU file runs
the same cases and asserts the census against the plan's own numbers (mj_debug_reduce_shape, mj_debug_reduce_launch) first.

A case is one PLAN: a few outputs (`Slot`) of files of one kind at one size and gap.  Every case exists for both readings of the
buffer of decoded pixels: "x" — rows of the image are contiguous, the row-major layouts, on the wide files — and "y" — columns
are contiguous, the x-major layouts, on the files with width and height exchanged and the case's size exchanged with them.  The
files are synthetic (tools/synth.py), made when first asked for; their pixels are the oracle's.  Neither a test file nor a
conftest: nothing here is collected."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from conftest import GOLDEN

TILE_SLOW = 8               # reduced rows per workgroup
OUT_ROW = 512               # reduced bytes of a row per workgroup at most: 64 lanes x 8 elements
STAGE = 4080                # bytes of a source row a wavefront stages at a time
LANE_BYTES = 8              # reduced bytes a lane stores at once
MAX_CELL = 65536

# name -> (seed, width, height, subsampling, restart interval) of the WIDE file; the other reading takes seed + 50 at height x width
SYNTH = {"P1": (1101, 1501, 23, "420", 7), "P3": (1103, 4590, 12, "grey", 0), "T": (1104, 700, 20, "420", 3), "G": (1106, 1030, 16, "grey", 5),
         "S": (1107, 100, 64, "420", 0), "SW": (1108, 1501, 157, "420", 11)}
BIG = "c2_512x512_420"
_raw, _pixels = {}, {}


def fast_of(layout: str) -> str:
    """which axis of the stored image is contiguous in the buffer the reduce launch reads"""
    return "x" if layout in ("rowmajor", "planar_rowmajor") else "y"


def raw(name: str, fast: str = "x") -> bytes:
    key = (name, fast)
    if key not in _raw:
        from tools import synth
        if name == BIG:
            _raw[key] = (GOLDEN / "files" / f"{BIG}.jpg").read_bytes()
        elif name == "WHITE":
            _raw[key] = synth.encode_rgb(np.full((512, 512, 3), 255, dtype=np.uint8), 90, "420", 0)
        else:
            seed, w, h, sub, ri = SYNTH[name]
            _raw[key] = synth.synth_jpeg(seed, w, h, 90, sub, ri) if fast == "x" else synth.synth_jpeg(seed + 50, h, w, 90, sub, ri)
    return _raw[key]


def pixels(name: str, fast: str = "x") -> np.ndarray:
    """the oracle's pixels of the file, row-major (h, w[, 3]), decoded once and never changed"""
    key = (name, fast)
    if key not in _pixels:
        from oracle import oracle
        a = np.ascontiguousarray(oracle.decode(raw(name, fast))["rgb"].swapaxes(0, 1))
        a.setflags(write=False)
        _pixels[key] = a
    return _pixels[key]


def dims(name: str, fast: str = "x"):
    if name in (BIG, "WHITE"):
        return (512, 512)
    _, w, h, _, _ = SYNTH[name]
    return (w, h) if fast == "x" else (h, w)


def ncomp(name: str) -> int:
    return 1 if name in SYNTH and SYNTH[name][3] == "grey" else 3


@dataclass(frozen=True)
class Slot:
    """one output: a file, the orientation it is shown in and a window (x, y, w, h) of the ORIENTED image (None: all of it) — as
    rois= or, in a case with `views`, as a view of the one decoded file"""
    file: str
    window: Optional[Tuple[int, int, int, int]] = None
    orientation: int = 1


@dataclass(frozen=True)
class Case:
    name: str
    fast: str
    slots: Tuple[Slot, ...]
    size: Tuple[int, int]
    gap: float
    mode: Optional[str] = None
    views: bool = False

    @property
    def cs(self) -> int:
        return ncomp(self.slots[0].file)

    @property
    def luma(self) -> bool:
        return self.mode == "L" and self.cs == 3

    @property
    def co(self) -> int:
        return 1 if self.luma else self.cs


def turned(size, fast: str, orientation: int = 1):
    """a size given for the wide file upright, as the case's call takes it: exchanged for the other file, and by a transposing
    orientation"""
    from tools import orient_model
    swap = (fast == "y") != orient_model.transposing(orientation)
    return (size[1], size[0]) if swap else tuple(size)


def reversing(fast: str, transposing: bool = False) -> Tuple[int, ...]:
    """the orientations that reverse the contiguous axis of the stored image, from tools/orient_model.py: bit 0 reverses the
    oriented image's columns, bit 1 its rows, and a transposing orientation shows the stored rows as columns"""
    from tools import orient_model
    out = []
    for o in range(1, 9):
        b = orient_model.bits(o)
        if bool(b & 4) == transposing and b & (1 if (fast == "x") != transposing else 2):
            out.append(o)
    return tuple(out)


# ---- one output's record: csrc/resize_plan.hip reduce_stage, restated with the models -----------------------------------------------
@dataclass(frozen=True)
class Record:
    rows: int               # of the image or window as the launch reads it: rows x len pixels
    len: int
    pitch: int              # pixels from one row to the next
    origin: int             # pixels from the buffer's first to the window's first
    f_slow: int
    f_fast: int
    phase_slow: int
    phase_fast: int
    shape: Tuple[int, ...]  # mj_debug_reduce_shape's: fx, fy, phase x, phase y, reduced width, reduced height — stored axes
    stored: Tuple[int, int, int, int]       # the window in the stored image

    @property
    def off_slow(self) -> int:
        return self.f_slow - self.phase_slow if self.phase_slow else 0

    @property
    def off_fast(self) -> int:
        return self.f_fast - self.phase_fast if self.phase_fast else 0

    @property
    def orows(self) -> int:
        return -(-self.rows // self.f_slow)

    @property
    def olen(self) -> int:
        return -(-self.len // self.f_fast)


def record(c: Case, s: Slot) -> Record:
    from tools import orient_model, reduce_model
    W, H = dims(s.file, c.fast)
    b = orient_model.bits(s.orientation)
    wo, ho = orient_model.oriented_size(s.orientation, W, H)
    win = s.window if s.window is not None else (0, 0, wo, ho)
    w, h = win[2:]
    fx, fy = reduce_model.reduce_factors(w, h, c.size[0], c.size[1], c.gap)
    phx, phy = (w % fx if b & 1 else 0), (h % fy if b & 2 else 0)
    sx, sy, sw, sh = orient_model.stored_window(s.orientation, W, H, win)
    if b & 4:
        fx, fy, phx, phy = fy, fx, phy, phx
    shape = (fx, fy, phx, phy, -(-sw // fx), -(-sh // fy))
    # (a window given as rois= is decoded on its own; a view is read out of the whole decoded image)
    if c.fast == "x":
        pitch, origin = (W, sy * W + sx) if c.views else (sw, 0)
        return Record(sh, sw, pitch, origin, fy, fx, phy, phx, shape, (sx, sy, sw, sh))
    pitch, origin = (H, sx * H + sy) if c.views else (sh, 0)
    return Record(sw, sh, pitch, origin, fx, fy, phx, phy, shape, (sx, sy, sw, sh))


def memory(c: Case, s: Slot) -> np.ndarray:
    """the decoded pixels the record of slot s reads, as they lie in the buffer: (rows, pitch, CS) bytes"""
    a = pixels(s.file, c.fast)
    if not c.views:
        x, y, w, h = record(c, s).stored
        a = a[y:y + h, x:x + w]
    if c.fast == "y":
        a = a.swapaxes(0, 1)
    return np.ascontiguousarray(a).reshape(a.shape[0], a.shape[1], -1)


def stored_window(c: Case, s: Slot) -> np.ndarray:
    """the stored window of slot s, row-major, in the components the launch writes: what tools/reduce_model.reduce takes"""
    from tools import mode_model
    x, y, w, h = record(c, s).stored
    return np.ascontiguousarray(mode_model.convert(pixels(s.file, c.fast)[y:y + h, x:x + w], "L" if c.luma else None))


def reduced(c: Case, s: Slot) -> np.ndarray:
    """tools/reduce_model.reduce of the slot's stored window, as the launch writes it: (reduced rows, reduced len, CO)"""
    from tools import reduce_model
    fx, fy, phx, phy = record(c, s).shape[:4]
    out = reduce_model.reduce(stored_window(c, s), fx, fy, phx, phy)
    if c.fast == "y":
        out = out.swapaxes(0, 1)
    return np.ascontiguousarray(out).reshape(out.shape[0], out.shape[1], -1)


def expected(c: Case, s: Slot, filter: str = "bilinear") -> np.ndarray:
    """the output of slot s, row-major: exif_transpose(img.convert(mode)).crop(window).resize(size, filter, reducing_gap=gap) by
    the models, on the oracle's pixels"""
    from tools import reduce_model, views_model
    rec = record(c, s)
    assert not reduce_model.tall(rec.shape[4] if s.orientation < 5 else rec.shape[5], rec.shape[5] if s.orientation < 5 else rec.shape[4], c.size[1]), (c.name, s)
    out = views_model.expected(pixels(s.file, c.fast), s.window, c.size, filter, s.orientation, c.mode, c.gap)
    out.setflags(write=False)
    return out


def finish(c: Case, s: Slot, red: np.ndarray, filter: str = "bilinear") -> np.ndarray:
    """the output of slot s from `red`, the reduced image as the launch writes it: the second step of tools/reduce_model.resize
    (which does not offer it alone) on the oriented reduced image — what carries a wrong byte of the launch to the output"""
    from tools import orient_model, reduce_model, resize_model
    W, H = dims(s.file, c.fast)
    w, h = s.window[2:] if s.window is not None else orient_model.oriented_size(s.orientation, W, H)
    fx, fy = reduce_model.reduce_factors(w, h, c.size[0], c.size[1], c.gap)
    img = red.swapaxes(0, 1) if c.fast == "y" else red
    img = orient_model.orient(img[:, :, 0] if img.shape[2] == 1 else img, s.orientation)
    if (fx, fy) == (1, 1):
        return resize_model.resize(img, c.size, filter)
    bx, by = (0.0, w / fx), (0.0, h / fy)
    if img.shape[1] != c.size[0] or float(np.float32(bx[1])) != c.size[0]:
        img = resize_model.resample_axis(img, c.size[0], 1, table=reduce_model.axis_table(img.shape[1], c.size[0], filter, bx))
    if img.shape[0] != c.size[1] or float(np.float32(by[1])) != c.size[1]:
        img = resize_model.resample_axis(img, c.size[1], 0, table=reduce_model.axis_table(img.shape[0], c.size[1], filter, by))
    return np.ascontiguousarray(img)


# ---- the launch and what every tile of it does ---------------------------------------------------------------------------------------
def launch(records, co: int, cs: int) -> dict:
    """how reduce_stage cuts the launch of a plan with these records: mj_debug_reduce_launch's numbers"""
    max_slow, max_fast = max(r.orows for r in records), max(r.olen for r in records)
    cap = OUT_ROW // co
    tiles_fast = -(-max_fast // cap)
    return {"tile_slow": TILE_SLOW, "tile_fast": -(-max_fast // tiles_fast), "tiles_slow": -(-max_slow // TILE_SLOW), "tiles_fast": tiles_fast,
            "piece": STAGE // cs}


def fast_cells(rec: Record, off=None):
    from tools import reduce_model
    if off is None:
        return reduce_model.cells(rec.len, rec.f_fast, rec.phase_fast)
    return [(max(0, p * rec.f_fast - off), min(rec.len, (p + 1) * rec.f_fast - off)) for p in range(rec.olen)]


def tiles(rec: Record, cut: dict, cells=None):
    """every tile of one output along the contiguous axis: (index, None) where the workgroup returns early, else (index, (p0, p1,
    xs, xe, [piece starts])) — its cells p0..p1 - 1, the source pixels xs..xe - 1 they cover, and where each staged piece begins"""
    cells = cells if cells is not None else fast_cells(rec)
    for tf in range(cut["tiles_fast"]):
        p0 = tf * cut["tile_fast"]
        if p0 >= rec.olen:
            yield tf, None
            continue
        p1 = min(p0 + cut["tile_fast"], rec.olen)
        xs, xe = cells[p0][0], cells[p1 - 1][1]
        yield tf, (p0, p1, xs, xe, list(range(xs, xe, cut["piece"])))


def census(c: Case) -> dict:
    """{"launch": the cut, "slots": [per output: record, and per tile along the contiguous axis its pieces, the cells that
    straddle a piece boundary, ne — the reduced bytes of its rows —, whether it returns early; the kinds of cell (mul[0..3]: bit 0
    partial along the contiguous axis, bit 1 along the rows) and how many tiles along the rows return early]}"""
    from tools import reduce_model
    recs = [record(c, s) for s in c.slots]
    cut = launch(recs, c.co, c.cs)
    slots = []
    for rec in recs:
        cells = fast_cells(rec)
        per_tile = []
        for tf, t in tiles(rec, cut, cells):
            if t is None:
                per_tile.append({"early": True, "pieces": 0, "straddle": [], "ne": 0, "x0": None})
                continue
            p0, p1, xs, xe, starts = t
            straddle = [p for p in range(p0, p1) for b in starts[1:] if cells[p][0] < b < cells[p][1]]
            per_tile.append({"early": False, "pieces": len(starts), "straddle": straddle, "ne": (p1 - p0) * c.co, "x0": xs})
        kinds = sorted({(2 if b - a != rec.f_slow else 0) | (1 if d - e != rec.f_fast else 0)
                        for a, b in reduce_model.cells(rec.rows, rec.f_slow, rec.phase_slow) for e, d in cells})
        slow_early = sum(1 for ts in range(cut["tiles_slow"]) if ts * TILE_SLOW >= rec.orows)
        slots.append({"record": rec, "tiles": per_tile, "kinds": kinds, "slow_early": slow_early})
    return {"launch": cut, "slots": slots}


# ---- the kernel's loop, restated so that each step can be got wrong ------------------------------------------------------------------
VARIANTS = ("drop_second_part", "boundary_twice", "mis_of_first_piece", "mis_of_first_row", "no_off_on_later_tiles", "full_multiplier_first_cell",
            "pitch_is_len", "luma_after")


def kernel(mem: np.ndarray, rec: Record, cut: dict, luma: bool, wrong: Optional[str] = None) -> np.ndarray:
    """What k_reduce<CS, LUMA> writes for one record, tile by tile and piece by piece as the kernel goes — (reduced rows, reduced
    len, CO) — from the bytes `mem` (rows, pitch, CS) of the buffer it reads; `wrong` gets one step wrong:
      drop_second_part            a cell that straddles a piece boundary loses its part in the later piece
      boundary_twice              the piece ends one pixel late: the pixel behind the boundary is summed in both pieces
      mis_of_first_piece          the staging row's misalignment is taken from the row's first piece for every piece
      mis_of_first_row            ... from the first source row of a reduced row for all its rows
      no_off_on_later_tiles       tiles behind the first take their cells without the phase's offset
      full_multiplier_first_cell  the partial first cell of a phased contiguous axis is divided as a full one
      pitch_is_len                rows are taken to lie `len` pixels apart, not `pitch`
      luma_after                  the components are reduced, then converted to L
    The buffer is taken to start at a multiple of 16 bytes."""
    from tools import mode_model, reduce_model
    if wrong == "luma_after":
        return mode_model.luma(*np.moveaxis(kernel(mem, rec, cut, False), -1, 0))[:, :, None]
    cs = mem.shape[2]
    co = 1 if luma else cs
    flat = mem.reshape(-1)
    pitch = rec.len if wrong == "pitch_is_len" else rec.pitch
    slow = reduce_model.cells(rec.rows, rec.f_slow, rec.phase_slow)
    starts = np.array([a for a, _ in slow])
    y = np.arange(rec.rows)
    first_y = np.repeat(starts, [b - a for a, b in slow])          # the first source row of every row's reduced row
    acc = np.zeros((rec.orows, rec.olen, co), dtype=np.int64)
    part = np.zeros(rec.olen, dtype=bool)

    def mis(yy, px):
        return ((rec.origin + yy * pitch + px) * cs) % 16

    for tf, t in tiles(rec, cut):
        if t is None:
            continue
        p0, p1 = t[:2]
        cells = fast_cells(rec, 0 if (wrong == "no_off_on_later_tiles" and tf >= 1) else rec.off_fast)
        xs, xe = cells[p0][0], cells[p1 - 1][1]
        for k, px in enumerate(range(xs, xe, cut["piece"])):
            pe = min(px + cut["piece"], xe)
            shift = 0
            if wrong == "mis_of_first_piece":
                shift = mis(y, xs) - mis(y, px)
            elif wrong == "mis_of_first_row":
                shift = mis(first_y, px) - mis(y, px)
            for p in range(p0, p1):
                c0, c1 = cells[p]
                q0, q1 = max(c0, px), min(c1, pe)
                if wrong == "drop_second_part" and k > 0 and c0 < px:
                    continue
                if wrong == "boundary_twice" and pe < xe:
                    q1 = min(c1, pe + 1)
                if q1 <= q0:
                    continue
                at = ((rec.origin + y[:, None] * pitch + np.arange(q0, q1)[None, :]) * cs + np.reshape(shift, (-1, 1)))[:, :, None] + np.arange(cs)
                v = flat[np.clip(at, 0, flat.size - 1)].astype(np.int64)                  # (rows, pixels, CS)
                v = mode_model.luma(v[..., 0], v[..., 1], v[..., 2]).astype(np.int64)[..., None] if luma else v
                acc[:, p] += np.add.reduceat(v.sum(axis=1), starts, axis=0)
        for p in range(p0, p1):
            part[p] = cells[p][1] - cells[p][0] != rec.f_fast
            if wrong == "full_multiplier_first_cell" and p == 0 and rec.off_fast:
                part[p] = False
    ps, pf = rec.rows % rec.f_slow or rec.f_slow, rec.len % rec.f_fast or rec.f_fast
    n = np.outer([ps if b - a != rec.f_slow else rec.f_slow for a, b in slow], np.where(part, pf, rec.f_fast)).astype(np.int64)
    mul = np.vectorize(reduce_model.multiplier, otypes=[np.int64])(n)
    return ((((acc + (n // 2)[:, :, None]) * mul[:, :, None]) & 0xFFFFFFFF) >> 24).astype(np.uint8)


# ---- the table ----------------------------------------------------------------------------------------------------------------------
P1_VIEWS = (None, (7, 2, 1480, 20), (701, 1, 800, 21))


def window_in(win, fast: str, W: int, H: int, orientation: int = 1):
    """a window (x, y, w, h) given in the wide file's upright axes, in the oriented axes of the case's file"""
    from tools import orient_model
    if win is None:
        return None
    x, y, w, h = win
    if fast == "y":
        x, y, w, h = y, x, h, w
    # the oriented window that shows this stored window: orient_model.stored_window, inverted (asserted below)
    wo, ho = orient_model.oriented_size(orientation, W, H)
    b = orient_model.bits(orientation)
    if b & 4:
        x, y, w, h = y, x, h, w
    if b & 1:
        x = wo - x - w
    if b & 2:
        y = ho - y - h
    assert orient_model.stored_window(orientation, W, H, (x, y, w, h)) == ((win[1], win[0], win[3], win[2]) if fast == "y" else tuple(win))
    return (x, y, w, h)


def table(fast: str):
    """the cases of one reading, by id (the issue's table; B's small file is 100 x 64 — see B below)"""
    rev, rev_t = reversing(fast), reversing(fast, transposing=True)
    t = {}
    t["P1"] = Case("P1", fast, (Slot("P1"),), turned((50, 6), fast), 1.0)
    t["P2"] = Case("P2", fast, (Slot("P1"),), turned((250, 6), fast), 2.0, mode="L")
    t["P3"] = Case("P3", fast, (Slot("P3"),), turned((255, 3), fast), 2.0)
    for o in rev:
        t[f"T_o{o}"] = Case(f"T_o{o}", fast, (Slot("T", None, o),), turned((116, 5), fast), 2.0)
    t[f"PT_o{rev[0]}"] = Case(f"PT_o{rev[0]}", fast, (Slot("P1", None, rev[0]),), turned((50, 6), fast), 1.0)
    # (a transposing orientation that reverses both stored axes: the plan reads the buffer as the other layout's plans do)
    ot = [o for o in rev_t if o in reversing("y" if fast == "x" else "x", transposing=True)][0]
    t[f"PT_o{ot}"] = Case(f"PT_o{ot}", fast, (Slot("P1", None, ot),), turned((50, 6), fast, ot), 1.0)
    t["G"] = Case("G", fast, (Slot("G"),), turned((257, 4), fast), 2.0)
    # B: the issue names a 128 x 64 file, whose reduced row (factor 1: 128 pixels) is longer than the tile of 117 — its second
    # tile would not return early.  100 x 64 (reduced row: 100 pixels) does.
    t["B"] = Case("B", fast, (Slot("T"), Slot("S")), turned((116, 5), fast), 2.0)
    t[f"B_o{rev[1]}{rev[0]}"] = Case(f"B_o{rev[1]}{rev[0]}", fast, (Slot("T", None, rev[1]), Slot("S", None, rev[0])), turned((116, 5), fast), 2.0)
    W, H = dims("P1", fast)
    for o in (1, rev[0]):
        t[f"V_o{o}"] = Case(f"V_o{o}", fast, tuple(Slot("P1", window_in(w, fast, W, H, o), o) for w in P1_VIEWS), turned((50, 6), fast), 1.0, views=True)
    t["C"] = Case("C", fast, (Slot(BIG),), (2, 2), 1.0)
    t["C_white"] = Case("C_white", fast, (Slot("WHITE"),), (2, 2), 1.0)
    return t


# ---- the sweep: one 1501 x 157 file, twelve windows per call, one call per orientation ---------------------------------------------
SWEEP_TARGETS = ((100, 5), (50, 6), (37, 9), (80, 4), (110, 7))         # along the file's long axis, along its short one
SWEEP_GAPS = (1.0, 1.5, 2.0, 3.0)
SWEEP_SEED = {"x": 25, "y": 25}           # (chosen by the census: tests/test_reduce_paths_host.py holds what the draw reaches)


def sweep(fast: str):
    """[Case] — one per orientation 1..8, twelve windows of the oriented image as rois=.  Per call a target and a gap are drawn;
    windows 0..3 are longer than 1360 pixels along the file's long axis, windows 4 and 5 just under twice target x gap long
    there (a factor of 1 and the longest reduced rows of the plan: where that exceeds a tile, several tiles), the rest anything.  A
    window that is tall in the model's sense or whose factors are both 1 is drawn again."""
    from tools import orient_model, reduce_model
    rng = np.random.default_rng(SWEEP_SEED[fast])
    W, H = dims("SW", fast)
    long_, short = max(W, H), min(W, H)
    cases = []
    for o in range(1, 9):
        target, gap = SWEEP_TARGETS[int(rng.integers(len(SWEEP_TARGETS)))], SWEEP_GAPS[int(rng.integers(len(SWEEP_GAPS)))]
        size = turned(target, fast, o)
        near = min(long_, int(2 * target[0] * gap) - 1)
        slots = []
        while len(slots) < 12:
            k = len(slots)
            ll = int(rng.integers(1361, long_ + 1)) if k < 4 else near - int(rng.integers(0, 3)) if k < 6 else int(rng.integers(1, long_ + 1))
            ss = int(rng.integers(1, short + 1))
            l0, s0 = int(rng.integers(0, long_ - ll + 1)), int(rng.integers(0, short - ss + 1))
            win = window_in((l0, s0, ll, ss), fast, W, H, o)
            fx, fy = reduce_model.reduce_factors(win[2], win[3], size[0], size[1], gap)
            if (fx, fy) == (1, 1) or reduce_model.tall(-(-win[2] // fx), -(-win[3] // fy), size[1]):
                continue
            slots.append(Slot("SW", win, o))
        cases.append(Case(f"sweep_o{o}", fast, tuple(slots), size, gap))
    return cases


def together(n: dict) -> dict:
    """of one plan's census: does it hold all four kinds of cell, a tile staged in pieces, several tiles, an early return"""
    tiles_ = [t for s in n["slots"] for t in s["tiles"]]
    kinds = {k for s in n["slots"] for k in s["kinds"]}
    return {"kinds": kinds == {0, 1, 2, 3}, "pieces": any(t["pieces"] >= 2 for t in tiles_), "straddle": any(t["straddle"] for t in tiles_),
            "tiles": n["launch"]["tiles_fast"] >= 2, "early": any(t["early"] for t in tiles_),
            "phased_later_tile": any(s["record"].phase_fast and len([t for t in s["tiles"] if not t["early"]]) >= 2 for s in n["slots"])}
