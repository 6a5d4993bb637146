"""The cases of tests/test_reduce_paths.py, held on the CPU to what they are meant to reach (no GPU): by tests/reduce_cases.census
every case takes k_reduce (csrc/reduce.hip) down the path its row of the table names — a row segment staged in two pieces with a
cell across the boundary, two tiles along the contiguous axis under a phase, a tile row of 500 or more bytes that is no multiple
of 8, a workgroup that returns early, a cell of 65536 pixels — and its image tells the kernel apart from each wrong variant of
the kernel's loop that applies to it (reduce_cases.kernel, a restatement of the loop with one step wrong; the right one is first
held to tools/reduce_model.reduce) — in the reduced image and, through the second step, in the output the GPU test compares.  A GPU
run that passes then means something.

The variants and where they apply (derived from the census, then held against the ids the table names):
  drop_second_part, boundary_twice   every output with a cell across a piece boundary: P1, P2, P3, PT, V
  mis_of_first_row                   every output whose cells hold rows that start at different alignments (all but P2's, whose cells
                                     are one row high, and C's, whose rows are 1536 bytes apart)
  no_off_on_later_tiles              a phase along the contiguous axis and two tiles: T, B under orientations
  full_multiplier_first_cell         a phase along the contiguous axis: T, PT, B and V under orientations
  pitch_is_len                       views narrower than the image: V
  luma_after                         P2
  mis_of_first_piece                 NOT a wrong variant of this kernel: a piece is 4080 bytes — 255 x 16 — in both instances, so every
                                     piece of a row starts at the alignment of its first; the restatement with that "mistake" is the
                                     kernel on every input, which is asserted, together with the reason.  What can go wrong with the
                                     alignment is taking it from another ROW: mis_of_first_row.
python tests/test_reduce_paths_host.py rewrites profiles/reduce_paths_census.txt."""
import ctypes

import numpy as np
import pytest

import reduce_cases as RC

FASTS = ("x", "y")


def differs(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape != b.shape or not np.array_equal(a, b)


def ids(fast: str, prefix: str):
    return [k for k in RC.table(fast) if k == prefix or k.startswith(prefix + "_")]


def applicable(c: RC.Case, k: int, n: dict) -> set:
    """the wrong variants that change what the kernel does for output k of case c, from the census n"""
    s = n["slots"][k]
    rec, live = s["record"], [t for t in s["tiles"] if not t["early"]]
    out = set()
    if any(t["straddle"] for t in live):
        out |= {"drop_second_part", "boundary_twice"}
    if (rec.pitch * c.cs) % 16 and rec.f_slow > 1:
        out.add("mis_of_first_row")
    if rec.phase_fast:
        out.add("full_multiplier_first_cell")
        if len(live) >= 2:
            out.add("no_off_on_later_tiles")
    if rec.pitch != rec.len:
        out.add("pitch_is_len")
    if c.luma:
        out.add("luma_after")
    return out


# ---- 1. every case reaches its path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", FASTS)
def test_every_case_reaches_the_path_its_row_names(fast):
    t = RC.table(fast)
    n = {k: RC.census(c) for k, c in t.items()}
    up = (lambda v: v) if fast == "x" else (lambda v: (v[1], v[0], v[3], v[2], v[5], v[4]))      # the table's numbers are the wide file's

    def only(k):
        (s,) = n[k]["slots"]
        return s, s["record"], s["tiles"]

    # P1: 30 x 3 to 51 x 8; two pieces of the 1501-pixel segment, cell 45 across pixel 1360; a partial last cell on both axes
    s, rec, tiles = only("P1")
    assert up(rec.shape) == (30, 3, 0, 0, 51, 8) and n["P1"]["launch"]["piece"] == 1360
    assert [(x["pieces"], x["straddle"]) for x in tiles] == [(2, [45])] and s["kinds"] == [0, 1, 2, 3]
    assert rec.len % rec.f_fast and rec.rows % rec.f_slow
    # P2: LUMA, 3 x 1 to 501 x 23; pieces; a 501-byte tile row — all 8 elements of a lane, 62 full 8-byte stores and a 5-byte tail
    s, rec, tiles = only("P2")
    assert t["P2"].luma and t["P2"].co == 1 and up(rec.shape) == (3, 1, 0, 0, 501, 23) and rec.f_slow == 1
    assert [(x["pieces"], x["straddle"], x["ne"]) for x in tiles] == [(2, [453], 501)]
    assert tiles[0]["ne"] >= 500 and tiles[0]["ne"] % RC.LANE_BYTES == 5 and tiles[0]["ne"] > 64 * (RC.LANE_BYTES - 1)
    assert n["P2"]["launch"]["tiles_slow"] == 3
    # P3: the grey instance's piece of 4080 pixels; 9 x 2 to 510 x 6; cell 453 across pixel 4080
    s, rec, tiles = only("P3")
    assert t["P3"].cs == 1 and n["P3"]["launch"]["piece"] == 4080 and up(rec.shape) == (9, 2, 0, 0, 510, 6)
    assert [(x["pieces"], x["straddle"], x["ne"]) for x in tiles] == [(2, [453], 510)] and tiles[0]["ne"] % RC.LANE_BYTES == 6
    # T: two tiles of 117 under phase 700 mod 3 = 1 — both orientations that reverse the long axis; the second tile starts at 349
    assert len(ids(fast, "T")) == 2
    for k in ids(fast, "T"):
        s, rec, tiles = only(k)
        assert up(rec.shape) == (3, 2, 1, 0, 234, 10) and rec.phase_fast == 1 and rec.off_fast == 2
        assert n[k]["launch"]["tiles_fast"] == 2 and n[k]["launch"]["tile_fast"] == 117
        assert [(x["early"], x["pieces"], x["x0"]) for x in tiles] == [(False, 1, 0), (False, 1, 349)]
    # PT: pieces and phase 1501 mod 30 = 1 together: the boundary 1360 lies in another cell than on the unphased grid; once under
    # a transposing orientation, whose plan reads the buffer as the other layout's plans do — with a phase on the rows as well
    assert len(ids(fast, "PT")) == 2 and sorted(t[k].slots[0].orientation >= 5 for k in ids(fast, "PT")) == [False, True]
    for k in ids(fast, "PT"):
        s, rec, tiles = only(k)
        assert (rec.f_fast, rec.f_slow, rec.phase_fast) == (30, 3, 1) and [(x["pieces"], x["straddle"]) for x in tiles] == [(2, [46])]
        assert (1360 - 1) % 30 and s["kinds"] == [0, 1, 2, 3]
        assert rec.phase_slow == (2 if t[k].slots[0].orientation >= 5 or fast == "y" else 0)
    # G: grey, 2 x 2 to 515 x 8: two tiles, 258 and 257
    s, rec, tiles = only("G")
    assert t["G"].cs == 1 and up(rec.shape) == (2, 2, 0, 0, 515, 8) and [x["ne"] for x in tiles] == [258, 257]
    # B: the small image's second tile returns early; the factors differ; upright and with the long axes reversed (a phase on T's file)
    assert len(ids(fast, "B")) == 2
    for k in ids(fast, "B"):
        big, small = n[k]["slots"]
        assert n[k]["launch"]["tiles_fast"] == 2 and [x["early"] for x in big["tiles"]] == [False, False] and [x["early"] for x in small["tiles"]] == [False, True]
        assert up(big["record"].shape)[:2] == (3, 2) and up(small["record"].shape)[:2] == (1, 6)
        assert big["record"].phase_fast == (0 if k == "B" else 1)
    # V: the whole file and two windows of it; a pitch that is not the window's length, pieces in two of the three, window origins
    # at odd byte offsets; upright and with the long axis reversed
    assert len(ids(fast, "V")) == 2
    for k in ids(fast, "V"):
        whole, wide, half = (s["record"] for s in n[k]["slots"])
        assert t[k].views and (whole.pitch, wide.pitch, half.pitch) == (1501, 1501, 1501) and (whole.len, wide.len, half.len) == (1501, 1480, 800)
        assert (wide.origin * 3) % 2 == 1 and (half.origin * 3) % 16 not in (0, (wide.origin * 3) % 16)
        assert [s["tiles"][0]["pieces"] for s in n[k]["slots"]] == [2, 2, 1] and all(s["tiles"][0]["straddle"] for s in n[k]["slots"][:2])
        assert (up(whole.shape)[:2], up(wide.shape)[:2], up(half.shape)[:2]) == ((30, 3), (29, 3), (16, 3))
        assert whole.phase_fast == wide.phase_fast == (0 if k == "V_o1" else 1)
    # C: a cell of 65536 pixels, the largest taken; the next size is refused
    from tools import reduce_model
    for k in ("C", "C_white"):
        s, rec, tiles = only(k)
        assert rec.shape == (256, 256, 0, 0, 2, 2) and rec.f_fast * rec.f_slow == RC.MAX_CELL == reduce_model.MAX_CELL
    fx, fy = reduce_model.reduce_factors(512, 512, 1, 2, 1.0)
    assert fx * fy == 2 * RC.MAX_CELL
    white = RC.pixels("WHITE", fast)
    assert white.min() == 255              # the largest sum: 65536 x 255, and with n / 2 added still below 2^24
    assert 65536 * 255 + 32768 < 1 << 24 and (65536 * 255 + 32768) * reduce_model.multiplier(65536) < 1 << 32
    # none is tall in the model's sense (reduce_cases.expected asserts it again where the GPU test asks for the expectation)
    for k, c in t.items():
        for s in n[k]["slots"]:
            sh = s["record"].shape
            w, h = (sh[5], sh[4]) if c.slots[0].orientation >= 5 else (sh[4], sh[5])
            assert not reduce_model.tall(w, h, c.size[1]), k


def test_the_census_constants_are_the_headers():
    """reduce_cases restates kReduceStage - 16, the 64 x 8 bytes of a tile row and tile_slow; the library's values are asserted on
    the GPU through mj_debug_reduce_launch, plan by plan — here the hook exists and refuses where there is no plan"""
    import re
    from conftest import ROOT
    text = (ROOT / "pyjpegdecoder_amd" / "csrc" / "mijpeg_internal.h").read_text()
    assert int(re.search(r"constexpr int kReduceStage = (\d+);", text).group(1)) - 16 == RC.STAGE
    assert int(re.search(r"constexpr int kReduceMaxCell = (\d+);", text).group(1)) == RC.MAX_CELL
    kernel = (ROOT / "pyjpegdecoder_amd" / "csrc" / "reduce.hip").read_text()
    assert int(re.search(r"constexpr int kReduceLaneElems = (\d+);", kernel).group(1)) == RC.LANE_BYTES and RC.OUT_ROW == 64 * RC.LANE_BYTES
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    lib = B.load_library()
    out = (ctypes.c_int32 * 5)()
    assert "mj_debug_reduce_launch" in B.EXPORTS and lib.mj_debug_reduce_launch(None, out) == B.MJ_ERR_INVALID
    assert "mj_debug_reduce_launch(" in (ROOT / "include" / "mijpeg.h").read_text()


# ---- 2. every case tells the wrong variants apart ------------------------------------------------------------------------------------
HELD = {"P1": {"drop_second_part", "boundary_twice", "mis_of_first_row"}, "P2": {"drop_second_part", "boundary_twice", "luma_after"},
        "P3": {"drop_second_part", "boundary_twice", "mis_of_first_row"}, "T": {"no_off_on_later_tiles", "full_multiplier_first_cell", "mis_of_first_row"},
        "PT": {"drop_second_part", "boundary_twice", "mis_of_first_row", "full_multiplier_first_cell"}, "G": {"mis_of_first_row"},
        "B": {"mis_of_first_row"},
        "V": {"drop_second_part", "boundary_twice", "mis_of_first_row", "pitch_is_len"}, "C": set()}


@pytest.mark.parametrize("fast", FASTS)
def test_every_case_tells_the_wrong_variants_apart(fast):
    t = RC.table(fast)
    held = {}
    for name, c in t.items():
        n = RC.census(c)
        for k, s in enumerate(c.slots):
            rec, mem, want = n["slots"][k]["record"], RC.memory(c, s), RC.reduced(c, s)
            right = RC.kernel(mem, rec, n["launch"], c.luma)
            assert not differs(right, want), (name, k, "the restatement itself is not the model")
            out = RC.expected(c, s)
            assert not differs(RC.finish(c, s, right), out), (name, k, "the second step on the stored-order reduced image is not the model's")
            # (a piece is a whole number of 16-byte lines: the alignment of a row's first piece IS that of every piece)
            assert (n["launch"]["piece"] * c.cs) % 16 == 0
            assert not differs(RC.kernel(mem, rec, n["launch"], c.luma, "mis_of_first_piece"), want), (name, k)
            for v in sorted(applicable(c, k, n)):
                wrong = RC.kernel(mem, rec, n["launch"], c.luma, v)
                assert differs(wrong, want), (name, k, v, "the image or the shape is too kind")
                # ... and the second step carries it to the bytes the GPU test compares
                assert differs(RC.finish(c, s, wrong), out), (name, k, v, "the wrong reduced bytes do not reach the output")
                held.setdefault(name, set()).add(v)
    for name in t:
        row = name.split("_")[0]
        assert held.get(name, set()) >= HELD[row], (name, held.get(name))
    # ... and what only the forms under an orientation hold
    for name in ids(fast, "B")[1:] + ids(fast, "V")[1:]:
        assert held[name] >= {"full_multiplier_first_cell"} | ({"no_off_on_later_tiles"} if name.startswith("B") else set()), (name, held[name])


# ---- 3. the library's host twin on the cases' own images ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", FASTS)
def test_the_host_twin_is_the_model_on_the_long_rows_and_the_largest_cell(fast):
    """mj_host_reduce on P1, P3, T and C — their phased forms and the white image included: tests/test_reduce_host.py holds it on
    images of at most 600 pixels a side"""
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    from tools import reduce_model
    if not B.LIB_PATH.exists():
        g.build()
    t = RC.table(fast)
    seen = 0
    for name in ["P1", "P3", "C", "C_white"] + ids(fast, "T") + ids(fast, "PT"):
        c = t[name]
        (s,) = c.slots
        a = RC.stored_window(c, s)
        fx, fy, phx, phy = RC.record(c, s).shape[:4]
        got = B.reduce(a, fx, fy, phx, phy)
        assert np.array_equal(got, reduce_model.reduce(a, fx, fy, phx, phy)), name
        seen += bool(phx or phy)
    assert seen == 4
    a = RC.pixels(RC.BIG, fast)
    with pytest.raises(ValueError):
        B.reduce(a, 512, 256)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
def sweep_counts(fast: str) -> dict:
    """over the eight plans of tests/test_reduce_paths.py's sweep: in how many each path occurs, and in how many all occur together"""
    counts = {"plans": 0, "windows": 0, "long_windows": 0, "kinds": 0, "pieces": 0, "straddle": 0, "tiles": 0, "early": 0, "phased_later_tile": 0,
              "together": 0, "factors_min": 99, "factors_max": 0}
    for c in RC.sweep(fast):
        n = RC.census(c)
        got = RC.together(n)
        counts["plans"] += 1
        counts["windows"] += len(c.slots)
        long_here = sum(1 for s in n["slots"] if s["record"].len > 1360)
        assert long_here >= 4, c.name
        counts["long_windows"] += long_here
        for k in ("kinds", "pieces", "straddle", "tiles", "early", "phased_later_tile"):
            counts[k] += got[k]
        counts["together"] += all(got[k] for k in ("kinds", "pieces", "tiles", "early"))
        for s in n["slots"]:
            f = s["record"].shape[:2]
            assert f != (1, 1)
            counts["factors_min"], counts["factors_max"] = min(counts["factors_min"], *f), max(counts["factors_max"], *f)
    return counts


# what the seeded draw reaches, by the census — plans out of eight in which each path occurs, and in which all four kinds of cell,
# a tile staged in pieces, several tiles and an early return occur TOGETHER; asserted so that a change of the draw or of the
# launch's cutting shows
SWEEP = {"x": {"plans": 8, "windows": 96, "long_windows": 34, "kinds": 8, "pieces": 6, "straddle": 6, "tiles": 5, "early": 5, "phased_later_tile": 4,
               "together": 3, "factors_min": 1, "factors_max": 40},
         "y": {"plans": 8, "windows": 96, "long_windows": 34, "kinds": 8, "pieces": 6, "straddle": 6, "tiles": 4, "early": 4, "phased_later_tile": 2,
               "together": 2, "factors_min": 1, "factors_max": 40}}


@pytest.mark.parametrize("fast", FASTS)
def test_the_sweep_holds_the_paths_together_in_single_plans(fast):
    n = sweep_counts(fast)
    assert n == SWEEP[fast], n
    assert n["together"] >= 2 and n["phased_later_tile"] >= 2 and n["long_windows"] >= 4 * 8 and n["factors_max"] >= 35


# ---- the census in profiles/ -----------------------------------------------------------------------------------------------------------
def census_table():
    lines = ["case reading output fx fy phase_x phase_y reduced_w reduced_h tile_fast tiles_fast tiles_slow piece | per tile along the contiguous axis: "
             "pieces/straddling cells/ne (early: the workgroup returns) | kinds of cell"]
    for fast in FASTS:
        for name, c in RC.table(fast).items():
            n = RC.census(c)
            cut = n["launch"]
            for k, s in enumerate(n["slots"]):
                tiles = " ".join("early" if x["early"] else f"{x['pieces']}/{','.join(map(str, x['straddle'])) or '-'}/{x['ne']}" for x in s["tiles"])
                lines.append(f"{name} {fast} {k} " + " ".join(map(str, s["record"].shape)) + f" {cut['tile_fast']} {cut['tiles_fast']} {cut['tiles_slow']} {cut['piece']}"
                             f" | {tiles} | {','.join(map(str, s['kinds']))}")
    for fast in FASTS:
        n = sweep_counts(fast)
        lines.append(f"sweep {fast}: " + " ".join(f"{k}={v}" for k, v in n.items()))
    return lines


def test_the_census_table_in_profiles_is_current():
    """profiles/reduce_paths_census.txt holds what the committed cases reach"""
    from conftest import ROOT
    assert (ROOT / "profiles" / "reduce_paths_census.txt").read_text().splitlines() == census_table()


if __name__ == "__main__":
    from conftest import ROOT
    (ROOT / "profiles" / "reduce_paths_census.txt").write_text("\n".join(census_table()) + "\n")
