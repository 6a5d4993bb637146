"""The lane walk's resolved AC tables (csrc/plan_tables.hip: build_resolved_tables, read by csrc/lanes13_walk.h in the stage-1 kernel
and in a fused launch's producers), checked on the host through mj_debug_resolved_tables: for every 16-bit code window (and random
value bits behind it) the table walk the kernel makes — main level, second-level table, finished and open entry fields — must give
the symbol, the advance, the bits consumed and the EXTENDed value the canonical code book gives (jpeg_decoder.py:366-377, :834-866,
bin_twos_complement :1636-1646).  At 10, 11, 12 and 13 index bits, in the stage-1 kernel's fixed stride and packed back to back as a
fused launch holds them.  Also here: stage<true>()'s cut of the 11-bit DC tables to the fused launch's 8 bits, restated."""
import numpy as np
import pytest

from pyjpegdecoder_amd import _binding as B
from tools import craft_jpeg as C

import base_cases as bc

STD = {k: (C._T[f"STD_{k}_BITS"], C._T[f"STD_{k}_VALS"]) for k in ("DC_LUMA", "DC_CHROMA", "AC_LUMA", "AC_CHROMA")}
SLOT_BYTES = 8192 * 4 + 144 * 32                        # kLanes13SlotBytes: the stage-1 kernel's stride
EOB = 64


def incomplete_table():
    """Codes of 2..16 bits that leave half of the code space unused: main-level entries without a code at every width, and a
    second-level table with a hole behind the last 16-bit code."""
    L = {0x01: 2, 0x02: 3, 0x00: 4, 0x11: 6, 0x03: 9, 0x21: 11, 0x04: 12, 0x12: 13, 0x31: 14, 0x05: 15, 0x41: 16, 0x13: 16, 0xF0: 16}
    return C.huffman_table(L)


def oversubscribed_table():
    """More codes of 3 bits than there are patterns left: the code counter runs past 2^l, and every code from there on has no
    pattern of its length (plan_tables.hip skips them, as the code book below does)."""
    bits = [0, 2, 6, 2, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    return bytes(bits), bytes([0x01, 0x02, 0x00, 0x03, 0x11, 0x04, 0x21, 0x12, 0x31, 0x05, 0x41, 0x13, 0x22, 0x06])


def most_prefixes_table():
    """256 codes of 14 bits: 128 prefixes at 13 bits (and 16 at 10), the most a table of 256 symbols can have behind any index."""
    return bytes([0] * 13 + [255, 0, 1]), bytes(range(256))


AC_TABLES = {"annexk_luma": STD["AC_LUMA"], "annexk_chroma": STD["AC_CHROMA"], "wide_0": C.wide_ac_table(0), "wide_3": C.wide_ac_table(3),
             "wide_5": C.wide_ac_table(5), "long_0": C.long_ac_table(0), "long_1": C.long_ac_table(1), "long_2": C.long_ac_table(2),
             "rare_luma": bc.rare_ac_table(0), "rare_chroma": bc.rare_ac_table(1), "incomplete": incomplete_table(),
             "oversubscribed": oversubscribed_table(), "most_prefixes": most_prefixes_table()}
GROUPS = [["annexk_luma", "annexk_chroma", "wide_0", "wide_3"], ["wide_5", "long_0", "long_1", "long_2"],
          ["rare_luma", "rare_chroma", "incomplete", "oversubscribed"], ["most_prefixes"]]


def book(bits, vals):
    """[(length, code, symbol)] of the canonical code, shortest first; codes past 2^length have no pattern."""
    out, code, k = [], 0, 0
    for l in range(1, 17):
        code <<= 1
        for _ in range(bits[l - 1]):
            if code < (1 << l) and k < len(vals):
                out.append((l, code, vals[k]))
            k += 1
            code += 1
    return out


def want_symbols(codes, w32):
    """(bits consumed, index advance | EOB | 0 = no such code, value) per window of w32 (uint64 array, 32 bits MSB first)."""
    ln = np.zeros(w32.size, dtype=np.int64)
    sym = np.zeros(w32.size, dtype=np.int64)
    for l, code, s in codes:                            # (the shortest code wins: the reference reads bit by bit)
        hit = (ln == 0) & ((w32 >> np.uint64(32 - l)) == code)
        ln[hit], sym[hit] = l, s
    size, run = sym & 15, sym >> 4
    eob = (ln > 0) & (sym == 0)
    raw = ((w32 << ln.astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.int64) >> (32 - size)
    raw[size == 0] = 0
    val = np.where((size > 0) & (raw >> np.maximum(size - 1, 0) == 0), raw - ((1 << size) - 1), raw)
    val[size == 0] = 0
    bits = np.where(eob, ln, ln + size)
    adv = np.where(ln == 0, 0, np.where(eob, EOB, run + 1))
    return np.where(ln == 0, 0, bits), adv, np.where((ln == 0) | eob, 0, val)


def table_symbols(words, off, ab, w32):
    """What lanes13_walk.h reads out of the table at byte offset `off` for the same windows: MJ_LOOK13 / MJ_CORE13 for a finished
    entry (bit 15 clear: value << 16 | 2 * advance << 8 | bits, advance 127 = end of block), L_open / L_arith for the rest (byte 1 =
    0x80 | 0x40 a second-level table at the byte offset in the high word | run + 1; byte 2 = code length, 0 = no such code; byte 3 =
    31 - size).  Also returns which windows took which path."""
    base = off // 4
    e = words[base + (w32 >> np.uint64(32 - ab)).astype(np.int64)].astype(np.int64)
    fin = (e & 0x8000) == 0
    second = ~fin & ((e & 0x4000) != 0)
    t5 = e.copy()
    sub = ((w32 >> np.uint64(16)) & np.uint64((1 << (16 - ab)) - 1)).astype(np.int64)
    assert ((e[second] >> 16) % 4 == 0).all() and ((e[second] >> 16) >= (1 << ab) * 4).all()
    t5[second] = words[base + (e[second] >> 16) // 4 + sub[second]].astype(np.int64)
    assert ((t5[~fin] & 0xC000) == 0x8000).all()                  # second-level tables hold open entries throughout
    ln = (t5 >> 16) & 0xFF
    run1 = (t5 >> 8) & 31
    size = 31 - ((t5 >> 24) & 0xFF)
    hw = (w32 << ln.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    raw = (hw.astype(np.int64) >> 1) >> (31 - size)
    val = raw - np.where(hw >> np.uint64(31) == 0, 0x7FFFFFFF >> (31 - size), 0)
    bits, adv = ln + size, np.where(run1 == 0, EOB, run1)
    nocode = ~fin & (ln == 0)
    bits[nocode], adv[nocode], val[nocode] = 0, 0, 0
    val[~fin & (run1 == 0)] = 0                                   # (end of block: the kernel leaves the lane's block there)
    adv2 = (e >> 8) & 0xFF
    assert (adv2[fin] % 2 == 0).all() or (adv2[fin][adv2[fin] % 2 == 1] == 127).all()
    f_val = ((e >> 16) & 0xFFFF).astype(np.uint16).astype(np.int16).astype(np.int64)
    bits = np.where(fin, e & 0xFF, bits)
    adv = np.where(fin, np.where(adv2 == 127, EOB, adv2 // 2), adv)
    val = np.where(fin, f_val, val)
    return (bits, adv, val), fin, second


@pytest.mark.parametrize("fixed", [True, False], ids=["stride", "packed"])
@pytest.mark.parametrize("ab", [10, 11, 12, 13])
def test_every_code_window_gives_the_book_symbol(ab, fixed):
    rng = np.random.default_rng(ab)
    for group in GROUPS:
        specs = [AC_TABLES[n] for n in group]
        got = B.resolved_tables(specs, [2] * len(specs), list(range(len(specs))), [ab] * 4, SLOT_BYTES if fixed else 0)
        assert got is not None, group
        words, offs = got
        if fixed:
            assert offs == [SLOT_BYTES * s for s in range(len(specs))] and words.size == len(specs) * SLOT_BYTES // 4
        else:
            assert all(o % 16 == 0 for o in offs) and offs[0] == 0 and words.size * 4 <= len(specs) * 65535
        w32 = (np.arange(1 << 16, dtype=np.uint64) << np.uint64(16)) | rng.integers(0, 1 << 16, 1 << 16).astype(np.uint64)
        for name, spec, off in zip(group, specs, offs):
            codes = book(*spec)
            want = want_symbols(codes, w32)
            got3, fin, second = table_symbols(words, off, ab, w32)
            for what, g, w in zip(("bits", "advance", "value"), got3, want):
                bad = np.nonzero(g != w)[0]
                assert bad.size == 0, (name, what, hex(int(w32[bad[0]])), int(g[bad[0]]), int(w[bad[0]]))
            # finished wherever code + value bits fit the index — and nowhere else; second level exactly behind longer codes
            for l, code, s in codes:
                first = code << (16 - l)
                total = l + (0 if s == 0 else s & 15)
                assert bool(fin[first]) == (total <= ab) and bool(second[first]) == (l > ab), (name, l, code, s)
            if not fixed:                                           # packed: as many second-level tables as prefixes, no more
                prefixes = {code >> (l - ab) for l, code, _ in codes if l > ab}
                size = ((1 << ab) + (1 + len(prefixes)) * (1 << (16 - ab))) * 4
                nxt = offs[offs.index(off) + 1] if offs.index(off) + 1 < len(offs) else words.size * 4
                assert nxt - off == (size + 15) // 16 * 16, name


def test_patterns_without_a_code_point_to_the_empty_table():
    """No such code at the main level: the pointer to second-level table 0, whose entries have code length 0; a hole inside a real
    second-level table: the same open entry.  The kernel's canonical search then says MJ_ST_BAD_CODE."""
    spec = incomplete_table()
    codes = book(*spec)
    for ab in (10, 11, 12, 13):
        for stride in (SLOT_BYTES, 0):
            words, (off,) = B.resolved_tables([spec], [2], [0], [ab] * 4, stride)
            main = words[:1 << ab]
            empty = ((1 << ab) * 4 << 16) | 0xC000
            used = np.zeros(1 << ab, dtype=bool)
            for l, code, _ in codes:
                if l <= ab:
                    used[code << (ab - l):(code + 1) << (ab - l)] = True
                else:
                    used[code >> (l - ab)] = True
            assert (main[~used] == empty).all() and (main[used] != empty).all() and (~used).sum() > (1 << ab) // 4
            assert (words[1 << ab:(1 << ab) + (1 << (16 - ab))] == 0x8000).all()
            last = max(code for l, code, _ in codes if l == 16)
            sub = int(main[last >> (16 - ab)]) >> 16
            assert int(main[last >> (16 - ab)]) & 0xC000 == 0xC000 and sub > (1 << ab) * 4
            assert words[sub // 4 + ((last + 1) & ((1 << (16 - ab)) - 1))] == 0x8000        # the hole behind the last code


def test_a_table_of_256_symbols_always_fits_and_a_short_stride_is_refused():
    """`build_resolved_tables` refuses a table with more second-level tables than its slot holds.  With 256 symbols at the most a
    table has 128 prefixes behind any index (256 codes one bit longer than it) — under the 143 the stage-1 kernel's stride holds at
    13 bits, and under what it holds at 10, 11 and 12: no batch is refused for that at the stride the library uses.  A shorter
    stride (the hook takes any) shows the refusal."""
    for ab in (10, 11, 12, 13):
        bits = [0] * 16
        bits[ab] = 255                                               # 255 codes of ab + 1 bits: 128 prefixes
        spec = (bytes(bits), bytes(range(255)))
        for stride in (SLOT_BYTES, 0):
            got = B.resolved_tables([spec], [2], [0], [ab] * 4, stride)
            assert got is not None
            assert len({int(w) >> 16 for w in got[0][:1 << ab] if int(w) & 0xC000 == 0xC000}) == 128 + 1      # (+ the empty table's pointer)
        short = ((1 << ab) + 100 * (1 << (16 - ab))) * 4
        assert B.resolved_tables([spec], [2], [0], [ab] * 4, short) is None
        assert B.resolved_tables([bc.rare_ac_table(0)], [2], [0], [ab] * 4, short) is not None
    with pytest.raises(ValueError):
        B.resolved_tables([STD["AC_LUMA"]], [2], [0], [9] * 4, 0)
    with pytest.raises(ValueError):
        B.resolved_tables([STD["AC_LUMA"]], [2], [0], [13] * 4, 4096)


def test_slots_and_widths_per_slot():
    """A fused launch's tables: component 0's at 13 bits, the others at 12, back to back; tables that are no AC table are left out."""
    specs = [STD["DC_LUMA"], STD["AC_LUMA"], STD["DC_CHROMA"], STD["AC_CHROMA"]]
    words, offs = B.resolved_tables(specs, [1, 2, 1, 2], [0, 0, 0, 1], [13, 12, 12, 12], 0)
    one, _ = B.resolved_tables([STD["AC_LUMA"]], [2], [0], [13] * 4, 0)
    two, _ = B.resolved_tables([STD["AC_CHROMA"]], [2], [0], [12] * 4, 0)
    assert offs == [0, one.size * 4] and np.array_equal(words, np.concatenate([one, two]))


# ---- the DC tables of a fused launch ------------------------------------------------------------------------------------------
def lut11_dc(bits, vals):
    """plan_create.hip's 11-bit DC table: (length << 8) | symbol for every index a code of at most 11 bits is a prefix of, else 0."""
    lut = np.zeros(1 << 11, dtype=np.uint16)
    for l, code, s in book(bits, vals):
        if l <= 11:
            lut[code << (11 - l):(code + 1) << (11 - l)] = (l << 8) | s
    return lut


def cut_to(lut11, dbits):
    """lanes13::stage<true>(): entry i of the shorter table is the 11-bit table's entry of the index padded with zeros, if its code
    fits the shorter index, else 0 ("longer": the canonical search from dbits + 1 bits on)."""
    e = lut11[np.arange(1 << dbits) << (11 - dbits)]
    return np.where((e >> 8) <= dbits, e, 0).astype(np.uint16)


@pytest.mark.parametrize("name", ["annexk_luma", "annexk_chroma", "long", "rare_luma", "rare_chroma"])
def test_dc_tables_cut_to_eight_bits(name):
    spec = {"annexk_luma": STD["DC_LUMA"], "annexk_chroma": STD["DC_CHROMA"], "long": C.long_dc_table(), "rare_luma": bc.rare_dc_table(0),
            "rare_chroma": bc.rare_dc_table(1)}[name]
    codes = book(*spec)
    cut = cut_to(lut11_dc(*spec), 8)
    for i in range(256):
        hit = [(l, s) for l, code, s in codes if l <= 8 and i >> (8 - l) == code]
        assert len(hit) <= 1
        assert cut[i] == ((hit[0][0] << 8) | hit[0][1] if hit else 0), (name, i)
    # every code of 9..11 bits — Annex K has them, for differences beyond +-255 (chroma) / +-1023 (luma) — is a zero entry here
    longer = [(l, code) for l, code, _ in codes if 9 <= l <= 11]
    assert longer and all(cut[code >> (l - 8)] == 0 for l, code in longer)
