"""The baseline stage 1's rare symbol paths: one small file per path (tools/craft_jpeg.craft_baseline_symbols), a plain model
of the entropy loop that decodes them, and the census that proves each file reaches the path it is named for.

The lane walks (lanes13_walk.h behind huffman_lanes13.hip and fused.hip, huffman_lanes.hip), the wave form (huffman.hip) and
the synchronisation form (huffman_sync.hip) decode the common symbol in a hand-scheduled round and leave it for a slow path
on everything else: an entry whose value bits do not fit the table's index, a code behind the index, a DC code behind the DC
table, a run past the block, coefficient 63, a pattern without a code.  The files the suite had reach these by the luck of an
encoder, one lane at a time; the rows below reach them on purpose, in files of ONE colour geometry (4:2:0, 64 x 32, one MCU row
per restart segment, all-ones quantisation tables) so that they decode side by side in the lanes of one wavefront and in one
fused launch.

The model (`walk`) restates baseline_dct_scan and its bit reader (jpeg_decoder.py:654-695, :805-866, :897-900) and counts only
what the STREAM determines (`new_census`).  "Finished", "open" and "second level" are a table's words (build_resolved_tables:
code + value bits within the index / the code within it / the code behind it) and are counted for every index width 8..13; the
round position of a symbol is the parity of the resolved symbols in front of it since the block began or the last unresolved
one was handled, as MJ_PAIR13 pairs them at 13 bits.  Where a lane's stream window or bit buffer stands is not modelled.

`walk` takes one WRONG variant at a time (WRONG_VARIANTS): a walk that differs from the model in one rule, which the row named
for it must tell from the model.

Host only; the expected results of every row are the reference's (tools/make_base_path_goldens.py ->
tests/golden/base_paths.npz)."""
from __future__ import annotations

from collections import Counter
from typing import Callable, Dict, List, NamedTuple, Optional

import numpy as np

from tools.craft_jpeg import _codes, craft_baseline_symbols, huffman_table

WIDTHS = (8, 9, 10, 11, 12, 13)
AB = 13                    # the stage-1 kernel's AC index; a fused launch's is 12 (MJ_FUSED_ACBITS: 10..13)
Y420 = ((2, 2), (1, 1), (1, 1))
ONES = [[1] * 64, [1] * 64]
W, H, MCUS, RI = 64, 32, 8, 4


class Refused(Exception):
    """The model's refusal: no code within 16 bits, or a stream that ends inside a symbol."""


# ======================================================================================================================
# The model walk
# ======================================================================================================================
class _Reader:
    """The reference's bit queue (:654-695): refilled one byte at a time, the byte behind a 0xFF skipped whatever it is."""

    def __init__(self, raw: bytes, pos: int, keep_stuffed: bool = False):
        self.raw, self.pos, self.acc, self.n, self.used, self.keep = raw, pos, 0, 0, 0, keep_stuffed
        self.stuffed, self.last_ff = 0, False

    def get(self, k: int) -> int:
        while k > self.n:
            if self.pos >= len(self.raw):
                raise Refused("the stream ends inside a symbol")
            b = self.raw[self.pos]
            self.pos += 2 if b == 0xFF and not self.keep else 1
            self.stuffed += b == 0xFF
            self.last_ff = b == 0xFF
            self.acc = ((self.acc << 8) | b) & ((1 << 64) - 1)
            self.n += 8
        if k == 0:
            return 0
        self.n -= k
        self.used += k
        return (self.acc >> self.n) & ((1 << k) - 1)

    def restart(self):
        self.acc, self.n, self.used = 0, 0, 0
        self.pos += 2


def code_book(bits, vals):
    """{(length, code): symbol} of the canonical code (:366-377)."""
    book, code, k = {}, 0, 0
    for length in range(1, 17):
        code <<= 1
        for _ in range(int(bits[length - 1])):
            if k < len(vals) and code < (1 << length):
                book.setdefault((length, code), int(vals[k]))
            k += 1
            code += 1
    return book


def _symbol(rd: _Reader, book):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | rd.get(1)
        s = book.get((length, code))
        if s is not None:
            return s, length, code
    raise Refused("no code within 16 bits")


def _extend(v: int, n: int, pow2: bool = False) -> int:
    return 0 if n == 0 else (v if v >> (n - 1) else v - ((1 << n) - (0 if pow2 else 1)))


def _i16(v: int) -> int:
    return ((v + 0x8000) & 0xFFFF) - 0x8000


WRONG_VARIANTS = {
    "over_reads": "an overshooting symbol consumes its value bits",
    "run0_eob": "(run, 0) ends the block",
    "run0_short": "(run, 0) advances by run only",
    "zrl15": "a ZRL advances 15",
    "extend_pow2": "EXTEND subtracts 2^n for a leading 0",
    "drop63": "a symbol on index 63 is dropped",
    "dc_clamp": "DC sums are clamped instead of wrapped",
    "no_reset": "predictors are kept over a restart",
    "keep_stuffed": "the byte behind an 0xFF is kept",
}


def kind_of(length: int, size: int, eob: bool, width: int) -> str:
    """What a table of `width` index bits makes of a symbol (build_resolved_tables): finished / open / second."""
    if length > width:
        return "second"
    return "finished" if length + (0 if eob else size) <= width else "open"


def new_census():
    return {"dc": Counter(), "ac": Counter(),          # (width, kind) -> symbols
            "dc_code_len": Counter(), "dc_comp_len": Counter(), "dc_size": Counter(), "ac_code_len": Counter(), "ac_size": Counter(), "ac_total": Counter(),
            "prefix": {w: {} for w in WIDTHS},         # AC codes behind `w` bits: (table, prefix) -> the codes seen
            "longest_dc": 0, "longest_ac": 0, "run0": Counter(), "c63": Counter(), "over": Counter(), "wait": set(),
            "dc_wrap": [],                              # (component, +1 | -1, byte offset in the entropy-coded data)
            "dc_wrapped_blocks": 0, "rst_large_pred": 0, "pad": Counter(), "stuffed": 0, "stuffed_last": 0,
            "seg_mcus": Counter(), "sparse_run": 0, "dense_blocks": 0, "refill_behind_over": 0, "blocks": 0, "refused": ""}


def walk(raw: bytes, wrong: Optional[str] = None, census: Optional[dict] = None):
    """The one interleaved scan of the baseline file `raw` -> (coefficient store int16 [blocks, 64], zig-zag, blocks in scan
    order; status "" or the refusal).  `census`: a new_census() to fill."""
    from pyjpegdecoder_amd._parse import parse_jpeg
    assert wrong is None or wrong in WRONG_VARIANTS
    cs = census if census is not None else new_census()
    p = parse_jpeg(raw)
    scan = p.scans[0]
    comps = [p.color_components[c] for c in scan.component_ids]
    nc = len(comps)
    reps = [c.horizontal_sampling * c.vertical_sampling if nc > 1 else 1 for c in comps]
    count = scan.mcu_count_h * scan.mcu_count_v
    ri = scan.restart_interval
    books = {d: code_book(s.bits.tolist(), s.vals.tolist()) for d, s in scan.huffman.items()}
    coef = np.zeros((count * sum(reps), 64), dtype=np.int64)
    rd = _Reader(raw, scan.entropy_start, wrong == "keep_stuffed")
    pred = [0] * nc
    wrapped = [False] * nc
    nb = seg_mcus = sparse = 0
    prev_over = False

    def seg_end():
        cs["pad"][rd.n] += 1
        cs["stuffed_last"] += rd.last_ff
        cs["seg_mcus"][seg_mcus] += 1

    try:
        for m in range(count):
            for i, c in enumerate(comps):
                tabs = scan.huffman_tables_id[scan.component_ids[i]]
                dcb, acb = books[tabs.dc & 3], books[(tabs.ac & 3) | 0x10]
                for _ in range(reps[i]):
                    blk = coef[nb]
                    nb += 1
                    cs["blocks"] += 1
                    size, length, _ = _symbol(rd, dcb)
                    for w in WIDTHS:
                        cs["dc"][(w, kind_of(length, size, False, w))] += 1
                    cs["dc_code_len"][length] += 1
                    cs["dc_comp_len"][(i, length)] += 1
                    dc_empty = size == 0
                    cs["dc_size"][size] += 1
                    cs["longest_dc"] = max(cs["longest_dc"], length + size)
                    diff = _extend(rd.get(size), size, wrong == "extend_pow2")
                    total = diff + pred[i]
                    if total != _i16(total):
                        cs["dc_wrap"].append((i, 1 if total > 0 else -1, rd.pos - scan.entropy_start))
                        wrapped[i] = not wrapped[i]
                    elif wrapped[i]:
                        cs["dc_wrapped_blocks"] += 1
                    pred[i] = max(-32768, min(32767, total)) if wrong == "dc_clamp" else _i16(total)
                    blk[0] = pred[i]
                    index, nsym, pos_in_round, prev, long_syms = 1, 0, 0, None, 0
                    while index < 64:
                        start = rd.used
                        hv, length, code = _symbol(rd, acb)
                        run, size = hv >> 4, hv & 15
                        eob = hv == 0
                        nsym += 1
                        for w in WIDTHS:
                            cs["ac"][(w, kind_of(length, size, eob, w))] += 1
                            if length > w:
                                cs["prefix"][w].setdefault((tabs.ac & 3, code >> (length - w)), set()).add(code)
                        kind = "zrl" if hv == 0xF0 else kind_of(length, size, eob, AB)
                        cs["ac_code_len"][length] += 1
                        cs["ac_size"][size] += 1
                        cs["ac_total"][length + (0 if eob else size)] += 1
                        here = pos_in_round
                        resolved = kind in ("finished", "zrl")
                        if kind == "open" and prev is not None:
                            cs["wait"].add((prev, start % 32))
                        prev = length + size if resolved and not eob else None
                        pos_in_round = (pos_in_round + 1) & 1 if resolved else 0
                        if prev_over and nsym <= 12 and length + size >= 24:
                            cs["refill_behind_over"] += 1
                        if eob:
                            break
                        if size == 0 and run < 15:
                            if wrong == "run0_eob":
                                break
                            land = index + run
                            cs["run0"][(run, "mid" if land < 63 else ("on63" if land == 63 else "over"))] += 1
                            index += run + (0 if wrong == "run0_short" else 1)
                            continue
                        index += 14 if (hv == 0xF0 and wrong == "zrl15") else run
                        if index >= 64:
                            cs["over"][(kind, here)] += 1
                            prev_over = True
                            if wrong == "over_reads":
                                rd.get(size)
                            break
                        if index == 63:
                            cs["c63"][(kind, here)] += 1
                        if size:
                            cs["longest_ac"] = max(cs["longest_ac"], length + size)
                            long_syms += 29 <= length + size <= 31
                            v = _extend(rd.get(size), size, wrong == "extend_pow2")
                            if not (wrong == "drop63" and index == 63):
                                blk[index] = v
                        index += 1
                    if nsym > 12:
                        prev_over = False
                    cs["dense_blocks"] += nsym >= 62 and long_syms >= 60
                    if dc_empty and nsym == 1 and eob:
                        sparse += 1
                        cs["sparse_run"] = max(cs["sparse_run"], sparse)
                    else:
                        sparse = 0
            seg_mcus += 1
            if ri > 0 and (m + 1) % ri == 0 and m + 1 != count:
                seg_end()
                cs["rst_large_pred"] += sum(abs(v) > 1000 for v in pred)
                rd.restart()
                seg_mcus = 0
                prev_over = False
                if wrong != "no_reset":
                    pred = [0] * nc
                    wrapped = [False] * nc
        seg_end()
        cs["stuffed"] = rd.stuffed
    except Refused as exc:
        cs["refused"] = str(exc)
        return coef.astype(np.int16), str(exc)
    return coef.astype(np.int16), ""


def walk_census(raw: bytes) -> dict:
    cs = new_census()
    walk(raw, census=cs)
    return cs


def overflow_mask(coef: np.ndarray, blocks_per_mcu: int) -> np.ndarray:
    """bool [MCUs]: an MCU with a block whose samples leave int16 before the reference's cast (:1570-1573; all-ones
    quantisation tables: the coefficients are the dequantised values).  With a margin of 256 for the + 128 and the rounding."""
    from pyjpegdecoder_amd._parse import undo_zigzag
    k = np.arange(8)
    c = np.where(k == 0, 2 ** -0.5, 1.0)[None, :] * np.cos((2 * k[:, None] + 1) * np.pi * k[None, :] / 16)     # [x, u]
    out = np.zeros(coef.shape[0], dtype=bool)
    for b in range(coef.shape[0]):
        if np.abs(coef[b].astype(np.int64)).sum() < 60000:       # (|sample| <= sum |c| / 4 at the most)
            continue
        xy = undo_zigzag(coef[b].astype(np.int16)).astype(np.float64)
        s = 0.25 * c @ xy @ c.T
        out[b] = np.abs(s).max() > 32767 - 256
    return out.reshape(-1, blocks_per_mcu).any(axis=1)


def pixel_mask(mcu_mask: np.ndarray, width: int, height: int) -> np.ndarray:
    """bool [width, height] (the reference's x-major image): True where the pixel comparison holds — outside the 16 x 16 MCUs of
    `mcu_mask` (4:2:0: the chroma blocks of an MCU reach all of it and nothing beyond it)."""
    mx = -(-width // 16)
    keep = np.ones((mx * 16, -(-height // 16) * 16), dtype=bool)
    for m in np.nonzero(mcu_mask)[0]:
        keep[(m % mx) * 16:(m % mx) * 16 + 16, (m // mx) * 16:(m // mx) * 16 + 16] = False
    return keep[:width, :height]


# ======================================================================================================================
# Tables
# ======================================================================================================================
def rare_ac_table(variant: int = 0, seed: int = 0):
    """(bits, vals) of an AC table with all 256 (run, size) symbols — (run, 0) for run 1..14 among them, which no encoder
    writes and the reference takes (:853-866) — and code lengths 2..16; the usual symbols short, a 13-bit and three 16-bit codes
    for size 15, (run, 0) symbols at 4..16 bits.  The code is incomplete: the patterns behind its last 16-bit code have none,
    inside that code's second-level table (for any index width) and, further up, at the main level.  variant 1: other lengths
    for the short symbols (a chroma table); seed: the order of the symbols that are not pinned."""
    pin = {0x01: 2, 0x00: 3, 0x02: 3, 0x11: 4, 0x10: 4, 0x21: 5, 0xF0: 5, 0x12: 5, 0x03: 5, 0x04: 6, 0x31: 6, 0x05: 6, 0x20: 6,
           0x06: 7, 0x41: 7, 0x30: 7, 0x22: 7, 0x13: 7, 0x07: 7, 0x14: 8, 0x40: 8, 0xD0: 8, 0x08: 8, 0x15: 8, 0x26: 8, 0x23: 8,
           0x50: 9, 0xE0: 9, 0x24: 9, 0x0C: 9, 0x16: 9, 0x60: 10, 0x25: 10, 0x17: 10, 0x70: 11, 0x18: 11, 0x1A: 11, 0x80: 12, 0x19: 12,
           0x0F: 13, 0x90: 13, 0x1B: 13, 0x2A: 13, 0x3F: 13, 0xA0: 14, 0x29: 14, 0x1C: 14, 0x2B: 14, 0x0A: 14,
           0xB0: 15, 0x2F: 15, 0x1E: 15, 0x0E: 15, 0x0B: 15, 0x3A: 15, 0xC0: 16, 0x1F: 16, 0x2E: 16, 0x0D: 16, 0x1D: 16, 0x09: 16, 0x3B: 16, 0x4A: 16}
    if variant == 1:
        for a, b in ((0x01, 0x00), (0x02, 0x11), (0x21, 0x04), (0x06, 0x14), (0x0C, 0x60), (0x0E, 0x0D), (0xC0, 0xB0), (0x10, 0x20)):
            pin[a], pin[b] = pin[b], pin[a]
    counts = {2: 1, 3: 2, 4: 2, 5: 4, 6: 4, 7: 6, 8: 10, 9: 14, 10: 18, 11: 22, 12: 26, 13: 30, 14: 30, 15: 30}
    rest = [s for s in range(256) if s not in pin]
    np.random.default_rng(1000 + seed).shuffle(rest)
    L = dict(pin)
    for l, n in counts.items():
        have = sum(1 for v in pin.values() if v == l)
        assert have <= n, (l, have)
        for _ in range(n - have):
            L[rest.pop()] = l
    for s in rest:
        L[s] = 16
    return huffman_table(L)


def rare_dc_table(variant: int = 0, seed: int = 0, with_16: bool = False):
    """(bits, vals) of a DC table with the sizes 0..15 (and 16): sizes 7..11 behind codes of 9, 10, 11, 12 and 15 bits, 12..15
    (and 16) behind 16-bit codes, the small sizes short.  Incomplete: sixteen ones are no code."""
    short = [2, 2, 3, 4, 5, 6, 7] if variant == 0 else [3, 3, 2, 3, 5, 6, 7]
    short = short[seed % 7:] + short[:seed % 7] if seed else short
    L = dict(zip(range(7), short))
    L.update({7: 9, 8: 10, 9: 11, 10: 12, 11: 15, 12: 16, 13: 16, 14: 16, 15: 16})
    if with_16:
        L[16] = 16
    return huffman_table(L)


class Tables:
    """The four tables of a row (DC luma, DC chroma, AC luma, AC chroma) and look-ups by what a symbol IS in them."""

    def __init__(self, seed: int = 0, with_16: bool = False):
        self.dc = [rare_dc_table(0, seed, with_16), rare_dc_table(1, seed, with_16)]
        self.ac = [rare_ac_table(0, seed), rare_ac_table(1, seed)]
        self.dcl = [{s: l for s, (_, l) in _codes(*t).items()} for t in self.dc]
        self.acl = [{s: l for s, (_, l) in _codes(*t).items()} for t in self.ac]
        self.acc = [_codes(*t) for t in self.ac]

    def find(self, k: int, pred, key=None):
        """The (run, size) of table k's symbols that satisfy pred(run, size, code length), smallest key first (default:
        run, then size)."""
        out = [(s >> 4, s & 15) for s, l in self.acl[k].items() if s not in (0x00, 0xF0) and pred(s >> 4, s & 15, l)]
        return sorted(out, key=key or (lambda rs: rs))

    def bits(self, k: int, items) -> int:
        n = 0
        for it in items:
            if it[0] == "dc":
                n += self.dcl[k][it[1]] + it[1]
            elif it[0] == "ac":
                n += self.acl[k][(it[1] << 4) | it[2]] + (it[2] if len(it) < 4 or it[3] is not None else 0)
            else:
                n += it[2]
        return n


TAB = Tables()
TAB16 = Tables(with_16=True)
K_OF_BLOCK = (0, 0, 0, 0, 1, 1)                      # table class (luma / chroma) of the six blocks of a 4:2:0 MCU
EOB = ("ac", 0, 0)
ZRL = ("ac", 15, 0)


def dc(diff: int):
    size = abs(diff).bit_length()
    return ("dc", size, diff if diff > 0 else diff + (1 << size) - 1)


def ac(run: int, v: int):
    size = abs(v).bit_length()
    return ("ac", run, size, v if v > 0 else v + (1 << size) - 1)


def sym(rs, sign: int = 1, low: int = 0):
    """The symbol (run, size) with a value of that size: the smallest magnitude plus `low`, of the sign given."""
    run, size = rs
    if size == 0:
        return ("ac", run, 0)
    return ac(run, sign * ((1 << (size - 1)) + low % (1 << (size - 1)) if size > 1 else 1))


def plain(n: int) -> list:
    """An ordinary block: a small DC step (they cancel in pairs), two or three short symbols, end of block."""
    return [dc(3 if n % 2 == 0 else -3), ac(0, 1 + n % 3), ac(n % 2, -1), ac(1, 2)][:3 + n % 2] + [EOB]


def reach(idx: int, parity: int, sign: int = 1) -> list:
    """AC symbols that carry the index from 1 to `idx` (2..63), an even (0) or odd (1) number of them, all finished entries."""
    out, n = [], idx - 1
    while n > 16:
        out.append(ZRL)
        n -= 16
    assert n >= 1
    if (len(out) + 1) % 2 != parity:
        if n >= 2:
            out.append(ac(n - 2, sign))
            n = 1
        else:                                       # (n == 1: one ZRL fewer, seventeen positions in two symbols)
            out.pop()
            out += [ac(15, sign), ac(0, -sign)]
            return out
    out.append(ac(n - 1, -sign))
    assert len(out) % 2 == parity
    return out


def crafted(units: list, tab: Tables = TAB, ri: int = RI, width: int = W, height: int = H) -> bytes:
    """The file that holds `units` (craft_baseline_symbols' MCUs and markers): 4:2:0, all-ones quantisation tables."""
    return craft_baseline_symbols(width, height, Y420, units, dc_tables=tab.dc, ac_tables=tab.ac, restart_interval=ri, qts=ONES)


def make(special: Dict[tuple, list], ri: int = RI, mcus: int = MCUS, tail=(), between=None) -> list:
    """The units of a file of the common kind: the blocks of `special` = {(MCU, block of the MCU): items}, every other block
    plain, a restart marker behind every `ri` MCUs.  (A row's builder returns its units; row_bytes crafts the file.)"""
    units = []
    for m in range(mcus):
        units.append([special.get((m, b), plain(m * 6 + b)) for b in range(6)])
        if ri and (m + 1) % ri == 0 and m + 1 != mcus:
            units += list((between or {}).get(m, [("rst",)]))
    return units + list(tail)


# ======================================================================================================================
# Rows
# ======================================================================================================================
def d_long(tab: Tables = TAB):
    """DC codes of 9, 10, 11, 12, 15 and 16 bits (sizes 7..12) in every component, differences that cancel in pairs."""
    sp, sizes = {}, [7, 8, 9, 10, 11, 12]
    for seg in range(2):
        for q in range(3):                                      # MCUs 0..2 of the segment: two sizes each, MCU 3 plain
            m = seg * 4 + q
            s1, s2 = sizes[2 * q], sizes[2 * q + 1]
            v1, v2 = (1 << s1) - 1 - m, (1 << (s2 - 1)) + m
            sp[(m, 0)] = [dc(v1), ac(0, 1), EOB]
            sp[(m, 1)] = [dc(-v1), ac(1, -2), EOB]
            sp[(m, 2)] = [dc(-v2), EOB]
            sp[(m, 3)] = [dc(v2), ac(0, 3), EOB]
        for b in (4, 5):                                        # chroma: one block per MCU, three sizes per segment
            d = [100 + b, 200 - b, -300] if seg == 0 else [-1000 - b, -1500 + b, 2500]
            for q, v in enumerate(d):
                sp[(seg * 4 + q, b)] = [dc(v), ac(q % 2, 1), EOB]
    return make(sp)


def d_size():
    """DC sizes 12..15 behind 16-bit codes (the 31-bit DC symbol), up and down again."""
    sp = {}
    mags = {12: 4000, 13: 8000, 14: 16000, 15: 32700}
    for seg in range(2):
        for q, s in enumerate((12, 13, 14, 15)):
            m = seg * 4 + q
            v = mags[s] - 7 * seg
            sp[(m, 1)] = [dc(v), ac(0, 1), EOB]
            sp[(m, 2)] = [dc(-v), EOB]
            b = 4 + (q + seg) % 2
            if q % 2 == 0:
                sp[(m, b)] = [dc(-v), ac(0, 2), EOB]
                sp[(m + 1, b)] = [dc(v), EOB]
    return make(sp)


def d_size_16():
    """DC size 16 behind a 16-bit code: 32 bits, the longest symbol a stream holds.  The sums wrap."""
    sp = {(1, 0): [("dc", 16, 0x9C40), ac(0, 1), EOB], (1, 2): [("dc", 16, 0x0001), EOB], (2, 4): [("dc", 16, 0xFFFF), EOB],
          (5, 1): [("dc", 16, 0x7FFF), ac(0, 2), EOB], (5, 5): [("dc", 16, 0x8000), EOB], (6, 3): [("dc", 16, 0x1234), EOB]}
    return crafted(make(sp), TAB16)


def d_wrap_mcus(stay: int = 1, n0: int = 0) -> list:
    """MCUs in which every component's predictor sum crosses +32767, stays wrapped for `stay` MCUs, and crosses back."""
    out = []

    def mcu(ld, cd, n):
        blocks = [[dc(ld[b])] + plain(n + b)[1:] if ld[b] else plain(n + b) for b in range(4)]
        return blocks + [[dc(cd)] + plain(n + 4)[1:] if cd else plain(n + 4), [dc(cd)] + plain(n + 5)[1:] if cd else plain(n + 5)]
    out.append(mcu([30000, 0, 0, 10000], 30000, n0))            # luma wraps inside the MCU, chroma is at +30000
    out.append(mcu([0, 0, 0, 0], 10000, n0 + 6))                # chroma wraps
    for k in range(stay):
        out.append(mcu([0, 0, 0, 0], 0, n0 + 12 + 6 * k))       # everything stays wrapped
    out.append(mcu([-10000, 0, 0, -30000], -10000, n0 + 18))    # back over the edge, luma to zero
    return out


def d_wrap():
    """+32767 crossed upwards in the first segment, -32768 downwards in the second; zero again behind the marker."""
    up = d_wrap_mcus(1)

    def neg(block):
        return [("dc", it[1], (~it[2]) & ((1 << it[1]) - 1)) if it[0] == "dc" and it[1] > 8 else it for it in block]
    down = [[neg(b) for b in m] for m in d_wrap_mcus(1, 24)]
    return up + [("rst",)] + down


def _spread(symbols: List[tuple], per_block: int = 4, tab: Tables = TAB, ks=(0, 1)) -> Dict[tuple, list]:
    """`symbols` = (table class, (run, size)) dealt out over the blocks of their class, `per_block` to a block, plain blocks
    between them; values of alternating sign."""
    sp, slots = {}, {0: [(m, b) for m in range(MCUS) for b in (1, 2, 3)], 1: [(m, b) for m in range(MCUS) for b in (4, 5) if (m + b) % 4]}
    n = 0
    for k in ks:
        mine = [rs for kk, rs in symbols if kk == k]
        at = 0
        while mine:
            blk, idx = [dc(2 if n % 2 else -2)], 1
            while mine and len(blk) <= per_block and idx + mine[0][0] < 62:
                rs = mine.pop(0)
                blk.append(sym(rs, 1 if n % 2 else -1, 5 * n))
                idx += rs[0] + 1
                n += 1
            sp[slots[k][at]] = blk + [EOB]
            at += 1
    return sp


def a_fin(tab: Tables = TAB):
    """Symbols whose code + value bits are exactly 9, 10, 11, 12 and 13: the last ones a table of that width finishes."""
    want = [(k, rs) for k in (0, 1) for w in (9, 10, 11, 12, 13) for rs in tab.find(k, lambda r, s, l: s and l + s == w)[:2]]
    return make(_spread(want, 3, tab))


def a_open(tab: Tables = TAB, ri: int = RI):
    """... 10, 11, 12, 13 and 14 (the first ones it does not), a 13-bit code with size 15, a 16-bit code with size 15."""
    want = [(k, rs) for k in (0, 1) for w in (9, 10, 11, 12, 13) for rs in tab.find(k, lambda r, s, l: s and l <= w < l + s and l + s == w + 1)[:2]]
    sp = _spread(want, 3, tab)
    for k, blocks in ((0, [(6, 0), (7, 0)]), (1, [(4, 4), (7, 5)])):
        s13 = tab.find(k, lambda r, s, l: s == 15 and l == 13)[0]
        s16 = tab.find(k, lambda r, s, l: s == 15 and l == 16)[0]
        sp[blocks[0]] = [dc(1), ac(0, 1), sym(s13, 1, 77), EOB]
        sp[blocks[1]] = [dc(-1), sym(s16, -1, 1234), ac(0, 2), EOB]
    return make(sp, ri=ri)


def a_2nd(tab: Tables = TAB):
    """Codes of 11..16 bits, every one the table has with a size of 1..6 and a run of at most 2."""
    want = [(k, rs) for k in (0, 1) for ln in (11, 12, 13, 14, 15, 16) for rs in tab.find(k, lambda r, s, l: l == ln and 1 <= s <= 7 and r <= 8)[:4]]
    return make(_spread(want, 5, tab))


def a_run0():
    """(run, 0) for run 1..14: in mid block, landing on index 63, carrying the index past it."""
    sp, slots = {}, [(m, b) for m in range(MCUS) for b in range(6) if b not in (0,)]
    mid = [[dc(1), ac(0, 1)] + [x for r in rr for x in (("ac", r, 0), ac(0, -1 if r % 2 else 2))] + [EOB] for rr in ((1, 2, 3, 4, 5, 6), (7, 8, 9, 10), (11, 12, 13), (14, 1))]
    on63 = [[dc(-1)] + reach(63 - r, r % 2) + [("ac", r, 0)] for r in range(1, 15)]
    over = [[dc(2)] + reach(min(63, 64 - r + r % 3), (r + 1) % 2) + [("ac", r, 0)] for r in range(1, 15)]
    for at, blk in zip(slots, mid + [x for pair in zip(on63, over) for x in pair]):
        sp[at] = blk
    return make(sp)


def _kinds(tab: Tables, k: int, min_run: int):
    """One symbol per entry kind with a run of at least min_run: finished, open, second level (sizes small), and the ZRL."""
    fin = tab.find(k, lambda r, s, l: r >= min_run and s and l + s <= AB)[0]
    opn = tab.find(k, lambda r, s, l: r >= min_run and l <= AB < l + s, key=lambda rs: (rs[0], rs[1]))[0]
    sec = tab.find(k, lambda r, s, l: r >= min_run and l > AB and 1 <= s <= 6)[0]
    return {"finished": fin, "open": opn, "second": sec, "zrl": (15, 0)}


def _long_block(tab: Tables, k: int, n: int) -> list:
    """A block of twelve symbols of 24..27 bits (codes of 14..16 bits, sizes 9..11): a dword a symbol for the lane's window."""
    pool = tab.find(k, lambda r, s, l: l >= 14 and 9 <= s <= 11 and r <= 3)
    assert len(pool) >= 4 and 12 * (max(r for r, _ in pool) + 1) < 62
    return [dc(1 if n % 2 else -1)] + [sym(pool[(n + j) % len(pool)], 1 if j % 2 else -1, 17 * j + n) for j in range(12)] + [EOB]


def _block_ends(over: bool):
    sp = {}
    at = {0: [(m, b) for m in range(MCUS) for b in (0, 2)], 1: [(m, 4) for m in range(MCUS)]}
    n = 0
    for k, kinds in ((0, ("finished", "open", "second", "zrl")), (1, ("finished", "open", "second", "zrl"))):
        ks = _kinds(TAB, k, 1 if over else 0)
        for kind in kinds:
            for parity in (0, 1):
                if k == 1 and parity == 1 and kind in ("finished", "zrl"):
                    continue                                       # (six chroma blocks, eight luma ones)
                run = ks[kind][0]
                idx = 63 - run if not over else min(63, 64 - run + (n % 2))
                s = sym(ks[kind], 1 if n % 2 else -1, 3 * n)
                if over and s[2]:
                    s = s[:3] + (None,)
                slot = at[k].pop(0)
                sp[slot] = [dc(2 if n % 2 else -2)] + reach(idx, parity) + [s]
                sp[(slot[0], slot[1] + 1)] = _long_block(TAB, k, n)      # the next block of the same lane: long symbols
                n += 1
    return make(sp)


def a_63():
    """A symbol of every entry kind that lands on coefficient 63, as the first and as the second of a two-symbol round."""
    return _block_ends(False)


def a_over():
    """... that carries the index past 63: its value bits are not in the stream."""
    return _block_ends(True)


def a_wait():
    """An unresolved symbol directly behind a finished one of every total length 3..13, starting at every bit phase 0..31 of
    its restart segment's stream (the luma blocks of both segments; as many as it takes)."""
    tab = TAB
    fins = {}
    for L in range(2, AB + 1):
        c = tab.find(0, lambda r, s, l: l + s == L and (s or r < 15), key=lambda rs: (rs[0], -rs[1]))
        if c:
            fins[L] = c[0]
    opens = sorted(tab.find(0, lambda r, s, l: l <= AB < l + s and r == 0), key=lambda rs: rs[1])
    by_parity = {p: next(rs for rs in opens if (tab.acl[0][rs[0] << 4 | rs[1]] + rs[1]) % 2 == p) for p in (0, 1)}
    todo = {(L, ph) for L in fins for ph in range(32)}
    units, pos, n = [], 0, 0
    order = sorted(fins)
    for m in range(MCUS):
        mcu = []
        for b in range(6):
            if b >= 4 or not todo:
                blk = plain(n)
            else:
                blk, idx = [dc(1 if n % 2 else -1)], 1
                here = pos + tab.bits(0, blk)
                while todo:
                    L = next((x for x in order if (x, (here + x) % 32) in todo), None)
                    if L is None:                                       # no pair is missing at this phase: one short symbol further
                        if idx > 58:
                            break
                        blk.append(ac(0, 1 if n % 2 else -1))
                        here += tab.bits(0, blk[-1:])
                        idx += 1
                        continue
                    f = fins[L]
                    o = by_parity[(L + 1) % 2]
                    if idx + f[0] + 1 + o[0] + 1 > 62:
                        break
                    pair = [sym(f, 1 if n % 2 else -1, n), sym(o, -1 if n % 2 else 1, n)]
                    todo.discard((L, (here + L) % 32))
                    here += tab.bits(0, pair)
                    idx += f[0] + 1 + o[0] + 1
                    blk += pair
                    n += 1
                blk.append(EOB)
            pos += tab.bits(K_OF_BLOCK[b], blk)
            mcu.append(blk)
            n += 1
        units.append(mcu)
        if m == 3:
            units.append(("rst",))
            pos = 0
    assert not todo, f"A-wait no longer fits the common geometry: {len(todo)} pairs left"
    return units


def _dense_block(tab: Tables, k: int, n: int) -> list:
    """62 or 63 symbols of 29..31 bits."""
    z = tab.find(k, lambda r, s, l: r == 0 and 29 <= l + s <= 31)
    o = tab.find(k, lambda r, s, l: r == 1 and 29 <= l + s <= 31)
    assert z and o
    blk = [dc(1 if n % 2 else -1)]
    if n % 2:
        blk += [sym(z[j % len(z)], 1 if j % 2 else -1, 31 * j + n) for j in range(61)] + [sym(o[0], 1, n)]
    else:
        blk += [sym(z[j % len(z)], -1 if j % 3 else 1, 0x3FFF - 97 * j) for j in range(63)]
    return blk


def _tame_dense_block(tab: Tables, n: int) -> list:
    """63 symbols of 29 bits whose samples stay inside int16: a 16-bit code with size 13, the smallest magnitudes, and the first
    of a fixed series of sign patterns that overflow_mask lets through."""
    rs = next(x for x in tab.find(0, lambda r, s, l: r == 0 and s == 13 and l == 16))
    for seed in range(200):
        signs = np.random.default_rng(seed + 1000 * n).integers(0, 2, 63) * 2 - 1
        zz = np.zeros((1, 64), dtype=np.int64)
        zz[0, 1:] = signs * (4096 + np.arange(63))
        if not overflow_mask(zz.repeat(6, axis=0), 6).any():
            return [dc(1 if n % 2 else -1)] + [ac(0, int(v)) for v in zz[0, 1:]]
    raise AssertionError("no sign pattern keeps the dense block inside int16")


def w_dense():
    """Both segments made of blocks of 62..63 symbols of 29..31 bits; the value bits of every other block run to ones."""
    return make({(m, b): _dense_block(TAB, K_OF_BLOCK[b], m * 6 + b) for m in range(MCUS) for b in range(6)})


def w_sparse():
    """16 MCUs to the row: 210 consecutive blocks of a zero-size DC symbol and an end of block, then two dense blocks (of luma, samples inside int16)."""
    empty = [("dc", 0), EOB]
    units, nb = [], 0
    for m in range(64):
        mcu = []
        for b in range(6):
            mcu.append(empty if 6 <= nb < 216 else (_tame_dense_block(TAB, nb) if nb in (216, 217) else plain(nb)))
            nb += 1
        units.append(mcu)
        if m == 47:
            units.append(("rst",))
    return craft_baseline_symbols(256, 64, Y420, units, dc_tables=TAB.dc, ac_tables=TAB.ac, restart_interval=48, qts=ONES)


def s_pad(first: int, second: Optional[int]):
    """Segments that end with `first` and `second` pad bits (None: the last data byte is 0xFF with its stuffed zero)."""
    def tail_for(pad, n0):
        mcus = [[plain(n0 + 6 * m + b) for b in range(6)] for m in range(4)]
        if pad is None:
            mcus[3][5] = [dc(1)] + reach(63, 0) + [("ac", 0, 10, 0x3FF)]
            return mcus
        for extra in range(64):
            mcus[3][5] = [dc(1)] + [ac(0, 1)] * (extra % 8) + [ac(2, 1)] * (extra // 8) + [EOB]
            total = sum(TAB.bits(K_OF_BLOCK[b], blk) for m in mcus for b, blk in enumerate(m))
            if (-total) % 8 == pad:
                return mcus
        raise AssertionError(pad)
    return tail_for(first, 0) + [("rst",)] + tail_for(second, 24)


def _last_code(tab: Tables, k: int):
    return max(c for c, l in tab.acc[k].values() if l == 16)


def x_nocode_dc():
    return make({(2, 1): [("bits", 0xFFFF, 16), ac(0, 1), EOB]})


def x_nocode_main():
    return make({(5, 4): [dc(1), ac(0, 1), ("bits", 0xFFFF, 16), EOB]})


def x_nocode_2nd():
    hole = _last_code(TAB, 0) + 1
    assert hole >> 3 == (hole - 1) >> 3                            # the same 13-bit prefix as the table's last code
    return make({(1, 2): [dc(1), ac(0, 1), ac(1, 2), ("bits", hole, 16), EOB]})


def x_extra():
    return make({}, between={3: [("rst", b"\x55")]})


def x_short():
    return make({(3, 5): _long_block(TAB, 1, 3)}, between={3: [("cut", 9), ("rst",)]})


def g_ragged():
    return crafted(a_open(ri=3), ri=3)


HEALTHY_COMMON = ["D-long", "D-size", "D-wrap", "A-fin", "A-open", "A-2nd", "A-run0", "A-63", "A-over", "A-wait", "W-dense",
                  "S-pad-07", "S-pad-16", "S-pad-25", "S-pad-34", "S-pad-ff"]
S_ALL_STAY = 60
S_ALL_W, S_ALL_H = 256, 16 * 11
OVERSHOOTS = ("A-run0", "A-over")          # rows with a symbol that lands behind its block


def s_all():
    """Every healthy row's MCUs back to back in one file without restart markers — but for the rows of OVERSHOOTS, which S-over
    holds: a symbol that lands behind its block voids the synchronisation form's chunk records by design (huffman_sync.hip), and
    a file with one is decoded by the serial walk whatever else it holds.  (The DC predictors run on; D-wrap's stretch of
    wrapped sums is drawn out to S_ALL_STAY MCUs so that it lies across chunk boundaries of 256 and of 512 bytes wherever it falls)."""
    from pyjpegdecoder_amd._parse import parse_jpeg
    units = []
    for name in [n for n in HEALTHY_COMMON if n not in OVERSHOOTS]:
        if name == "D-wrap":
            units += d_wrap_mcus(S_ALL_STAY)
            continue
        units += row_mcus(name)
    n = (S_ALL_W // 16) * (S_ALL_H // 16)
    assert len(units) <= n, len(units)
    units += [[plain(7 * m + b) for b in range(6)] for m in range(n - len(units))]
    raw = craft_baseline_symbols(S_ALL_W, S_ALL_H, Y420, units, dc_tables=TAB.dc, ac_tables=TAB.ac, qts=ONES)
    assert parse_jpeg(raw).scans[0].restart_interval == 0
    return raw


def s_over():
    """The rows of OVERSHOOTS back to back without restart markers (64 x 64: 16 MCUs)."""
    units = [u for name in OVERSHOOTS for u in row_mcus(name)]
    return craft_baseline_symbols(64, 64, Y420, units, dc_tables=TAB.dc, ac_tables=TAB.ac, qts=ONES)



def row_mcus(name: str) -> list:
    """The MCUs (no markers) of a row of the common kind."""
    row_bytes(name)
    return [u for u in _units[name] if not isinstance(u, tuple)]


def t_own(i: int):
    """A file of the common geometry with four tables of its own (the A-open symbols, looked up in ITS tables)."""
    tab = Tables(seed=10 + i)
    return crafted(a_open(tab), tab)


# ---- the table ----------------------------------------------------------------------------------------------------------------
class Row(NamedTuple):
    name: str
    make: Callable[[], bytes]
    reached: Callable[[dict], bool]      # the census of the model walk -> the row reaches its path
    refused: str = ""                    # the status class the library must end the file with ("" = healthy)
    ref: str = ""                        # the exception the reference raises on it
    wrong: tuple = ()                    # the wrong variants this row must tell from the model
    common: bool = True                  # the common geometry, Huffman tables TAB
    masked: bool = False                 # blocks whose samples leave int16 may occur (the pixel comparison masks them)


def _tot(cs, n):
    return cs["ac_total"][n] >= 1


ROWS = [
    Row("D-long", d_long, lambda cs: all(cs["dc_comp_len"][(c, l)] >= 1 for c in range(3) for l in (9, 10, 11, 12, 15, 16))
        and cs["dc"][(8, "second")] >= 36 and cs["dc"][(9, "second")] >= 28 and cs["dc"][(11, "second")] >= 12 and not cs["dc_wrap"]),
    Row("D-size", d_size, lambda cs: all(cs["dc_size"][s] >= 4 for s in (12, 13, 14, 15)) and cs["longest_dc"] == 31 and not cs["dc_wrap"]),
    Row("D-wrap", d_wrap, lambda cs: {(c, d) for c, d, _ in cs["dc_wrap"]} == {(c, d) for c in range(3) for d in (1, -1)}
        and cs["dc_wrapped_blocks"] >= 12 and cs["rst_large_pred"] >= 2, wrong=("dc_clamp", "no_reset")),
    Row("A-fin", a_fin, lambda cs: all(_tot(cs, w) for w in (9, 10, 11, 12, 13)) and all(cs["ac"][(w, "finished")] >= 4 for w in (9, 10, 11, 12, 13)),
        wrong=("extend_pow2",)),
    Row("A-open", a_open, lambda cs: all(_tot(cs, w + 1) and cs["ac"][(w, "open")] >= 4 for w in (9, 10, 11, 12, 13)) and cs["ac_total"][28] >= 2
        and cs["ac_total"][31] >= 2 and cs["longest_ac"] == 31 and cs["ac_size"][15] >= 4),
    Row("A-2nd", a_2nd, lambda cs: all(cs["ac_code_len"][l] >= 4 for l in (11, 12, 13, 14, 15, 16))
        and all(len(cs["prefix"][w]) >= 3 and max(map(len, cs["prefix"][w].values())) >= 2 for w in (10, 11, 12, 13))),
    Row("A-run0", a_run0, lambda cs: all(cs["run0"][(r, where)] >= 1 for r in range(1, 15) for where in ("mid", "on63", "over")),
        wrong=("run0_eob", "run0_short")),
    Row("A-63", a_63, lambda cs: all(cs["c63"][(k, p)] >= 1 for k in ("finished", "open", "second", "zrl") for p in (0, 1)),
        wrong=("drop63", "zrl15")),
    Row("A-over", a_over, lambda cs: all(cs["over"][(k, p)] >= 1 for k in ("finished", "open", "second", "zrl") for p in (0, 1))
        and cs["refill_behind_over"] >= 8 * 12, wrong=("over_reads",)),
    Row("A-wait", a_wait, lambda cs: all((L, ph) in cs["wait"] for L in range(3, 14) for ph in range(32))),
    Row("W-dense", w_dense, lambda cs: cs["dense_blocks"] == 48 and cs["stuffed"] >= 40, wrong=("keep_stuffed",), masked=True),
    Row("W-sparse", w_sparse, lambda cs: cs["sparse_run"] >= 200 and cs["dense_blocks"] == 2 and cs["ac_total"][29] >= 126, common=False),
    Row("S-pad-07", lambda: s_pad(0, 7), lambda cs: cs["pad"] == Counter({0: 1, 7: 1})),
    Row("S-pad-16", lambda: s_pad(1, 6), lambda cs: cs["pad"] == Counter({1: 1, 6: 1})),
    Row("S-pad-25", lambda: s_pad(2, 5), lambda cs: cs["pad"] == Counter({2: 1, 5: 1})),
    Row("S-pad-34", lambda: s_pad(3, 4), lambda cs: cs["pad"] == Counter({3: 1, 4: 1})),
    Row("S-pad-ff", lambda: s_pad(None, None), lambda cs: cs["stuffed_last"] == 2),
    Row("X-nocode-dc", x_nocode_dc, lambda cs: "no code" in cs["refused"], refused="bad_code", ref="CorruptedJpeg"),
    Row("X-nocode-main", x_nocode_main, lambda cs: "no code" in cs["refused"], refused="bad_code", ref="CorruptedJpeg"),
    Row("X-nocode-2nd", x_nocode_2nd, lambda cs: "no code" in cs["refused"], refused="bad_code", ref="CorruptedJpeg"),
    Row("X-extra", x_extra, lambda cs: bool(cs["refused"]), refused="desync", ref="CorruptedJpeg"),   # (its walk runs on behind the spare byte, into a pattern without a code)
    Row("X-short", x_short, lambda cs: "ends inside" in cs["refused"], refused="overrun", ref="IndexError"),
    Row("G-ragged", g_ragged, lambda cs: cs["seg_mcus"] == Counter({3: 2, 2: 1}) and cs["ac_total"][31] >= 2, common=False),
    Row("S-all", s_all, lambda cs: cs["seg_mcus"] == Counter({(S_ALL_W // 16) * (S_ALL_H // 16): 1}) and cs["dense_blocks"] == 48
        and len(cs["dc_wrap"]) >= 6, common=False, masked=True),
    Row("S-over", s_over, lambda cs: cs["seg_mcus"] == Counter({16: 1}) and sum(cs["over"].values()) >= 8 and sum(n for (r, w), n in cs["run0"].items() if w == "over") >= 14,
        common=False),
] + [Row(f"T-own-{i}", (lambda i=i: t_own(i)), lambda cs: cs["ac_total"][31] >= 2 and cs["ac_total"][28] >= 2, common=False) for i in range(6)]
# Not a row with a golden: the reference adds a DC difference of size 16 to its int16 predictor as a Python integer, which NumPy
# refuses as out of bounds (an OverflowError, not a rule of the format).  The file is held to the oracle in every form.
EXTRA = [Row("D-size-16", d_size_16, lambda cs: cs["dc_size"][16] == 6 and cs["longest_dc"] == 32 and len(cs["dc_wrap"]) >= 2, common=False)]
ROW = {r.name: r for r in ROWS + EXTRA}
HEALTHY = [r for r in ROWS if not r.refused]
REFUSED = [r for r in ROWS if r.refused]
COMMON = [r for r in HEALTHY if r.common]
assert [r.name for r in COMMON] == HEALTHY_COMMON

_made: Dict[str, bytes] = {}
_units: Dict[str, list] = {}


def row_bytes(name: str) -> bytes:
    """The row's file.  A builder returns the file, or — rows of the common kind — its units, which are crafted here."""
    if name not in _made:
        got = ROW[name].make()
        if isinstance(got, list):
            _units[name] = got
            got = crafted(got)
        _made[name] = got
    return _made[name]


# ---- what a set of inputs reaches, event by event (profiles/base_paths_census.txt) -------------------------------------------
EVENTS = ([f"dc_{k}_{w}" for w in WIDTHS for k in ("finished", "open", "second")] + [f"ac_{k}_{w}" for w in WIDTHS for k in ("finished", "open", "second")]
          + ["dc_symbol_bits_max", "ac_symbol_bits_max", "dc_size_max", "ac_size_max", "run0_mid", "run0_on63", "run0_over",
             "c63_finished", "c63_open", "c63_second", "over_finished", "over_open", "over_second", "over_zrl", "wait_pairs", "dc_sum_wraps",
             "pad_kinds", "stuffed_bytes", "stuffed_last", "dense_blocks", "sparse_run_max", "refused"])
_MAXED = {e for e in EVENTS if e.endswith("_max")}


def summary(cs: dict) -> Dict[str, int]:
    out = {}
    for w in WIDTHS:
        for k in ("finished", "open", "second"):
            out[f"dc_{k}_{w}"] = cs["dc"][(w, k)]
            out[f"ac_{k}_{w}"] = cs["ac"][(w, k)]
    out.update(dc_symbol_bits_max=cs["longest_dc"], ac_symbol_bits_max=cs["longest_ac"], dc_size_max=max(cs["dc_size"], default=0),
               ac_size_max=max(cs["ac_size"], default=0), wait_pairs=len(cs["wait"]), dc_sum_wraps=len(cs["dc_wrap"]), pad_kinds=len(cs["pad"]),
               stuffed_bytes=cs["stuffed"], stuffed_last=cs["stuffed_last"], dense_blocks=cs["dense_blocks"], sparse_run_max=cs["sparse_run"],
               refused=int(bool(cs["refused"])))
    for where in ("mid", "on63", "over"):
        out[f"run0_{where}"] = sum(n for (r, wh), n in cs["run0"].items() if wh == where)
    for k in ("finished", "open", "second", "zrl"):
        if k != "zrl":
            out[f"c63_{k}"] = sum(n for (kk, _), n in cs["c63"].items() if kk == k)
        out[f"over_{k}"] = sum(n for (kk, _), n in cs["over"].items() if kk == k)
    return {e: int(out[e]) for e in EVENTS}
