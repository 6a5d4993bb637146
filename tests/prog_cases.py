"""The progressive stage 1's rare symbol paths: one small file per path (tools/craft_jpeg.craft_progressive_symbols), a plain
model of the scan walk that decodes them, and the census that proves each file reaches the path it is named for.

The three hand-scheduled symbol loops of progressive_fast.hip (walk_ac_first, the scout, the placing walk_ac_refine) leave
with an exit code into a slow path for everything that is not a short (run, size) symbol: a code longer than the 11-bit
table, a ZRL, an EOBn, a run that ends behind the band, a full band; walk_dc_first has its own miss path behind a 9-bit
table.  The files the suite had before reach these by the luck of their inputs (profiles/prog_paths_census.txt); the rows
below reach them on purpose.

The model (`walk`) restates the reference's rules (jpeg_decoder.py:974-1057 DC scans, :1060-1298 AC scans) and counts, per
scan, only what the STREAM determines: symbol classes, code lengths against the two table widths, code + value bits,
end-of-band runs in blocks / block rows / band launches, correction bits per symbol and per block, the distance in bits
between consecutive symbol starts, history extremes.  Where the kernels' 64-bit windows lie is not modelled (nothing on the
device could hold such a model to account); window events are forced in stream terms — a symbol that starts 128 or more bits
behind the previous one always starts the windows again, 65 or more bits of short symbols always advance them.

`walk` also takes `spec_refine` (negative history refined by subtraction, T.81 G.1.2.3) and one WRONG variant at a time
(WRONG_VARIANTS): a walk that differs from the model in one rule, which the row named for it must tell from the model.

Host only; the expected results of every row are the reference's (tools/make_prog_path_goldens.py ->
tests/golden/prog_paths.npz)."""
from __future__ import annotations

from collections import Counter
from typing import Callable, Dict, List, NamedTuple, Optional

import numpy as np

from tools.craft_jpeg import _T, _ac_prog_table, craft_progressive_symbols, long_ac_table, long_dc_table

K_LUT_BITS = 11           # kProgLutBits: the AC tables of the stream walks resolve codes up to this length
K_DC_LUT_BITS = 9         # kProgDcLutBits


class Refused(Exception):
    """The model's refusal: no code within 16 bits, a position behind 63, a run past the scan in a refining scan, a stream
    that ends inside a symbol."""


# ======================================================================================================================
# The model walk
# ======================================================================================================================
class _Reader:
    """The reference's bit queue (:654-695): refilled one byte at a time, the byte behind a 0xFF skipped whatever it is."""

    def __init__(self, raw: bytes, pos: int):
        self.raw, self.pos, self.acc, self.n, self.used = raw, pos, 0, 0, 0

    def get(self, k: int) -> int:
        while k > self.n:
            if self.pos >= len(self.raw):
                raise Refused("the stream ends inside a symbol")
            b = self.raw[self.pos]
            self.pos += 2 if b == 0xFF else 1
            self.acc = ((self.acc << 8) | b) & ((1 << 160) - 1)
            self.n += 8
        if k == 0:
            return 0
        self.n -= k
        self.used += k
        return (self.acc >> self.n) & ((1 << k) - 1)

    def unget(self, k: int):                     # (the wrong variant "mod32" only)
        self.n += k
        self.used -= k

    def restart(self):
        self.acc, self.n = 0, 0
        self.pos += 2


def _code_book(spec):
    book, code, k = {}, 0, 0
    for length, count in enumerate(spec.bits.tolist(), start=1):
        code <<= 1
        for _ in range(count):
            if k < spec.vals.size:
                book[(length, code)] = int(spec.vals[k])
            k += 1
            code += 1
    return book


def _symbol(rd: _Reader, book):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | rd.get(1)
        s = book.get((length, code))
        if s is not None:
            return s, length
    raise Refused("no code within 16 bits")


def _extend(v: int, n: int) -> int:
    return 0 if n == 0 else (v if v >> (n - 1) else v - ((1 << n) - 1))


def _i16(v: int) -> int:
    return ((v + 0x8000) & 0xFFFF) - 0x8000


WRONG_VARIANTS = {
    "run_se": "a run is bounded by Se instead of 63: a coefficient behind the band is dropped",
    "zrl_nonzero": "a refining ZRL counts the non-zero coefficients it passes too",
    "corr_front": "the correction bits are read in front of their symbol's value bits",
    "sign": "the sign of a coefficient placed by a refining scan is inverted",
    "eob_self": "an end-of-band run does not count the block that raised it",
    "eob8": "an end-of-band run's length is cut to 8 bits",
    "mod32": "the bits a symbol consumed are taken modulo 32",
    "dc_clamp": "a DC predictor sum is clamped to 16 bits instead of wrapped",
    "no_reset": "the DC predictors are not reset at a restart marker",
}
# ("DC differences not wrapped to 16 bits" as plain unwrapped arithmetic cannot be told from the model in a 16-bit store: the
# predictor sum, the shift by Al and the store are all ring operations modulo 2^16.  The variant that CAN differ keeps the
# sum in range by clamping; that is the one held here.)


def new_census():
    return {"kind": "", "scan": None, "class": Counter(), "code_len": Counter(), "coef_bits": Counter(), "eobn_bits": Counter(),
            "size": Counter(), "sign": Counter(), "full": 0, "zrl_cross": 0, "zrl_last": 0, "behind": 0, "corr_outside": 0,
            "run_blocks": Counter(), "run_rows": 0, "run_bands": 0, "run_end_band": 0, "run_end_scan": 0, "run_overshoot": 0,
            "corr_sym_max": 0, "corr_blk_max": 0, "corr_bits": 0, "corr_ones": 0, "gap_max": 0, "gap_128": 0, "short_stretch": 0,
            "hist_max": 0, "hist_min": 64, "blocks": 0, "seg_blocks": Counter(), "dc_wrap": 0, "refused": ""}


def walk(raw: bytes, spec_refine: bool = False, wrong: Optional[str] = None, census: Optional[list] = None, upto: Optional[int] = None):
    """Every scan of the progressive file `raw` -> the coefficient store int16 [blocks, 64], zig-zag, blocks in the interleaved
    order of the final pass (MCU raster, component, block of the MCU).  Raises Refused where the reference raises.  `census`:
    a list that receives one new_census() per scan."""
    from pyjpegdecoder_amd._parse import parse_jpeg
    assert wrong is None or wrong in WRONG_VARIANTS
    p = parse_jpeg(raw)
    comps = list(p.color_components.values())
    order = {cid: i for i, cid in enumerate(p.color_components)}
    nc = len(comps)
    hs = [c.horizontal_sampling if nc > 1 else 1 for c in comps]
    vs = [c.vertical_sampling if nc > 1 else 1 for c in comps]
    hmax, vmax = max(hs), max(vs)
    mcus_x, mcus_y = -(-p.image_width // (8 * hmax)), -(-p.image_height // (8 * vmax))
    first = [sum(hs[j] * vs[j] for j in range(i)) for i in range(nc)]
    bpm = sum(h * v for h, v in zip(hs, vs))
    coef = np.zeros((mcus_x * mcus_y * bpm, 64), dtype=np.int64)

    def block(c, bx, by):
        return ((by // vs[c]) * mcus_x + bx // hs[c]) * bpm + first[c] + (by % vs[c]) * hs[c] + bx % hs[c]

    for scan in p.scans[:upto]:
        cs = new_census()
        cs["scan"] = ([order[c] for c in scan.component_ids], scan.spectral_start, scan.spectral_end, scan.bit_high, scan.bit_low)
        if census is not None:
            census.append(cs)
        try:
            _walk_scan(raw, scan, order, hs, vs, block, coef, spec_refine, wrong, cs)
        except Refused as exc:
            cs["refused"] = str(exc)
            raise
    return coef.astype(np.int16)


def _walk_scan(raw, scan, order, hs, vs, block, coef, spec, wrong, cs):
    rd = _Reader(raw, scan.entropy_start)
    ss, se, ah, al = scan.spectral_start, scan.spectral_end, scan.bit_high, scan.bit_low
    refining = ah != 0
    count, smh, ri = scan.mcu_count, scan.mcu_count_h, scan.restart_interval
    sc = [order[c] for c in scan.component_ids]
    nsc = len(sc)
    books = {d: _code_book(s) for d, s in scan.huffman.items()}
    seg_blocks = 0

    def consumed(total):                         # (wrong variant: a 5-bit "bits consumed" field)
        if wrong == "mod32" and total >= 32:
            rd.unget(32)

    if ss == 0:     # ------------------------------------------------------------------------------ DC scans (:974-1057)
        cs["kind"] = "dc_refine" if refining else "dc_first"
        pred = [0] * nsc
        m = 0
        while m < count:
            for i, c in enumerate(sc):
                h, v = (hs[c], vs[c]) if nsc > 1 else (1, 1)
                for r in range(h * v):
                    bx, by = ((m % smh) * h + r % h, (m // smh) * v + r // h) if nsc > 1 else (m % smh, m // smh)
                    blk = coef[block(c, bx, by)]
                    cs["blocks"] += 1
                    seg_blocks += 1
                    if refining:
                        blk[0] = _i16(int(blk[0]) | _i16(rd.get(1) << al))
                        cs["class"]["dc_bit"] += 1
                        continue
                    size, length = _symbol(rd, books[scan.huffman_tables_id[scan.component_ids[i]].dc & 3])
                    cs["class"]["dc"] += 1
                    cs["code_len"][length] += 1
                    cs["size"][size] += 1
                    cs["coef_bits"][(size, length + size)] += 1
                    diff = _extend(rd.get(size), size)
                    consumed(length + size)
                    total = diff + pred[i]
                    if total != _i16(total):
                        cs["dc_wrap"] += 1
                    pred[i] = max(-32768, min(32767, total)) if wrong == "dc_clamp" else _i16(total)
                    blk[0] = _i16(pred[i] << al)
            m += 1
            if ri > 0 and m % ri == 0 and m != count:
                rd.restart()
                cs["seg_blocks"][seg_blocks] += 1
                seg_blocks = 0
                if not refining and wrong != "no_reset":
                    pred = [0] * nsc
        cs["seg_blocks"][seg_blocks] += 1
        return

    # --------------------------------------------------------------------------------------------- AC scans (:1060-1298)
    cs["kind"] = "ac_refine" if refining else "ac_first"
    c = sc[0]
    book = books[(scan.huffman_tables_id[scan.component_ids[0]].ac & 3) | 0x10]
    rows_per_band = vs[c]                        # one MCU row per band launch (MJ_PROG_ROWS = 1)
    last_start = [None]                          # where the previous symbol started, in consumed bits
    stretch = [0]

    def symbol():
        at = rd.used
        if last_start[0] is not None:
            gap = at - last_start[0]
            cs["gap_max"] = max(cs["gap_max"], gap)
            cs["gap_128"] += gap >= 128
            stretch[0] = stretch[0] + gap if gap < 32 else 0
            cs["short_stretch"] = max(cs["short_stretch"], stretch[0])
        last_start[0] = at
        s, length = _symbol(rd, book)
        cs["code_len"][length] += 1
        return s, length

    def correct(blk, queue, per_block):
        n = len(queue)
        cs["corr_sym_max"] = max(cs["corr_sym_max"], n)
        per_block[0] += n
        for k in queue:
            bit = rd.get(1)
            cs["corr_bits"] += 1
            cs["corr_ones"] += bit
            cs["corr_outside"] += k > se
            v = int(blk[k])
            blk[k] = _i16(v + (-(bit << al) if v < 0 else (bit << al))) if spec else _i16(v | _i16(bit << al))
        queue.clear()

    def run_event(m0, length):
        end = m0 + length                        # the first block behind the run
        cs["run_blocks"][length] += 1
        lastb = min(end, count) - 1
        cs["run_rows"] = max(cs["run_rows"], lastb // smh - m0 // smh)
        cs["run_bands"] = max(cs["run_bands"], lastb // (smh * rows_per_band) - m0 // (smh * rows_per_band))
        cs["run_overshoot"] += end > count
        cs["run_end_scan"] += end == count
        cs["run_end_band"] += end < count and end % (smh * rows_per_band) == 0 and length > 1

    m = 0
    eob_run = 0
    while m < count:
        blk = coef[block(c, m % smh, m // smh)]
        cs["blocks"] += 1
        index = ss
        queue: List[int] = []
        per_block = [0]
        if refining:
            nh = int(np.count_nonzero(blk[ss:se + 1]))
            cs["hist_max"], cs["hist_min"] = max(cs["hist_max"], nh), min(cs["hist_min"], nh)
        m_raise = m
        while index <= se:
            hv, length = symbol()
            run, size = hv >> 4, hv & 15
            zero_run = 0
            if hv == 0:
                cs["class"]["eob0"] += 1
                cs["eobn_bits"][(0, length)] += 1
                eob_run = 1
                break
            elif hv == 0xF0:
                cs["class"]["zrl"] += 1
                zero_run = 16
            elif size == 0:
                extra = rd.get(run)
                consumed(length + run)
                cs["class"]["eobn"] += 1
                cs["eobn_bits"][(run, length + run)] += 1
                eob_run = (1 << run) + extra
                if wrong == "eob8":
                    eob_run &= 0xFF
                break
            else:
                cs["class"]["coef"] += 1
                cs["size"][size] += 1
                cs["coef_bits"][(size, length + size)] += 1
                zero_run = run
            if not refining:
                index += zero_run
            elif wrong == "zrl_nonzero" and hv == 0xF0:
                for _ in range(16):
                    if index > 63:
                        raise Refused("a zero run passes position 63")
                    if blk[index] != 0:
                        queue.append(index)
                    index += 1
            else:
                while zero_run > 0:
                    if index > 63 or (wrong == "run_se" and index > se):
                        raise Refused("a zero run passes position 63")
                    if blk[index] == 0:
                        zero_run -= 1
                    else:
                        queue.append(index)
                    index += 1
            if hv == 0xF0:
                cs["zrl_cross"] += index > se + 1
                cs["zrl_last"] += index == se + 1
            if size > 0:
                if wrong == "corr_front" and refining:
                    k = index                                            # what the value's own search will pass
                    ahead = list(queue)
                    while k <= 63 and blk[k] != 0:
                        ahead.append(k)
                        k += 1
                    correct(blk, ahead, per_block)
                    queue.clear()
                    value = _extend(rd.get(size), size)
                    if k > 63:
                        raise Refused("no zero left for a new coefficient")
                    index = k
                else:
                    value = _extend(rd.get(size), size)
                    consumed(length + size)
                    if index > 63:
                        raise Refused("a coefficient behind position 63")
                    if refining:
                        while blk[index] != 0:
                            queue.append(index)
                            index += 1
                            if index > 63:
                                raise Refused("no zero left for a new coefficient")
                if wrong == "sign" and refining:
                    value = -value
                if wrong == "run_se" and index > se:
                    pass
                else:
                    blk[index] = _i16(value << al)
                    cs["behind"] += index > se
                    cs["full"] += index == se
                    cs["sign"][1 if value > 0 else -1] += 1
                index += 1
            if refining:
                correct(blk, queue, per_block)
        if index > se:
            m += 1
        if wrong == "eob_self" and eob_run:
            eob_run += 1
        if eob_run:
            run_event(m_raise, eob_run)
        if not refining:
            m += eob_run
            eob_run = 0
        else:
            while eob_run > 0:
                if m >= count:
                    raise Refused("an end-of-band run passes the scan's last block in a refining scan")
                blk = coef[block(c, m % smh, m // smh)]
                if index == ss:                  # a block the run covers whole
                    cs["blocks"] += 1
                    nh = int(np.count_nonzero(blk[ss:se + 1]))
                    cs["hist_max"], cs["hist_min"] = max(cs["hist_max"], nh), min(cs["hist_min"], nh)
                    cs["corr_blk_max"] = max(cs["corr_blk_max"], per_block[0])
                    per_block = [0]
                if blk[index] != 0:
                    bit = rd.get(1)
                    cs["corr_bits"] += 1
                    cs["corr_ones"] += bit
                    per_block[0] += 1
                    v = int(blk[index])
                    blk[index] = _i16(v + (-(bit << al) if v < 0 else (bit << al))) if spec else _i16(v | _i16(bit << al))
                index += 1
                if index > se:
                    eob_run -= 1
                    m += 1
                    index = ss
        cs["corr_blk_max"] = max(cs["corr_blk_max"], per_block[0])
        if ri > 0 and m % ri == 0 and m != count:
            rd.restart()
            last_start[0] = None
            stretch[0] = 0


# ======================================================================================================================
# Stream items
# ======================================================================================================================
ZRL = ("ac", 0xF0)
EOB0 = ("ac", 0x00)


def ac(run: int, size: int, bits: int = 0):
    return ("ac", (run << 4) | size, bits)


def val(run: int, v: int):
    """(run, size of v) with v's value bits."""
    size = abs(v).bit_length()
    return ("ac", (run << 4) | size, v if v > 0 else v + (1 << size) - 1)


def eob(blocks: int):
    n = blocks.bit_length() - 1
    return ("ac", n << 4, blocks - (1 << n))


def bits(value: int, n: int):
    return ("bits", value, n)


def dc(i: int, diff: int):
    size = abs(diff).bit_length()
    return ("dc", i, size, diff if diff > 0 else diff + (1 << size) - 1)


def first_block(ss: int, se: int, values: Dict[int, int]) -> list:
    """The symbols of one block of a first scan: `values` = {zig-zag position: value}, ZRLs where a run needs them, EOB0 behind
    the last one unless it sits on Se."""
    out, k = [], ss
    for pos in sorted(values):
        r = pos - k
        while r > 15:
            out.append(ZRL)
            r -= 16
        out.append(val(r, values[pos]))
        k = pos + 1
    if k <= se:
        out.append(EOB0)
    return out


def refine_block(hist: set, ss: int, se: int, new: Dict[int, int], corr: Callable[[int], int] = lambda k: k & 1, end: bool = True) -> list:
    """The symbols of one block of a refining scan, conformant: `hist` = the positions earlier scans left non-zero (updated
    here), `new` = {position: +1 | -1} to place, corr(position) = the correction bit of a history coefficient.  With `end`
    the block closes with EOB0 and the corrections of the rest of the band, where anything of the band is left."""
    out, queue, zeros, k = [], [], 0, ss
    last = max(new) if new else ss - 1
    while k <= last:
        if k in hist:
            queue.append(k)
        elif k in new:
            out.append(ac(zeros, 1, 1 if new[k] > 0 else 0))
            out += [bits(corr(q), 1) for q in queue]
            queue, zeros = [], 0
        else:
            zeros += 1
            if zeros == 16:
                # (a ZRL ends on its sixteenth zero: nothing behind it is queued yet)
                out.append(ZRL)
                out += [bits(corr(q), 1) for q in queue]
                queue, zeros = [], 0
        k += 1
    hist |= set(new)
    if end and last < se:
        out.append(EOB0)
        out += [bits(corr(q), 1) for q in range(last + 1, se + 1) if q in hist]
    return out


# ======================================================================================================================
# Rows
# ======================================================================================================================
GREY = ((1, 1),)
DC_STD = (_T["STD_DC_LUMA_BITS"], _T["STD_DC_LUMA_VALS"])
DC_STD_C = (_T["STD_DC_CHROMA_BITS"], _T["STD_DC_CHROMA_VALS"])
DC_TABLES = [DC_STD, long_dc_table(), DC_STD_C]
AC_TABLES = [long_ac_table(0), long_ac_table(1), long_ac_table(2), _ac_prog_table(0)]     # (3: every (run, size <= 10), 3..14 bits)


def grey(width, height, scans, dc_zero=True, ri=0):
    """A greyscale file: an all-zero DC scan (unless the row brings its own), then `scans` = (Ss, Se, Ah, Al, AC table, items)."""
    n = -(-width // 8) * -(-height // 8)
    full = []
    if dc_zero:
        items = []
        for b in range(n):
            items.append(("dc", 0, 0))
            if ri and (b + 1) % ri == 0 and b + 1 != n:
                items.append(("rst",))
        full.append(((0,), 0, 0, 0, 0, [(0, 0)], items))
    for sc in scans:
        if len(sc) == 7:
            full.append(sc)
        else:
            ss, se, ah, al, t, items = sc
            full.append(((0,), ss, se, ah, al, [(0, t)], items))
    return craft_progressive_symbols(width, height, GREY, full, dc_tables=DC_TABLES, ac_tables=AC_TABLES, restart_interval=ri)


def _flat(blocks):
    return [it for b in blocks for it in b]


# ---- first AC scans ------------------------------------------------------------------------------------------------------
def f_full():
    return grey(16, 8, [
        (1, 5, 0, 0, 0, _flat([first_block(1, 5, {1: 3, 5: 1}), [ac(4, 1, 1)]])),
        (6, 6, 0, 1, 0, _flat([[ac(0, 2, 3)], [EOB0]])),                                  # Ss == Se
        (7, 63, 0, 0, 0, _flat([[ZRL, ZRL, ZRL, ac(8, 1, 1)], [EOB0]])),                  # the full band ends at 63
    ])


def f_zrl():
    return grey(24, 8, [
        (1, 40, 0, 0, 0, _flat([[ZRL, ac(0, 1, 1), EOB0], [ZRL, ZRL, ZRL], [ac(0, 1, 0), EOB0]])),    # 4-bit ZRLs; 1 + 48 crosses Se = 40
        (41, 52, 0, 1, 1, _flat([[ac(1, 1, 1), ZRL], [ZRL], [EOB0]])),                    # 12-bit ZRLs that cross Se
        (53, 63, 0, 0, 2, _flat([[ZRL], [ac(0, 1, 1), ZRL], [EOB0]])),                    # 16-bit ZRLs
    ])


def f_long():
    return grey(32, 8, [(1, 63, 0, 0, 0, _flat([
        [ac(3, 1, 1), ac(4, 1, 0), ac(0, 11, 0x7FF), ac(1, 2, 2), EOB0],                  # 11, 12, 12, 12-bit codes
        [ac(5, 1, 1), ac(0, 12, 0x800), ac(0, 13, 0x1FFF), ac(1, 10, 0x155), ac(0, 13, 0), EOB0],     # 15-bit codes
        [ac(6, 1, 0), ac(0, 14, 0x2AAA), ac(0, 15, 0x7FFF), ac(0, 15, 1), ac(0, 14, 0x1555), EOB0],   # 16-bit codes; 16 + 15 = 31
        [ac(15, 2, 1), ac(0, 12, 0x7FF), EOB0]]))])


def f_eobn():
    return grey(64, 64, [(1, 63, 0, 0, 0, _flat([
        [EOB0], [eob(2)], [ac(0, 1, 1), eob(5)], [eob(8)], [ac(2, 2, 1), eob(16)], [eob(32)]]))])
    # EOB0; 5+1, 6+2, 7+3 bits inside the table; 8+4 = 12 and 8+5 = 13 behind it


def f_run_rows_1():
    return grey(8, 64, [(1, 63, 0, 0, 0, _flat([[ac(0, 1, 1), eob(3)], [eob(4)], [ac(0, 1, 1), EOB0]]))])


def f_run_rows_3():
    return grey(24, 40, [(1, 63, 0, 0, 0, _flat([[eob(7)], [ac(0, 1, 0), eob(8)]]))])


def f_run_bands():
    return grey(16, 64, [(1, 63, 0, 0, 0, _flat([[ac(0, 1, 1), eob(6)], [eob(9)], [ac(0, 1, 1), EOB0]]))])


def f_run_over():
    return grey(16, 64, [(1, 63, 0, 0, 0, _flat([[eob(8)], [ac(1, 1, 1), eob(100)]]))])


def f_run_big_1024():
    runs = [256, 512, 1024, 2048, 4096, 8192]
    blocks = [[ac(0, 1, 1), eob(r + 1)] for r in runs]                                    # the coded block counts as the run's first
    left = 128 * 128 - sum(r + 1 for r in runs)
    return grey(1024, 1024, [(1, 63, 0, 0, 0, _flat(blocks + [[ac(0, 2, 3), eob(left)]]))])


def f_run_big_2048():
    return grey(2048, 1024, [(1, 63, 0, 0, 0, _flat([[ac(0, 1, 1), EOB0], [eob(32767)]]))])   # 16 + 14 bits


def f_behind():
    return grey(16, 8, [(1, 10, 0, 0, 0, _flat([[ac(1, 1, 1), ac(14, 1, 1)], [EOB0]]))])      # 3 + 14 = 17 > Se: placed


def f_behind_63():
    return grey(16, 8, [(50, 60, 0, 0, 0, _flat([[ac(15, 1, 1)], [EOB0]]))])                  # 65: refused


def f_nocode():
    return grey(16, 8, [(1, 63, 0, 0, 0, [ac(0, 1, 1), bits(0xFFFF, 16), bits(0xFFFF, 16), EOB0, EOB0])])


def f_ff():
    blk = [ac(0, 15, 0x7FFF) if k & 1 else ac(0, 10, 0x3FF) for k in range(1, 64)]
    return grey(32, 16, [(1, 63, 0, 0, 0, blk * 8)])


def _colour_dc(factors, mcus):
    items = []
    for _ in range(mcus):
        for i, (h, v) in enumerate(factors):
            items += [("dc", i, 0)] * (h * v)
    return ((0, 1, 2), 0, 0, 0, 0, [(0, 0), (2, 0), (2, 0)], items)


def f_410():
    f = ((4, 2), (1, 1), (1, 1))
    luma = _flat([[ac(0, 2, 3), EOB0], [eob(10)], [ac(2, 1, 1), EOB0], [eob(20)]])
    return craft_progressive_symbols(64, 32, f, [_colour_dc(f, 4), ((0,), 1, 63, 0, 0, [(0, 0)], luma)], dc_tables=DC_TABLES, ac_tables=AC_TABLES)


def f_3x():
    f = ((3, 1), (1, 1), (1, 1))
    luma = _flat([[ac(0, 2, 3), EOB0], [eob(6)], [ac(2, 1, 1), ZRL, ac(0, 12, 0xABC), EOB0], [eob(4)]])
    return craft_progressive_symbols(48, 16, f, [_colour_dc(f, 4), ((0,), 1, 63, 0, 0, [(0, 0)], luma)], dc_tables=DC_TABLES, ac_tables=AC_TABLES)


# ---- refining AC scans ---------------------------------------------------------------------------------------------------
def _ones(k):
    return 1


def r_zrl():
    h0, h1 = {5: 1, 30: -1}, {k: (1 if k & 1 else -1) for k in range(1, 9)}
    first = _flat([first_block(1, 40, h0), first_block(1, 40, h1), [EOB0]])
    s0, s1 = set(h0), set(h1)
    b0 = refine_block(s0, 1, 40, {40: 1}, end=False)                  # two ZRLs with zeros left, then the band's last position
    b1 = [ZRL] + [bits(k & 1, 1) for k in range(1, 9)] + [ZRL]          # 32 zeros at 9..40: the second ZRL uses the band's last
    return grey(24, 8, [(1, 40, 0, 1, 0, first), (1, 40, 1, 0, 0, _flat([b0, b1, [EOB0]]))])


def r_zrl_behind():
    first = _flat([first_block(1, 20, {3: 1}), [EOB0]])
    return grey(16, 8, [(1, 20, 0, 1, 0, first), (1, 20, 1, 0, 0, _flat([[ZRL, bits(1, 1), ac(0, 1, 1), ZRL], [EOB0]]))])   # 16th zero at 34


def r_zrl_none():
    return grey(16, 8, [(50, 63, 0, 1, 0, [eob(2)]), (50, 63, 1, 0, 0, [ZRL, EOB0, EOB0])])       # 14 zeros left: refused


def r_lut():
    h = {2: 1, 40: -1}
    first = _flat([first_block(1, 63, h)] * 4)
    ref1 = _flat([[ac(0, 1, 1), ac(10, 1, 0), bits(1, 1), ac(11, 1, 1), EOB0],            # 11, 11 and 12-bit codes (table 1)
                  [ac(12, 1, 1), bits(0, 1), ac(13, 1, 0), EOB0],                         # 15 and 16 bits
                  [ac(1, 1, 1), bits(1, 1), ac(1, 1, 0), ac(2, 1, 1), ac(3, 1, 0), ac(4, 1, 1), ac(5, 1, 0), ac(6, 1, 1)],   # 2..7 bits
                  [ac(7, 1, 1), bits(1, 1), ac(8, 1, 0), ac(9, 1, 1), EOB0]])             # 8, 9, 10 bits: 10 + 1 = 11 just fits
    ref2 = _flat([[ac(0, 1, 1), ac(1, 1, 0), ac(2, 1, 1), EOB0, bits(1, 1)],              # table 0: (0, 1) in 3 bits, 4 and 5
                  [ac(3, 1, 1), EOB0, bits(0, 1)],                                        # an 11-bit code: 12 bits, "look again"
                  [ac(4, 1, 1), ac(5, 1, 0), bits(1, 1), ac(6, 1, 1), EOB0],              # 12, 15, 16 bits
                  [ac(7, 1, 0), EOB0, bits(1, 1)]])
    return grey(32, 8, [(1, 63, 0, 1, 0, first), (1, 30, 1, 0, 1, ref1), (31, 63, 1, 0, 0, ref2)])


def r_lut16():
    first = _flat([first_block(1, 63, {4: 1})] * 2)
    ref = _flat([[ac(0, 1, 1), ac(0, 1, 0), ac(1, 1, 1), bits(1, 1), ac(15, 1, 0), EOB0], [ZRL, bits(0, 1), ac(2, 1, 1), eob(1)]])
    return grey(16, 8, [(1, 63, 0, 1, 0, first), (1, 63, 1, 0, 2, ref)])                  # table 2: (0, 1), ZRL, (15, 1) at 16 bits


def _levels(first_al):
    """first scan at Al = first_al, then one refining scan per level down to 0; every refining scan places coefficients of
    both signs, which the next one corrects."""
    hist = [{3: 5, 9: -3, 20: 1}, {1: -1, 2: 2, 63: -7}, {}, {10: 4}]
    scans = [(1, 63, 0, first_al, 3, _flat([first_block(1, 63, h) for h in hist]))]
    sets = [set(h) for h in hist]
    for lvl in range(first_al - 1, -1, -1):
        new = [{4 + lvl: 1, 30 + 3 * lvl: -1}, {5 + lvl: -1, 40: 1} if lvl == 1 else {6 + lvl: 1}, {1 + lvl: -1, 62 - lvl: 1}, {}]
        new = [{k: v for k, v in n.items() if k not in s} for n, s in zip(new, sets)]
        scans.append((1, 63, lvl + 1, lvl, 3, _flat([refine_block(s, 1, 63, n, corr=lambda k, l=lvl: (k + l) & 1) for s, n in zip(sets, new)])))
    return grey(32, 8, scans)


def r_sign():
    return _levels(3)


def r_levels():
    return _levels(2)


def r_size():
    first = _flat([first_block(1, 63, {2: 1}), [EOB0]])
    ref = _flat([[ac(0, 2, 3), ac(1, 10, 0x2AB), bits(1, 1), ac(0, 2, 0), EOB0], [ac(1, 10, 0x155), EOB0]])
    return grey(16, 8, [(1, 63, 0, 1, 0, first), (1, 63, 1, 0, 0, ref)])


def r_eob():
    h = {2: 1, 7: -1, 33: 1}
    first = _flat([first_block(1, 63, h)] * 16)
    sets = [set(h) for _ in range(16)]
    b0 = refine_block(sets[0], 1, 63, {5: -1})                        # EOB0 mid-block, corrections for the rest of the band
    b1 = [EOB0] + [bits(1, 1), bits(0, 1), bits(1, 1)]                # EOB0 at block start
    run1 = [eob(4)] + [bits(b, 1) for b in (1, 1, 0) * 4]             # blocks 2..5: ends on a band's last block
    run2 = [eob(10)] + [bits(b, 1) for b in (0, 1, 1) * 10]           # blocks 6..15: over five bands to the scan's end
    return grey(16, 64, [(1, 63, 0, 1, 0, first), (1, 63, 1, 0, 0, _flat([b0, b1, run1, run2]))])


def r_run_over():
    h = {2: 1, 7: -1}
    first = _flat([first_block(1, 63, h)] * 4)
    b0 = refine_block(set(h), 1, 63, {5: 1})                          # a block of its own first: the run is raised mid-scan
    run = [eob(9)] + [bits(b, 1) for b in (1, 0) * 3]                 # blocks 1..3 (over a band's end) and six more the scan has not
    return grey(16, 16, [(1, 63, 0, 1, 0, first), (1, 63, 1, 0, 0, _flat([b0, run]))])


def r_hist():
    full = {k: (1 if k % 3 else -1) for k in range(1, 64)}
    h62 = {k: (1 if k & 1 else -1) for k in range(1, 63)}
    h50 = {k: (-1 if k % 5 else 1) for k in range(1, 51)}
    hist = [full, {}, h62, h50, h50, h50, {7: 1}]
    first = _flat([first_block(1, 63, h) if h else [EOB0] for h in hist])
    b0 = [EOB0] + [bits(1, 1)] * 63                                   # the whole band is history: correction bits all ones
    b1 = [EOB0]                                                       # no history
    b2 = [ac(0, 1, 0)] + [bits(k & 1, 1) for k in range(62)]          # one symbol passes 62 corrections and fills the band
    run = [eob(3)] + [bits((k * 7 >> 2) & 1, 1) for k in range(150)]  # 150 correction bits in front of the next symbol
    b6 = [ac(2, 1, 1), EOB0, bits(1, 1)]
    return grey(56, 8, [(1, 63, 0, 1, 0, first), (1, 63, 1, 0, 0, _flat([b0, b1, b2, run, b6]))])


def r_behind():
    first_lo = _flat([first_block(1, 10, {2: 1}), [EOB0]])
    first_hi = _flat([first_block(11, 63, {11: 2, 12: -2}), [EOB0]])
    # ten zeros from 1: 1, 3..10 and — past 11 and 12, which are history outside the band — 13; the coefficient lands on 14
    ref = _flat([[ac(10, 1, 1), bits(1, 1), bits(1, 1), bits(1, 1)], [EOB0]])
    return grey(16, 8, [(1, 10, 0, 1, 0, first_lo), (11, 63, 0, 0, 0, first_hi), (1, 10, 1, 0, 0, ref)])


def r_behind_63():
    return grey(16, 8, [(50, 55, 0, 1, 0, [eob(2)]), (50, 55, 1, 0, 0, [ac(15, 1, 1), EOB0, EOB0])])   # needs 15 zeros, has 14


# ---- DC scans ------------------------------------------------------------------------------------------------------------
_D_LONG = [32767, 2049, -4097, 8200, -513, 1025, -32767, 16384]       # sizes 15, 12, 13, 14, 10, 11, 15, 15: the sum wraps twice


def d_long():
    return grey(64, 8, [((0,), 0, 0, 0, 0, [(1, 0)], [dc(0, d) for d in _D_LONG])], dc_zero=False)


def d_long_al():
    return grey(64, 8, [((0,), 0, 0, 0, 2, [(1, 0)], [dc(0, d) for d in _D_LONG]),
                        ((0,), 0, 0, 2, 1, [(1, 0)], [bits(0b10110010, 8)])], dc_zero=False)


def d_long_16():
    return grey(32, 8, [((0,), 0, 0, 0, 0, [(1, 0)], [dc(0, 5), dc(0, 40000), dc(0, -65535), dc(0, 65535)])], dc_zero=False)   # 16 + 16 = 32


def d_none():
    return grey(32, 8, [((0,), 0, 0, 0, 0, [(1, 0)], [dc(0, 5), bits(0xFFFF, 16), bits(0xFFFF, 16), dc(0, 1), dc(0, 1)])], dc_zero=False)


def _lcg_diffs(n, seed):
    out, x = [], seed
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        size = (x >> 8) % 12
        mag = ((x >> 12) % (1 << size)) | (1 << size) >> 1 if size else 0
        out.append(mag if x & 0x40 else -mag)
    return out


def _d_groups(ri):
    f = ((1, 1), (1, 1), (1, 1))
    n = 49                                                             # 56 x 56: 147 and 98 blocks in the two interleaved scans
    d = _lcg_diffs(5 * n, 77 + ri)

    def scan(comps, tabs, al, base):
        items, k = [], base
        for m in range(n):
            for i in range(len(comps)):
                items.append(dc(i, d[k] >> 3 if tabs[i][0] != 1 else d[k]))           # (the Annex-K tables end at size 11)
                k += 1
            if ri and (m + 1) % ri == 0 and m + 1 != n:
                items.append(("rst",))
        return (comps, 0, 0, 0, al, tabs, items)
    s3 = scan((0, 1, 2), [(1, 0), (0, 0), (2, 0)], 0, 0)
    scans = [s3] if ri else [scan((0, 2), [(1, 0), (2, 0)], 1, 0), scan((1,), [(0, 0)], 0, 2 * n),
                             ((0, 2), 0, 0, 1, 0, [(1, 0), (2, 0)], [bits((m * 5 >> 1) & 1, 1) for m in range(2 * n)])]
    return craft_progressive_symbols(56, 56, f, scans, dc_tables=DC_TABLES, ac_tables=AC_TABLES, restart_interval=ri)


def d_groups_3():
    f = ((1, 1), (1, 1), (1, 1))
    d = _lcg_diffs(147, 5)
    items = [dc(i, d[3 * m + i] if i == 0 else d[3 * m + i] >> 3) for m in range(49) for i in range(3)]
    return craft_progressive_symbols(56, 56, f, [((0, 1, 2), 0, 0, 0, 0, [(1, 0), (0, 0), (2, 0)], items)], dc_tables=DC_TABLES, ac_tables=AC_TABLES)


def d_groups_2():
    return _d_groups(0)


def d_groups_dri():
    return _d_groups(5)


def d_refine():
    d = _lcg_diffs(64, 9)
    ri, n = 45, 64

    def with_rst(items):
        out = []
        for b, it in enumerate(items):
            out.append(it)
            if (b + 1) % ri == 0 and b + 1 != n:
                out.append(("rst",))
        return out
    return grey(64, 64, [((0,), 0, 0, 0, 2, [(1, 0)], with_rst([dc(0, v) for v in d])),
                         ((0,), 0, 0, 2, 1, [(1, 0)], with_rst([bits((b * 3 >> 1) & 1, 1) for b in range(n)])),
                         ((0,), 0, 0, 1, 0, [(1, 0)], with_rst([bits((b * 5 >> 2) & 1, 1) for b in range(n)]))], dc_zero=False, ri=ri)


# ---- the table ----------------------------------------------------------------------------------------------------------------
def _scans(cs, kind):
    return [c for c in cs if c["kind"] == kind]


def _any(cs, kind, pred):
    return any(pred(c) for c in _scans(cs, kind))


class Row(NamedTuple):
    name: str
    make: Callable[[], bytes]
    reached: Callable[[list], bool]      # the census of the model walk -> the row reaches its path
    refused: bool = False                # the reference raises on this file
    wrong: tuple = ()                    # the wrong variants this row must tell from the model
    big: bool = False
    conformant: bool = True              # False: a first AC scan holds what no encoder writes (the chunked walks may hand it back)


F, R, D = "ac_first", "ac_refine", "dc_first"
ROWS = [
    Row("F-full", f_full, lambda cs: all(c["full"] >= 1 for c in _scans(cs, F)) and any(c["scan"][1] == c["scan"][2] for c in _scans(cs, F))),
    Row("F-zrl", f_zrl, lambda cs: _any(cs, F, lambda c: c["class"]["zrl"] and c["code_len"][4] and c["zrl_cross"])
        and _any(cs, F, lambda c: c["class"]["zrl"] and c["code_len"][12]) and _any(cs, F, lambda c: c["class"]["zrl"] and c["code_len"][16]), conformant=False),
    Row("F-long", f_long, lambda cs: _any(cs, F, lambda c: all(c["code_len"][l] for l in (11, 12, 15, 16)) and c["coef_bits"][(15, 31)]
                                          and all(c["size"][s] for s in (11, 12, 13, 14, 15)))),
    Row("F-eobn", f_eobn, lambda cs: _any(cs, F, lambda c: c["class"]["eob0"] and any(0 < n and b <= K_LUT_BITS for n, b in c["eobn_bits"])
                                          and any(n and b > K_LUT_BITS for n, b in c["eobn_bits"])), wrong=("eob_self",)),
    Row("F-run-rows-1", f_run_rows_1, lambda cs: _any(cs, F, lambda c: c["run_rows"] >= 2)),
    Row("F-run-rows-3", f_run_rows_3, lambda cs: _any(cs, F, lambda c: c["run_rows"] >= 2)),
    Row("F-run-bands", f_run_bands, lambda cs: _any(cs, F, lambda c: c["run_bands"] >= 3 and c["run_end_band"] and c["run_end_scan"])),
    Row("F-run-over", f_run_over, lambda cs: _any(cs, F, lambda c: c["run_overshoot"]), conformant=False),
    Row("F-run-big-1024", f_run_big_1024, lambda cs: _any(cs, F, lambda c: all(c["run_blocks"][r + 1] for r in (256, 512, 1024, 2048, 4096, 8192))),
        wrong=("eob8",), big=True),
    Row("F-run-big-2048", f_run_big_2048, lambda cs: _any(cs, F, lambda c: c["run_blocks"][32767] and c["eobn_bits"][(14, 30)]), big=True),
    Row("F-behind", f_behind, lambda cs: _any(cs, F, lambda c: c["behind"] == 1), wrong=("run_se",), conformant=False),
    Row("F-behind-63", f_behind_63, lambda cs: _any(cs, F, lambda c: "behind position 63" in c["refused"]), refused=True),
    Row("F-nocode", f_nocode, lambda cs: _any(cs, F, lambda c: "no code" in c["refused"]), refused=True),
    Row("F-ff", f_ff, lambda cs: _any(cs, F, lambda c: c["full"] == 8 and c["size"][15] > 200 and c["short_stretch"] >= 65)),
    Row("F-410", f_410, lambda cs: _any(cs, F, lambda c: c["run_rows"] >= 1)),
    Row("F-3x", f_3x, lambda cs: _any(cs, F, lambda c: c["run_rows"] >= 1 and c["size"][12])),
    Row("R-zrl", r_zrl, lambda cs: _any(cs, R, lambda c: c["class"]["zrl"] >= 4 and c["zrl_last"] and c["full"])),
    Row("R-zrl-behind", r_zrl_behind, lambda cs: _any(cs, R, lambda c: c["zrl_cross"]), wrong=("zrl_nonzero",)),
    Row("R-zrl-none", r_zrl_none, lambda cs: _any(cs, R, lambda c: "passes position 63" in c["refused"]), refused=True),
    Row("R-lut", r_lut, lambda cs: _any(cs, R, lambda c: all(c["coef_bits"][(1, l + 1)] for l in (2, 10, 11, 12, 15, 16)))
        and _any(cs, R, lambda c: all(c["coef_bits"][(1, l + 1)] for l in (3, 11, 12, 15, 16))), wrong=("corr_front",)),
    Row("R-lut16", r_lut16, lambda cs: _any(cs, R, lambda c: c["coef_bits"][(1, 17)] >= 3 and c["code_len"][16] >= 4)),
    Row("R-sign", r_sign, lambda cs: all(any(c["scan"][4] == al and c["sign"][1] and c["sign"][-1] for c in _scans(cs, R)) for al in (0, 1, 2)),
        wrong=("sign",)),
    Row("R-levels", r_levels, lambda cs: [c["scan"][3:] for c in _scans(cs, R)] == [(2, 1), (1, 0)] and _scans(cs, R)[1]["hist_max"] >= 5),
    Row("R-size", r_size, lambda cs: _any(cs, R, lambda c: c["size"][2] and c["size"][10])),
    Row("R-eob", r_eob, lambda cs: _any(cs, R, lambda c: c["class"]["eob0"] >= 2 and c["class"]["eobn"] >= 2 and c["run_bands"] >= 4
                                        and c["run_end_band"] and c["run_end_scan"])),
    Row("R-run-over", r_run_over, lambda cs: _any(cs, R, lambda c: c["run_overshoot"] and c["run_bands"] >= 1
                                                  and "passes the scan's last block" in c["refused"]), refused=True),
    Row("R-hist", r_hist, lambda cs: _any(cs, R, lambda c: c["hist_max"] == 63 and c["hist_min"] == 0 and c["corr_sym_max"] >= 62
                                          and c["gap_128"] >= 1 and c["corr_blk_max"] == 63)),
    Row("R-behind", r_behind, lambda cs: _any(cs, R, lambda c: c["behind"] == 1 and c["corr_outside"] == 2), wrong=("run_se",)),
    Row("R-behind-63", r_behind_63, lambda cs: _any(cs, R, lambda c: "passes position 63" in c["refused"]), refused=True),
    Row("D-long", d_long, lambda cs: _any(cs, D, lambda c: all(c["code_len"][l] for l in range(10, 16)) and c["dc_wrap"] >= 2 and c["scan"][4] == 0),
        wrong=("dc_clamp",)),
    Row("D-long-al", d_long_al, lambda cs: _any(cs, D, lambda c: c["dc_wrap"] >= 2 and c["scan"][4] == 2)),
    Row("D-none", d_none, lambda cs: _any(cs, D, lambda c: "no code" in c["refused"]), refused=True),
    Row("D-groups-3", d_groups_3, lambda cs: _any(cs, D, lambda c: len(c["scan"][0]) == 3 and c["blocks"] == 147)),
    Row("D-groups-2", d_groups_2, lambda cs: _any(cs, D, lambda c: len(c["scan"][0]) == 2 and c["blocks"] == 98)),
    Row("D-groups-dri", d_groups_dri, lambda cs: _any(cs, D, lambda c: c["seg_blocks"][15] == 9 and c["seg_blocks"][12] == 1), wrong=("no_reset",)),
    Row("D-refine", d_refine, lambda cs: len(_scans(cs, "dc_refine")) == 2 and all(c["seg_blocks"][45] for c in _scans(cs, "dc_refine"))),
]
# Not a row: the reference adds a DC difference of size 16 to its int16 predictor as a Python integer, which its array library
# refuses as out of bounds (an OverflowError of NumPy's, not a rule of the format), so there is no reference result to commit.
# The file is kept for the one 32-bit symbol a stream can hold (16-bit code + 16 value bits): the model against the oracle and
# against the "mod32" variant on the host, the library against the oracle on the GPU.
EXTRA = [Row("D-long-16", d_long_16, lambda cs: _any(cs, D, lambda c: c["coef_bits"][(16, 32)] >= 3), wrong=("mod32",))]
ROW = {r.name: r for r in ROWS + EXTRA}

_made: Dict[str, bytes] = {}


def row_bytes(name: str) -> bytes:
    if name not in _made:
        _made[name] = ROW[name].make()
    return _made[name]


def census_line(name: str, cs: list) -> str:
    """One line per scan: the counts that the rows' thresholds are written in."""
    out = []
    for c in cs:
        comps, ss, se, ah, al = c["scan"]
        if c["kind"].startswith("dc"):
            out.append(f"{name} {c['kind']} c{comps} Ah{ah} Al{al}: blocks {c['blocks']} codes>{K_DC_LUT_BITS}b {sum(n for l, n in c['code_len'].items() if l > K_DC_LUT_BITS)}"
                       f" max_size {max(c['size'], default=0)} max_bits {max((b for _, b in c['coef_bits']), default=0)} wraps {c['dc_wrap']}"
                       f" seg_blocks_max {max(c['seg_blocks'], default=0)}")
            continue
        eobn = sorted({n for n, _ in c["eobn_bits"]})
        out.append(f"{name} {c['kind']} {ss}-{se} Ah{ah} Al{al}: " + " ".join(f"{k} {c['class'][k]}" for k in ("coef", "zrl", "eob0", "eobn"))
                   + f" codes>{K_LUT_BITS}b {sum(n for l, n in c['code_len'].items() if l > K_LUT_BITS)} max_code {max(c['code_len'], default=0)}"
                   f" max_size {max(c['size'], default=0)} max_bits {max([b for _, b in c['coef_bits']] + [b for _, b in c['eobn_bits']], default=0)}"
                   f" eobn {eobn} run_max {max(c['run_blocks'], default=0)} rows {c['run_rows']} bands {c['run_bands']}"
                   f" end_band {c['run_end_band']} end_scan {c['run_end_scan']} over {c['run_overshoot']} full {c['full']}"
                   f" zrl_cross {c['zrl_cross']} behind {c['behind']} corr_sym {c['corr_sym_max']} corr_blk {c['corr_blk_max']}"
                   f" corr_out {c['corr_outside']} gap_max {c['gap_max']} gap128 {c['gap_128']} short_stretch {c['short_stretch']}"
                   f" hist {c['hist_min'] if c['kind'] == 'ac_refine' else 0}..{c['hist_max']}" + (f" REFUSED: {c['refused']}" if c["refused"] else ""))
    return "\n".join(out)


# ---- what a set of inputs reaches, event by event (profiles/prog_paths_census.txt) -------------------------------------------
EVENTS = ["ac_codes_12_16", "ac_codes_15_16", "ac_sizes_11_15", "ac_symbol_bits_max", "dc_codes_10_16", "dc_size_max", "dc_symbol_bits_max",
          "eobn_max_n", "eobn_behind_table", "run_blocks_max", "run_rows_max", "run_bands_max", "run_ends_on_band", "run_ends_scan",
          "run_overshoots", "band_full", "zrl", "zrl_crosses_se", "placed_behind_se", "corrections_behind_se",
          "refine_size_above_1", "refine_symbols_12_bits_up", "corrections_per_symbol_max", "corrections_per_block_max", "gap_bits_max",
          "gaps_128_up", "short_stretch_bits_max", "history_max", "dc_sum_wraps", "dc_segment_blocks_max", "refused_scans"]
_MAXED = {e for e in EVENTS if e.endswith("_max") or e == "eobn_max_n"}


def summary(cs: list) -> Dict[str, int]:
    """The census of one file (a list of scans) as the events of EVENTS: counts summed over the scans, extremes as maxima."""
    out = dict.fromkeys(EVENTS, 0)

    def put(key, v):
        out[key] = max(out[key], int(v)) if key in _MAXED else out[key] + int(v)
    for c in cs:
        put("refused_scans", bool(c["refused"]))
        if c["kind"].startswith("dc"):
            put("dc_codes_10_16", sum(n for l, n in c["code_len"].items() if l > K_DC_LUT_BITS))
            put("dc_size_max", max(c["size"], default=0))
            put("dc_symbol_bits_max", max((b for _, b in c["coef_bits"]), default=0))
            put("dc_sum_wraps", c["dc_wrap"])
            put("dc_segment_blocks_max", max(c["seg_blocks"], default=0))
            continue
        refining = c["kind"] == "ac_refine"
        put("ac_codes_12_16", sum(n for l, n in c["code_len"].items() if l > K_LUT_BITS))
        put("ac_codes_15_16", sum(n for l, n in c["code_len"].items() if l >= 15))
        put("ac_sizes_11_15", sum(n for s, n in c["size"].items() if s > 10))
        put("ac_symbol_bits_max", max([b for _, b in c["coef_bits"]] + [b for _, b in c["eobn_bits"]], default=0))
        put("eobn_max_n", max((n for n, _ in c["eobn_bits"]), default=0))
        put("eobn_behind_table", sum(k for (n, b), k in c["eobn_bits"].items() if b > K_LUT_BITS))
        put("run_blocks_max", max(c["run_blocks"], default=0))
        put("run_rows_max", c["run_rows"])
        put("run_bands_max", c["run_bands"])
        put("run_ends_on_band", c["run_end_band"])
        put("run_ends_scan", c["run_end_scan"])
        put("run_overshoots", c["run_overshoot"])
        put("band_full", c["full"])
        put("zrl", c["class"]["zrl"])
        put("zrl_crosses_se", c["zrl_cross"])
        put("placed_behind_se", c["behind"])
        put("corrections_behind_se", c["corr_outside"])
        put("refine_size_above_1", sum(n for s, n in c["size"].items() if s > 1) if refining else 0)
        put("refine_symbols_12_bits_up", sum(k for (s, b), k in c["coef_bits"].items() if b >= 12) if refining else 0)
        put("corrections_per_symbol_max", c["corr_sym_max"])
        put("corrections_per_block_max", c["corr_blk_max"])
        put("gap_bits_max", c["gap_max"])
        put("gaps_128_up", c["gap_128"])
        put("short_stretch_bits_max", c["short_stretch"])
        put("history_max", c["hist_max"])
    return out


def walk_census(raw: bytes) -> list:
    cs: list = []
    try:
        walk(raw, census=cs)
    except Refused:
        pass
    return cs
