"""Write baseline JPEG files symbol by symbol, with ANY per-component sampling factors — test inputs for layouts no
encoder at hand produces (4:1:0, 1x4, luma below the chroma resolution, factors of 3 ...).

The coefficients are random (the decoders under test do not care what the picture shows) unless craft_baseline is handed
the blocks to write (tests/stage2_families.py: coefficients chosen against the fast stage 2's rare paths); the Huffman
and, by default, the quantisation tables are the Annex-K ones of tools/std_tables.h.  Input-generation tooling only;
nothing here is on the decode path."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent


def _std_tables():
    txt = (_HERE / "std_tables.h").read_text()
    out = {}
    for name, body in re.findall(r"(STD_\w+)\[\d+\]\s*=\s*\{([^}]*)\}", txt):
        out[name] = bytes(int(t, 16) for t in re.findall(r"0x([0-9a-fA-F]{2})", body))
    return out


_T = _std_tables()


def _codes(bits: bytes, vals: bytes):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            k += 1
            code += 1
        code <<= 1
    return out


_DC = [_codes(_T["STD_DC_LUMA_BITS"], _T["STD_DC_LUMA_VALS"]), _codes(_T["STD_DC_CHROMA_BITS"], _T["STD_DC_CHROMA_VALS"])]
_AC = [_codes(_T["STD_AC_LUMA_BITS"], _T["STD_AC_LUMA_VALS"]), _codes(_T["STD_AC_CHROMA_BITS"], _T["STD_AC_CHROMA_VALS"])]


def _seg(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value: int, length: int):
        self.acc = (self.acc << length) | (value & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0x00)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _category(v: int) -> int:
    return int(abs(v)).bit_length()


def _value_bits(v: int, size: int) -> int:
    return v if v >= 0 else v + (1 << size) - 1


def random_block(rng, density: float, max_size: int, dc_size: int):
    """64 zig-zag coefficients; index 0 holds the DC DIFFERENCE."""
    zz = np.zeros(64, dtype=np.int64)
    s = int(rng.integers(0, dc_size + 1))
    if s:
        mag = int(rng.integers(1 << (s - 1), 1 << s))
        zz[0] = mag if rng.random() < 0.5 else -mag
    p = density * np.exp(-np.arange(1, 64) / 20.0)
    hit = rng.random(63) < p
    for k in np.nonzero(hit)[0] + 1:
        s = int(rng.integers(1, max_size + 1))
        mag = int(rng.integers(1 << (s - 1), 1 << s))
        zz[k] = mag if rng.random() < 0.5 else -mag
    return zz


def _encode_block(w: _Bits, zz, dc_codes, ac_codes):
    d = int(zz[0])
    s = _category(d)
    w.put(*dc_codes[s])
    if s:
        w.put(_value_bits(d, s), s)
    run = 0
    last = int(np.max(np.nonzero(zz[1:])[0])) + 1 if np.any(zz[1:]) else 0
    for k in range(1, last + 1):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac_codes[0xF0])
            run -= 16
        s = _category(v)
        w.put(*ac_codes[(run << 4) | s])
        w.put(_value_bits(v, s), s)
        run = 0
    if last < 63:
        w.put(*ac_codes[0x00])


def wide_ac_table(seed: int = 0):
    """(bits, vals) of an AC table that holds every (run, size) symbol with sizes 0..15 and run 0..15 that fits 256 symbols —
    the reference takes whatever size a symbol names (jpeg_decoder.py:862) — with code lengths from 2 to 16 bits, so that
    finished LUT entries, entries whose value bits are taken arithmetically, and second-level tables all occur."""
    rng = np.random.default_rng(seed)
    likely = [0x00, 0x01, 0x02, 0x11, 0x03, 0x21, 0xF0, 0x04, 0x12, 0x31, 0x05, 0x41]
    rest = [(r << 4) | s for s in range(0, 16) for r in range(16) if ((r << 4) | s) not in likely and not (s == 0 and r not in (0, 15))]
    rng.shuffle(rest)
    order = likely + rest
    counts = {2: 1, 3: 1, 4: 2, 5: 4, 6: 4, 7: 8, 8: 12, 9: 20, 10: 24, 11: 30, 12: 30, 13: 30, 14: 30, 15: 24, 16: len(order) - 220}
    assert sum(counts.values()) == len(order) and counts[16] > 0
    return bytes(counts.get(l, 0) for l in range(1, 17)), bytes(order)


def craft_baseline(width: int, height: int, factors, seed: int = 0, restart_interval: int = 0, density: float = 0.35,
                   max_size: int = 5, dc_size: int = 5, tables=None, ac_tables=None, blocks=None, qts=None) -> bytes:
    """A baseline file of `width` x `height` with one interleaved scan; `factors` = ((h, v), ...) per component (1 or 3 of them).
    `tables` = per component (dc table, ac table) as indices into the table lists (default: luma tables for the first
    component, chroma tables for the others); `ac_tables` = extra (bits, vals) AC tables behind the two Annex-K ones (index
    2..): files whose components share or swap tables, up to four tables per class.
    `blocks` = the coefficients to write instead of random ones: int16 [n_blocks, 64], zig-zag, in MCU order (the order of
    the scan: every MCU its first component's h*v blocks, then the others'), index 0 the ABSOLUTE DC — the DC differences
    (per component, from 0 again behind every restart marker) are formed here.  `qts` = up to two quantisation tables of 64
    zig-zag entries 1..255 in place of the Annex-K luma / chroma ones (table 0: first component, table 1: the others).
    Every value must have a code: the Annex-K tables end at DC size 11 and AC size 10 (wide_ac_table: 15)."""
    factors = [tuple(f) for f in factors]
    ncomp = len(factors)
    assert ncomp in (1, 3)
    rng = np.random.default_rng(seed)
    hmax = max(h for h, _ in factors) if ncomp > 1 else 1
    vmax = max(v for _, v in factors) if ncomp > 1 else 1
    mcw, mch = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    out = bytearray(b"\xFF\xD8")
    qt_bytes = [_T["STD_QT_LUMA_ZZ"], _T["STD_QT_CHROMA_ZZ"]]
    if qts is not None:
        assert 1 <= len(qts) <= 2
        for t, q in enumerate(qts):
            q = [int(v) for v in np.asarray(q).reshape(-1)]
            assert len(q) == 64 and all(1 <= v <= 255 for v in q), "a quantisation table is 64 zig-zag entries 1..255"
            qt_bytes[t] = bytes(q)
    out += _seg(0xDB, b"\x00" + qt_bytes[0])
    out += _seg(0xDB, b"\x01" + qt_bytes[1])
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp])
    for c, (h, v) in enumerate(factors):
        sof += bytes([c + 1, (h << 4) | v, 0 if c == 0 else 1])
    out += _seg(0xC0, sof)
    if tables is None:
        tables = [(0, 0) if c == 0 else (1, 1) for c in range(ncomp)]
    tables = [tuple(t) for t in tables]
    ac_specs = [(_T["STD_AC_LUMA_BITS"], _T["STD_AC_LUMA_VALS"]), (_T["STD_AC_CHROMA_BITS"], _T["STD_AC_CHROMA_VALS"])] + list(ac_tables or [])
    dc_specs = [(_T["STD_DC_LUMA_BITS"], _T["STD_DC_LUMA_VALS"]), (_T["STD_DC_CHROMA_BITS"], _T["STD_DC_CHROMA_VALS"])]
    ac_codes = [_codes(b, v) for b, v in ac_specs]
    for t in range(4):
        if t in {d for d, _ in tables}:
            out += _seg(0xC4, bytes([t]) + dc_specs[t][0] + dc_specs[t][1])
        if t in {a for _, a in tables}:
            out += _seg(0xC4, bytes([0x10 | t]) + ac_specs[t][0] + ac_specs[t][1])
    if restart_interval:
        out += _seg(0xDD, restart_interval.to_bytes(2, "big"))
    sos = bytes([ncomp])
    for c in range(ncomp):
        sos += bytes([c + 1, (tables[c][0] << 4) | tables[c][1]])
    sos += bytes([0, 63, 0])
    out += _seg(0xDA, sos)
    w = _Bits()
    n_mcu = mcw * mch
    rst = 0
    if blocks is not None:
        blocks = np.asarray(blocks)
        per_mcu = sum(h * v for h, v in factors) if ncomp > 1 else 1
        assert blocks.shape == (n_mcu * per_mcu, 64), f"blocks must be [{n_mcu * per_mcu}, 64] for this geometry, not {blocks.shape}"
    pred = [0] * ncomp                              # (blocks=) the DC predictors
    nb = 0
    for m in range(n_mcu):
        for c, (h, v) in enumerate(factors):
            rep = h * v if ncomp > 1 else 1
            for _ in range(rep):
                if blocks is not None:
                    zz = blocks[nb].astype(np.int64)
                    nb += 1
                    dc = int(zz[0])
                    zz[0] = dc - pred[c]
                    pred[c] = dc
                    assert _category(int(zz[0])) in _DC[tables[c][0]], f"block {nb - 1}: no code for a DC difference of {int(zz[0])}"
                    top = int(np.abs(zz[1:]).max())
                    assert all(((r << 4) | _category(top)) in ac_codes[tables[c][1]] for r in range(16 if top else 0)), \
                        f"block {nb - 1}: AC table {tables[c][1]} has no code for a value of {top}"
                    _encode_block(w, zz, _DC[tables[c][0]], ac_codes[tables[c][1]])
                    continue
                # (the Annex-K tables have no symbol for sizes above 10)
                _encode_block(w, random_block(rng, density, max_size if tables[c][1] >= 2 else min(max_size, 10), dc_size),
                              _DC[tables[c][0]], ac_codes[tables[c][1]])
        if restart_interval and (m + 1) % restart_interval == 0 and m + 1 != n_mcu:
            w.flush()
            w.out += bytes([0xFF, 0xD0 + (rst & 7)])
            rst += 1
            pred = [0] * ncomp
    w.flush()
    out += w.out
    out += b"\xFF\xD9"
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# Progressive files, scan by scan.  Nothing is transformed: every scan's symbols are drawn at random, subject only to what
# a decoder has seen so far (a refining scan sends a correction bit for every coefficient earlier scans left non-zero and
# may place +-1 where they left zero), so any scan script is possible — DC scans over a subset of the components,
# arbitrary bands, several refinement levels, long end-of-band runs, restart intervals.  The symbol order of the
# refining scans follows T.81 G.1.2.3 / figure G.7 (zero runs count zero-history coefficients only; corrections follow
# the symbol that passes them; an end-of-band run carries the corrections of everything it skips).

def _ac_prog_table(seed: int):
    """A Huffman table holding every (run, size) symbol a progressive AC scan can use (sizes 0..10; size 0 = EOBn / ZRL), code
    lengths from 3 to 14 bits so that LUT hits, long codes and second-level tables all occur."""
    rng = np.random.default_rng(seed)
    syms = [(r << 4) | s for s in range(0, 11) for r in range(16)]
    likely = [0x00, 0x01, 0x11, 0x02, 0x21, 0x10, 0xF0, 0x31, 0x41, 0x12, 0x03, 0x20]
    rest = [s for s in syms if s not in likely]
    rng.shuffle(rest)
    order = likely + rest
    counts = {3: 2, 4: 2, 5: 4, 6: 6, 7: 10, 8: 16, 9: 24, 10: 32, 12: 40, 14: 40}
    assert sum(counts.values()) == len(order) == 176
    bits = bytes(counts.get(l, 0) for l in range(1, 17))
    return bits, bytes(order)


DEFAULT_SCRIPT = [   # libjpeg's default for three components: (components, Ss, Se, Ah, Al)
    ((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
    ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0),
]


def craft_progressive(width: int, height: int, factors, seed: int = 0, script=None, restart_interval: int = 0,
                      density: float = 0.2, new_density: float = 0.08, empty_block: float = 0.3, max_size: int = 4, dc_size: int = 4) -> bytes:
    factors = [tuple(f) for f in factors]
    ncomp = len(factors)
    assert ncomp in (1, 3)
    script = script or (DEFAULT_SCRIPT if ncomp == 3 else [((0,), 0, 0, 0, 1), ((0,), 1, 63, 0, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)])
    rng = np.random.default_rng(seed)
    hmax = max(h for h, _ in factors) if ncomp > 1 else 1
    vmax = max(v for _, v in factors) if ncomp > 1 else 1
    mcw, mch = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    ac_bits, ac_vals = _ac_prog_table(seed)
    ac_codes = _codes(ac_bits, ac_vals)
    out = bytearray(b"\xFF\xD8")
    out += _seg(0xDB, b"\x00" + _T["STD_QT_LUMA_ZZ"])
    out += _seg(0xDB, b"\x01" + _T["STD_QT_CHROMA_ZZ"])
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp])
    for c, (h, v) in enumerate(factors):
        sof += bytes([c + 1, (h << 4) | v, 0 if c == 0 else 1])
    out += _seg(0xC2, sof)
    out += _seg(0xC4, b"\x00" + _T["STD_DC_LUMA_BITS"] + _T["STD_DC_LUMA_VALS"])
    out += _seg(0xC4, b"\x01" + _T["STD_DC_CHROMA_BITS"] + _T["STD_DC_CHROMA_VALS"])
    out += _seg(0xC4, b"\x10" + ac_bits + ac_vals)
    out += _seg(0xC4, b"\x11" + ac_bits + ac_vals)
    if restart_interval:
        out += _seg(0xDD, restart_interval.to_bytes(2, "big"))
    # what a decoder holds so far: non-zero flags per component, [block row][block column][zig-zag index], padded to whole MCUs
    fh = [(h, v) if ncomp > 1 else (1, 1) for h, v in factors]
    nz = [np.zeros((mch * v, mcw * h, 64), dtype=bool) for h, v in fh]

    for comps, ss, se, ah, al in script:
        # (table selectors: DC table 0 / 1 and AC table 0 / 1 for luma / the others)
        sos = bytes([len(comps)]) + b"".join(bytes([c + 1, ((0 if c == 0 else 1) << 4) | (0 if c == 0 else 1)]) for c in comps)
        sos += bytes([ss, se, (ah << 4) | al])
        out += _seg(0xDA, sos)
        w = _Bits()
        rst = [0]

        def restart_marker():
            w.flush()
            w.out.extend(bytes([0xFF, 0xD0 + (rst[0] & 7)]))
            rst[0] += 1

        if ss == 0:                                                    # ---- DC scan
            assert se == 0
            if len(comps) > 1:
                n_mcu = mcw * mch
            else:
                h, v = fh[comps[0]]
                bwn = -(-(width * h) // (hmax * 8)) if ncomp > 1 else -(-width // 8)
                bhn = -(-(height * v) // (vmax * 8)) if ncomp > 1 else -(-height // 8)
                n_mcu = bwn * bhn
            for m in range(n_mcu):
                for c in comps:
                    h, v = fh[c]
                    rep = h * v if len(comps) > 1 else 1
                    for _ in range(rep):
                        if ah == 0:
                            s = int(rng.integers(0, dc_size + 1))
                            w.put(*_DC[0 if c == 0 else 1][s])
                            if s:
                                w.put(int(rng.integers(0, 1 << s)), s)
                        else:
                            w.put(int(rng.integers(0, 2)), 1)
                if restart_interval and (m + 1) % restart_interval == 0 and m + 1 != n_mcu:
                    restart_marker()
            w.flush()
            out += w.out
            continue
        # ---- AC scan of one component, its own block raster (:612-619)
        assert len(comps) == 1
        c = comps[0]
        h, v = fh[c]
        bwn = -(-(width * h) // (hmax * 8)) if ncomp > 1 else -(-width // 8)
        bhn = -(-(height * v) // (vmax * 8)) if ncomp > 1 else -(-height // 8)
        n_mcu = bwn * bhn
        codes = ac_codes
        eobrun = [0]
        be = []                                                        # correction bits waiting behind the end-of-band run

        def emit_eobrun():
            if eobrun[0] > 0:
                nb = eobrun[0].bit_length() - 1
                w.put(*codes[nb << 4])
                if nb:
                    w.put(eobrun[0] & ((1 << nb) - 1), nb)
                eobrun[0] = 0
            for b in be:
                w.put(b, 1)
            be.clear()

        for m in range(n_mcu):
            by, bx = divmod(m, bwn)
            flags = nz[c][by, bx]
            if ah == 0:                                                # first scan of the band
                r = 0
                if rng.random() >= empty_block:
                    for k in range(ss, se + 1):
                        if rng.random() >= density * np.exp(-(k - ss) / 24.0):
                            r += 1
                            continue
                        emit_eobrun()
                        while r > 15:
                            w.put(*codes[0xF0])
                            r -= 16
                        s = int(rng.integers(1, max_size + 1))
                        w.put(*codes[(r << 4) | s])
                        w.put(int(rng.integers(0, 1 << s)), s)
                        flags[k] = True
                        r = 0
                else:
                    r = se - ss + 1
                if r > 0:
                    eobrun[0] += 1
                    if eobrun[0] == 0x7FFF:
                        emit_eobrun()
            else:                                                      # refining scan
                kinds = np.zeros(64, dtype=np.int8)                    # 0 stays zero, 1 history, 2 new
                kinds[flags] = 1
                if rng.random() >= empty_block:
                    new = (~flags) & (rng.random(64) < new_density)
                    kinds[new] = 2
                band = range(ss, se + 1)
                eob_at = max([k for k in band if kinds[k] == 2], default=-1)
                r, br = 0, []
                for k in band:
                    if kinds[k] == 0:
                        r += 1
                        continue
                    while r > 15 and k <= eob_at:
                        emit_eobrun()
                        w.put(*codes[0xF0])
                        r -= 16
                        for b in br:
                            w.put(b, 1)
                        br = []
                    if kinds[k] == 1:
                        br.append(int(rng.integers(0, 2)))
                        continue
                    emit_eobrun()
                    w.put(*codes[(r << 4) | 1])
                    w.put(int(rng.integers(0, 2)), 1)
                    for b in br:
                        w.put(b, 1)
                    br = []
                    r = 0
                    flags[k] = True
                if r > 0 or br:
                    eobrun[0] += 1
                    be.extend(br)
                    if eobrun[0] == 0x7FFF or len(be) > 900:
                        emit_eobrun()
            if restart_interval and (m + 1) % restart_interval == 0 and m + 1 != n_mcu:
                emit_eobrun()
                restart_marker()
        emit_eobrun()
        w.flush()
        out += w.out
    out += b"\xFF\xD9"
    return bytes(out)


Y420 = ((2, 2), (1, 1), (1, 1))
CRAFTED_PROGRESSIVE = [   # the files of tests/golden/crafted_progressive.npz (tools/make_layout_goldens.py; seed 200 + position)
    # name, arguments of craft_progressive
    ("default_420_dri3", dict(width=50, height=37, factors=Y420, restart_interval=3)),
    ("dc_y_cb_then_cr", dict(width=50, height=37, factors=Y420,            # interleaved DC scan over a SUBSET of the components
                             script=[((0, 1), 0, 0, 0, 0), ((2,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)])),
    ("dc_y_cr_refined", dict(width=41, height=33, factors=((2, 1), (1, 1), (1, 1)),   # ... refined through the same subsets
                             script=[((0, 2), 0, 0, 0, 2), ((1,), 0, 0, 0, 1), ((0,), 1, 63, 0, 1), ((0, 2), 0, 0, 2, 1), ((1,), 1, 63, 0, 0),
                                     ((2,), 1, 20, 0, 0), ((0, 2), 0, 0, 1, 0), ((1,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0), ((2,), 21, 63, 0, 0)])),
    ("bands_444_two_levels", dict(width=33, height=21, factors=((1, 1), (1, 1), (1, 1)), new_density=0.15,
                                  script=[((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 9, 0, 2), ((0,), 10, 40, 0, 2), ((0,), 41, 63, 0, 2), ((1,), 1, 63, 0, 2),
                                          ((2,), 1, 63, 0, 2), ((0,), 1, 63, 2, 1), ((1,), 1, 63, 2, 1), ((2,), 1, 63, 2, 1), ((0,), 1, 30, 1, 0),
                                          ((0,), 31, 63, 1, 0), ((1,), 1, 63, 1, 0), ((2,), 1, 63, 1, 0)])),
    ("grey_sparse_long_eob_runs", dict(width=120, height=64, factors=((1, 1),), empty_block=0.9, density=0.05)),
    ("y4x2", dict(width=70, height=40, factors=((4, 2), (1, 1), (1, 1)))),              # 4:1:0
    ("y1x1_c2x2", dict(width=40, height=40, factors=((1, 1), (2, 2), (2, 2)))),
    ("y3x1_dri", dict(width=50, height=20, factors=((3, 1), (1, 1), (1, 1)), restart_interval=2)),
    ("y2x4", dict(width=30, height=70, factors=((2, 4), (1, 1), (1, 1)))),
]


# ---------------------------------------------------------------------------------------------------------------------
# Progressive files from an explicit description (tests/prog_cases.py): nothing is drawn, nothing is checked — every scan is
# the list of stream items its author wants, so symbols no conformant encoder writes (a run that ends behind the band, a
# size of 10 in a refining scan, a bit pattern without a code) can be written as easily as the usual ones.

def huffman_table(lengths):
    """(bits, vals) of the canonical table in which symbol s has a code of lengths[s] bits (symbols of one length in the
    order given).  The lengths may leave codes unused (Kraft sum below one): then some bit patterns match no code."""
    order = sorted(lengths.items(), key=lambda kv: kv[1])           # (stable: the given order within one length)
    counts = [0] * 17
    for _, l in order:
        assert 1 <= l <= 16
        counts[l] += 1
    assert sum(c << (16 - l) for l, c in enumerate(counts) if l) < (1 << 16), "the code lengths leave no pattern unused"
    return bytes(counts[1:]), bytes(s for s, _ in order)


def long_ac_table(variant: int = 0):
    """An AC table for progressive scans whose code lengths include 11, 12, 15 and 16 bits and whose symbols reach size 15.
    variant 0: the usual symbols ((run, 1), EOB0, ZRL, small EOBn) short, the large sizes and the long end-of-band runs long —
      0x31 11 bits, 0x41 / 0x0B / 0x12 12 bits, 0x51 / 0x0C / 0x0D 15 bits, 0x61 / 0x0E / 0x0F / 0xE0 16 bits;
    variant 1: ZRL, EOB0 and the end-of-band runs behind the 11-bit table (ZRL 12 bits, EOB0 13, EOB1 15, EOB2 16) and
      (0, 1) at 11 bits exactly;
    variant 2: ZRL at 16 bits, (0, 1) at 16 bits, EOB0 at 15.
    Every variant leaves the all-ones pattern (and more) without a code."""
    if variant == 0:
        L = {0x00: 3, 0x01: 3, 0x11: 4, 0xF0: 4, 0x02: 5, 0x10: 5, 0x21: 5, 0x0A: 6, 0x20: 6, 0x03: 6, 0x30: 7, 0x71: 7, 0xF1: 7,
             0x22: 7, 0x40: 8, 0x04: 8, 0x50: 8, 0x91: 8, 0xE1: 8, 0x60: 9, 0x70: 9, 0x05: 9, 0xA1: 9, 0x80: 10, 0x90: 10, 0x06: 10,
             0x81: 10, 0x31: 11, 0xA0: 11, 0x07: 11, 0x41: 12, 0x0B: 12, 0x12: 12, 0xB0: 12, 0x08: 13, 0xC0: 13, 0x09: 14, 0xD0: 14,
             0x51: 15, 0x0C: 15, 0x0D: 15, 0x1A: 15, 0x61: 16, 0x0E: 16, 0x0F: 16, 0xE0: 16, 0xF2: 16}
    elif variant == 1:
        L = {0x11: 2, 0x21: 3, 0x02: 4, 0x31: 4, 0x41: 5, 0x03: 6, 0x51: 6, 0x61: 7, 0x71: 8, 0x81: 9, 0x91: 10, 0x01: 11, 0xA1: 11,
             0xF0: 12, 0xB1: 12, 0x00: 13, 0x30: 13, 0x10: 15, 0xC1: 15, 0x20: 16, 0xE0: 16, 0xD1: 16}
    else:
        L = {0x11: 2, 0x21: 3, 0x02: 4, 0x10: 4, 0x31: 5, 0x20: 6, 0x41: 7, 0x51: 12, 0x00: 15, 0x01: 16, 0xF0: 16, 0xF1: 16}
    return huffman_table(L)


def long_dc_table():
    """A DC table holding the sizes 0..16 (the reference takes whatever size a symbol names, :1017) with codes of 2..16 bits:
    sizes 0..9 inside a 9-bit table, size 10 at 10 bits, 11 at 11, 12 at 12, 13 at 13, 14 at 14, 15 at 15, 16 at 16."""
    L = {0: 2, 1: 3, 2: 3, 3: 4, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 10, 11: 11, 12: 12, 13: 13, 14: 14, 15: 15, 16: 16}
    return huffman_table(L)


def craft_progressive_symbols(width: int, height: int, factors, scans, dc_tables=None, ac_tables=None, restart_interval: int = 0) -> bytes:
    """A progressive file of `width` x `height`, `factors` = ((h, v), ...) per component (1 or 3), written item by item.
    `dc_tables` / `ac_tables` = up to four (bits, vals) each (default: the Annex-K luma and chroma ones), sent once in front
    of the first scan.  `scans` = a list of (components, Ss, Se, Ah, Al, tables, items): `tables` = per scan component the
    (DC table, AC table) indices; `items` = what the scan's entropy-coded segment holds, in order:
      ("dc", i, size[, bits])  the code of `size` in the DC table of the scan's i-th component, then the low `size` bits of `bits`
      ("ac", rs[, bits])       the code of symbol rs = run << 4 | size in the scan's AC table, then the low n bits of `bits`:
                               n = size, or for size 0 and run < 15 (an end-of-band run of (1 << run) + bits blocks) n = run
      ("bits", value, n)       n raw bits: correction bits, the bits of a refining DC scan, anything else
      ("rst",)                 pad to a byte with ones and write the next restart marker
    The last byte of every scan is padded with ones.  A symbol without a code in its table is an error here."""
    factors = [tuple(f) for f in factors]
    ncomp = len(factors)
    assert ncomp in (1, 3)
    dc_tables = list(dc_tables or [(_T["STD_DC_LUMA_BITS"], _T["STD_DC_LUMA_VALS"]), (_T["STD_DC_CHROMA_BITS"], _T["STD_DC_CHROMA_VALS"])])
    ac_tables = list(ac_tables or [(_T["STD_AC_LUMA_BITS"], _T["STD_AC_LUMA_VALS"]), (_T["STD_AC_CHROMA_BITS"], _T["STD_AC_CHROMA_VALS"])])
    assert len(dc_tables) <= 4 and len(ac_tables) <= 4
    dc_codes = [_codes(bytes(b), bytes(v)) for b, v in dc_tables]
    ac_codes = [_codes(bytes(b), bytes(v)) for b, v in ac_tables]
    out = bytearray(b"\xFF\xD8")
    out += _seg(0xDB, b"\x00" + _T["STD_QT_LUMA_ZZ"])
    out += _seg(0xDB, b"\x01" + _T["STD_QT_CHROMA_ZZ"])
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp])
    for c, (h, v) in enumerate(factors):
        sof += bytes([c + 1, (h << 4) | v, 0 if c == 0 else 1])
    out += _seg(0xC2, sof)
    for t, (b, v) in enumerate(dc_tables):
        out += _seg(0xC4, bytes([t]) + bytes(b) + bytes(v))
    for t, (b, v) in enumerate(ac_tables):
        out += _seg(0xC4, bytes([0x10 | t]) + bytes(b) + bytes(v))
    if restart_interval:
        out += _seg(0xDD, restart_interval.to_bytes(2, "big"))
    for comps, ss, se, ah, al, tables, items in scans:
        tables = [tuple(t) for t in tables]
        assert len(tables) == len(comps)
        sos = bytes([len(comps)]) + b"".join(bytes([c + 1, (d << 4) | a]) for c, (d, a) in zip(comps, tables))
        out += _seg(0xDA, sos + bytes([ss, se, (ah << 4) | al]))
        w = _Bits()
        rst = 0
        for it in items:
            if it[0] == "dc":
                size = it[2]
                w.put(*dc_codes[tables[it[1]][0]][size])
                if size:
                    w.put(it[3], size)
            elif it[0] == "ac":
                rs = it[1]
                w.put(*ac_codes[tables[0][1]][rs])
                n = (rs & 15) or (rs >> 4 if rs >> 4 < 15 else 0)
                if n:
                    w.put(it[2], n)
            elif it[0] == "bits":
                if it[2]:
                    w.put(it[1], it[2])
            else:
                assert it[0] == "rst"
                w.flush()
                w.out += bytes([0xFF, 0xD0 + (rst & 7)])
                rst += 1
        w.flush()
        out += w.out
    out += b"\xFF\xD9"
    return bytes(out)


def craft_baseline_symbols(width: int, height: int, factors, mcus, dc_tables=None, ac_tables=None, tables=None,
                           restart_interval: int = 0, qts=None) -> bytes:
    """The baseline twin of craft_progressive_symbols: a file of `width` x `height` with one interleaved scan, `factors` =
    ((h, v), ...) per component (1 or 3), written item by item; nothing is drawn and nothing is checked.  `dc_tables` /
    `ac_tables` = up to four (bits, vals) each (default: the Annex-K luma and chroma ones); `tables` = per component the (DC
    table, AC table) indices (default: table 0 for the first component, 1 for the others); `qts` as in craft_baseline.
    `mcus` = what the entropy-coded segment holds, in order — the caller writes every MCU and every restart marker:
      [block, ...]             one MCU: a list of blocks in the scan's order (the component of a block follows from its place),
                               each block a list of
          ("dc", size[, bits])       the code of `size` in the block's DC table, then the low `size` bits of `bits`
          ("ac", run, size[, bits])  the code of run << 4 | size in its AC table, then the low `size` bits of `bits`;
                                     bits = None: the value bits are NOT written (what follows a run past index 63)
          ("bits", value, n)         n raw bits
      ("rst",) / ("rst", extra)  pad to a byte with ones, write `extra` (spare bytes, default none) and the next restart marker
      ("bytes", b)               pad to a byte with ones and write the bytes b as they are
      ("cut", n)                 pad to a byte with ones and drop the last n bytes written (a truncated segment)
    The last byte is padded with ones.  A symbol without a code in its table is an error here."""
    factors = [tuple(f) for f in factors]
    ncomp = len(factors)
    assert ncomp in (1, 3)
    dc_tables = list(dc_tables or [(_T["STD_DC_LUMA_BITS"], _T["STD_DC_LUMA_VALS"]), (_T["STD_DC_CHROMA_BITS"], _T["STD_DC_CHROMA_VALS"])])
    ac_tables = list(ac_tables or [(_T["STD_AC_LUMA_BITS"], _T["STD_AC_LUMA_VALS"]), (_T["STD_AC_CHROMA_BITS"], _T["STD_AC_CHROMA_VALS"])])
    assert len(dc_tables) <= 4 and len(ac_tables) <= 4
    if tables is None:
        tables = [(0, 0) if c == 0 else (1, 1) for c in range(ncomp)]
    tables = [tuple(t) for t in tables]
    dc_codes = [_codes(bytes(b), bytes(v)) for b, v in dc_tables]
    ac_codes = [_codes(bytes(b), bytes(v)) for b, v in ac_tables]
    out = bytearray(b"\xFF\xD8")
    qt_bytes = [_T["STD_QT_LUMA_ZZ"], _T["STD_QT_CHROMA_ZZ"]]
    for t, q in enumerate(qts or []):
        q = [int(v) for v in np.asarray(q).reshape(-1)]
        assert t < 2 and len(q) == 64 and all(1 <= v <= 255 for v in q), "a quantisation table is 64 zig-zag entries 1..255"
        qt_bytes[t] = bytes(q)
    out += _seg(0xDB, b"\x00" + qt_bytes[0])
    out += _seg(0xDB, b"\x01" + qt_bytes[1])
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp])
    for c, (h, v) in enumerate(factors):
        sof += bytes([c + 1, (h << 4) | v, 0 if c == 0 else 1])
    out += _seg(0xC0, sof)
    for t in range(4):                                             # (the order craft_baseline writes them in)
        if t in {d for d, _ in tables}:
            out += _seg(0xC4, bytes([t]) + bytes(dc_tables[t][0]) + bytes(dc_tables[t][1]))
        if t in {a for _, a in tables}:
            out += _seg(0xC4, bytes([0x10 | t]) + bytes(ac_tables[t][0]) + bytes(ac_tables[t][1]))
    if restart_interval:
        out += _seg(0xDD, restart_interval.to_bytes(2, "big"))
    sos = bytes([ncomp])
    for c in range(ncomp):
        sos += bytes([c + 1, (tables[c][0] << 4) | tables[c][1]])
    out += _seg(0xDA, sos + bytes([0, 63, 0]))
    comp_of_block = [c for c, (h, v) in enumerate(factors) for _ in range(h * v if ncomp > 1 else 1)]
    w = _Bits()
    rst = 0
    for unit in mcus:
        if isinstance(unit, tuple):
            w.flush()
            if unit[0] == "rst":
                w.out += bytes(unit[1]) if len(unit) > 1 else b""
                w.out += bytes([0xFF, 0xD0 + (rst & 7)])
                rst += 1
            elif unit[0] == "bytes":
                w.out += bytes(unit[1])
            else:
                assert unit[0] == "cut"
                del w.out[len(w.out) - unit[1]:]
            continue
        assert len(unit) == len(comp_of_block), f"an MCU of this layout has {len(comp_of_block)} blocks, not {len(unit)}"
        for c, block in zip(comp_of_block, unit):
            for it in block:
                if it[0] == "dc":
                    w.put(*dc_codes[tables[c][0]][it[1]])
                    if it[1]:
                        w.put(it[2], it[1])
                elif it[0] == "ac":
                    w.put(*ac_codes[tables[c][1]][(it[1] << 4) | it[2]])
                    if it[2] and (len(it) < 4 or it[3] is not None):
                        w.put(it[3] if len(it) > 3 else 0, it[2])
                else:
                    assert it[0] == "bits"
                    if it[2]:
                        w.put(it[1], it[2])
    w.flush()
    out += w.out
    out += b"\xFF\xD9"
    return bytes(out)


# ---- random files of both kinds (tests, tools/stress_crafted.py, tools/crosscheck_reference.py --crafted) ----------------
def random_baseline(rng, seed: int) -> bytes:
    """Any factors 1..4 per component (at most 16 blocks per MCU), 1..119 pixels a side, with and without restart intervals."""
    f = [(int(rng.integers(1, 5)), int(rng.integers(1, 5))) for _ in range(3)]
    while sum(h * v for h, v in f) > 16:
        f = [(int(rng.integers(1, 5)), int(rng.integers(1, 5))) for _ in range(3)]
    w, h = int(rng.integers(1, 120)), int(rng.integers(1, 120))
    return craft_baseline(w, h, f, seed=seed, restart_interval=int(rng.integers(0, 4)), density=float(rng.uniform(0.05, 0.6)),
                          max_size=int(rng.integers(1, 8)), dc_size=int(rng.integers(1, 8)))


def random_script(rng, factors):
    """A scan script for `factors`: the DC components in random groups (a component on its own must be 1x1: the reference
    cannot walk the other kind), bands cut at random, successive approximation up to three levels deep, the scans of the
    components interleaved at random (every scan behind the ones it refines)."""
    nc = len(factors)
    comps = list(range(nc))
    a = int(rng.integers(0, 3))
    lone_ok = [c for c in comps if factors[c] == (1, 1) or nc == 1]
    groups = [tuple(comps)]
    if nc == 3 and lone_ok and rng.random() < 0.6:
        c = int(rng.choice(lone_ok))
        groups = [tuple(x for x in comps if x != c), (c,)]
        if rng.random() < 0.5:
            groups.reverse()
    script = [(g, 0, 0, 0, a) for g in groups]
    dc_ref = [[(g, 0, 0, lvl + 1, lvl) for g in groups] for lvl in range(a - 1, -1, -1)]
    ac = {c: [] for c in comps}
    for c in comps:
        al = int(rng.integers(0, 3))
        cuts = sorted(set([1, 64] + [int(x) for x in rng.integers(2, 64, size=int(rng.integers(0, 3)))]))
        ac[c].append([((c,), cuts[j], cuts[j + 1] - 1, 0, al) for j in range(len(cuts) - 1)])
        for lvl in range(al - 1, -1, -1):
            cuts = sorted(set([1, 64] + [int(x) for x in rng.integers(2, 64, size=int(rng.integers(0, 2)))]))
            ac[c].append([((c,), cuts[j], cuts[j + 1] - 1, lvl + 1, lvl) for j in range(len(cuts) - 1)])
    stages = [dc_ref] + [ac[c] for c in comps]          # lists of stages; the stages of one list stay in order
    while any(stages):
        j = int(rng.choice([k for k, s_ in enumerate(stages) if s_]))
        script += stages[j].pop(0)
    return script


def random_progressive(rng, seed: int) -> bytes:
    """A random layout the reference can finish (every component 1x1 or at the full resolution, or greyscale), a random
    script, 1..89 pixels a side."""
    H, V = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    while H * V + 2 > 16:                                       # (16 blocks per MCU is what the MI355X path holds; T.81 allows 10)
        H, V = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    kind = int(rng.integers(0, 4))
    factors = [((H, V), (1, 1), (1, 1)), ((1, 1), (H, V), (H, V)), ((H, V), (H, V), (1, 1)), ((1, 1),)][kind]
    if sum(h * v for h, v in factors) > 16:
        factors = ((H, V), (1, 1), (1, 1))
    return craft_progressive(int(rng.integers(1, 90)), int(rng.integers(1, 90)), factors, seed=seed, script=random_script(rng, factors),
                             restart_interval=int(rng.choice([0, 0, 1, 3, 7])), density=float(rng.uniform(0.05, 0.4)),
                             new_density=float(rng.uniform(0.02, 0.25)), empty_block=float(rng.uniform(0.0, 0.95)),
                             max_size=int(rng.integers(1, 7)), dc_size=int(rng.integers(1, 7)))
