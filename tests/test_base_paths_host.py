"""CPU half of the baseline stage 1's rare-path rows (tests/base_cases.py): the model walk is the oracle's walk on every row and
on every baseline input the suite had; the oracle reproduces what the reference made of every row (tests/golden/base_paths.npz);
every row's census shows its path reached; every wrong variant of the walk is told from the model by the row named for it; the
host layer accepts the rows.  tests/test_base_paths.py holds the kernels to the same files.

`python tests/test_base_paths_host.py` rewrites profiles/base_paths_census.txt."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
if str(ROOT / "tests") not in sys.path:
    sys.path.insert(0, str(ROOT / "tests"))

import base_cases as bc                                  # noqa: E402
from base_cases import COMMON, EVENTS, EXTRA, HEALTHY, REFUSED, ROWS, row_bytes, summary, walk, walk_census   # noqa: E402

GOLDEN = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "base_paths.npz")


def _oracle(raw):
    from oracle import oracle
    return oracle.decode(raw)


def existing_inputs():
    """(name, bytes) of the baseline inputs with one interleaved scan the suite had before these rows: the small fixtures of
    tests/golden/files and the layouts of odd_layouts.npz.  (The files other tests write as they run — the three hand-written
    greyscale streams of test_gpu_parity.py among them — are not counted.)"""
    import json
    from pyjpegdecoder_amd._parse import parse_jpeg
    out = []
    idx = json.loads((GOLDEN / "files" / "index.json").read_text())
    for n in sorted(idx):
        if n.startswith("prog_") or "sampled" in idx[n]:
            continue
        raw = (GOLDEN / "files" / f"{n}.jpg").read_bytes()
        if len(parse_jpeg(raw).scans) == 1:
            out.append((n, raw))
    g = np.load(GOLDEN / "odd_layouts.npz")
    out += [("odd:" + k[:-4], g[k].tobytes()) for k in sorted(g.files) if k.endswith(".jpg")]
    return out


# ---- the crafter ---------------------------------------------------------------------------------------------------------------
def test_the_symbol_writer_writes_what_craft_baseline_writes():
    """craft_baseline_symbols against the older writer: the same blocks, handed over item by item, give the same bytes."""
    from tools import craft_jpeg as C
    rng = np.random.default_rng(3)
    blocks = np.zeros((4 * 6, 64), dtype=np.int16)
    blocks[:, 0] = np.cumsum(rng.integers(-20, 21, 24))
    blocks[:, 1:9] = rng.integers(-31, 32, (24, 8))
    blocks[5, 63] = 7
    want = C.craft_baseline(32, 32, bc.Y420, blocks=blocks, restart_interval=2)
    units, pred, nb = [], [0, 0, 0], 0
    for m in range(4):
        mcu = []
        for b in range(6):
            c = (0, 0, 0, 0, 1, 2)[b]
            zz = blocks[nb].astype(int)
            nb += 1
            items = [bc.dc(int(zz[0]) - pred[c])]
            pred[c] = int(zz[0])
            run = 0
            for k in range(1, 64):
                if zz[k] == 0:
                    run += 1
                    continue
                while run > 15:
                    items.append(bc.ZRL)
                    run -= 16
                items.append(bc.ac(run, int(zz[k])))
                run = 0
            if zz[63] == 0:
                items.append(bc.EOB)
            mcu.append(items)
        units.append(mcu)
        if m == 1:
            units.append(("rst",))
            pred = [0, 0, 0]
    assert C.craft_baseline_symbols(32, 32, bc.Y420, units, restart_interval=2) == want


def test_the_tables_hold_the_lengths_and_symbols_asked_for():
    from tools.craft_jpeg import _codes
    for variant in (0, 1):
        ac = _codes(*bc.rare_ac_table(variant))
        assert len(ac) == 256 and {l for _, l in ac.values()} == set(range(2, 17))
        assert ac[0x0F][1] == 13 and ac[0x1F][1] == 16 and all(ac[r << 4][1] >= 4 for r in range(1, 15))
        assert max(c for c, l in ac.values() if l == 16) < 0xFFF0                     # the code is incomplete: patterns without a code
        dc = _codes(*bc.rare_dc_table(variant))
        assert sorted(dc) == list(range(16)) and [dc[s][1] for s in range(7, 16)] == [9, 10, 11, 12, 15, 16, 16, 16, 16]
    assert sorted(_codes(*bc.rare_dc_table(0, with_16=True))) == list(range(17))
    assert len({bc.rare_ac_table(v, s) for v in (0, 1) for s in range(7)} | {bc.rare_dc_table(v, s) for v in (0, 1) for s in range(7)}) == 28


def test_the_committed_files_are_the_rows(gold):
    assert sorted({k.rsplit(".", 1)[0] for k in gold.files}) == sorted(r.name for r in ROWS)
    for r in ROWS:
        assert gold[r.name + ".jpg"].tobytes() == row_bytes(r.name), r.name
        assert ((r.name + ".refused") in gold.files) == bool(r.ref), r.name
        if r.ref:
            assert bytes(gold[r.name + ".refused"]).decode() == r.ref
        assert len(row_bytes(r.name)) < 20000, r.name


def test_the_common_rows_are_one_uniform_batch():
    """One geometry, one restart interval, and few enough tables for the resolved lane form and a fused launch (at most three AC
    and four DC tables in the batch, none in both roles)."""
    from pyjpegdecoder_amd._parse import parse_jpeg
    seen = set()
    for r in COMMON + REFUSED:
        p = parse_jpeg(row_bytes(r.name))
        sc = p.scans[0]
        assert (p.image_width, p.image_height, sc.restart_interval, sc.mcu_count_h, sc.mcu_count_v) == (64, 32, 4, 4, 2), r.name
        assert [(c.horizontal_sampling, c.vertical_sampling) for c in p.color_components.values()] == [(2, 2), (1, 1), (1, 1)]
        assert all(int(v) == 1 for q in sc.quantization_zz.values() for v in q)
        seen |= {(d >> 4, s.bits.tobytes(), s.vals.tobytes()) for d, s in sc.huffman.items()}
    assert len(seen) == 4


# ---- model, oracle, reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", HEALTHY + EXTRA, ids=lambda r: r.name)
def test_model_is_the_oracle_on_the_rows(row):
    coef, status = walk(row_bytes(row.name))
    assert status == "" and np.array_equal(coef, _oracle(row_bytes(row.name))["coef"])


@pytest.mark.parametrize("row", REFUSED, ids=lambda r: r.name)
def test_model_and_oracle_refuse_the_refused_rows(row):
    _, status = walk(row_bytes(row.name))
    want = 1 if "no code" in status else 2
    assert status
    with pytest.raises(RuntimeError, match=f"status {want}"):
        _oracle(row_bytes(row.name))


def test_model_is_the_oracle_on_the_inputs_the_suite_had():
    inputs = existing_inputs()
    assert len(inputs) >= 25
    for name, raw in inputs:
        coef, status = walk(raw)
        assert status == "" and np.array_equal(coef, _oracle(raw)["coef"]), name


@pytest.mark.parametrize("row", HEALTHY, ids=lambda r: r.name)
def test_oracle_reproduces_the_reference_on_the_rows(row, gold):
    got = _oracle(row_bytes(row.name))
    assert np.array_equal(got["coef"], gold[row.name + ".coef"])
    keep = bc.pixel_mask(gold[row.name + ".mask"], *got["rgb"].shape[:2])
    assert np.array_equal(got["rgb"][keep], gold[row.name + ".rgb"][keep])


def test_masked_blocks_only_where_the_table_allows_them(gold):
    """A block whose reference samples leave int16 before the cast is left out of the pixel comparison (by the MCU).  Such MCUs
    occur in the rows made of 29..31-bit symbols only; every other row is compared whole.  The mask in the golden is the one the
    coefficients give."""
    for r in HEALTHY:
        mask = gold[r.name + ".mask"]
        assert np.array_equal(mask, bc.overflow_mask(gold[r.name + ".coef"], 6)), r.name
        assert r.masked == bool(mask.any()), r.name
    assert [r.name for r in HEALTHY if r.masked] == ["W-dense", "S-all"]              # (S-all holds W-dense's eight MCUs)
    assert gold["W-dense.mask"].all() and gold["S-all.mask"].sum() == 8


# ---- the census ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS + EXTRA, ids=lambda r: r.name)
def test_every_row_reaches_its_path(row):
    cs = walk_census(row_bytes(row.name))
    print("\n" + row.name + " " + " ".join(f"{e} {v}" for e, v in summary(cs).items() if v))
    assert row.reached(cs), row.name
    assert bool(cs["refused"]) == bool(row.refused)


def test_s_all_lays_the_wrapped_dc_sums_across_chunk_boundaries():
    """S-all: the first upward wrap of every component and its wrap back lie in different 256-byte and different 512-byte chunks
    of the entropy-coded data (the synchronisation form carries the three sums across chunk records as packed 16-bit fields)."""
    cs = walk_census(row_bytes("S-all"))
    for c in range(3):
        ev = [(d, at) for cc, d, at in cs["dc_wrap"] if cc == c]
        up = next(i for i, (d, _) in enumerate(ev) if d == 1)
        assert ev[up + 1][0] == -1
        for chunk in (256, 512):
            assert ev[up][1] // chunk < ev[up + 1][1] // chunk, (c, chunk, ev[up], ev[up + 1])
    assert cs["dc_wrapped_blocks"] >= 6 * bc.S_ALL_STAY


def test_t_own_is_more_tables_than_one_workgroup_holds():
    from pyjpegdecoder_amd._parse import parse_jpeg
    tabs = set()
    for i in range(6):
        tabs |= {(d, s.bits.tobytes(), s.vals.tobytes()) for d, s in parse_jpeg(row_bytes(f"T-own-{i}")).scans[0].huffman.items()}
    assert len(tabs) == 24


def census_table():
    before = [(n, summary(walk_census(raw))) for n, raw in existing_inputs()]
    after = [(r.name, summary(walk_census(row_bytes(r.name)))) for r in ROWS + EXTRA]

    def total(rows):
        return [str(max(s[e] for _, s in rows) if e in bc._MAXED else sum(s[e] for _, s in rows)) for e in EVENTS]
    lines = ["input " + " ".join(EVENTS)]
    lines += [n + " " + " ".join(str(s[e]) for e in EVENTS) for n, s in before]
    lines.append("TOTAL_before " + " ".join(total(before)))
    lines += [n + " " + " ".join(str(s[e]) for e in EVENTS) for n, s in after]
    lines.append("TOTAL_rows " + " ".join(total(after)))
    return lines


@pytest.fixture(scope="module")
def table():
    return census_table()


def test_the_census_table_in_profiles_is_current(table):
    """profiles/base_paths_census.txt: what the inputs the suite had reach, and what the rows reach, event by event"""
    assert (ROOT / "profiles" / "base_paths_census.txt").read_text().splitlines() == table


def test_the_rows_reach_what_the_older_inputs_never_did(table):
    t = {ln.split()[0]: dict(zip(EVENTS, map(int, ln.split()[1:]))) for ln in table if ln.startswith("TOTAL")}
    b, a = t["TOTAL_before"], t["TOTAL_rows"]
    for e in ("dc_second_11", "run0_mid", "run0_on63", "run0_over", "over_finished", "over_open", "over_second", "over_zrl",
              "dc_sum_wraps", "dense_blocks", "refused"):
        assert b[e] == 0 and a[e] > 0, e
    # (codes of 14..16 bits and coefficient 63 behind one are in the Annex-K tables' reach: the older inputs have them, one lane at a time)
    assert b["ac_second_13"] > 0 and b["c63_second"] > 0 and b["c63_open"] > 0
    assert b["ac_symbol_bits_max"] < 31 == a["ac_symbol_bits_max"] and b["dc_symbol_bits_max"] < 31 <= a["dc_symbol_bits_max"] == 32
    assert b["dc_size_max"] <= 11 and a["dc_size_max"] == 16 and b["ac_size_max"] <= 10 and a["ac_size_max"] == 15
    assert a["wait_pairs"] >= 11 * 32 and a["sparse_run_max"] >= 200 > b["sparse_run_max"]


# ---- wrong variants ---------------------------------------------------------------------------------------------------------
def _differs(name, wrong):
    good, st = walk(row_bytes(name))
    bad, st2 = walk(row_bytes(name), wrong=wrong)
    return st != st2 or not np.array_equal(good, bad)


@pytest.mark.parametrize("name,wrong", [(r.name, w) for r in ROWS + EXTRA for w in r.wrong])
def test_wrong_variants_are_told_from_the_model(name, wrong):
    assert _differs(name, wrong), bc.WRONG_VARIANTS[wrong]


def test_every_wrong_variant_has_its_row():
    assert {w for r in ROWS + EXTRA for w in r.wrong} == set(bc.WRONG_VARIANTS)


def test_wrong_variants_stay_silent_on_plain_files():
    """The variants are wrong about the rare paths only: on a row without its event a variant IS the model, which is why random
    files never told them apart.  (Each is silent on at least one other row; none is silent on its own.)"""
    assert not _differs("S-pad-16", "over_reads") and not _differs("S-pad-16", "run0_eob") and not _differs("S-pad-16", "zrl15")
    assert not _differs("A-fin", "dc_clamp") and not _differs("S-pad-16", "drop63")
    no_ff = next(r.name for r in COMMON if walk_census(row_bytes(r.name))["stuffed"] == 0)
    assert not _differs(no_ff, "keep_stuffed")


# ---- the host layer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS + EXTRA, ids=lambda r: r.name)
def test_the_host_layer_accepts_the_rows(row):
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import check_supported
    check_supported(parse_jpeg(row_bytes(row.name)))


def test_prepare_batch_takes_the_common_rows_as_one_batch():
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    files = [row_bytes(r.name) for r in COMMON]
    prep = prepare_batch(files, B.MJ_LAYOUT_XMAJOR, 0)
    assert len(prep.shapes) == len(files) and prep.n_huff == 4
    prep = prepare_batch([row_bytes(f"T-own-{i}") for i in range(6)], B.MJ_LAYOUT_XMAJOR, 0)
    assert prep.n_huff == 24


if __name__ == "__main__":
    (ROOT / "profiles" / "base_paths_census.txt").write_text("\n".join(census_table()) + "\n")
