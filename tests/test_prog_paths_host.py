"""CPU half of the progressive stage 1's rare-path rows (tests/prog_cases.py): the model walk is the oracle's walk on every row
and on every progressive input the suite had; the oracle reproduces what the reference made of every row
(tests/golden/prog_paths.npz); every row's census shows its path reached; every wrong variant of the walk is told from the
model by the row named for it; the host layer accepts the rows.  tests/test_prog_paths.py holds the kernels to the same files.

`python tests/test_prog_paths_host.py` rewrites profiles/prog_paths_census.txt."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
if str(ROOT / "tests") not in sys.path:
    sys.path.insert(0, str(ROOT / "tests"))

import prog_cases as pc                                  # noqa: E402
from prog_cases import EVENTS, EXTRA, ROWS, Refused, row_bytes, summary, walk, walk_census   # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
OK = [r for r in ROWS if not r.refused]
REFUSED = [r for r in ROWS if r.refused]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "prog_paths.npz")


def _oracle(raw):
    from oracle import oracle
    return oracle.decode(raw)


def existing_inputs():
    """(name, bytes) of the progressive inputs the suite had before these rows: the Pillow-written fixtures, the crafted files
    decoded by the reference, the 36 random scripts of test_crafted_progressive_random_scripts_against_the_oracle.  (The files
    other tests have Pillow write as they run depend on the installed encoder and are not counted.)"""
    import json
    from tools.craft_jpeg import random_progressive
    out = []
    for n in sorted(json.loads((GOLDEN / "files" / "index.json").read_text())):
        if n.startswith("prog_"):
            out.append((n, (GOLDEN / "files" / f"{n}.jpg").read_bytes()))
    g = np.load(GOLDEN / "crafted_progressive.npz")
    out += [("crafted:" + k[:-4], g[k].tobytes()) for k in sorted(g.files) if k.endswith(".jpg")]
    rng = np.random.default_rng(11)
    out += [(f"random:{i}", random_progressive(rng, 3000 + i)) for i in range(36)]
    return out


# ---- the crafter ---------------------------------------------------------------------------------------------------------------
def test_the_older_crafters_write_the_bytes_they_wrote():
    """craft_progressive is untouched by the new functions beside it: the committed crafted files come out byte for byte."""
    from tools.craft_jpeg import CRAFTED_PROGRESSIVE as PROGRESSIVE, craft_progressive
    g = np.load(GOLDEN / "crafted_progressive.npz")
    for i, (name, kw) in enumerate(PROGRESSIVE):
        assert craft_progressive(seed=200 + i, **kw) == g[name + ".jpg"].tobytes(), name


def test_the_new_tables_hold_the_lengths_and_sizes_asked_for():
    from tools.craft_jpeg import _codes, long_ac_table, long_dc_table
    ac = _codes(*long_ac_table(0))
    assert {11, 12, 15, 16} <= {l for _, l in ac.values()} and {s & 15 for s in ac} >= set(range(16))
    assert ac[0x0F][1] == 16 and ac[0xE0][1] == 16
    assert _codes(*long_ac_table(1))[0xF0][1] == 12 and _codes(*long_ac_table(1))[0x01][1] == 11
    assert _codes(*long_ac_table(2))[0xF0][1] == 16 and _codes(*long_ac_table(2))[0x01][1] == 16
    dc = _codes(*long_dc_table())
    assert sorted(dc) == list(range(17)) and [dc[s][1] for s in range(10, 17)] == list(range(10, 17))


def test_the_committed_files_are_the_rows(gold):
    assert sorted({k.split(".")[0] for k in gold.files}) == sorted(r.name for r in ROWS)
    for r in ROWS:
        assert gold[r.name + ".jpg"].tobytes() == row_bytes(r.name), r.name
        assert ((r.name + ".refused") in gold.files) == r.refused, r.name
        assert r.big or (len(row_bytes(r.name)) < 4096 and max(_shape(row_bytes(r.name))) <= 64), r.name


def _shape(raw):
    from pyjpegdecoder_amd._parse import parse_jpeg
    p = parse_jpeg(raw)
    return p.image_width, p.image_height


# ---- model, oracle, reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", OK + EXTRA, ids=lambda r: r.name)
def test_model_is_the_oracle_on_the_rows(row):
    assert np.array_equal(walk(row_bytes(row.name)), _oracle(row_bytes(row.name))["coef"])


@pytest.mark.parametrize("row", REFUSED, ids=lambda r: r.name)
def test_model_and_oracle_refuse_the_refused_rows(row, gold):
    with pytest.raises(Refused):
        walk(row_bytes(row.name))
    with pytest.raises(RuntimeError, match="status"):
        _oracle(row_bytes(row.name))
    assert bytes(gold[row.name + ".refused"]).decode() in ("IndexError", "CorruptedJpeg")      # what the reference raised


def test_model_is_the_oracle_on_the_inputs_the_suite_had():
    for name, raw in existing_inputs():
        assert np.array_equal(walk(raw), _oracle(raw)["coef"]), name


@pytest.mark.parametrize("row", OK, ids=lambda r: r.name)
def test_oracle_reproduces_the_reference_on_the_rows(row, gold):
    got = _oracle(row_bytes(row.name))
    assert np.array_equal(got["coef"], gold[row.name + ".coef"])
    assert np.array_equal(got["planes"], gold[row.name + ".planes"])
    assert np.array_equal(got["rgb"], gold[row.name + ".rgb"])


def test_spec_refine_goldens_are_the_models(gold):
    changed = 0
    for r in OK:
        if r.name.startswith("R-"):
            want = walk(row_bytes(r.name), spec_refine=True)
            assert np.array_equal(gold[r.name + ".spec_coef"], want), r.name
            diff = want != gold[r.name + ".coef"]
            assert (gold[r.name + ".coef"][diff] < 0).all(), r.name          # the switch touches negative history only
            changed += bool(diff.any())
    assert changed >= 5


# ---- the census ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS + EXTRA, ids=lambda r: r.name)
def test_every_row_reaches_its_path(row):
    cs = walk_census(row_bytes(row.name))
    print("\n" + pc.census_line(row.name, cs))
    assert row.reached(cs), row.name
    assert bool(cs[-1]["refused"]) == row.refused


def test_window_events_in_stream_terms():
    """A symbol that starts 128 or more bits behind the previous symbol's start (AcWindows::start again), and 65 or more bits of
    consecutive short symbols (advance), in first and in refining scans."""
    s = {r.name: summary(walk_census(row_bytes(r.name))) for r in OK}
    assert s["R-hist"]["gaps_128_up"] >= 1 and s["R-hist"]["gap_bits_max"] >= 150
    assert s["F-ff"]["short_stretch_bits_max"] >= 65 and s["R-sign"]["short_stretch_bits_max"] >= 65
    # a first scan's symbol moves the position by 31 bits at the most (16 + 15), a DC symbol by 32: no 128-bit gap exists there
    assert max(s[n]["gap_bits_max"] for n in s if n.startswith("F-")) <= 31


def test_f_ff_wraps_the_stream_ring():
    """F-ff's AC scan: more than 1 KiB of entropy-coded bytes (the 256-dword ring of the stream walks wraps), dense with stuffed
    0xFF bytes."""
    from pyjpegdecoder_amd._parse import parse_jpeg
    raw = row_bytes("F-ff")
    scan = parse_jpeg(raw).scans[-1]
    seg = raw[scan.entropy_start:scan.entropy_end]
    # (fifteen value bits of ones cover a whole byte wherever they start: a stuffed byte for each of the 31 x 8 symbols of size 15)
    assert scan.spectral_start == 1 and len(seg) > 1024 and seg.count(b"\xff\x00") >= 31 * 8


def census_table():
    before = [(n, summary(walk_census(raw))) for n, raw in existing_inputs()]
    after = [(r.name, summary(walk_census(row_bytes(r.name)))) for r in ROWS + EXTRA]

    def total(rows):
        return [str(max(s[e] for _, s in rows) if e in pc._MAXED else sum(s[e] for _, s in rows)) for e in EVENTS]
    lines = ["input " + " ".join(EVENTS)]
    lines += [n + " " + " ".join(str(s[e]) for e in EVENTS) for n, s in before]
    lines.append("TOTAL_before " + " ".join(total(before)))
    lines += [n + " " + " ".join(str(s[e]) for e in EVENTS) for n, s in after]
    lines.append("TOTAL_rows " + " ".join(total(after)))
    return lines


def test_the_census_table_in_profiles_is_current():
    """profiles/prog_paths_census.txt: what the inputs the suite had reach, and what the rows reach, event by event"""
    assert (ROOT / "profiles" / "prog_paths_census.txt").read_text().splitlines() == census_table()


def test_the_rows_reach_what_the_older_inputs_never_did():
    t = {ln.split()[0]: dict(zip(EVENTS, map(int, ln.split()[1:]))) for ln in census_table() if ln.startswith("TOTAL")}
    b, a = t["TOTAL_before"], t["TOTAL_rows"]
    for e in ("ac_codes_15_16", "ac_sizes_11_15", "dc_codes_10_16", "run_overshoots", "placed_behind_se", "corrections_behind_se",
              "refine_size_above_1", "zrl_crosses_se", "gaps_128_up", "dc_sum_wraps", "refused_scans"):
        assert b[e] == 0 and a[e] > 0, e
    assert b["ac_symbol_bits_max"] < 31 == a["ac_symbol_bits_max"] and b["dc_symbol_bits_max"] < 32 == a["dc_symbol_bits_max"]
    assert b["eobn_max_n"] <= 7 and a["eobn_max_n"] == 14 and a["run_blocks_max"] == 32767


# ---- wrong variants ---------------------------------------------------------------------------------------------------------
def _differs(name, wrong):
    try:
        return not np.array_equal(walk(row_bytes(name)), walk(row_bytes(name), wrong=wrong))
    except Refused:
        return True


@pytest.mark.parametrize("name,wrong", [(r.name, w) for r in ROWS + EXTRA for w in r.wrong])
def test_wrong_variants_are_told_from_the_model(name, wrong):
    assert _differs(name, wrong), pc.WRONG_VARIANTS[wrong]


def test_every_wrong_variant_has_its_row():
    assert {w for r in ROWS + EXTRA for w in r.wrong} == set(pc.WRONG_VARIANTS)


def test_consumed_bits_modulo_32_with_and_without_the_long_symbols():
    """A 5-bit field holds the 31 bits of the longest AC symbol and not the 32 of the longest DC symbol."""
    assert not _differs("F-long", "mod32") and _differs("D-long-16", "mod32") and not _differs("D-long", "mod32")


# ---- the host layer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", OK + EXTRA, ids=lambda r: r.name)
def test_the_host_layer_accepts_the_rows(row):
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import check_supported
    check_supported(parse_jpeg(row_bytes(row.name)))


def test_prepare_batch_takes_every_row():
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    for r in OK:
        prep = prepare_batch([row_bytes(r.name)], B.MJ_LAYOUT_XMAJOR, 0)
        assert len(prep.shapes) == 1, r.name


if __name__ == "__main__":
    (ROOT / "profiles" / "prog_paths_census.txt").write_text("\n".join(census_table()) + "\n")
