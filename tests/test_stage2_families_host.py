"""The input families of tests/stage2_families.py, on the CPU: every family reaches — by the oracle's own planes and IDCT
seam — the rare decision of the fast stage 2 it is named after, in every layout and both output orders; its files decode
(through the oracle) to the blocks that went in; and tools/craft_jpeg.craft_baseline writes what it wrote before it took
blocks= and qts=.  tests/test_stage2_rare_paths.py drives the same images through the kernel."""
import hashlib

import numpy as np
import pytest

import stage2_families as F
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

CASES = [(lay, fam) for lay in F.LAYOUTS for fam in F.families_of(lay)]


def _census(layout, family):
    out = []
    for k, img in enumerate(F.images(layout, family)):
        ref = F.oracle_of(layout, family, k)
        for t in (False, True):
            c = F.census(img, ref, t)
            print(f"{layout} {family} {img.name} {img.width}x{img.height} {'row-major' if t else 'x-major'}: " +
                  ", ".join(f"{k_}={v}" for k_, v in c.items() if k_ not in ("geo", "transposed")))
            out.append((img, ref, t, c))
    return out


@pytest.mark.parametrize("layout,family", CASES)
def test_files_carry_the_blocks_and_stay_inside_int16(layout, family):
    from oracle import oracle
    for k, img in enumerate(F.images(layout, family)):
        ref = F.oracle_of(layout, family, k)
        assert np.array_equal(ref["coef"], img.blocks), "oracle.decode(craft(blocks))['coef'] is not the blocks"
        # the int16 bound of every block: sum |dequantised coefficient| / 4 + 128 <= 32767
        nby = img.factors[0][0] * img.factors[0][1] if len(img.factors) == 3 else 1
        per = nby + 2 if len(img.factors) == 3 else 1
        q = np.stack([img.qts[0] if (j < nby) else img.qts[1] for j in range(per)]).astype(np.int64)
        deq = np.abs(img.blocks.astype(np.int64).reshape(-1, per, 64)) * q[None]
        assert deq.max() <= 32767 and deq.sum(axis=-1).max() <= F.INT16_SUM
        seam = ref["idct"].astype(np.int64)
        assert seam.min() > -32768 and seam.max() < 32767
        # and the write_coef route's expectation is the same picture
        again = oracle.reconstruct(ref["parsed"], img.blocks)
        assert np.array_equal(again["rgb"], ref["rgb"])


@pytest.mark.parametrize("layout", F.COLOUR)
def test_tie_family_reaches_the_b_tie(layout):
    for img, ref, t, c in _census(layout, "tie"):
        assert c["cb125"] >= 1000
        assert c["mcus_bracket"] >= 0.3 * c["mcus"]
        assert c["mcus_far"] == 0
        if layout in F.SUBSAMPLED:
            assert c["cb125_interp_only"] >= 100
        assert c["strips_slow_and_plain"] >= 10                     # tie lanes next to plain ones in one strip


@pytest.mark.parametrize("layout", F.COLOUR)
def test_green_family_reaches_the_patch_threshold(layout):
    for img, ref, t, c in _census(layout, "green"):
        assert c["green_hits"] >= 200
        assert all(n > 0 for n in c["green_by_part"]), c["green_by_part"]          # every 8-row part of the MCU (both halves of a 16-row one)
        assert all(n > 0 for n in c["green_by_turn"]), c["green_by_turn"]          # every turn of a lane (SV = 2 geometries: both)
        assert len(c["green_by_turn"]) == c["geo"].sv
        assert c["strips_green_and_plain"] >= 10
        # ... and in strips the kernel STAGES (whole dwords per run, no slow MCU anywhere in the strip): only there does the patch
        # happen in LDS; elsewhere the hit's lane goes through the exact routine
        assert c["stageable"]
        assert c["green_staged_hits"] >= 200
        assert all(n > 0 for n in c["green_staged_by_part"]), c["green_staged_by_part"]
        assert all(n > 0 for n in c["green_staged_by_turn"]), c["green_staged_by_turn"]
    # hits behind an upsample: MCUs with a gradient (not DC-only chroma) hold hits too
    img, ref = F.images(layout, "green")[0], F.oracle_of(layout, "green", 0)
    nby = img.factors[0][0] * img.factors[0][1]
    graded = (img.blocks.reshape(-1, nby + 2, 64)[:, nby:, 1:] != 0).any(axis=(1, 2)).reshape(img.mcus[1], img.mcus[0])
    mw, mh = F.mcu_px(layout)
    X, Y = np.meshgrid(np.arange(img.width), np.arange(img.height), indexing="ij")
    cb, cr = ref["planes"][..., 1].astype(np.int64) - 128, ref["planes"][..., 2].astype(np.int64) - 128
    hit = (F.green_remainder(cb, cr) >= 24999) & graded[Y // mh, X // mw]
    print(f"{layout} green: {int(hit.sum())} hits in MCUs whose chroma has a gradient")
    assert hit.sum() >= 20


@pytest.mark.parametrize("layout", F.COLOUR)
def test_range_family_reaches_the_r_edge_and_beyond(layout):
    for img, ref, t, c in _census(layout, "range"):
        for comp in ("cb", "cr"):
            for m in (249, 250, 251):
                assert c["src_mag"][comp][m] > 0, (comp, m)
        assert c["src_abs_max"] >= 1000
        assert c["mcus_far"] >= 10 and c["mcus_slow"] <= 0.6 * c["mcus"]
        assert c["strips_slow_and_plain"] >= 4
        # the R tie itself, visible: pixels with |cr| = 250 whose R = Y + 1.402 cr lies inside (0, 255), for odd and for even Y
        yy, cr = ref["planes"][..., 0].astype(np.int64), ref["planes"][..., 2].astype(np.int64) - 128
        r = yy + 1.402 * cr
        at = (np.abs(cr) == 250) & (r > 1) & (r < 254)
        print(f"{layout} range: {int((at & (yy % 2 == 1)).sum())} / {int((at & (yy % 2 == 0)).sum())} pixels at |cr| = 250 with unclamped R and odd / even Y")
        assert (at & (yy % 2 == 1)).sum() >= 20 and (at & (yy % 2 == 0)).sum() >= 20


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
def test_clamp_family_saturates_both_ends(layout):
    for img, ref, t, c in _census(layout, "clamp"):
        assert c["y_min"] <= -300 and c["y_max"] >= 600
        assert c["y_below_0"] >= 1000 and c["y_above_255"] >= 1000
        assert all(n >= 1000 for n in c["sat_0"] + c["sat_255"] + c["unclamped"])


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
def test_wild_family_mixes_the_lanes_of_a_strip(layout):
    for img, ref, t, c in _census(layout, "wild"):
        assert c["y_min"] < -500 and c["y_max"] > 700
        if layout != "grey":
            assert c["src_abs_max"] >= 1000
            assert 0.15 * c["mcus"] <= c["mcus_slow"] <= 0.7 * c["mcus"]
            assert c["strips_slow_and_plain"] >= 3
            # a slow lane, a lane whose green is redone and a plain lane in ONE strip
            assert c["green_hits"] >= 200 and c["strips_all_three"] >= 3


@pytest.mark.parametrize("layout", F.COLOUR)
def test_staged_windows_reach_the_patch_in_the_window_instance(layout):
    """The windows of stage2_families.staged_windows, per image and output order: the window instance can stage their strips, some
    of them cut at the window's top and bottom, and — in the green and the planted images — pixels at the green threshold lie
    in staged strips: in every 8-row part of the MCU, in every turn of a lane, and in strips the window cuts."""
    for family in F.families_of(layout):
        for k, img in enumerate(F.images(layout, family)):
            ref = F.oracle_of(layout, family, k)
            wins = F.staged_windows(img)
            assert "staged" in wins and (family != "green" or "staged_shifted" in wins)
            for name, win in wins.items():
                assert all(v % 4 == 0 for v in win) and win[0] % 8 == 4 and win[1] % 8 == 4 and (win[0] + win[2]) % 8 == 4 and (win[1] + win[3]) % 8 == 4
                for t in (False, True):
                    c = F.window_census(img, ref, win, t)
                    print(f"{layout} {family} {img.name} {name} {win} {'row-major' if t else 'x-major'}: " +
                          ", ".join(f"{k_}={v}" for k_, v in c.items() if k_ != "geo"))
                    assert c["eligible"]
                    if family in ("green", "clamp") or img.name.endswith("_D"):
                        assert c["staged_strips"] >= 4 and c["staged_strips_cut_at_the_top"] >= 1 and c["staged_strips_cut_at_the_bottom"] >= 1
                    if family == "green":
                        assert c["green_staged_hits"] >= 200 and c["green_staged_in_cut_strips"] >= 20
                        assert all(n > 0 for n in c["green_staged_by_part"]), c["green_staged_by_part"]
                        assert all(n > 0 for n in c["green_staged_by_turn"]), c["green_staged_by_turn"]
                    if family == "planted" and name == "staged":
                        assert c["green_staged_hits"] >= 64          # a planted green MCU, the only rare one of its staged strip


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
def test_planted_family_one_rare_mcu_per_strip(layout):
    for img, ref, t, c in _census(layout, "planted"):
        p = F.planted_census(img, ref, t)
        print(f"    planted: {p}")
        assert p["strips_with_more"] == 0 and p["strips_with_one"] == len(img.planted) >= 5
        assert p["first_of_strip"] >= 1 and p["last_of_full_strip"] >= 1
        assert p["first_column"] >= 1 and p["last_column"] >= 1
        assert p["in_last_strip"] >= 1 and 1 <= p["last_strip_rows"] <= 5
        if layout != "grey":
            # the planted MCUs are the rare ones and nothing else is
            assert c["mcus_slow"] + c["mcus_green"] == len(img.planted) and c["mcus_slow"] >= 3 and c["mcus_green"] >= 1
            assert c["strips_slow_and_plain"] >= 3          # (a planted MCU alone in a last strip of one MCU has no neighbour)


def test_sizes_cover_the_store_paths():
    """Between them, the sizes give: H * 3 (row-major: W * 3) both a multiple of 4 and not; a last strip with fewer MCUs than a
    full one; a last strip of fewer than 16 bytes of a column; a partial MCU at the far edge; a batch of two odd-sized images."""
    for layout in F.LAYOUTS:
        nc = len(F.LAYOUTS[layout])
        imgs = [i for fam in F.families_of(layout) for i in F.images(layout, fam)]
        mw, mh = F.mcu_px(layout)
        for t in (False, True):
            geo = F.kernel_geo(layout, t)
            run = [(i.width if t else i.height) for i in imgs]
            across = [(i.height if t else i.width) for i in imgs]
            assert any(r * nc % 4 == 0 for r in run) and (nc == 1 or any(r * nc % 4 for r in run)), (layout, t)
            assert any(geo.mh <= r % geo.strip < geo.strip - geo.mh for r in run), (layout, t)             # a short last strip of whole MCUs
            assert any(0 < (r % geo.strip) * nc < 16 for r in run), (layout, t)
            assert any(a % geo.mw for a in across), (layout, t)
        a, b = F.batch_pair(layout)
        assert (a.width * a.height * nc) % 4 != 0


@pytest.mark.parametrize("args,kw", [
    ((64, 48, [(2, 2), (1, 1), (1, 1)]), dict(seed=3, restart_interval=4)),
    ((200, 120, [(2, 1), (1, 1), (1, 1)]), dict(seed=3, restart_interval=7)),          # (tests/test_roi.py's file)
])
def test_craft_baseline_without_blocks_is_unchanged(args, kw):
    """Calls without blocks= / qts= write the bytes they wrote before the arguments existed (digests taken from the writer as it
    was), and the same random blocks handed back through blocks= with the Annex-K tables through qts= give the same file."""
    from oracle import oracle
    from tools import craft_jpeg
    raw = craft_jpeg.craft_baseline(*args, **kw)
    assert hashlib.sha256(raw).hexdigest() == _OLD_DIGESTS[(args[0], args[1], kw["seed"])]
    coef = oracle.decode(raw)["coef"]
    t = craft_jpeg._T
    again = craft_jpeg.craft_baseline(*args, restart_interval=kw["restart_interval"], blocks=coef,
                                      qts=[np.frombuffer(t["STD_QT_LUMA_ZZ"], dtype=np.uint8), np.frombuffer(t["STD_QT_CHROMA_ZZ"], dtype=np.uint8)])
    # (the random writer draws DC DIFFERENCES and ignores restarts when it does; the decoder's absolute DC handed back gives the same differences)
    assert again == raw


def test_craft_baseline_refuses_what_it_cannot_code():
    from tools import craft_jpeg
    blocks = np.zeros((1, 64), dtype=np.int16)
    blocks[0, 0] = 2048                                        # DC size 12: the Annex-K tables end at 11
    with pytest.raises(AssertionError):
        craft_jpeg.craft_baseline(8, 8, [(1, 1)], blocks=blocks)
    blocks[0, 0], blocks[0, 5] = 0, 1024                       # AC size 11: Annex K ends at 10 ...
    with pytest.raises(AssertionError):
        craft_jpeg.craft_baseline(8, 8, [(1, 1)], blocks=blocks)
    raw = craft_jpeg.craft_baseline(8, 8, [(1, 1)], blocks=blocks, tables=[(0, 2)], ac_tables=[craft_jpeg.wide_ac_table(1)])   # ... wide_ac_table at 15
    from oracle import oracle
    assert np.array_equal(oracle.decode(raw)["coef"], blocks)
    with pytest.raises(AssertionError):
        craft_jpeg.craft_baseline(8, 8, [(1, 1)], blocks=blocks[:, :63])
    with pytest.raises(AssertionError):
        craft_jpeg.craft_baseline(8, 8, [(1, 1)], qts=[np.zeros(64)])


_OLD_DIGESTS = {
    (64, 48, 3): "5620c2b148721a88d72ec12b219a43381f3c2292176c32718595a8776cb6067e",
    (200, 120, 3): "153eecedfa51ba59872ae6dbc391b69de6066b9be8acf31642c9a00b6fc67aa4",
}
