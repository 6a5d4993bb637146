"""The strip worker's DC-only blocks (csrc/reconstruct_fast_strips.h, phase A) against the oracle: rounds of eight blocks that
mix DC-only and AC blocks in every group position, through the stage-2 kernel alone (production and seam instance, both
output orders) and through the fused launch; and the offline issue-cost tool (tools/issue_cost.py) on a hand-written snippet.

A strip's blocks are numbered bt = MCU-in-strip * blocks-per-MCU + block; round r handles bt = 8r .. 8r + 7, block bt in the
8-lane group bt % 8.  4:2:0 at 64 x 64 is four strips (one per MCU column in x-major output, one per MCU row in row-major) of
24 blocks = 3 rounds; 4:1:1 at 256 x 32 is eight strips of 24 blocks in x-major and four of 48 (6 rounds) in row-major.  (With
strips twice as tall as the 64 lanes' MCUs — strip_sv — no layout has a half-empty last round any more: 4:1:1's used to.)
GPU tests need a real MI355X: run with `-m gpu`."""
import functools

import numpy as np
import pytest

import stage2_families as F
from conftest import GOLDEN, ROOT

ORDERS = ("xmajor", "rowmajor")
SIZES = {"420": (64, 64), "411": (256, 32)}
CASES = ("all_dc", "none_dc", "one_dc", "one_ac", "negative", "mod8", "wrap", "zero", "flagged")


# ---- the blocks of a case ------------------------------------------------------------------------------------------------
def _strips(layout, order):
    """(number of strips, blocks per strip, index function (strip, bt) -> block number in the file's MCU order)."""
    w, h = SIZES[layout]
    mw, mh = F.mcu_px(layout)
    mcw, mch = w // mw, h // mh
    nb = sum(a * b for a, b in F.LAYOUTS[layout])
    tmw = F.kernel_geo(layout, order == "rowmajor").tmw
    if order == "xmajor":            # a strip = tmw MCU rows of one MCU column
        assert mch == tmw
        return mcw, tmw * nb, lambda s, bt: ((bt // nb) * mcw + s) * nb + bt % nb
    assert mcw == tmw                # row-major: the worker runs on the transposed image, a strip = tmw MCUs of one MCU row
    return mch, tmw * nb, lambda s, bt: (s * mcw + bt // nb) * nb + bt % nb


@functools.lru_cache(maxsize=None)
def tie_blocks():
    """Golden blocks (dequantised, [x][y]) with AC coefficients whose exact IDCT has a sample ON a half-integer: the fp32 level
    must flag them (its error there is 0.5 up to rounding).  Returned in zig-zag order."""
    from pyjpegdecoder_amd._parse import ZZ_GRID
    g = np.load(GOLDEN / "idct_blocks.npz")["blocks"].astype(np.int64)
    u = np.arange(8)
    K = 0.5 * np.where(u == 0, np.sqrt(0.5), 1.0)[None, :] * np.cos((2 * u[:, None] + 1) * u[None, :] * np.pi / 16)      # K[x][u]
    out = []
    for b in g:
        if not np.any(b.reshape(64)[1:]):
            continue
        s = K @ b.astype(np.float64) @ K.T            # (ties are integer combinations that cancel exactly: 1e-9 is far above float64 noise)
        if np.abs(np.abs(s - np.floor(s)) - 0.5).min() > 1e-9:
            continue
        zz = np.zeros(64, dtype=np.int64)
        for x in range(8):
            for y in range(8):
                zz[ZZ_GRID[y, x]] = b[x, y]
        out.append(zz)
        if len(out) == 16:
            break
    return out


def build(case, layout, order):
    """(blocks int16 [n, 64], (luma table, chroma table), which[strip][bt] in {'dc', 'ac', 'flag'})."""
    rng = np.random.default_rng([20261018, CASES.index(case), list(SIZES).index(layout), ORDERS.index(order)])
    n_strips, nbt, at = _strips(layout, order)
    nb = sum(a * b for a, b in F.LAYOUTS[layout])
    nby = nb - 2
    ql, qc = np.full(64, 3, dtype=np.uint8), np.full(64, 5, dtype=np.uint8)
    if case == "mod8":
        ql, qc = np.full(64, 4, dtype=np.uint8), np.full(64, 1, dtype=np.uint8)
    elif case == "wrap":
        ql, qc = np.full(64, 1, dtype=np.uint8), np.full(64, 1, dtype=np.uint8)
        ql[0], qc[0] = 7, 2
    elif case == "flagged":
        ql, qc = np.full(64, 1, dtype=np.uint8), np.full(64, 1, dtype=np.uint8)
    blocks = np.zeros((n_strips * nbt, 64), dtype=np.int64)
    which = [[None] * nbt for _ in range(n_strips)]
    ties = tie_blocks() if case == "flagged" else []
    for s in range(n_strips):
        for bt in range(nbt):
            r, p = divmod(bt, 8)
            luma = bt % nb < nby
            mark = (3 * s + r) % 8
            if case == "all_dc":
                kind = "dc"
            elif case == "none_dc":
                kind = "ac"
            elif case == "one_dc":
                kind = "dc" if p == mark else "ac"
            elif case == "one_ac":
                kind = "ac" if p == mark else "dc"
            elif case == "flagged":
                # round r: a DC-only block at `mark`, a flagged block beside it; and the flagged block of round r + 1 sits where
                # round r had its DC-only block (the DC-only block of round r + 1 where round r had its flagged one)
                a, b = (s + 2) % 8, (s + 5) % 8
                kind = "dc" if p == (a if r % 2 == 0 else b) else ("flag" if p == (b if r % 2 == 0 else a) else ("ac" if (p + s) % 3 else "dc"))
            else:
                kind = "dc" if (p + r + s) % 2 == 0 else "ac"
            which[s][bt] = kind
            v = np.zeros(64, dtype=np.int64)
            if kind == "flag":
                v = ties[(s * nbt + bt) % len(ties)].copy()
            else:
                q0 = int(ql[0] if luma else qc[0])
                if case == "negative":
                    v[0] = -int(rng.integers(1, 1000 // q0))
                elif case == "mod8":                  # DC * q = 4 (mod 8), both signs: an exact tie of DC * q / 8
                    v[0] = int(rng.choice((-1, 1))) * ((2 * int(rng.integers(0, 100)) + 1) if luma else (8 * int(rng.integers(0, 100)) + 4))
                elif case == "wrap" and kind == "dc":
                    # DC * q as int16: 32767, -32767, 98301 -> 32765, -98301 -> -32765 (luma, q = 7); 32766, -32768, 32768 -> -32768, -32770 -> 32766 (chroma, q = 2)
                    v[0] = int(rng.choice((4681, -4681, 14043, -14043) if luma else (16383, -16384, 16384, -16385)))
                elif case == "zero" and kind == "dc":
                    v[0] = 0
                else:
                    v[0] = int(rng.integers(-1000 // q0, 1000 // q0 + 1))
                if kind == "ac":
                    for k in rng.choice(np.arange(1, 20), size=int(rng.integers(1, 4)), replace=False):
                        v[k] = int(rng.choice((-12, -7, -3, -1, 1, 2, 5, 12)))
                    if case == "one_ac" and rng.random() < 0.5:      # the only AC coefficient of the round in the block's LAST row
                        v[1:] = 0
                        v[63] = 1
            blocks[at(s, bt)] = v
    assert blocks.min() >= -32768 and blocks.max() <= 32767
    return blocks.astype(np.int16), (ql, qc), which


def test_cases_cover_every_group_position():
    """Host only: across the strips of a case every one of the eight group positions is the round's only DC-only block (one_dc)
    and its only AC block (one_ac); every mixed case has luma and chroma DC-only blocks in one round; `flagged` has, in some
    round, a flagged block beside a DC-only one and in the next round each in the other's position."""
    for layout in SIZES:
        nb = sum(a * b for a, b in F.LAYOUTS[layout])
        for order in ORDERS:
            for case, lone in (("one_dc", "dc"), ("one_ac", "ac")):
                _, _, which = build(case, layout, order)
                seen = set()
                for strip in which:
                    for r in range(len(strip) // 8):
                        pos = [p for p in range(8) if strip[8 * r + p] == lone]
                        assert len(pos) == 1
                        seen.add(pos[0])
                assert seen == set(range(8)), (layout, order, case, seen)
            for case in ("negative", "mod8", "wrap", "zero", "all_dc"):
                _, _, which = build(case, layout, order)
                both = 0
                for strip in which:
                    for r in range(len(strip) // 8):
                        dcs = [8 * r + p for p in range(8) if strip[8 * r + p] == "dc"]
                        both += any(bt % nb < nb - 2 for bt in dcs) and any(bt % nb >= nb - 2 for bt in dcs)
                        assert case == "all_dc" or any(strip[8 * r + p] == "ac" for p in range(8))
                assert both > 0, (layout, order, case)
            _, _, which = build("flagged", layout, order)
            for strip in which:
                for r in range(len(strip) // 8 - 1):
                    dc = [p for p in range(8) if strip[8 * r + p] == "dc"]
                    fl = [p for p in range(8) if strip[8 * r + p] == "flag"]
                    assert len(fl) == 1 and dc
                    assert strip[8 * (r + 1) + fl[0]] == "dc" and any(strip[8 * (r + 1) + p] == "flag" for p in dc)
    blocks, (ql, qc), which = build("wrap", "420", "xmajor")
    dq = (blocks[:, 0].astype(np.int64) * np.where(np.arange(len(blocks)) % 6 < 4, int(ql[0]), int(qc[0]))).astype(np.int16)
    assert {32767, -32767, -32768} <= set(dq.tolist())
    assert len(tie_blocks()) >= 4


# ---- stage 2 alone -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decs():
    from pyjpegdecoder_amd import BatchDecoder
    d = {order: BatchDecoder(device=0, layout=order, segment="host") for order in ORDERS}
    yield d
    for x in d.values():
        x.close()


@functools.lru_cache(maxsize=None)
def _carrier(layout, tables):
    """A file of this geometry and these tables with all-zero blocks (the plan's geometry; the coefficients are written), parsed."""
    from tools import craft_jpeg
    from oracle import oracle
    w, h = SIZES[layout]
    nb = sum(a * b for a, b in F.LAYOUTS[layout])
    mw, mh = F.mcu_px(layout)
    qts = tuple(np.frombuffer(t, dtype=np.uint8) for t in tables)
    raw = craft_jpeg.craft_baseline(w, h, F.LAYOUTS[layout], restart_interval=w // mw,
                                    blocks=np.zeros(((w // mw) * (h // mh) * nb, 64), dtype=np.int16), qts=qts)
    return raw, oracle.decode(raw)["parsed"]


def _stage2(dec, raw, blocks, flags):
    from pyjpegdecoder_amd import _binding as B
    _, plan = dec.plan([raw], flags)
    try:
        plan.write_coef(blocks)
        plan.execute_stage2()
        plan.sync()
        seams = bool(flags & B.MJ_FLAG_KEEP_PLANES)
        out = plan.read(rgb=True, planes=seams, idct=seams)
        out["levels"] = plan.idct_levels() if seams else None
    finally:
        plan.close()
    assert not out["status"].any()
    return out


def _laid_out(rgb, order):
    return np.ascontiguousarray(rgb.swapaxes(0, 1) if order == "rowmajor" else rgb)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("layout", list(SIZES))
@pytest.mark.parametrize("case", CASES)
def test_mixed_rounds_through_stage2(decs, case, layout, order):
    """Host-written coefficients through the production instance of the stage-2 kernel and through its seam instance: pixels,
    IDCT seam and planes are the oracle's, and the level counts say that no DC-only block was sent on by level 1 (DC * q = 4
    mod 8 is an exact tie of the fp32 transform: only the DC-only mask keeps such a block off level 2) while every planted tie
    block was."""
    from pyjpegdecoder_amd import _binding as B
    from oracle import oracle
    blocks, (ql, qc), which = build(case, layout, order)
    raw, parsed = _carrier(layout, (ql.tobytes(), qc.tobytes()))
    want = oracle.reconstruct(parsed, blocks, want_idct=True)
    w = _laid_out(want["rgb"], order)
    fast = _stage2(decs[order], raw, blocks, 0)["rgb"].reshape(w.shape)
    bad = np.argwhere(fast != w)
    assert bad.shape[0] == 0, f"{bad.shape[0]} bytes differ, first at {bad[0].tolist()}"
    seam = _stage2(decs[order], raw, blocks, B.MJ_FLAG_KEEP_PLANES | B.MJ_FLAG_KEEP_IDCT)
    assert np.array_equal(seam["idct"].reshape(want["idct"].shape), want["idct"])
    assert np.array_equal(seam["planes"].reshape(want["planes"].shape), want["planes"])
    assert np.array_equal(seam["rgb"].reshape(w.shape), w)
    n_blocks, sent_on, _ = seam["levels"]
    kinds = [k for strip in which for k in strip]
    assert n_blocks == len(kinds)
    assert kinds.count("flag") <= sent_on <= len(kinds) - kinds.count("dc"), (seam["levels"], kinds.count("flag"), kinds.count("dc"))


# ---- the fused launch ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused_files():
    """Four 128 x 64 4:2:0 files, one restart interval per MCU row: MCU columns 0-1 flat (DC-only blocks), 2-3 noisy, 4-7 both
    inside one MCU (which blocks of the MCU are flat differs from MCU to MCU and file to file)."""
    from tools import craft_jpeg
    out = []
    for k in range(4):
        rng = np.random.default_rng([20261018, 77, k])
        mcw, mch, nb = 8, 4, 6
        blocks = np.zeros((mch, mcw, nb, 64), dtype=np.int64)
        blocks[..., 0] = rng.integers(-100, 101, size=(mch, mcw, nb))
        noisy = np.zeros((mch, mcw, nb), dtype=bool)
        noisy[:, 2:4] = True
        noisy[:, 4:] = rng.random((mch, mcw - 4, nb)) < 0.5
        ac = np.rint(rng.laplace(0.0, 6.0, size=(mch, mcw, nb, 64)) * np.exp(-np.arange(64) / 10.0)).astype(np.int64)
        ac[..., 0] = 0
        ac[..., 1] |= 1                                   # (a noisy block has an AC coefficient for certain)
        blocks += ac * noisy[..., None]
        out.append(craft_jpeg.craft_baseline(128, 64, F.LAYOUTS["420"], restart_interval=mcw, blocks=blocks.reshape(-1, 64).astype(np.int16),
                                             qts=(np.full(64, 6, dtype=np.uint8), np.full(64, 9, dtype=np.uint8))))
    return tuple(out)


def _execute_poisoned(ctx, prep, n, torch, opts):
    """(output, statuses, stage1_form) of a plan under library options: the coefficient store poisoned, then one execute."""
    from pyjpegdecoder_amd import _binding as B
    for k, v in opts:
        B.set_option(k, v)
    try:
        dev = torch.device("cuda", 0)
        d_blob = torch.from_numpy(prep.blob).to(dev)
        torch.cuda.synchronize()
        plan = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), {"prep": prep, "n_images": n})
        try:
            out = torch.zeros(plan.info.rgb_bytes, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            plan.fill_coef(0x5A)
            plan.execute(0, out.data_ptr())
            plan.sync()
            return out.cpu().numpy(), plan.read(rgb=False)["status"], plan.stage1_form()
        finally:
            plan.close()
    finally:
        for k, _ in opts:
            B.set_option(k, None)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_fused_launch_on_flat_and_noisy_content(decs, order):
    """The smallest uniform batch (16 files, doubled until the plan reports MJ_FORM_FUSED) of files with flat, noisy and mixed MCUs:
    the fused launch's bytes are the two launches', every distinct file is the oracle's image, every status is 0."""
    torch = pytest.importorskip("torch")
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    from oracle import oracle
    dec, files = decs[order], fused_files()
    n = 16
    while True:
        batch = [files[i % len(files)] for i in range(n)]
        prep = prepare_batch(batch, dec.layout, 0)
        fused, st, form = _execute_poisoned(dec.ctx, prep, n, torch, [("MJ_HUFFMAN", "lanes")])
        if form & B.MJ_FORM_FUSED or n >= 1024:
            break
        n *= 2
    assert form & B.MJ_FORM_FUSED, (n, form)
    assert not st.any()
    two, st2, form2 = _execute_poisoned(dec.ctx, prep, n, torch, [("MJ_HUFFMAN", "lanes"), ("MJ_FUSED", "0")])
    assert not form2 & B.MJ_FORM_FUSED and not st2.any()
    assert np.array_equal(fused, two), "the fused launch differs from the two launches"
    got = fused.reshape(n, -1)
    for k, f in enumerate(files):
        w = _laid_out(oracle.decode(f)["rgb"], order).reshape(-1)
        for i in range(k, n, len(files)):
            assert np.array_equal(got[i], w), (k, i)


# ---- tools/issue_cost.py -------------------------------------------------------------------------------------------------
def test_issue_cost_tool_classes():
    """Host only: the tool parses the committed probe file and a snippet written for this test (tests/golden/issue_cost_snippet.s);
    a VOP2 select on VCC, a VOP3 select on an SGPR pair, an add with an SGPR source and a plain add fall into four different
    cost classes, priced in that order from dear to cheap."""
    import io
    from tools import issue_cost as ic
    costs = ic.parse_probe(ROOT / "profiles" / "r02_issue_rate_probe.txt")
    assert costs["v_add_u32"] < 1.5 and costs["v_cndmask_b32"] > 10 and costs["v_cndmask_b32 e64 sgpr mask"] < 3.5
    got = {}
    for mn, ops in (("v_cndmask_b32_e32", "v0, v9, v0, vcc"), ("v_cndmask_b32_e64", "v0, v9, v0, s[2:3]"),
                    ("v_add_u32_e32", "v1, s7, v62"), ("v_add_u32_e32", "v1, v7, v62")):
        got[(mn, ops)] = ic.classify(mn, ops, costs)
    classes = [c for c, _ in got.values()]
    assert classes == ["select_vop2_vcc", "select_e64", "sgpr_operand", "simple"] and len(set(classes)) == 4
    cyc = [k for _, k in got.values()]
    assert cyc[0] > cyc[2] > cyc[1] > cyc[3]
    buf = io.StringIO()
    assert ic.report(GOLDEN / "issue_cost_snippet.s", ["k_snippet<2,false>"], costs, min_valu=1, out=buf) == 1
    text = buf.getvalue()
    assert "phaseA-round" in text and "phaseB-pixels" in text
    rows = {ln.split()[0]: ln for ln in text.splitlines() if ln.strip().startswith((".LBB", "%bb", "entry"))}
    assert "select_vop2_vcc 4" in rows[".LBB0_2"] and "select_e64 4" in rows[".LBB0_3"]
    assert ic.mangled_fragment("k_fused<2,2,false,false>") == "k_fusedILi2ELi2ELb0ELb0EE"
