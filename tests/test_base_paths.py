"""The baseline stage 1's rare symbol paths on the GPU: every row of tests/base_cases.py against what the reference made of it
(tests/golden/base_paths.npz), coefficient store and pixels byte for byte, in both layouts and in every decode form — the wave
form, the two lane forms and their launch shapes, the synchronisation form with both counting walks, the GPU marker scan, and
the fused launch with every table width it can be given.  The rows of the common geometry decode as ONE batch, side by side in the
lanes of a wavefront, in two orders.  tests/test_base_paths_host.py proves on the host that each row reaches its path.
Needs a real MI355X: run with `-m gpu`."""
import numpy as np
import pytest

from conftest import GOLDEN
from base_cases import COMMON, EXTRA, OVERSHOOTS, REFUSED, pixel_mask, row_bytes

pytestmark = pytest.mark.gpu

NAMES = [r.name for r in COMMON]
ORDERS = {"ascending": NAMES, "reversed": NAMES[::-1]}
LANES = {"MJ_HUFFMAN": "lanes", "MJ_FUSED": "0"}
FORMS = {      # name: (options, GPU marker scan)
    "wave": ({"MJ_HUFFMAN": "wave"}, False),
    "lanes": (LANES, False),
    "lanes_8_per_wave": (dict(LANES, MJ_LANES_PER_WAVE="8"), False),
    "lanes_64_per_wave": (dict(LANES, MJ_LANES_PER_WAVE="64"), False),
    "lanes_one_wave": (dict(LANES, MJ_LANES_WAVES="1"), False),
    "lanes_ring_64": (dict(LANES, MJ_LANES_RING="64"), False),
    "lanes11": ({"MJ_HUFFMAN": "lanes11", "MJ_FUSED": "0"}, False),
    "sync_classic": ({"MJ_HUFFMAN": "sync", "MJ_SYNC_COUNT": "classic"}, False),
    "sync_resolved_10": ({"MJ_HUFFMAN": "sync", "MJ_SYNC_COUNT": "resolved", "MJ_SYNC_BITS": "10", "MJ_SYNC_CHUNK": "256"}, False),
    "sync_resolved_12": ({"MJ_HUFFMAN": "sync", "MJ_SYNC_COUNT": "resolved", "MJ_SYNC_BITS": "12", "MJ_SYNC_CHUNK": "256"}, False),
    "sync_resolved_13": ({"MJ_HUFFMAN": "sync", "MJ_SYNC_COUNT": "resolved", "MJ_SYNC_BITS": "13", "MJ_SYNC_CHUNK": "256"}, False),
    "gpu_marker_scan": ({}, True),
    "gpu_marker_scan_lanes": (LANES, True),
}
FUSED = {      # name: (options, row-major)
    "default": ({}, False),
    "acbits_10": ({"MJ_FUSED_ACBITS": "10"}, False),
    "acbits_11": ({"MJ_FUSED_ACBITS": "11"}, False),
    "acbits_13": ({"MJ_FUSED_ACBITS": "13"}, False),
    "luma_13": ({"MJ_FUSED_LUMA13": "1"}, False),
    "one_consumer": ({"MJ_FUSED_CONSUMERS": "1"}, False),
    "blob_order": ({"MJ_SEG_ORDER": "blob"}, False),
    "striped": ({"MJ_SEG_ORDER": "striped"}, False),
    "row_major": ({}, True),
    "row_major_acbits_10": ({"MJ_FUSED_ACBITS": "10"}, True),
}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "base_paths.npz")


@pytest.fixture(scope="module")
def ctx():
    from pyjpegdecoder_amd import _binding as B
    c = B.Context(0)
    yield c
    c.close()


def _want_form(B, opts, form):
    """what MJ_HUFFMAN asks for is what the plan reports"""
    kind = opts.get("MJ_HUFFMAN")
    if kind == "wave":
        assert form & 15 == B.MJ_FORM_WAVE, form
    elif kind == "lanes":
        assert form & 15 == B.MJ_FORM_LANES and form & B.MJ_FORM_RESOLVED, form
    elif kind == "lanes11":
        assert form & 15 == B.MJ_FORM_LANES and not form & B.MJ_FORM_RESOLVED, form
    elif kind == "sync":
        assert form & 15 == B.MJ_FORM_SYNC, form
        assert bool(form & B.MJ_FORM_COUNT_RESOLVED) == (opts.get("MJ_SYNC_COUNT") == "resolved"), form
    if opts.get("MJ_FUSED") == "0":
        assert not form & B.MJ_FORM_FUSED, form


def _run(ctx, files, rowmajor=False, flags=0, gpu_scan=False, executes=1):
    """One plan over `files`: (coefficients per file, image per file in the reference's axes, statuses, stage1_form).  With
    executes=3 the coefficient store is POISONED in front of every execute (a fused launch's reconstruction wavefronts read what
    its decoder wavefronts have just written) and the three outputs must be one, as test_gpu_parity._decode_plan holds them."""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    parsed = [parse_jpeg(f, headers_only=True) for f in files] if gpu_scan else None
    prep = prepare_batch(files, B.MJ_LAYOUT_ROWMAJOR if rowmajor else B.MJ_LAYOUT_XMAJOR, flags, parsed)
    plan = B.Plan(ctx, prep.to_c(), {"prep": prep, "n_images": len(files)})
    try:
        form = plan.stage1_form()
        _run.shape = plan.shape()                                 # (mj_debug_plan_shape of the latest plan)
        keep = None
        for k, poison in enumerate((0x5A, 0xC3, 0x7E)[:executes]):
            if executes > 1:
                plan.fill_coef(poison)
            try:
                plan.execute()
                plan.sync()
                out = plan.read(rgb=True, coef=True)
            except B.BackendError as exc:                         # (a device that has reported an error is not given more work)
                pytest.exit(f"the GPU reported an error, nothing more is run on it: {exc}", returncode=3)
            if keep is None:
                keep = out
            else:
                assert np.array_equal(out["rgb"], keep["rgb"]) and np.array_equal(out["coef"], keep["coef"]), f"execute {k} of the plan differs from its first"
                assert np.array_equal(out["status"], keep["status"])
        coefs, imgs, po = [], [], 0
        for k, (w, h, nc) in enumerate(prep.shapes):
            b0 = plan.image_offsets(k)[0]
            b1 = plan.image_offsets(k + 1)[0] if k + 1 < len(files) else plan.info.total_blocks
            coefs.append(keep["coef"][b0:b1])
            px = keep["rgb"][po:po + w * h * nc]
            imgs.append(np.swapaxes(px.reshape(h, w, nc), 0, 1) if rowmajor else px.reshape(w, h, nc))
            po += w * h * nc
        return coefs, imgs, keep["status"], form
    finally:
        plan.close()


def _settled(ctx, files, rowmajor, out, may=()):
    """The synchronisation form hands an image back (MJ_ST_UNCONVERGED) where its chunk records do not chain, and the host layer
    decodes it again with the serial walk (MJ_FLAG_NO_SYNC) — which would hide a counting walk that mis-steps.  So an image
    comes back here only if the test names it in `may` (and says why it must); every other status stays as it is."""
    from pyjpegdecoder_amd import _binding as B
    coefs, imgs, status, form = out
    again = [i for i, s in enumerate(status) if s == B.MJ_ST_UNCONVERGED]
    if again:
        print(f"handed back by the synchronisation rounds: {again}")
        assert form & 15 == B.MJ_FORM_SYNC and set(again) <= set(may), (again, list(may))
        c2, i2, s2, _ = _run(ctx, [files[i] for i in again], rowmajor, flags=B.MJ_FLAG_NO_SYNC)
        status = status.copy()
        for j, i in enumerate(again):
            coefs[i], imgs[i], status[i] = c2[j], i2[j], s2[j]
    return coefs, imgs, status, form


def _hold(gold, names, coefs, imgs, status, tag):
    assert not np.asarray(status).any(), (tag, list(status))
    for name, coef, img in zip(names, coefs, imgs):
        assert np.array_equal(coef, gold[name + ".coef"]), (tag, name, "coefficients")
        keep = pixel_mask(gold[name + ".mask"], *img.shape[:2])
        assert np.array_equal(img[keep], gold[name + ".rgb"][keep]), (tag, name, "pixels")


def test_the_committed_files_are_the_rows(gold):
    for name in NAMES + [r.name for r in REFUSED] + ["G-ragged", "S-all", "S-over", "W-sparse"] + [f"T-own-{i}" for i in range(6)]:
        assert gold[name + ".jpg"].tobytes() == row_bytes(name), name


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("form", list(FORMS))
def test_common_rows_in_one_batch(ctx, gold, tune, form, order):
    """Every healthy row of the common geometry in one batch — 32 restart segments, the lanes of one wavefront in the lane forms —
    in both layouts: the coefficient store and the pixels."""
    from pyjpegdecoder_amd import _binding as B
    opts, gpu_scan = FORMS[form]
    for k, v in opts.items():
        tune(k, v)
    names = ORDERS[order]
    files = [row_bytes(n) for n in names]
    for rowmajor in (False, True):
        out = _run(ctx, files, rowmajor, gpu_scan=gpu_scan)
        if not gpu_scan:
            _want_form(B, opts, out[3])
        else:                                                     # (segment lengths unknown at plan time: never the chunks)
            assert out[3] & 15 in (B.MJ_FORM_WAVE, B.MJ_FORM_LANES) and (out[3] & 15 == B.MJ_FORM_LANES) == ("MJ_HUFFMAN" in opts), out[3]
        assert not out[3] & B.MJ_FORM_FUSED
        # A symbol that lands behind its block voids the chunk records of the RESOLVED counting walk by design (huffman_sync.hip,
        # k_count: "the step does not look for it"): there the rows of OVERSHOOTS come back for the serial walk.  The classic
        # walk leaves such a symbol's value bits unread itself and settles every row, and no other row may come back from
        # either: a segment is at most 24 chunks of 256 bytes (W-dense), a repair round (a link of the resolved walk's repair)
        # settles at least the first chunk that is still wrong, and 32 are queued.
        resolved = opts.get("MJ_SYNC_COUNT") == "resolved"
        may = [i for i, n in enumerate(names) if n in OVERSHOOTS and resolved]
        assert not resolved or all(out[2][i] == B.MJ_ST_UNCONVERGED for i in may), list(out[2])
        _hold(gold, names, *_settled(ctx, files, rowmajor, out, may)[:3], (form, order, "rowmajor" if rowmajor else "xmajor"))


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("variant", list(FUSED))
def test_common_rows_through_the_fused_launch(ctx, gold, tune, variant, order):
    """The same batch as ONE launch of both stages: the producers run lanes13_walk.h with tables of their own widths (a 12-bit main
    level, or 10 / 11 / 13; component 0's at 13), second-level tables packed back to back, DC tables cut to 8 bits.  Three executes
    with the coefficient store poisoned; coefficients read back as well."""
    from pyjpegdecoder_amd import _binding as B
    opts, rowmajor = FUSED[variant]
    tune("MJ_HUFFMAN", "lanes")
    for k, v in opts.items():
        tune(k, v)
    names = ORDERS[order]
    files = [row_bytes(n) for n in names]
    layout = B.MJ_LAYOUT_ROWMAJOR if rowmajor else B.MJ_LAYOUT_XMAJOR
    # W-dense's segments are a hundred times the others' length: left alone the plan deals the segments out by length (mode 2)
    by_length = opts.get("MJ_SEG_ORDER") != "blob"
    coefs, imgs, status, form = _run(ctx, files, rowmajor, executes=3)
    assert form & B.MJ_FORM_FUSED and form & 15 == B.MJ_FORM_LANES and form & B.MJ_FORM_RESOLVED, form
    # what the PLAN decided (mj_debug_plan_shape: 1 fused, 12 segment order, 25 segments dealt out by length = the hand-off across
    # workgroups, mode 2) — and the rule's answer for a batch of that order
    shape = _run.shape
    assert shape[1] == 1 and shape[12] == (2 if by_length else 0) and shape[25] == int(by_length), shape[:28]
    assert B.fused_applies_rule(layout, 2, 2, 4, 2, 4, n_images=len(files), traits=2 if shape[12] == 2 else 0) == (2 if by_length else 1)
    _hold(gold, names, coefs, imgs, status, (variant, order))


@pytest.mark.parametrize("form", ["lanes", "lanes11", "wave"])
def test_a_lane_past_its_last_mcu_while_the_others_go_on(ctx, gold, tune, form):
    """G-ragged (restart interval 3: segments of 3, 3 and 2 MCUs) in one batch with the common rows (4 and 4)."""
    from pyjpegdecoder_amd import _binding as B
    opts = FORMS[form][0]
    for k, v in opts.items():
        tune(k, v)
    names = NAMES[:5] + ["G-ragged"] + NAMES[5:]
    files = [row_bytes(n) for n in names]
    for rowmajor in (False, True):
        coefs, imgs, status, got = _run(ctx, files, rowmajor)
        _want_form(B, opts, got)
        _hold(gold, names, coefs, imgs, status, (form, rowmajor))


def test_ragged_segments_through_the_row_major_fused_launch(ctx, gold, tune):
    from pyjpegdecoder_amd import _binding as B
    tune("MJ_HUFFMAN", "lanes")
    assert B.fused_applies_rule(B.MJ_LAYOUT_ROWMAJOR, 2, 2, 4, 2, 3, n_images=2) == 1
    names = ["G-ragged", "G-ragged"]
    coefs, imgs, status, form = _run(ctx, [row_bytes(n) for n in names], True, executes=3)
    assert form & B.MJ_FORM_FUSED, form
    _hold(gold, names, coefs, imgs, status, "G-ragged")


@pytest.mark.parametrize("form", ["wave", "lanes", "lanes11", "sync_classic", "sync_resolved_12", "fused_row_major"])
def test_many_blocks_to_a_dword_then_a_dense_block(ctx, gold, tune, form):
    """W-sparse (its own geometry, 16 MCUs to the row): 210 blocks of five bits, the stream window not advanced, then 63 symbols
    of 29 bits."""
    from pyjpegdecoder_amd import _binding as B
    opts = {"MJ_HUFFMAN": "lanes"} if form == "fused_row_major" else FORMS[form][0]
    for k, v in opts.items():
        tune(k, v)
    files = [row_bytes("W-sparse")] * 3
    for rowmajor in ((True,) if form == "fused_row_major" else (False, True)):
        out = _run(ctx, files, rowmajor, executes=3 if form == "fused_row_major" else 1)
        _want_form(B, opts, out[3])
        assert bool(out[3] & B.MJ_FORM_FUSED) == (form == "fused_row_major")
        _hold(gold, ["W-sparse"] * 3, *_settled(ctx, files, rowmajor, out)[:3], (form, rowmajor))      # (healthy, five chunks: none may come back)


@pytest.mark.parametrize("chunk", ["256", "512"])
@pytest.mark.parametrize("count", ["classic", "resolved"])
def test_every_row_back_to_back_without_restart_markers(ctx, gold, tune, count, chunk):
    """S-all through the synchronisation form: the rare symbols at many offsets of the chunks, D-wrap's wrapped DC sums carried
    across chunk records (16-bit fields, packed adds) — host test: across boundaries of 256 and of 512 bytes.  It must SETTLE ON
    THE DEVICE, status 0, with both counting walks at both chunk sizes: a file that came back would be decoded by the serial walk,
    and a counting walk that mis-stepped on a 31-bit DC symbol or a second-level code would go unseen.  A repair round (a link of
    the resolved walk's repair) settles at least the first chunk that is still wrong, and W-dense's part, 44 chunks of 256 bytes
    of 29-bit symbols, does not synchronise by itself: as many rounds as chunks are needed.  32 are queued by default — enough
    for the 31 chunks of 512 bytes; for the 61 of 256 the test queues 64 (MJ_SYNC_ROUNDS).
    S-over, the rows with a symbol behind its block: settles with the classic walk (which leaves that symbol's value bits
    unread), comes back from the resolved one by design."""
    from pyjpegdecoder_amd import _binding as B
    opts = {"MJ_HUFFMAN": "sync", "MJ_SYNC_COUNT": count, "MJ_SYNC_CHUNK": chunk}
    if chunk == "256":
        opts["MJ_SYNC_ROUNDS"] = "64"
    for k, v in opts.items():
        tune(k, v)
    for name in ("S-all", "S-over"):
        files = [row_bytes(name)]
        for rowmajor in (False, True):
            out = _run(ctx, files, rowmajor)
            _want_form(B, opts, out[3])
            assert _run.shape[5] == int(chunk) and _run.shape[6] <= int(opts.get("MJ_SYNC_ROUNDS", 32)), _run.shape[:8]
            back = name == "S-over" and count == "resolved"
            assert out[2][0] == (B.MJ_ST_UNCONVERGED if back else 0), (name, list(out[2]))
            _hold(gold, [name], *_settled(ctx, files, rowmajor, out, [0] if back else ())[:3], (name, count, chunk, rowmajor))


@pytest.mark.parametrize("name", ["S-all", "S-over"])
def test_every_row_back_to_back_on_the_serial_walk(ctx, gold, name):
    from pyjpegdecoder_amd import _binding as B
    coefs, imgs, status, form = _run(ctx, [row_bytes(name)], flags=B.MJ_FLAG_NO_SYNC)
    assert form & 15 != B.MJ_FORM_SYNC, form
    _hold(gold, [name], coefs, imgs, status, "no_sync")


@pytest.mark.parametrize("force", [None, "lanes", "sync", "wave"])
def test_files_with_four_tables_of_their_own(ctx, gold, tune, force):
    """T-own: 24 tables in a batch of six files — more than the lane forms hold at once.  The form the plan reports is recorded;
    what is pinned is the result."""
    from pyjpegdecoder_amd import _binding as B
    if force:
        tune("MJ_HUFFMAN", force)
    names = [f"T-own-{i}" for i in range(6)]
    files = [row_bytes(n) for n in names]
    for rowmajor in (False, True):
        out = _run(ctx, files, rowmajor)
        print(f"T-own, MJ_HUFFMAN {force}: form {out[3]:#x}")
        assert not out[3] & B.MJ_FORM_RESOLVED and not out[3] & B.MJ_FORM_FUSED, out[3]      # (24 tables: no resolved tables, no fused launch)
        assert force != "wave" or out[3] == B.MJ_FORM_WAVE
        _hold(gold, names, *_settled(ctx, files, rowmajor, out)[:3], (force, rowmajor))      # (healthy files: none may come back)


@pytest.mark.parametrize("force", ["lanes", "sync"])
def test_files_with_their_own_tables_in_runs_of_64(ctx, gold, tune, force):
    """T-own again, every file 64 times in a row: a workgroup's segments now come from two files at the most, its table list fits,
    and the lane form loads each workgroup's own tables (MJ_FORM_WG_TABLES) — the tables of the crafted symbols among them."""
    from pyjpegdecoder_amd import _binding as B
    tune("MJ_HUFFMAN", force)
    names = [f"T-own-{i}" for i in range(6) for _ in range(64)]
    files = [row_bytes(n) for n in names]
    out = _run(ctx, files)
    print(f"T-own x 64, MJ_HUFFMAN {force}: form {out[3]:#x}")
    assert out[3] in (B.MJ_FORM_LANES | B.MJ_FORM_WG_TABLES, B.MJ_FORM_SYNC | B.MJ_FORM_WG_TABLES, B.MJ_FORM_WAVE), out[3]
    _hold(gold, names, *_settled(ctx, files, False, out)[:3], force)                     # (segments of a few chunks: none may come back)


@pytest.mark.parametrize("form", list(FORMS) + ["fused_" + v for v in FUSED])
def test_the_32_bit_dc_symbol_against_the_oracle(ctx, tune, form):
    """D-size-16: a 16-bit DC code with 16 value bits, in every form and fused variant the common rows run in.  The reference has
    no result (its array library refuses the sum), so this file is held to the oracle.  A DC size above 15 has no place in the
    resolved counting tables: never MJ_FORM_COUNT_RESOLVED, whatever MJ_SYNC_COUNT asks for."""
    from oracle import oracle
    from pyjpegdecoder_amd import _binding as B
    fused = form.startswith("fused_")
    opts, second = FUSED[form[6:]] if fused else FORMS[form]
    opts = dict(opts, MJ_HUFFMAN="lanes") if fused else opts
    for k, v in opts.items():
        tune(k, v)
    raw = row_bytes(EXTRA[0].name)
    want = oracle.decode(raw)
    files = [raw, row_bytes("A-fin"), raw]
    for rowmajor in ((second,) if fused else (False, True)):
        out = _run(ctx, files, rowmajor, gpu_scan=(not fused and second), executes=3 if fused else 1)
        assert not out[3] & B.MJ_FORM_COUNT_RESOLVED, out[3]
        if opts.get("MJ_SYNC_COUNT") == "resolved":               # (asked for, and not given)
            assert out[3] & 15 == B.MJ_FORM_SYNC, out[3]
        elif fused or not second:
            _want_form(B, opts, out[3])
        assert bool(out[3] & B.MJ_FORM_FUSED) == fused, out[3]
        coefs, imgs, status, _ = _settled(ctx, files, rowmajor, out)          # (three healthy files of two chunks a segment: none may come back)
        assert not status.any(), list(status)
        for i in (0, 2):
            assert np.array_equal(coefs[i], want["coef"]), (form, rowmajor, i)
            assert np.array_equal(imgs[i], want["rgb"]), (form, rowmajor, i)


STATUS = {"bad_code": "MJ_ST_BAD_CODE", "desync": "MJ_ST_DESYNC", "overrun": "MJ_ST_OVERRUN"}


@pytest.mark.parametrize("form", ["wave", "lanes", "lanes11", "sync_classic", "fused"])
@pytest.mark.parametrize("row", REFUSED, ids=lambda r: r.name)
def test_refused_rows_end_in_their_status_and_leave_their_neighbours_alone(ctx, gold, tune, row, form):
    """One damaged file per call, healthy rows on both sides, one execute: the file ends in the status of its kind (all of them
    CorruptedJpeg to the caller), never MJ_ST_INTERNAL; the healthy rows come out byte for byte."""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd import CorruptedJpeg
    from pyjpegdecoder_amd.batch import raise_for_status
    opts = {"MJ_HUFFMAN": "lanes"} if form == "fused" else FORMS[form][0]
    for k, v in opts.items():
        tune(k, v)
    names = ["A-63", "A-over", row.name, "A-wait", "D-wrap"]
    files = [row_bytes(n) for n in names]
    out = _run(ctx, files)
    _want_form(B, opts, out[3])
    assert bool(out[3] & B.MJ_FORM_FUSED) == (form == "fused")
    coefs, imgs, status, _ = _settled(ctx, files, False, out)      # (nothing may come back: the refused row's status is this form's, the classic walk settles its neighbours)
    print(f"{row.name} {form}: status {list(status)}")
    assert B.MJ_ST_INTERNAL not in list(status)
    assert status[2] == getattr(B, STATUS[row.refused]), list(status)
    with pytest.raises(CorruptedJpeg):
        raise_for_status(status.copy(), list(range(5)))
    keep = [0, 1, 3, 4]
    _hold(gold, [names[i] for i in keep], [coefs[i] for i in keep], [imgs[i] for i in keep], status[keep], (row.name, form))
