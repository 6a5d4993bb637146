"""What the request-route tests share (tests/test_request_routes.py on the MI355X, tests/test_request_routes_host.py with a
stand-in back end): ONE expectation for a file under (window, size, dtype, normalize, mirror flag, layout), the call's
interleaved file list with its windows and flags, the damaged calls, and the reading of the plans a call made — which files
every plan held, which went round again, into which slots.

The expectation is the oracle's pixels sliced to the window; with ``size`` tools/resize_model.resize of them,
tools/normalize_model.normalize for a float dtype (bit patterns), the flip along the width for a set flag; then the layout."""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from conftest import GOLDEN
from test_resize import as_layout, rowmajor_window
from test_roi import _corrupt_segment, mcu_size, window_kinds

LAYOUT_NAMES = ("xmajor", "rowmajor", "planar", "planar_rowmajor")          # by MJ_LAYOUT_* value
SIZE = (40, 28)
# per component and all different: a swapped channel shows
NORMALIZE = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))

_resized = {}


def create_with(lib, ctx, batch_c, h, **fields) -> int:
    """mj_plan_create_with(ctx, &batch_c, &request, &h) as a C caller makes it: ``fields`` are mj_plan_request's, the rest of the
    request zeroed — ctypes arrays of RoiC / PlaceC as they are, an OutputDescC by pointer, NumPy arrays by address."""
    import ctypes

    from pyjpegdecoder_amd import _binding as B
    r = B.PlanRequestC()
    for name, v in fields.items():
        setattr(r, name, v.ctypes.data if isinstance(v, np.ndarray) else ctypes.pointer(v) if isinstance(v, B.OutputDescC) else v)
    return lib.mj_plan_create_with(ctx, None if batch_c is None else ctypes.byref(batch_c), ctypes.byref(r), ctypes.byref(h))


def expected(full: np.ndarray, win=None, size=None, dtype=None, normalize=None, mirror: bool = False, layout: str = "xmajor",
             key=None) -> np.ndarray:
    """One file's output: ``full`` is the oracle's (W, H[, 3]) image.  uint8 pixels, or the bit patterns (uint16 / uint32) of
    a float ``dtype``.  ``key``: something that names ``full`` — the resize is then kept per (key, window, size)."""
    from tools import normalize_model, resize_model
    win = tuple(int(v) for v in win) if win is not None else (0, 0, full.shape[0], full.shape[1])
    img = rowmajor_window(full, win)
    if size is None:
        assert dtype in (None, "uint8") and normalize is None and not mirror, "dtype, normalize and mirror need size"
        return as_layout(img, layout)
    k = (key, win, tuple(size))
    if key is None or k not in _resized:
        _resized[k] = resize_model.resize(img, tuple(size))
    out = _resized[k]
    name = dtype or ("float32" if normalize is not None else "uint8")
    if name != "uint8":
        mean, std = normalize if normalize is not None else (None, None)
        if out.ndim == 2 and mean is not None:
            mean, std = float(np.ravel(mean)[0]), float(np.ravel(std)[0])
        out = normalize_model.normalize(out, name, mean, std)
    if mirror:
        out = out[:, ::-1]
    return as_layout(out, layout)


def differ(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a, b)


def bits_of(t) -> np.ndarray:
    """A result (NumPy array, or torch tensor on the GPU) as uint8 pixels or as the bit patterns of its float elements."""
    if isinstance(t, np.ndarray):
        return t if t.dtype == np.uint8 else t.view({2: np.uint16, 4: np.uint32}[t.dtype.itemsize])
    from test_normalize import bits_of as torch_bits
    return torch_bits(t)


# ---- the call ---------------------------------------------------------------------------------------------------------------
@dataclass
class CallFile:
    name: str
    raw: bytes
    kind: str                       # "ordinary" | "declined" (the native front end hands it to Python) | "tail" | "unconverged"
    window: object                  # which of test_roi.window_kinds, or (x, y, width, height)
    mirror: bool
    full: Optional[np.ndarray] = None
    win: Optional[tuple] = None


def with_com(raw: bytes) -> bytes:
    """A COM segment between the scan and EOI: the GPU marker scan hands such a file back (MJ_ST_TAIL)."""
    assert raw[-2:] == b"\xff\xd9"
    return raw[:-2] + b"\xff\xfe\x00\x06abcd" + b"\xff\xd9"


def without_one_restart_marker(raw: bytes, seg: int = 2) -> bytes:
    from pyjpegdecoder_amd._parse import parse_jpeg
    off = int(parse_jpeg(raw).scans[0].segment_offsets[seg])
    assert raw[off - 2] == 0xFF and 0xD0 <= raw[off - 1] <= 0xD7
    return raw[:off - 2] + raw[off:]


def finish(entries: List[CallFile]) -> List[CallFile]:
    """Every entry's oracle pixels and its window (test_roi.window_kinds of its size and MCU)."""
    from oracle import oracle
    for e in entries:
        e.full = oracle.decode(e.raw)["rgb"]
        e.win = window_kinds(e.full.shape[0], e.full.shape[1], *mcu_size(e.raw))[e.window] if isinstance(e.window, str) else e.window
    return entries


_call = []


def call_files() -> List[CallFile]:
    """The call every route decodes: three-component files of every kind, no kind contiguous; tail and unconverged files at
    non-adjacent positions, none the first file of its first-round plan when the call goes in one piece (the plans are: 4:2:0
    with restart markers 0 3 7 12, 4:4:4 with restart markers 2 6 11, 4:2:0 without 1 4 8 10, the progressive file 5, the odd
    layout 9) or as ITER_BATCHES — assert_second_rounds holds the plans a call made to that.  (Cut into three parts the plans
    are smaller, and there some second-round files do lead theirs.)  Files of equal size have different windows; the flags
    follow neither the kinds nor the positions."""
    if _call:
        return _call
    from tools import synth
    g = np.load(GOLDEN / "odd_layouts.npz")
    odd = sorted(k for k in g.files if k.endswith(".jpg"))[0]
    s = synth.synth_jpeg
    # restart intervals of one or two MCUs and small files without markers: under the options that keep the synchronisation
    # rounds from settling (256-byte chunks, no run-up, no repair rounds) a segment of one chunk still decodes in the first round
    entries = [
        CallFile("a0_420_dri1", s(501, 200, 120, 85, "420", 1), "ordinary", "inner", True),
        CallFile("c0_420_nodri_small", s(502, 32, 16, 60, "420", 0, 2.0), "ordinary", "last_mcu", False),
        CallFile("b0_444_dri2", s(503, 96, 64, 85, "444", 2), "ordinary", "aligned", False),
        CallFile("tail_com_420_dri1", with_com(s(504, 200, 120, 85, "420", 1)), "tail", "last_mcu", True),
        CallFile("unconverged_0", s(4242, 640, 480, 85, "420", 0, 12.0), "unconverged", (37, 21, 90, 50), True),
        CallFile("prog_70x50_420", (GOLDEN / "files" / "prog_70x50_420_pil.jpg").read_bytes(), "declined", (10, 9, 33, 21), False),
        CallFile("tail_many_markers", s(77, 512, 512, 85, "444", 1, 10.0), "tail", "inner", True),
        CallFile("a1_420_dri1", s(505, 200, 120, 85, "420", 1), "ordinary", "row", False),
        CallFile("tail_com_420_nodri_small", with_com(s(506, 32, 16, 60, "420", 0, 2.0)), "tail", "inner", False),
        CallFile("odd_" + odd[:-4], g[odd].tobytes(), "declined", "full", True),
        CallFile("unconverged_1", s(4243, 640, 480, 85, "420", 0, 12.0), "unconverged", "last_mcu", False),
        CallFile("b1_444_dri2", s(507, 96, 64, 85, "444", 2), "ordinary", (17, 3, 40, 40), True),
        CallFile("a2_420_dri1", s(508, 200, 120, 85, "420", 1), "ordinary", "aligned", True),
    ]
    _call.extend(finish(entries))
    return _call


def positions(entries: List[CallFile], kind: str) -> List[int]:
    return [i for i, e in enumerate(entries) if e.kind == kind]


# the iterator's batches, as positions in the call: ordinary files of one kind (one pipelined plan), tail and declined files
# (the one-call path; each tail file behind an ordinary one of its kind), files without restart markers — one pipelined plan
# whose collect() sends the tail and the unconverged files round again — and an empty batch
ITER_BATCHES = ([0, 7], [2, 12, 3, 5, 6, 9, 11], [1, 4, 8, 10], [])

# (rois, size, dtype, normalize, mirror) of a call — True: the call's own windows / flags
COMBINATIONS = {
    "none": dict(rois=False, size=None, dtype=None, normalize=None, mirror=False),
    "rois": dict(rois=True, size=None, dtype=None, normalize=None, mirror=False),
    "size": dict(rois=False, size=SIZE, dtype=None, normalize=None, mirror=False),
    "size_rois": dict(rois=True, size=SIZE, dtype=None, normalize=None, mirror=False),
    "float16": dict(rois=True, size=SIZE, dtype="float16", normalize=NORMALIZE, mirror=True),
    "float32": dict(rois=True, size=SIZE, dtype="float32", normalize=NORMALIZE, mirror=True),
    "bfloat16": dict(rois=True, size=SIZE, dtype="bfloat16", normalize=NORMALIZE, mirror=True),
}


def call_kwargs(entries: List[CallFile], combo: dict, rois_allowed: bool = True) -> dict:
    """The keyword arguments of decode / decode_device for these files under a combination."""
    kw = {}
    if combo["rois"] and rois_allowed:
        kw["rois"] = [e.win for e in entries]
    if combo["size"] is not None:
        kw["size"] = combo["size"]
    if combo["dtype"] is not None:
        kw.update(dtype=combo["dtype"], normalize=combo["normalize"])
    if combo["mirror"]:
        kw["mirror"] = [e.mirror for e in entries]
    return kw


def expectation(e: CallFile, combo: dict, layout: str, rois_allowed: bool = True, win="own", mirror="own") -> np.ndarray:
    w = (e.win if win == "own" else win) if (combo["rois"] and rois_allowed) else None
    m = (e.mirror if mirror == "own" else mirror) if combo["mirror"] else False
    return expected(e.full, w, combo["size"], combo["dtype"], combo["normalize"] if combo["dtype"] else None, m, layout,
                    key=e.name)


def check_outputs(got, entries: List[CallFile], combo: dict, layout: str, what, rois_allowed: bool = True):
    """Slot by slot: a list of ragged outputs or one dense array / tensor, against the expectation of every file."""
    assert len(got) == len(entries), what
    if combo["size"] is not None and len(entries):
        got = bits_of(got)
    for i, e in enumerate(entries):
        want = expectation(e, combo, layout, rois_allowed)
        have = got[i] if combo["size"] is not None else bits_of(got[i])
        assert have.dtype == want.dtype and have.shape == want.shape, (what, i, e.name, have.shape, want.shape)
        assert np.array_equal(have, want), (what, i, e.name)


def window_fits(win, e: CallFile) -> bool:
    x, y, w, h = win
    return x + w <= e.full.shape[0] and y + h <= e.full.shape[1]


def neighbours(entries: List[CallFile], i: int) -> List[int]:
    """the file before and the file after file ``i`` of the call"""
    return [j for j in (i - 1, i + 1) if 0 <= j < len(entries)]


def assert_expectations_tell_files_apart(entries: List[CallFile], combos, layouts, rois_allowed: bool = True):
    """Without this the slot-by-slot comparison could pass for a decoder that mixes files up: for every combination the
    expectations of all files are pairwise different, a file's expectation changes with its flag, and it changes when the file
    is given the window of the file before it, of the file after it, or of any other file of the call.  A window that does not
    lie inside the file (a small file beside a large one) is left out: no image comes of it — mj_plan_create refuses the
    plan, which test_request_routes.py holds the library to for exactly these pairs, and the stand-in plan of
    test_request_routes_host.py refuses it likewise — so such a mix-up raises and cannot pass."""
    for cname in combos:
        combo = COMBINATIONS[cname]
        for layout in layouts:
            want = [expectation(e, combo, layout, rois_allowed) for e in entries]
            for i in range(len(entries)):
                for j in range(i + 1, len(entries)):
                    assert differ(want[i], want[j]), (cname, layout, entries[i].name, entries[j].name)
            if combo["mirror"]:
                for i, e in enumerate(entries):
                    assert differ(want[i], expectation(e, combo, layout, rois_allowed, mirror=not e.mirror)), (cname, layout, e.name)
            if combo["rois"] and rois_allowed:
                for i, e in enumerate(entries):
                    for j, o in enumerate(entries):
                        if j != i and window_fits(o.win, e):
                            assert differ(want[i], expectation(e, combo, layout, win=o.win)), (cname, layout, e.name, "with the window of", o.name)


def windows_that_do_not_fit(entries: List[CallFile]):
    """[(file, window of the file before or after it that does not lie inside it)]"""
    return [(e, entries[j].win) for i, e in enumerate(entries) for j in neighbours(entries, i) if not window_fits(entries[j].win, e)]


# ---- the damaged calls ------------------------------------------------------------------------------------------------------
def damaged_calls():
    """[(what, entries, position of the damaged file, plan-local position it must NOT be reported at)] — mixed kinds; the
    damaged file is the second of its kind, so its position in its plan (1, and 0 in a second round) is not its position in
    the call (3).  Once a first-round file (a restart marker removed: MJ_ST_DESYNC from the GPU's own segmentation), once a
    tail file (a COM segment behind the scan and a restart segment without a Huffman code: found in the second round)."""
    from tools import synth
    s = synth.synth_jpeg
    good = s(601, 200, 120, 85, "420", 13)
    first_round = without_one_restart_marker(s(602, 200, 120, 85, "420", 13))
    second_round = with_com(_corrupt_segment(s(603, 200, 120, 85, "420", 13), 1))
    out = []
    for what, bad in (("first_round", first_round), ("second_round", second_round)):
        entries = [CallFile("e0_444", s(604, 96, 64, 85, "444", 2), "ordinary", "inner", False),
                   CallFile("e1_420", good, "ordinary", "inner", True),
                   CallFile("e2_nodri", s(605, 32, 16, 60, "420", 0, 2.0), "ordinary", "inner", False),
                   CallFile("e3_damaged", bad, "damaged", "inner", True),
                   CallFile("e4_444", s(606, 96, 64, 85, "444", 2), "ordinary", "inner", True)]
        out.append((what, entries, 3))
    return out


def one_kind_batch() -> List[CallFile]:
    """Five good 4:2:0 files with restart markers: the native front end takes them as ONE pipelined plan."""
    from tools import synth
    return finish([CallFile(f"p{i}_420", synth.synth_jpeg(610 + i, 200, 120, 85, "420", 13), "ordinary", "inner", bool(i & 1))
                   for i in range(5)])


def damaged_one_kind_calls():
    """[(what, entries, position of the damaged file)] — files of ONE kind (4:2:0 with restart markers), which the native
    front end makes one pipelined plan of, so that the error comes out of a NARROWED request whose positions are not the
    call's.  "in_parts": six files for decode_device(parts=3), the last without one restart marker — file 5 of the call is
    file 1 of the third part.  "collects_redo": one batch of the iterator with a good tail file at 1 and a corrupt one at 4 —
    collect() sends those two round again as a request of their own, in whose plans the corrupt file is file 1."""
    from tools import synth
    s = synth.synth_jpeg
    in_parts = one_kind_batch() + [CallFile("p5_damaged", without_one_restart_marker(s(615, 200, 120, 85, "420", 13)), "damaged", "inner", True)]
    redo = [CallFile("q0_420", s(620, 200, 120, 85, "420", 13), "ordinary", "inner", False),
            CallFile("q1_tail", with_com(s(621, 200, 120, 85, "420", 13)), "tail", "inner", True),
            CallFile("q2_420", s(622, 200, 120, 85, "420", 13), "ordinary", "inner", True),
            CallFile("q3_420", s(623, 200, 120, 85, "420", 13), "ordinary", "inner", False),
            CallFile("q4_damaged", with_com(_corrupt_segment(s(624, 200, 120, 85, "420", 13), 1)), "damaged", "inner", True)]
    return [("in_parts", in_parts, 5), ("collects_redo", redo, 4)]


def assert_reported_from_a_narrowed_request(what, held: List[List[int]], at: int):
    """``held``: the files of every plan of the failed call, in the order the plans were made.  The plan that reported the
    damaged file is the latest that held it; the file's position in it is not ``at`` — a message that names the plan's own
    position would not pass for the right one."""
    holders = [h for h in held if at in h]
    assert holders, (what, "no plan held the damaged file", held)
    reporter = holders[-1]
    assert reporter.index(at) != at, (what, "the damaged file sits at its call position in the plan that reported it", reporter)
    if what == "in_parts":
        assert reporter == [4, 5] and len(holders) == 1, (what, "the third part is not a plan of its own", held)
    if what == "collects_redo":
        assert holders[0] == list(range(5)), (what, "the batch was not one pipelined plan", held)
        assert reporter == [1, 4] and len(holders) >= 2, (what, "the damage was not found in collect()'s redo", held)


def good_call():
    return [e for e in call_files() if e.kind in ("ordinary", "declined")]


# ---- reading the plans of a call --------------------------------------------------------------------------------------------
@dataclass
class PlanRecord:
    n_images: int
    flags: int
    slots: Optional[tuple]          # (slot of every image, slots of the array) as the plan was given them
    files: List[bytes]              # the plan's files, read back from its blob


def record_of(batch_c, keepalive, slots) -> PlanRecord:
    prep = keepalive["prep"]
    offs = [int(o) for o in prep.file_offsets]
    blobs = [prep.blob[offs[k]:offs[k + 1]].tobytes() for k in range(len(offs) - 1)]
    sl = None if slots is None else ([int(v) for v in slots[0]], int(slots[1]))
    return PlanRecord(int(batch_c.n_images), int(batch_c.flags), sl, blobs)


def files_of(rec: PlanRecord, raws: List[bytes]) -> List[int]:
    """Which files of ``raws`` (all different) a plan holds, in the plan's order."""
    out = []
    for chunk in rec.files:
        hits = [i for i, r in enumerate(raws) if (len(r) + 3) & ~3 == len(chunk) and chunk.startswith(r)]
        assert len(hits) == 1, "a plan holds a file that is not of this call, or the call's files are not all different"
        out.append(hits[0])
    assert len(out) == rec.n_images
    return out


def records_by_batch(records: List[PlanRecord], raws: List[bytes], batches) -> List[List[PlanRecord]]:
    """The plans of an iterator's run sorted by the batch (``batches``: positions in ``raws``) whose files they hold."""
    out = [[] for _ in batches]
    for rec in records:
        owners = {next(k for k, b in enumerate(batches) if i in b) for i in files_of(rec, raws)}
        assert len(owners) == 1, "a plan holds files of two batches"
        out[owners.pop()].append(rec)
    return out


def assert_second_rounds(records: List[PlanRecord], entries: List[CallFile], dense_on_device: bool, what,
                         one_plan_each: bool = True, redo_is_a_request: bool = False):
    """The plans of ONE call (or one batch), in the order they were made: every file is in a first plan; the files that went
    round again under MJ_FLAG_NO_SYNC are exactly the unconverged ones, the others that went round again exactly the tail
    files; nothing else was decoded twice.  ``dense_on_device``: every plan's slots are its files' positions in the call.
    ``one_plan_each``: the call is not cut into parts — one MJ_FLAG_NO_SYNC plan holds all unconverged files, and no file that
    goes round again is the first of its first plan (where slot 0 of a plan is also right by accident).
    ``redo_is_a_request``: the iterator's collect() sends tail and unconverged files through the one-call path together, whose
    own first plan holds both before they part."""
    from pyjpegdecoder_amd import _binding as B
    raws = [e.raw for e in entries]
    seen, again_sync, again_tail, nosync_plans, first_at = set(), [], [], [], {}
    for rec in records:
        idxs = files_of(rec, raws)
        for k, i in enumerate(idxs):
            first_at.setdefault(i, k)
        if dense_on_device:
            assert rec.slots is not None and rec.slots == (idxs, len(entries)), (what, rec.slots, idxs)
        later = [i for i in idxs if i in seen]
        if rec.flags & B.MJ_FLAG_NO_SYNC:
            assert later == idxs, (what, "a first-round plan carries MJ_FLAG_NO_SYNC", idxs)
            again_sync += idxs
            nosync_plans.append(sorted(idxs))
        elif later:
            assert later == idxs, (what, "a plan mixes first-round and second-round files", idxs)
            again_tail += idxs
        seen.update(idxs)
    assert seen == set(range(len(entries))), (what, "files without a plan", sorted(set(range(len(entries))) - seen))
    tail, unconverged = positions(entries, "tail"), positions(entries, "unconverged")
    assert sorted(again_sync) == unconverged, (what, "MJ_FLAG_NO_SYNC plans held", sorted(again_sync), "unconverged", unconverged)
    # (a tail file without restart markers that met the synchronisation form again in its second round would be among the
    # MJ_FLAG_NO_SYNC files as well, which the line above forbids: the call's tail files are small enough not to)
    if redo_is_a_request:
        assert set(again_tail) - set(unconverged) == set(tail), (what, "second-round plans held", sorted(again_tail), "tail", tail)
        assert sorted(i for i in again_tail if i in unconverged) in ([], unconverged), (what, again_tail)
    else:
        assert sorted(again_tail) == tail, (what, "second-round plans held", sorted(again_tail), "tail", tail)
    if one_plan_each:
        assert nosync_plans == ([unconverged] if unconverged else []), (what, nosync_plans)
        assert all(first_at[i] > 0 for i in tail + unconverged), (what, "a second-round file leads its first plan", first_at)
