"""BatchDecoder.decode's routing without a GPU: `_binding.Context` and `_binding.Plan` are stand-ins (as tests/test_queue.py does
for the image queue).  The stand-in plan computes every image with the oracle and the resize / normalize models from the
keyword arguments `Plan` is given — rois, size, slots, output, each per image of THAT plan — and returns scripted statuses:
MJ_ST_TAIL for the tail files while the GPU would segment them, MJ_ST_UNCONVERGED for the unconverged ones until the plan
carries MJ_FLAG_NO_SYNC, a corrupt status for a damaged file.  An image whose status is not 0 is left as filler bytes.  So what
is held to the expectation here is the host's part alone: which file, window, flag and slot every plan of a call gets, what
comes back in which place, and which position an error names.  The stand-in reads nothing of batch._Request."""
from types import SimpleNamespace

import numpy as np
import pytest

from routes_common import (COMBINATIONS, ITER_BATCHES, LAYOUT_NAMES, assert_expectations_tell_files_apart,
                           assert_reported_from_a_narrowed_request, assert_second_rounds, call_files, call_kwargs, check_outputs,
                           damaged_calls, damaged_one_kind_calls, expected, files_of, finish, one_kind_batch, positions, record_of,
                           records_by_batch, windows_that_do_not_fit)

HOST_COMBOS = ("none", "rois", "size", "size_rois", "float16", "float32")
FILLER = 0xEE


class _Backend:
    """The stand-in device: statuses by file (``script``: raw bytes -> "tail" | "unconverged" | ("corrupt", status) |
    ("tail_corrupt", status)), the plans made, how many are open."""

    def __init__(self, script=None, known=()):
        self.script = dict(script or {})
        self.records, self.plans, self.contexts, self.pixels = [], [], [], {}
        self.known = list(known)            # the files a natively assembled batch may hold (it keeps no parse of them)
        self.tensors = {}                   # address -> array of every stand-in tensor (see _torch_stand_in)

    def raw_of(self, prep, k: int) -> bytes:
        if prep.parsed[k] is not None:
            return prep.parsed[k].raw
        chunk = prep.blob[int(prep.file_offsets[k]):int(prep.file_offsets[k + 1])].tobytes()
        (raw,) = [r for r in self.known if (len(r) + 3) & ~3 == len(chunk) and chunk.startswith(r)]
        return raw

    def full(self, raw: bytes) -> np.ndarray:
        from oracle import oracle
        if raw not in self.pixels:
            self.pixels[raw] = oracle.decode(raw)["rgb"]
        return self.pixels[raw]

    def install(self, monkeypatch):
        from pyjpegdecoder_amd import _binding as B
        be = self

        class Context:
            def __init__(self, device=0):
                self.device, self.closed = device, False
                be.contexts.append(self)

            def wait_event(self, hip_event):
                pass

            def close(self):
                self.closed = True

        class Plan:
            def __init__(self, ctx, batch_c, keepalive, rois=None, size=None, slots=None, output=None):
                prep = keepalive["prep"]
                n = int(batch_c.n_images)
                assert n == keepalive["n_images"] == len(prep.parsed)
                for name, per_image in (("rois", rois), ("slots", slots[0] if slots is not None else None),
                                        ("mirror", output[3] if output is not None else None)):
                    assert per_image is None or len(per_image) == n, f"{name}: {len(per_image)} entries for a plan of {n} images"
                assert size is not None or (slots is None and output is None)
                for k, (w, h, _) in enumerate(prep.shapes if rois is not None else ()):     # as mj_plan_create does
                    x, y, ww, wh = rois[k]
                    if ww <= 0 or wh <= 0 or x < 0 or y < 0 or x + ww > w or y + wh > h:
                        raise B.BackendError(f"image {k}: window (x {x}, y {y}, width {ww}, height {wh}) is empty or not inside the {w}x{h} image")
                self.raws = [be.raw_of(prep, k) for k in range(n)]
                self.layout, self.flags = LAYOUT_NAMES[int(batch_c.layout)], int(batch_c.flags)
                self.rois, self.size, self.slots, self.output = rois, size, slots, output
                self.closed = self.executed = False
                self.dest = None
                be.records.append(record_of(batch_c, keepalive, slots))
                be.plans.append(self)
                self.status = np.array([self._status(r) for r in self.raws], dtype=np.int32)
                # (a file whose status is not 0 has no pixels: the oracle refuses a damaged one)
                self.images = [self._image(k) if self.status[k] == 0 else None for k in range(n)]
                es = B.DTYPE_BYTES[output[0]] if output is not None else 1
                self.nbytes = [(size[0] * size[1] if size is not None else (rois[k][2] * rois[k][3] if rois is not None else w * h)) * nc * es
                               for k, (w, h, nc) in enumerate(prep.shapes)]
                assert all(im is None or im.nbytes == nb for im, nb in zip(self.images, self.nbytes))
                self.info = SimpleNamespace(rgb_bytes=self.nbytes[0] * int(slots[1]) if (slots is not None and n) else sum(self.nbytes))

            def _status(self, raw: bytes) -> int:
                role = be.script.get(raw)
                gpu_segmented = bool(self.flags & B.MJ_FLAG_GPU_SEGMENT)
                if role == "tail" or (isinstance(role, tuple) and role[0] == "tail_corrupt"):
                    if gpu_segmented:
                        return B.MJ_ST_TAIL
                    return role[1] if isinstance(role, tuple) else 0
                if role == "unconverged":
                    return 0 if self.flags & B.MJ_FLAG_NO_SYNC else B.MJ_ST_UNCONVERGED
                if isinstance(role, tuple) and role[0] == "corrupt":
                    return role[1]
                return 0

            def _image(self, k: int) -> np.ndarray:
                dtype, mean, std, mirror = self.output if self.output is not None else (None, None, None, None)
                return expected(be.full(self.raws[k]), self.rois[k] if self.rois is not None else None, self.size, dtype,
                                (mean, std) if mean is not None else None, bool(mirror[k]) if mirror is not None else False,
                                self.layout, key=self.raws[k])

            def _filled(self) -> np.ndarray:
                """the plan's output: images back to back, or with ``size`` one slot per image of an array of ``slots[1]``"""
                if self.size is None:
                    parts = [im.tobytes() if im is not None else bytes([FILLER]) * nb for im, nb in zip(self.images, self.nbytes)]
                    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
                out = np.full(self.info.rgb_bytes, FILLER, dtype=np.uint8)
                per = self.nbytes[0] if self.nbytes else 0
                for k, im in enumerate(self.images):
                    s = int(self.slots[0][k]) if self.slots is not None else k
                    if im is not None:
                        out[s * per:(s + 1) * per] = np.frombuffer(im.tobytes(), dtype=np.uint8)
                return out

            def execute(self, stream=0, rgb_device=None):
                assert not self.closed
                self.executed = True
                if isinstance(rgb_device, int) and rgb_device:
                    rgb_device = be.tensors[rgb_device]
                if isinstance(rgb_device, np.ndarray) and self.size is None:          # a caller's buffer: the images back to back
                    rgb_device.reshape(-1).view(np.uint8)[:self.info.rgb_bytes] = self._filled()
                elif isinstance(rgb_device, np.ndarray):                              # a caller's array: only this plan's slots
                    flat, per = rgb_device.reshape(-1).view(np.uint8), self.nbytes[0]
                    mine = self._filled()
                    for k, st in enumerate(self.status):
                        s = int(self.slots[0][k]) if self.slots is not None else k
                        if st == 0:
                            flat[s * per:(s + 1) * per] = mine[s * per:(s + 1) * per]

            def sync(self):
                assert self.executed and not self.closed

            def read(self, rgb=True, coef=False, planes=False, idct=False):
                assert self.executed and not self.closed
                return {"rgb": self._filled() if rgb else None, "coef": None, "planes": None, "idct": None, "status": self.status.copy()}

            def close(self):
                self.closed = True

        monkeypatch.setattr(B, "Context", Context)
        monkeypatch.setattr(B, "Plan", Plan)
        return self

    def take_records(self):
        out, self.records = self.records, []
        return out


def _script(entries):
    return {e.raw: e.kind for e in entries if e.kind in ("tail", "unconverged")}


def test_the_expectations_tell_the_files_of_the_call_apart():
    assert_expectations_tell_files_apart(call_files(), HOST_COMBOS + ("bfloat16",), ("xmajor", "planar_rowmajor"))
    assert_expectations_tell_files_apart(call_files(), ("size_rois", "float16"), ("rowmajor", "planar"))
    entries = call_files()
    tail, unconverged = positions(entries, "tail"), positions(entries, "unconverged")
    assert len(tail) >= 2 and len(unconverged) >= 2
    for pos in (tail, unconverged):
        assert all(b - a > 1 for a, b in zip(pos, pos[1:]))
    flags = [e.mirror for e in entries]
    assert 5 <= sum(flags) <= 8
    for kind in ("ordinary", "tail", "unconverged", "declined"):
        assert len({entries[i].mirror for i in positions(entries, kind)}) == 2, kind
    for i, a in enumerate(entries):
        for b in entries[i + 1:]:
            assert a.full.shape != b.full.shape or a.win != b.win, (a.name, b.name)


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
@pytest.mark.parametrize("combo", HOST_COMBOS)
def test_decode_every_slot_through_second_rounds(monkeypatch, combo, layout):
    """segment="gpu": the tail files go round again host-segmented, the unconverged ones under MJ_FLAG_NO_SYNC, and every
    slot of the call holds its own file, window and flag."""
    from pyjpegdecoder_amd import BatchDecoder
    entries = call_files()
    be = _Backend(_script(entries)).install(monkeypatch)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        got = dec.decode([e.raw for e in entries], **call_kwargs(entries, COMBINATIONS[combo]))
        assert isinstance(got, list) == (COMBINATIONS[combo]["size"] is None)
        check_outputs(got, entries, COMBINATIONS[combo], layout, (combo, layout))
        assert_second_rounds(be.take_records(), entries, False, (combo, layout))
        assert all(p.closed for p in be.plans)
    finally:
        dec.close()
    assert all(c.closed for c in be.contexts)


def test_decode_host_segmentation_has_no_second_round(monkeypatch):
    from pyjpegdecoder_amd import BatchDecoder
    entries = call_files()
    be = _Backend({e.raw: "tail" for e in entries if e.kind == "tail"}).install(monkeypatch)
    dec = BatchDecoder(device=0, layout="xmajor", segment="host")
    try:
        for combo in HOST_COMBOS:
            got = dec.decode([e.raw for e in entries], **call_kwargs(entries, COMBINATIONS[combo]))
            check_outputs(got, entries, COMBINATIONS[combo], "xmajor", combo)
            records = be.take_records()
            assert sum(r.n_images for r in records) == len(entries), "a file was decoded twice"
    finally:
        dec.close()


@pytest.mark.parametrize("combo", ["size", "size_rois", "float16", "float32", "bfloat16"])
def test_plans_of_parts_of_a_request_fill_their_own_slots_of_one_array(monkeypatch, combo):
    """The device routes give every plan (slots of its files, slots of the array) and one array for all plans: a request
    narrowed to each kind's files, then to the files that go round again, through BatchDecoder._plan, as _decode_request does."""
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import OutputSpec, _group_by_kind, _Request, normalize_rois, prepare_batch
    entries = call_files()
    c = COMBINATIONS[combo]
    raws = [e.raw for e in entries]
    be = _Backend(_script(entries)).install(monkeypatch)
    dec = BatchDecoder(device=0, layout="planar_rowmajor", segment="gpu", gpu_segment_min_files=1)
    es = {None: 1, "float16": 2, "bfloat16": 2, "float32": 4}[c["dtype"]]
    dest = np.full((len(entries), 3, c["size"][1], c["size"][0] * es), FILLER, dtype=np.uint8)
    out = OutputSpec(c["dtype"], c["normalize"][0], c["normalize"][1], [e.mirror for e in entries]) if c["dtype"] else None
    wins = normalize_rois([e.win for e in entries], [e.full.shape[:2] for e in entries]) if c["rois"] else None
    req = _Request(raws, wins, c["size"], out, dest, list(range(len(entries))))
    parsed = {}
    work = [(idxs, 0) for idxs in _group_by_kind(raws, range(len(raws)), parsed, True)]
    assert len(work) >= 5
    try:
        while work:
            idxs, flags = work.pop(0)
            sub = req.narrow(idxs)
            prep = prepare_batch(sub.files, dec.layout, flags, [parsed[i] for i in idxs])
            plan = dec._plan(sub, prep)
            plan.execute(0, dest)
            st = plan.read(rgb=False)["status"]
            plan.close()
            tail = [i for i, s in zip(idxs, st) if s == B.MJ_ST_TAIL]
            unconverged = [i for i, s in zip(idxs, st) if s == B.MJ_ST_UNCONVERGED]
            assert not set(st.tolist()) - {0, B.MJ_ST_TAIL, B.MJ_ST_UNCONVERGED}
            if tail:
                from pyjpegdecoder_amd._parse import parse_jpeg
                parsed.update({i: parse_jpeg(raws[i]) for i in tail})
                work.append((tail, 0))
            if unconverged:
                work.append((unconverged, B.MJ_FLAG_NO_SYNC))
        got = dest.reshape(len(entries), -1).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[es]).reshape(len(entries), 3, c["size"][1], c["size"][0])
        check_outputs(got, entries, c, "planar_rowmajor", combo)
        assert_second_rounds(be.take_records(), entries, True, combo)
    finally:
        dec.close()


@pytest.mark.parametrize("what", ["first_round", "second_round"])
def test_errors_name_the_position_in_the_call(monkeypatch, what):
    """A damaged file at position 3 of the call, second of its plan (and alone in its second-round plan): the message names 3."""
    from pyjpegdecoder_amd import BatchDecoder, CorruptedJpeg
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.errors import BackendError
    entries, at = next((e, a) for w, e, a in damaged_calls() if w == what)
    bad = entries[at].raw
    role = ("corrupt", B.MJ_ST_DESYNC) if what == "first_round" else ("tail_corrupt", B.MJ_ST_BAD_CODE)
    text = "restart markers are not where" if what == "first_round" else "no Huffman code"
    raws = [e.raw for e in entries]
    good = finish([e for e in entries if e is not entries[at]])
    for kw in ({}, {"size": (16, 12), "mirror": [True, False, True, False, True]}):
        be = _Backend({bad: role}).install(monkeypatch)
        dec = BatchDecoder(device=0, segment="gpu", gpu_segment_min_files=1)
        try:
            with pytest.raises(CorruptedJpeg, match=rf"^image {at}: Failed to decode image \({text}") as err:
                dec.decode(raws, **kw)
            assert not isinstance(err.value, BackendError)
            records = be.take_records()
            assert all(p.closed for p in be.plans), "a plan stayed open behind the exception"
            # ... and 3 is not where the file sits in the plan that reported it
            assert records[-1].files.index(next(f for f in records[-1].files if f.startswith(bad))) != at
            assert (len(records[-1].files) == 1) == (what == "second_round")
            got = dec.decode([e.raw for e in good])
            check_outputs(got, good, COMBINATIONS["none"], "xmajor", (what, "after the exception"))
            assert all(p.closed for p in be.plans)
        finally:
            dec.close()
    # MJ_ST_INTERNAL is not the file's fault: BackendError, with the position in the call as well
    be = _Backend({bad: ("corrupt", B.MJ_ST_INTERNAL)}).install(monkeypatch)
    dec = BatchDecoder(device=0, segment="gpu", gpu_segment_min_files=1)
    try:
        with pytest.raises(BackendError, match=rf"^image {at}: "):
            dec.decode(raws)
        assert all(p.closed for p in be.plans)
    finally:
        dec.close()


def test_raise_for_status_and_triage_name_what_the_caller_indexed():
    """The first failing image of a plan is named by its entry of ``index``; without one, by its position in the plan (the
    JpegDecoder class surface, whose plan is the call).  Tail and unconverged entries are no errors."""
    from pyjpegdecoder_amd import CorruptedJpeg
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import _Request, _triage, raise_for_status
    from pyjpegdecoder_amd.errors import BackendError
    st = np.array([0, 0, B.MJ_ST_OVERRUN, B.MJ_ST_BAD_CODE], dtype=np.int32)
    with pytest.raises(CorruptedJpeg, match=r"^image 2: Failed to decode image \(a restart segment ends"):
        raise_for_status(st)
    with pytest.raises(CorruptedJpeg, match=r"^image 11: Failed to decode image \(a restart segment ends"):
        raise_for_status(st, [5, 7, 11, 13])
    with pytest.raises(BackendError, match=r"^image 13: "):
        raise_for_status(np.array([0, 0, 0, B.MJ_ST_INTERNAL], dtype=np.int32), np.array([5, 7, 11, 13]))
    raise_for_status(np.zeros(3, dtype=np.int32), [4, 5, 6])
    st = np.array([B.MJ_ST_TAIL, 0, B.MJ_ST_UNCONVERGED, B.MJ_ST_DESYNC], dtype=np.int32)
    with pytest.raises(CorruptedJpeg, match=r"^image 9: "):
        _triage(st.copy(), [1, 4, 6, 9])
    with pytest.raises(CorruptedJpeg, match=r"^image 40: "):                    # a part of a call: request-local 9 is file 40
        _triage(st.copy(), [1, 4, 6, 9], index=[10, 20, 30, 40])
    assert _triage(st[:3].copy(), [1, 4, 6], index=[10, 20, 30]) == ([1], [6])   # (what goes round again stays request-local)
    # the positions travel with a narrowed request, through two levels (a part of a call, then its second round)
    req = _Request([b"a", b"b", b"c", b"d", b"e", b"f"])
    assert req.index is None
    part = req.narrow(range(2, 6))
    assert part.index == [2, 3, 4, 5] and part.narrow([3, 1]).index == [5, 3]


# ---- the device routes, with a stand-in for torch as well -------------------------------------------------------------------
class _Tensor:
    """What batch.py asks of a torch tensor, over a NumPy array."""

    def __init__(self, a, be):
        self.a, self.be = a, be

    shape = property(lambda self: self.a.shape)
    dtype = property(lambda self: self.a.dtype)

    def data_ptr(self):
        self.be.tensors[self.a.ctypes.data] = self.a
        return self.a.ctypes.data

    def numel(self):
        return self.a.size

    def numpy(self):
        return self.a

    def to(self, device, non_blocking=False):
        return _Tensor(self.a.copy(), self.be)

    def record_stream(self, stream):
        pass

    def reshape(self, *shape):
        return _Tensor(self.a.reshape(*shape), self.be)

    def __getitem__(self, key):
        return _Tensor(self.a[key], self.be)

    def __len__(self):
        return len(self.a)


def _torch_stand_in(be):
    import contextlib

    class Stream:
        cuda_stream = 7

        def __init__(self, device=None):
            pass

        def wait_stream(self, other):
            pass

    class Event:
        cuda_event = 9

        def record(self, stream=None):
            pass

        def synchronize(self):
            pass

    def empty(shape, dtype=np.uint8, device=None, pin_memory=False):
        return _Tensor(np.full(shape, FILLER, dtype=np.uint8).view(dtype) if isinstance(shape, int) else
                       np.full(tuple(shape[:-1]) + (shape[-1] * np.dtype(dtype).itemsize,), FILLER, dtype=np.uint8).view(dtype), be)

    cuda = SimpleNamespace(Stream=Stream, Event=Event, current_stream=lambda device=None: Stream(),
                           stream=lambda st: contextlib.nullcontext())
    # (bfloat16: NumPy has no such type — two bytes per element is all the host code needs of it)
    return SimpleNamespace(device=lambda kind, index=0: (kind, index), cuda=cuda, empty=empty, from_numpy=lambda a: _Tensor(a, be),
                           uint8=np.dtype(np.uint8), float16=np.dtype(np.uint16), bfloat16=np.dtype(np.uint16), float32=np.dtype(np.uint32))


def _unwrap(got):
    return got.a if isinstance(got, _Tensor) else [t.a for t in got]


DEVICE_COMBOS = HOST_COMBOS + ("bfloat16",)


@pytest.mark.parametrize("route", ["one_call_native", "one_call_python", "three_parts"])
@pytest.mark.parametrize("combo", DEVICE_COMBOS)
def test_decode_device_every_slot_through_second_rounds(monkeypatch, combo, route):
    """decode_device with the stand-ins: the native front end (host code, the real one) sorts the call into plans and a rest, a
    declined group is regrouped, second rounds write the call's slots of the one tensor — in one call and cut into three parts."""
    import sys
    from pyjpegdecoder_amd import BatchDecoder
    entries = call_files()
    raws = [e.raw for e in entries]
    be = _Backend(_script(entries), known=raws).install(monkeypatch)
    monkeypatch.setitem(sys.modules, "torch", _torch_stand_in(be))
    c = COMBINATIONS[combo]
    dec = BatchDecoder(device=0, layout="planar_rowmajor", segment="gpu", gpu_segment_min_files=1, native_host=route != "one_call_python")
    try:
        got = dec.decode_device(raws, parts=3 if route == "three_parts" else 1, **call_kwargs(entries, c))
        check_outputs(_unwrap(got), entries, c, "planar_rowmajor", (route, combo))
        assert_second_rounds(be.take_records(), entries, c["size"] is not None, (route, combo), one_plan_each=route != "three_parts")
        assert all(p.closed for p in be.plans)
    finally:
        dec.close()


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("combo", ["none", "size", "float16", "bfloat16"])
def test_decode_device_iter_every_slot_through_collects_redo(monkeypatch, combo, depth):
    """decode_device_iter with the stand-ins: the batch of files without restart markers is one pipelined plan whose collect()
    sends the tail file and the unconverged files round again and puts what comes back where those files sit in the batch."""
    import sys
    from pyjpegdecoder_amd import BatchDecoder
    entries = call_files()
    batches = [[entries[i] for i in b] for b in ITER_BATCHES]
    be = _Backend(_script(entries), known=[e.raw for e in entries]).install(monkeypatch)
    monkeypatch.setitem(sys.modules, "torch", _torch_stand_in(be))
    c = COMBINATIONS[combo]
    kw = call_kwargs(entries, c, rois_allowed=False)
    if "mirror" in kw:
        kw["mirror"] = iter([[e.mirror for e in b] for b in batches])
    dec = BatchDecoder(device=0, layout="xmajor", segment="gpu", gpu_segment_min_files=1)
    try:
        outs = list(dec.decode_device_iter([[e.raw for e in b] for b in batches], depth=depth, **kw))
        assert len(outs) == len(batches)
        for k, (b, got) in enumerate(zip(batches, outs)):
            check_outputs(_unwrap(got), b, c, "xmajor", (combo, depth, "batch", k), rois_allowed=False)
        by_batch = records_by_batch(be.take_records(), [e.raw for e in entries], ITER_BATCHES)
        for k, b in enumerate(batches[:3]):
            assert_second_rounds(by_batch[k], b, c["size"] is not None, (combo, depth, "batch", k), redo_is_a_request=True)
        assert len(by_batch[0]) == 1, "the batch of ordinary files is one plan"
        assert by_batch[2][0].n_images == len(batches[2]) and len(by_batch[2]) >= 3, "the batch was not one pipelined plan"
        assert all(p.closed for p in be.plans)
    finally:
        dec.close()


@pytest.mark.parametrize("what", ["in_parts", "collects_redo"])
def test_errors_from_a_narrowed_request_name_the_position_in_the_call(monkeypatch, what):
    """Files of one kind, so that the plans are the pipelined ones of _device_iter: decode_device(parts=3) whose damaged file
    is 5 of the call and 1 of the third part's plan; a batch of decode_device_iter whose corrupt tail file is 4 of the batch
    and 1 of the request collect() sends round again.  Both name the position in the call (in the batch)."""
    import sys
    from pyjpegdecoder_amd import BatchDecoder, CorruptedJpeg
    from pyjpegdecoder_amd import _binding as B
    call, at = next((e, a) for w, e, a in damaged_one_kind_calls() if w == what)
    raws = [e.raw for e in call]
    good = one_kind_batch()
    good_raws = [e.raw for e in good]
    known = raws + [r for r in good_raws if r not in raws]
    flags = [e.mirror for e in call]
    script = {call[at].raw: ("corrupt", B.MJ_ST_DESYNC)} if what == "in_parts" else {call[1].raw: "tail", call[at].raw: ("tail_corrupt", B.MJ_ST_BAD_CODE)}
    text = "restart markers are not where" if what == "in_parts" else "no Huffman code"
    for kw in ({}, {"size": (16, 12), "mirror": flags}):
        be = _Backend(script, known=known).install(monkeypatch)
        monkeypatch.setitem(sys.modules, "torch", _torch_stand_in(be))
        dec = BatchDecoder(device=0, segment="gpu", gpu_segment_min_files=1)
        try:
            with pytest.raises(CorruptedJpeg, match=rf"^image {at}: Failed to decode image \({text}"):
                if what == "in_parts":
                    dec.decode_device(raws, parts=3, **kw)
                else:
                    list(dec.decode_device_iter([good_raws, raws], **({**kw, "mirror": iter([False, flags])} if kw else kw)))
            held = [files_of(r, known) for r in be.take_records()]
            assert_reported_from_a_narrowed_request(what, [h for h in held if max(h) < len(raws)], at)
            assert all(p.closed for p in be.plans), "a plan stayed open behind the exception"
            got = dec.decode_device(good_raws)
            check_outputs(_unwrap(got), good, COMBINATIONS["none"], "xmajor", (what, "after the exception"))
            assert all(p.closed for p in be.plans)
        finally:
            dec.close()


def test_the_stand_in_refuses_a_window_that_does_not_lie_inside_its_file(monkeypatch):
    """... as mj_plan_create does (tests/test_request_routes.py): what assert_expectations_tell_files_apart leaves out raises."""
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    pairs = windows_that_do_not_fit(call_files())
    assert pairs
    _Backend().install(monkeypatch)
    dec = BatchDecoder(device=0)
    for e, win in pairs:
        prep = prepare_batch([e.raw], B.MJ_LAYOUT_XMAJOR, 0)
        with pytest.raises(B.BackendError, match="not inside"):
            B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 1}, rois=[win])
    dec.close()
