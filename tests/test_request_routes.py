"""Per-file arguments on the routes where a file goes round again, on the MI355X: one interleaved call of every kind of
three-component file — ordinary ones, files the native front end declines, files the GPU marker scan hands back (MJ_ST_TAIL)
and files whose synchronisation rounds are kept from settling (MJ_ST_UNCONVERGED) — through decode, decode_device (one call,
in parts) and decode_device_iter, with windows, a fixed size, float dtypes, normalisation and mirror flags.  Every slot is held
to routes_common.expected (oracle, resize model, normalize model; floats as bit patterns); a recording `_binding.Plan` proves
that the second rounds ran, with which files and into which slots.  A damaged file is named by its position in the call."""
import numpy as np
import pytest

from routes_common import (COMBINATIONS, ITER_BATCHES, assert_expectations_tell_files_apart, assert_reported_from_a_narrowed_request,
                           assert_second_rounds, call_files, call_kwargs, check_outputs, damaged_calls, damaged_one_kind_calls,
                           files_of, good_call, one_kind_batch, positions, record_of, records_by_batch, windows_that_do_not_fit)

pytestmark = pytest.mark.gpu

HOST_COMBOS = ("none", "rois", "size", "size_rois", "float16", "float32")            # decode returns NumPy: no bfloat16
DEVICE_COMBOS = HOST_COMBOS + ("bfloat16",)
ITER_COMBOS = ("none", "size", "float16", "float32", "bfloat16")                      # decode_device_iter takes no rois
ALL_LAYOUTS = ("xmajor", "rowmajor", "planar", "planar_rowmajor")
TWO_LAYOUTS = ("xmajor", "planar_rowmajor")


@pytest.fixture(scope="module")
def entries():
    """The call — after the check, on the CPU, that its expectations can tell a mixed-up decode from a right one."""
    out = call_files()
    assert_expectations_tell_files_apart(out, DEVICE_COMBOS, TWO_LAYOUTS)
    assert_expectations_tell_files_apart(out, DEVICE_COMBOS, ("rowmajor", "planar"))
    assert_expectations_tell_files_apart(out, ITER_COMBOS, TWO_LAYOUTS, rois_allowed=False)
    tail, unconverged = positions(out, "tail"), positions(out, "unconverged")
    assert len(tail) >= 2 and len(unconverged) >= 2
    assert all(b - a > 1 for pos in (tail, unconverged) for a, b in zip(pos, pos[1:]))
    assert sorted(i for b in ITER_BATCHES for i in b) == list(range(len(out)))
    assert all(out[i].kind == "ordinary" for i in ITER_BATCHES[0])
    assert set(positions(out, "unconverged")) <= set(ITER_BATCHES[2]) and ITER_BATCHES[3] == []
    return out


@pytest.fixture
def unsettled(tune):
    """The synchronisation form for every plan that can take it, and nothing that lets a chain of chunks settle: no run-up in
    front of the chunks, the shortest chunks, no repair rounds."""
    for name, value in (("MJ_HUFFMAN", "sync"), ("MJ_SYNC_WARM", "0"), ("MJ_SYNC_CHUNK", "256"), ("MJ_SYNC_ROUNDS", "0")):
        tune(name, value)


@pytest.fixture
def plans(monkeypatch):
    """`_binding.Plan` wrapped: every plan a decoder makes is noted (routes_common.PlanRecord) before it is created."""
    from pyjpegdecoder_amd import _binding as B

    class Recorder:
        def __init__(self):
            self.records, self.made = [], []

        def take(self):
            out, self.records = self.records, []
            return out

        def all_closed(self) -> bool:
            return all(not p.handle for p in self.made)

    rec = Recorder()

    class RecordingPlan(B.Plan):
        def __init__(self, ctx, batch_c, keepalive, rois=None, size=None, slots=None, output=None):
            rec.records.append(record_of(batch_c, keepalive, slots))
            super().__init__(ctx, batch_c, keepalive, rois=rois, size=size, slots=slots, output=output)
            rec.made.append(self)

    monkeypatch.setattr(B, "Plan", RecordingPlan)
    return rec


def assert_the_rounds_do_not_settle(dec, entries, plans):
    """A bare plan over the unconverged files, no fallback layer: MJ_ST_UNCONVERGED for each — else nothing below means much."""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    raws = [e.raw for e in entries if e.kind == "unconverged"]
    prep = prepare_batch(raws, B.MJ_LAYOUT_XMAJOR, 0)
    plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(raws)})
    try:
        assert plan.stage1_form() & 15 == B.MJ_FORM_SYNC
        plan.execute()
        plan.sync()
        status = plan.read(rgb=False)["status"].tolist()
    finally:
        plan.close()
    assert status == [B.MJ_ST_UNCONVERGED] * len(raws), status
    plans.take()


def _is_dense(combo: str) -> bool:
    return COMBINATIONS[combo]["size"] is not None


def test_a_window_that_does_not_lie_inside_its_file_is_refused(entries):
    """What assert_expectations_tell_files_apart leaves out: a file given its neighbour's window where that window does not
    lie inside it.  No image comes of that — the library refuses the plan, a window plan and a resized one alike."""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd.batch import prepare_batch
    from pyjpegdecoder_amd.errors import BackendError
    pairs = windows_that_do_not_fit(entries)
    assert pairs, "every neighbour's window fits: nothing is left out, and this test can go"
    dec = BatchDecoder(device=0)
    try:
        for e, win in pairs:
            for size in (None, (40, 28)):
                prep = prepare_batch([e.raw], B.MJ_LAYOUT_XMAJOR, 0)
                with pytest.raises(BackendError, match="not inside"):
                    B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 1}, rois=[win], size=size).close()
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode(entries, unsettled, plans, layout):
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        assert_the_rounds_do_not_settle(dec, entries, plans)
        for combo in HOST_COMBOS:
            got = dec.decode(raws, **call_kwargs(entries, COMBINATIONS[combo]))
            assert isinstance(got, np.ndarray) == _is_dense(combo)
            check_outputs(got, entries, COMBINATIONS[combo], layout, ("decode", combo, layout))
            assert_second_rounds(plans.take(), entries, False, ("decode", combo, layout))
        assert plans.all_closed()
    finally:
        dec.close()


@pytest.mark.parametrize("native_host", [True, False], ids=["native_front_end", "python_front_end"])
@pytest.mark.parametrize("layout", ALL_LAYOUTS)
def test_decode_device_in_one_call(entries, unsettled, plans, layout, native_host):
    """parts=1.  With the native front end the call is sorted into several native plans and a rest for the Python path; with
    ``size`` every plan — the second rounds too — writes its files' slots of the one tensor."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1, native_host=native_host)
    try:
        assert_the_rounds_do_not_settle(dec, entries, plans)
        for combo in DEVICE_COMBOS:
            got = dec.decode_device(raws, parts=1, **call_kwargs(entries, COMBINATIONS[combo]))
            assert isinstance(got, torch.Tensor) == _is_dense(combo)
            check_outputs(got, entries, COMBINATIONS[combo], layout, ("decode_device", combo, layout, native_host))
            assert_second_rounds(plans.take(), entries, _is_dense(combo), ("decode_device", combo, layout, native_host))
        assert plans.all_closed()
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode_device_in_three_parts(entries, unsettled, plans, layout):
    """parts=3: the cuts (after files 3 and 7) fall between second-round files — a tail file ends the first part, an unconverged
    one starts the second, the third holds one of each — and every part's plans still write the CALL's slots."""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    cut = [len(raws) * i // 3 for i in range(4)]
    assert entries[cut[1] - 1].kind == "tail" and entries[cut[1]].kind == "unconverged"
    assert {e.kind for e in entries[cut[2]:]} >= {"tail", "unconverged"}
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        assert_the_rounds_do_not_settle(dec, entries, plans)
        for combo in DEVICE_COMBOS:
            got = dec.decode_device(raws, parts=3, **call_kwargs(entries, COMBINATIONS[combo]))
            check_outputs(got, entries, COMBINATIONS[combo], layout, ("parts=3", combo, layout))
            records = plans.take()
            assert_second_rounds(records, entries, _is_dense(combo), ("parts=3", combo, layout), one_plan_each=False)
            for rec in records:                                   # no plan reaches across a cut
                idxs = files_of(rec, raws)
                assert len({sum(i >= c for c in cut[1:3]) for i in idxs}) == 1, idxs
        assert plans.all_closed()
    finally:
        dec.close()


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode_device_iter(entries, unsettled, plans, layout, depth):
    """Three batches and an empty one: ordinary files of one kind (one pipelined plan), tail and declined files (the one-call
    path), files without restart markers — a pipelined plan whose collect() sends its tail file and its unconverged files round
    again through a narrowed request.  ``mirror`` comes batch by batch."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    batches = [[entries[i] for i in b] for b in ITER_BATCHES]
    raws = [e.raw for e in entries]
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        assert_the_rounds_do_not_settle(dec, entries, plans)
        for combo in ITER_COMBOS:
            c = COMBINATIONS[combo]
            kw = call_kwargs(entries, c, rois_allowed=False)
            if "mirror" in kw:
                kw["mirror"] = iter([[e.mirror for e in b] for b in batches])
            outs = list(dec.decode_device_iter([[e.raw for e in b] for b in batches], depth=depth, **kw))
            assert len(outs) == len(batches)
            by_batch = records_by_batch(plans.take(), raws, ITER_BATCHES)
            for k, (b, got) in enumerate(zip(batches, outs)):
                what = ("decode_device_iter", combo, layout, depth, "batch", k)
                assert isinstance(got, torch.Tensor) == _is_dense(combo)
                check_outputs(got, b, c, layout, what, rois_allowed=False)
                if b:
                    assert_second_rounds(by_batch[k], b, _is_dense(combo), what, redo_is_a_request=True)
            assert len(by_batch[0]) == 1, "the batch of ordinary files is one plan"
            # the third batch went as ONE pipelined plan first: its second rounds came out of collect()
            assert by_batch[2][0].n_images == len(batches[2]) and len(by_batch[2]) >= 3
        assert plans.all_closed()
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_host_segmentation_is_the_control_without_second_rounds(entries, plans, layout):
    """segment="host", the library's own choices: no file is handed back, none goes round again — the same expectations."""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    dec = BatchDecoder(device=0, layout=layout, segment="host")
    try:
        for route, combos in (("decode", HOST_COMBOS), ("decode_device", DEVICE_COMBOS)):
            for combo in combos:
                got = getattr(dec, route)(raws, **call_kwargs(entries, COMBINATIONS[combo]))
                check_outputs(got, entries, COMBINATIONS[combo], layout, ("host", route, combo, layout))
                records = plans.take()
                assert sorted(i for rec in records for i in files_of(rec, raws)) == list(range(len(raws))), (route, combo)
        assert plans.all_closed()
    finally:
        dec.close()


@pytest.mark.parametrize("what", ["first_round", "second_round"])
def test_errors_name_the_position_in_the_call(plans, what):
    """A call of mixed kinds with one damaged file at position 3, the second file of its plan: CorruptedJpeg names image 3 from
    decode, decode_device and (per batch) decode_device_iter — when the first round finds the damage, and when the file is a
    tail file whose damage shows in its second round, in a plan of its own.  Afterwards the decoder decodes a good call, and no
    plan is left open."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder, CorruptedJpeg
    call, at = next((e, a) for w, e, a in damaged_calls() if w == what)
    raws = [e.raw for e in call]
    good = good_call()
    good_raws = [e.raw for e in good]
    size_kw = {"size": (16, 12), "mirror": [True, False, True, False, True]}
    for native_host in (True, False):
        dec = BatchDecoder(device=0, segment="gpu", gpu_segment_min_files=1, native_host=native_host)
        try:
            routes = [("decode", lambda kw: dec.decode(raws, **kw)),
                      ("decode_device", lambda kw: dec.decode_device(raws, **kw)),
                      ("decode_device_iter", lambda kw: list(dec.decode_device_iter(
                          [good_raws, raws], **({**kw, "mirror": iter([False, kw["mirror"]])} if kw else kw))))]
            for name, call_route in routes:
                for kw in ({}, size_kw):
                    with pytest.raises(CorruptedJpeg, match=rf"^image {at}: Failed to decode image") as err:
                        call_route(kw)
                    held = [files_of(r, raws + good_raws) for r in plans.take()]
                    reporter = [h for h in held if at in h][-1]                 # the latest plan that held the damaged file
                    assert reporter.index(at) != at, (name, str(err.value), "position 3 is also where the file sits in its plan", held)
                    if what == "second_round":
                        assert reporter == [at] and sum(at in h for h in held) == 2, (name, str(err.value), "the damage was not found in a second round", held)
                    torch.cuda.synchronize()
                    assert plans.all_closed(), (name, "a plan stayed open behind the exception")
                    # the same decoder, a good call
                    got = dec.decode_device(good_raws) if name != "decode" else dec.decode(good_raws)
                    check_outputs(got, good, COMBINATIONS["none"], "xmajor", (what, name, "after the exception"))
                    plans.take()
            assert plans.all_closed()
        finally:
            dec.close()


@pytest.mark.parametrize("what", ["in_parts", "collects_redo"])
def test_errors_from_a_narrowed_request_name_the_position_in_the_call(plans, what):
    """Files of one kind, so that the plans are the pipelined ones of _device_iter.  decode_device(parts=3): the damaged file
    is 5 of the call and 1 of the third part's plan.  decode_device_iter: the damaged file is a corrupt tail file, 4 of its
    batch; collect() sends it round again with the good tail file at 1, and in that request's plans it is file 1.  Both name
    the position in the call (in the batch)."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder, CorruptedJpeg
    call, at = next((e, a) for w, e, a in damaged_one_kind_calls() if w == what)
    raws = [e.raw for e in call]
    good = one_kind_batch()
    good_raws = [e.raw for e in good]
    known = raws + [r for r in good_raws if r not in raws]
    flags = [e.mirror for e in call]
    dec = BatchDecoder(device=0, segment="gpu", gpu_segment_min_files=1)
    try:
        for kw in ({}, {"size": (16, 12), "mirror": flags}):
            with pytest.raises(CorruptedJpeg, match=rf"^image {at}: Failed to decode image") as err:
                if what == "in_parts":
                    dec.decode_device(raws, parts=3, **kw)
                else:
                    list(dec.decode_device_iter([good_raws, raws], **({**kw, "mirror": iter([False, flags])} if kw else kw)))
            held = [files_of(r, known) for r in plans.take()]
            assert_reported_from_a_narrowed_request(what, [h for h in held if max(h) < len(raws)], at)
            torch.cuda.synchronize()
            assert plans.all_closed(), (what, str(err.value), "a plan stayed open behind the exception")
            got = dec.decode_device(good_raws)
            check_outputs(got, good, COMBINATIONS["none"], "xmajor", (what, "after the exception"))
            plans.take()
        assert plans.all_closed()
    finally:
        dec.close()
