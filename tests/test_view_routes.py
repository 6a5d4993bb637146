"""Views and what is per view on the routes where a file goes round again, on the MI355X: the call of
tests/view_routes_common.py — the thirteen files of tests/routes_common.py (ordinary, declined, MJ_ST_TAIL, MJ_ST_UNCONVERGED) as
some thirty interleaved views behind a leading entry that is no JPEG — through decode, decode_device (one call, three parts) and
decode_device_iter, as views alone, with mode and a bicubic resize, with places, fill, float16 normalisation and mirror flags, with
a NEAREST affine transform (index tables among the matrices) and with a bicubic one on turned files, with a colour chain per view
behind a float16 output, with a bicubic perspective transform on turned files and with a NEAREST one in front of chains in mode "L".  Every view is held to
view_routes_common.expect (the models on the oracle's pixels; floats as bit patterns); a recording `_binding.Plan` proves that the
second rounds ran and that every plan got exactly its own views' slots, windows, matrices, coefficients, chains, places and flags.  A damaged file is
named by its position in the caller's list.  tests/test_view_routes_host.py holds, on the CPU, that these expectations tell a
decoder that mixes views up from a right one."""
import numpy as np
import pytest

import view_routes_common as VC
from routes_common import ITER_BATCHES, assert_second_rounds, call_files, damaged_calls, files_of, finish, positions, record_of
from test_request_routes import assert_the_rounds_do_not_settle, unsettled  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

# two layouts per combination, all four for one
LAYOUTS_OF = {"views": ("xmajor", "planar_rowmajor"), "L_bicubic": ("rowmajor", "planar"), "places_f16": ("xmajor", "planar_rowmajor"),
              "affine_nearest": ("rowmajor", "planar_rowmajor"), "affine_bicubic_orient": ("xmajor", "rowmajor", "planar", "planar_rowmajor"),
              "colour_f16": ("xmajor", "rowmajor", "planar", "planar_rowmajor"), "perspective_bicubic_orient": ("rowmajor", "planar"),
              "perspective_nearest_colour_L": ("xmajor", "planar_rowmajor")}
CASES = [(c, lay) for c, lays in LAYOUTS_OF.items() for lay in lays]


@pytest.fixture(scope="module")
def call():
    out = VC.make_call(call_files())
    VC.assert_the_call_is_interleaved(out)
    return out


@pytest.fixture
def plans(monkeypatch):
    """`_binding.Plan` wrapped: every plan a decoder makes is noted, with every keyword it was given, before it is created"""
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
        def __init__(self, ctx, batch_c, keepalive, rois=None, size=None, slots=None, output=None, **kw):
            rec.records.append(VC.ViewPlanRecord(record_of(batch_c, keepalive, slots), dict(kw, rois=rois, size=size, slots=slots, output=output)))
            super().__init__(ctx, batch_c, keepalive, rois=rois, size=size, slots=slots, output=output, **kw)
            rec.made.append(self)

    monkeypatch.setattr(B, "Plan", RecordingPlan)
    return rec


def _check_plans(plans, call, cname, on_device, what, **kw):
    records = plans.take()
    kw.setdefault("one_plan_each", True)
    kw["one_plan_each"] = kw["one_plan_each"] and not VC.COMBOS[cname].get("orientation")
    assert_second_rounds([r.rec for r in records], call.entries, False, what, **kw)
    VC.assert_bare_plans(VC.assert_plans_hold_their_views(records, call, cname, on_device, what), call, cname, what)


@pytest.mark.parametrize("cname,layout", CASES)
def test_every_view_through_second_rounds(call, unsettled, plans, cname, layout):  # noqa: F811
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        assert_the_rounds_do_not_settle(dec, call.entries, plans)
        kw = VC.call_kwargs(call, cname)
        got = dec.decode(call.files, **kw)
        assert isinstance(got, np.ndarray)
        VC.check_outputs(got, call, cname, layout, ("decode", cname, layout))
        _check_plans(plans, call, cname, False, ("decode", cname, layout))
        for parts in (1, 3):
            got = dec.decode_device(call.files, parts=parts, **kw)
            assert isinstance(got, torch.Tensor)
            VC.check_outputs(got, call, cname, layout, ("decode_device", parts, cname, layout))
            _check_plans(plans, call, cname, True, ("decode_device", parts, cname, layout), one_plan_each=parts == 1)
        assert plans.all_closed()
    finally:
        dec.close()


@pytest.mark.parametrize("cname,layout", [(c, lay) for c, lay in CASES if not VC.COMBOS[c].get("places")])
def test_every_view_through_collects_redo(call, unsettled, plans, cname, layout):  # noqa: F811
    """decode_device_iter: views, flags, matrices, coefficients, chains and orientations come batch by batch (the list forms of resize_to and place would
    have to fit every batch, so the iterator is not given them); the third batch is one pipelined plan whose collect() sends its tail
    file and its unconverged files round again through a narrowed request"""
    from pyjpegdecoder_amd import BatchDecoder
    entries = call.entries
    raws = [e.raw for e in entries]
    calls = [VC.make_call([entries[i] for i in b], list(b)) for b in ITER_BATCHES]
    kw = VC.iter_kwargs(calls, cname)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        assert_the_rounds_do_not_settle(dec, entries, plans)
        outs = list(dec.decode_device_iter([c.files for c in calls], depth=2, **kw))
        assert len(outs) == len(calls)
        records = plans.take()
        for n, (c, got) in enumerate(zip(calls, outs)):
            what = ("decode_device_iter", cname, layout, "batch", n)
            VC.check_outputs(got, c, cname, layout, what)
            mine = [r for r in records if files_of(r.rec, raws)[0] in ITER_BATCHES[n]]
            if c.entries:
                assert_second_rounds([r.rec for r in mine], c.entries, False, what, one_plan_each=not VC.COMBOS[cname].get("orientation"),
                                     redo_is_a_request=True)
                VC.assert_plans_hold_their_views(mine, c, cname, True, what)
        assert plans.all_closed()
    finally:
        dec.close()


@pytest.mark.parametrize("what", ["first_round", "second_round"])
def test_errors_name_the_position_in_the_callers_list(plans, what):
    """a views call with one damaged file — found by the first round, or a tail file whose damage shows in its second round, in a
    plan of its own: CorruptedJpeg names the file's position in the caller's list, the leading non-JPEG counted, which is not its
    position in the plan that reported it; afterwards no plan is open"""
    import torch
    from pyjpegdecoder_amd import BatchDecoder, CorruptedJpeg
    entries, at = next((e, a) for w, e, a in damaged_calls() if w == what)
    finish([e for i, e in enumerate(entries) if i != at])
    entries[at].full = np.zeros_like(entries[1].full)              # (no pixels: the windows of its views need its size only)
    assert entries[at].full.shape[:2] == (200, 120)
    call = VC.make_call(entries)
    named = at + 1
    dec = BatchDecoder(device=0, segment="gpu", gpu_segment_min_files=1)
    try:
        for cname in ("views", "affine_bicubic_orient", "perspective_bicubic_orient", "colour_f16"):
            kw = VC.call_kwargs(call, cname)
            for name, route in (("decode", lambda: dec.decode(call.files, **kw)), ("decode_device", lambda: dec.decode_device(call.files, **kw)),
                                ("decode_device_iter", lambda: list(dec.decode_device_iter(
                                    [call.files], **{k: (iter([v]) if k in VC.PER_BATCH else v) for k, v in kw.items()})))):
                with pytest.raises(CorruptedJpeg, match=rf"^image {named}: Failed to decode image") as err:
                    route()
                holders = [h for h in (files_of(r.rec, call.files) for r in plans.take()) if named in h]
                # (the message match above is what tells the three numberings apart: the file is named - 1 among the files that are
                # read and 0 or 1 in the plan that reported it)
                assert holders and holders[-1].index(named) < 2 < named - 1, (name, str(err.value), holders)
                if what == "second_round":
                    assert holders[-1] == [named] and len(holders) == 2, (name, "the damage was not found in a second round", holders)
                torch.cuda.synchronize()
                assert plans.all_closed(), (name, "a plan stayed open behind the exception")
    finally:
        dec.close()


def test_an_affine_refusal_names_the_output_and_the_file_in_the_callers_numbering(call, plans):
    from pyjpegdecoder_amd import BatchDecoder
    tail = positions(call.entries, "tail")[1]
    v = [v for v in call.views if v.file == tail + 1][1]
    dec = BatchDecoder(device=0, segment="gpu", gpu_segment_min_files=1)
    try:
        for cname in ("affine_nearest", "affine_bicubic_orient"):
            kw = VC.call_kwargs(call, cname)
            kw["affine"] = list(kw["affine"])
            kw["affine"][v.k] = (1.0, 0.0, 40000.0, 0.0, 1.0, 0.0)
            for route in (dec.decode, dec.decode_device):
                with pytest.raises(ValueError, match=rf"^affine: output {v.k} \(file {v.file}\): a corner of the output has a source coordinate"):
                    route(call.files, **kw)
        assert not plans.take(), "a plan was made for a call that is refused"
    finally:
        dec.close()


def test_a_perspective_refusal_and_a_bad_chain_name_the_output_in_the_callers_numbering(call, plans):
    from pyjpegdecoder_amd import BatchDecoder
    tail = positions(call.entries, "tail")[1]
    v = [v for v in call.views if v.file == tail + 1][1]
    cases = [("perspective_bicubic_orient", "perspective", (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, float("inf"), 0.0),
              rf"^perspective: output {v.k} \(file {v.file}\): a coefficient is not finite"),
             ("perspective_nearest_colour_L", "perspective", (1.0, 0.0, float("nan"), 0.0, 1.0, 0.0, 0.0, 0.0),
              rf"^perspective: output {v.k} \(file {v.file}\): a coefficient is not finite"),
             ("colour_f16", "color_ops", (("posterize", 9),), rf"^color_ops: output {v.k}: posterize takes 1\.\.8 bits"),
             ("perspective_nearest_colour_L", "color_ops", (("invert",), ("posterize", 9)), rf"^color_ops: output {v.k}: posterize takes 1\.\.8 bits")]
    dec = BatchDecoder(device=0, segment="gpu", gpu_segment_min_files=1)
    try:
        for cname, name, bad, text in cases:
            kw = VC.call_kwargs(call, cname)
            kw[name] = list(kw[name])
            kw[name][v.k] = bad
            for route in (dec.decode, dec.decode_device):
                with pytest.raises(ValueError, match=text):
                    route(call.files, **kw)
        assert not plans.take(), "a plan was made for a call that is refused"
    finally:
        dec.close()
