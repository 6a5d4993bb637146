"""Views and what is per view on the routes where a file goes round again, without a GPU: the call of
tests/view_routes_common.py through BatchDecoder.decode, decode_device (one call, three parts) and decode_device_iter with stand-ins
for `_binding.Context`, `_binding.Plan` and torch, as tests/test_request_routes_host.py does for calls without views.  The stand-in
plan takes every keyword `_Request.plan_kwargs` can produce and computes output k of the plan from what THAT plan was given, per
view of that plan — views, orientation, mode, filter, places / fill, affine or perspective, colour, output, slots — with
tools/affine_model.expected or tools/perspective_model.expected on the oracle's pixels, tools/colour_model.apply_chain and
tools/normalize_model; it reads nothing of batch._Request, and it refuses a window that does not lie inside
its oriented image, as the library does.  Statuses are scripted as in test_request_routes_host.py.  So what is held here is the
host's part alone: which file, window, flag, matrix, coefficient set, chain, place and slot every view of every plan gets —
through `_Request.narrow` at every level —, and which position an error names."""
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import view_routes_common as VC
from routes_common import (ITER_BATCHES, LAYOUT_NAMES, assert_second_rounds, call_files, damaged_calls, damaged_one_kind_calls, files_of,
                           positions, record_of)
from test_request_routes_host import FILLER, _Backend, _script, _torch_stand_in, _unwrap
from test_resize import as_layout

_images = {}


class _ViewBackend(_Backend):
    """test_request_routes_host's stand-in device with a plan that knows views and everything that is per view"""

    def install(self, monkeypatch):
        from pyjpegdecoder_amd import _binding as B
        be = self
        super().install(monkeypatch)                  # (the stand-in Context)

        class Plan:
            def __init__(self, ctx, batch_c, keepalive, rois=None, size=None, slots=None, output=None, orientation=None, filter=None, mode=None,
                         places=None, fill=None, reducing_gap=None, views=None, affine=None, colour=None, perspective=None):
                prep = keepalive["prep"]
                n = int(batch_c.n_images)
                assert n == keepalive["n_images"] == len(prep.parsed) and reducing_gap is None
                assert size is not None or (slots is None and output is None and views is None and places is None and affine is None
                                            and colour is None and perspective is None)
                assert affine is None or perspective is None
                self.kw = dict(rois=rois, size=size, slots=slots, output=output, orientation=orientation, filter=filter, mode=mode, places=places,
                               fill=fill, views=views, affine=affine, colour=colour, perspective=perspective)
                turns = list(orientation) if orientation is not None else [1] * n
                assert len(turns) == n
                dims = [(h, w) if o >= 5 else (w, h) for (w, h, _), o in zip(prep.shapes, turns)]
                if views is None:                     # one output per image: its window, or all of it
                    views = [(i, rois[i] if rois is not None else None) for i in range(n)]
                self.views = [(int(f), tuple(int(t) for t in w) if w is not None else (0, 0) + dims[int(f)]) for f, w in views]
                n_out = len(self.views)
                for name, per_output in (("slots", slots[0] if slots is not None else None), ("mirror", output[3] if output is not None else None),
                                         ("places", places), ("affine", affine[0] if affine is not None else None), ("colour", colour),
                                         ("perspective", perspective[0] if perspective is not None else None)):
                    assert per_output is None or len(per_output) == n_out, f"{name}: {len(per_output)} entries for a plan of {n_out} outputs"
                for k, (f, (x, y, ww, wh)) in enumerate(self.views):          # as mj_plan_create_with does
                    assert 0 <= f < n
                    w, h = dims[f]
                    if ww <= 0 or wh <= 0 or x < 0 or y < 0 or x + ww > w or y + wh > h:
                        raise B.BackendError(f"view {k}: window (x {x}, y {y}, width {ww}, height {wh}) is empty or not inside the {w}x{h} image")
                self.raws = [be.raw_of(prep, k) for k in range(n)]
                self.layout, self.flags = LAYOUT_NAMES[int(batch_c.layout)], int(batch_c.flags)
                self.size, self.slots, self.output, self.turns = size, slots, output, turns
                self.closed = self.executed = False
                rec = VC.ViewPlanRecord(record_of(batch_c, keepalive, slots), self.kw, self)
                be.records.append(rec)
                be.plans.append(self)
                self.status = np.array([self._status(r) for r in self.raws], dtype=np.int32)
                self.ncomp = B.MODES[mode] if mode is not None else int(prep.shapes[0][2])
                es = B.DTYPE_BYTES[output[0]] if output is not None else 1
                self.per = (size[0] * size[1] if size is not None else 0) * self.ncomp * es
                self.images = [self._image(k) if self.status[f] == 0 else None for k, (f, _) in enumerate(self.views)] if size is not None else []
                assert all(im is None or im.nbytes == self.per for im in self.images)
                self.info = SimpleNamespace(rgb_bytes=self.per * (int(slots[1]) if slots is not None else n_out))

            def _image(self, k: int) -> np.ndarray:
                from tools import affine_model, colour_model, normalize_model, perspective_model
                f, win = self.views[k]
                kw = self.kw
                dtype, mean, std, mirror = self.output if self.output is not None else (None, None, None, None)
                a, resample, afill = (kw["affine"][0][k], kw["affine"][1], tuple(kw["affine"][2])) if kw["affine"] is not None else (None, "nearest", (0,))
                if kw["perspective"] is not None:
                    a, resample, afill = kw["perspective"][0][k], kw["perspective"][1], tuple(kw["perspective"][2])
                model = perspective_model if kw["perspective"] is not None else affine_model
                chain = kw["colour"][k] if kw["colour"] is not None else None
                place = tuple(kw["places"][k]) if kw["places"] is not None else tuple(self.size) + (0, 0)
                fill = tuple(kw["fill"]) if kw["fill"] is not None else (0,)
                flip = bool(mirror[k]) if mirror is not None else False
                key = (self.raws[f], a, win, tuple(self.size), resample, afill, kw["filter"], self.turns[f], kw["mode"], place, fill, dtype, chain,
                       None if mean is None else (tuple(np.ravel(mean)), tuple(np.ravel(std))))
                if key not in _images:
                    px = np.ascontiguousarray(be.full(self.raws[f]).swapaxes(0, 1))
                    one = lambda t: (t if len(t) == self.ncomp else t * self.ncomp) if self.ncomp == 3 else t[0]          # noqa: E731
                    rm = model.expected(px, a, win, self.size, resample=resample, affine_fill=one(afill), filter=kw["filter"] or "bilinear",
                                               orientation=self.turns[f], mode=kw["mode"], resized=place[:2], xy=place[2:], fill=one(fill))
                    rm = colour_model.apply_chain(rm, chain)
                    if dtype not in (None, "uint8"):
                        rm = normalize_model.normalize(rm, dtype, mean, std)
                    _images[key] = rm
                rm = _images[key]
                return as_layout(rm[:, ::-1] if flip else rm, self.layout)

            def _filled(self) -> np.ndarray:
                out = np.full(self.info.rgb_bytes, FILLER, dtype=np.uint8)
                for k, im in enumerate(self.images):
                    s = int(self.slots[0][k]) if self.slots is not None else k
                    if im is not None:
                        out[s * self.per:(s + 1) * self.per] = np.frombuffer(im.tobytes(), dtype=np.uint8)
                return out

            def execute(self, stream=0, rgb_device=None):
                assert not self.closed
                self.executed = True
                if isinstance(rgb_device, int) and rgb_device:
                    rgb_device = be.tensors[rgb_device]
                if isinstance(rgb_device, np.ndarray):                # the call's array: only this plan's slots, only finished views
                    flat, mine = rgb_device.reshape(-1).view(np.uint8), self._filled()
                    for k, im in enumerate(self.images):
                        s = int(self.slots[0][k]) if self.slots is not None else k
                        if im is not None:
                            flat[s * self.per:(s + 1) * self.per] = mine[s * self.per:(s + 1) * self.per]

            def sync(self):
                assert self.executed and not self.closed

            def read(self, rgb=True, coef=False, planes=False, idct=False):
                assert self.executed and not self.closed
                return {"rgb": self._filled() if rgb else None, "coef": None, "planes": None, "idct": None, "status": self.status.copy()}

            def close(self):
                self.closed = True

        def _status(plan, raw: bytes) -> int:          # test_request_routes_host's script, unchanged
            role = be.script.get(raw)
            gpu_segmented = bool(plan.flags & B.MJ_FLAG_GPU_SEGMENT)
            if role == "tail" or (isinstance(role, tuple) and role[0] == "tail_corrupt"):
                if gpu_segmented:
                    return B.MJ_ST_TAIL
                return role[1] if isinstance(role, tuple) else 0
            if role == "unconverged":
                return 0 if plan.flags & B.MJ_FLAG_NO_SYNC else B.MJ_ST_UNCONVERGED
            if isinstance(role, tuple) and role[0] == "corrupt":
                return role[1]
            return 0
        Plan._status = _status
        monkeypatch.setattr(B, "Plan", Plan)
        return self


@pytest.fixture(scope="module")
def call():
    out = VC.make_call(call_files())
    VC.assert_the_call_is_interleaved(out)
    return out


def test_the_expectations_tell_the_views_of_the_call_apart(call):
    VC.assert_expectations_tell_views_apart(call, list(VC.COMBOS), ("xmajor",))
    VC.assert_expectations_tell_views_apart(call, ("places_f16", "affine_bicubic_orient", "colour_f16", "perspective_nearest_colour_L"), ("planar_rowmajor",))


def _decoder(layout, **kw):
    from pyjpegdecoder_amd import BatchDecoder
    return BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1, **kw)


def _check_plans(be, call, cname, on_device, what, one_plan_each=True):
    records = be.take_records()
    assert_second_rounds([r.rec for r in records], call.entries, False, what,
                         one_plan_each=one_plan_each and not VC.COMBOS[cname].get("orientation"))
    # (files_of by the call's own list: the plan's files are positions in the CALLER's list, the leading non-JPEG counted)
    VC.assert_bare_plans(VC.assert_plans_hold_their_views(records, call, cname, on_device, what), call, cname, what)
    assert all(p.closed for p in be.plans), what


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
@pytest.mark.parametrize("cname", list(VC.COMBOS))
def test_decode_every_view_through_second_rounds(monkeypatch, call, cname, layout):
    be = _ViewBackend(_script(call.entries)).install(monkeypatch)
    dec = _decoder(layout)
    try:
        got = dec.decode(call.files, **VC.call_kwargs(call, cname))
        assert isinstance(got, np.ndarray)
        VC.check_outputs(got, call, cname, layout, ("decode", cname, layout))
        _check_plans(be, call, cname, False, ("decode", cname, layout))
    finally:
        dec.close()
    assert all(c.closed for c in be.contexts)


@pytest.mark.parametrize("route", ["one_call_native", "one_call_python", "three_parts"])
@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
@pytest.mark.parametrize("cname", list(VC.COMBOS))
def test_decode_device_every_view_through_second_rounds(monkeypatch, call, cname, layout, route):
    be = _ViewBackend(_script(call.entries), known=call.files[1:]).install(monkeypatch)
    monkeypatch.setitem(sys.modules, "torch", _torch_stand_in(be))
    dec = _decoder(layout, native_host=route != "one_call_python")
    try:
        got = dec.decode_device(call.files, parts=3 if route == "three_parts" else 1, **VC.call_kwargs(call, cname))
        VC.check_outputs(_unwrap(got), call, cname, layout, (route, cname, layout))
        _check_plans(be, call, cname, True, (route, cname, layout), one_plan_each=route != "three_parts")
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
@pytest.mark.parametrize("cname", [c for c in VC.COMBOS if not VC.COMBOS[c].get("places")])
def test_decode_device_iter_every_view_through_collects_redo(monkeypatch, call, cname, layout):
    """(the list forms of resize_to and place would have to fit every batch: the iterator is not given them)"""
    entries = call.entries
    calls = [VC.make_call([entries[i] for i in b], list(b)) for b in ITER_BATCHES]
    be = _ViewBackend(_script(entries), known=[e.raw for e in entries]).install(monkeypatch)
    monkeypatch.setitem(sys.modules, "torch", _torch_stand_in(be))
    kw = VC.iter_kwargs(calls, cname)
    dec = _decoder(layout)
    try:
        outs = list(dec.decode_device_iter([c.files for c in calls], depth=2, **kw))
        assert len(outs) == len(calls)
        records = be.take_records()
        for n, (c, got) in enumerate(zip(calls, outs)):
            what = (cname, layout, "batch", n)
            VC.check_outputs(_unwrap(got), c, cname, layout, what)
            mine = [r for r in records if r.rec.files and files_of(r.rec, [e.raw for e in entries])[0] in ITER_BATCHES[n]]
            if c.entries:
                assert_second_rounds([r.rec for r in mine], c.entries, False, what, one_plan_each=not VC.COMBOS[cname].get("orientation"),
                                     redo_is_a_request=True)
                VC.assert_plans_hold_their_views(mine, c, cname, True, what)
        assert all(p.closed for p in be.plans)
    finally:
        dec.close()


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def _damaged(what):
    from pyjpegdecoder_amd import _binding as B
    for w, entries, at in damaged_calls():
        if w == what:
            role = ("corrupt", B.MJ_ST_DESYNC) if what == "first_round" else ("tail_corrupt", B.MJ_ST_BAD_CODE)
            return entries, at, {entries[at].raw: role}, "restart markers are not where" if what == "first_round" else "no Huffman code"
    for w, entries, at in damaged_one_kind_calls():
        if w == what:
            if what == "in_parts":
                return entries, at, {entries[at].raw: ("corrupt", B.MJ_ST_DESYNC)}, "restart markers are not where"
            return entries, at, {entries[1].raw: "tail", entries[at].raw: ("tail_corrupt", B.MJ_ST_BAD_CODE)}, "no Huffman code"


def _finish_damaged(entries, at):
    """the damaged file has no pixels: the views' windows need its size only"""
    from routes_common import finish
    finish([e for i, e in enumerate(entries) if i != at and e.full is None])
    if entries[at].full is None:
        # (the damaged file of each of these calls is 200 x 120, as the good files of its kind are)
        entries[at].full = np.zeros_like(next(e.full for e in entries if e is not entries[at] and e.full.shape[:2] == (200, 120)))
    return entries


@pytest.mark.parametrize("cname", ["views", "affine_bicubic_orient", "perspective_bicubic_orient", "colour_f16"])
@pytest.mark.parametrize("what", ["first_round", "second_round", "in_parts", "collects_redo"])
def test_errors_name_the_position_in_the_callers_list(monkeypatch, what, cname):
    """a views call whose damaged file is found in a first round, in a second round, in the third part of a call and in collect()'s
    redo: the message names the file's position in the caller's list — the leading non-JPEG counted —, which is neither its
    position among the files that are read nor its position in the plan that reported it"""
    from pyjpegdecoder_amd import CorruptedJpeg
    entries, at, script, text = _damaged(what)
    call = VC.make_call(_finish_damaged(entries, at))
    named = at + 1
    kw = VC.call_kwargs(call, cname)
    routes = {"first_round": ("decode", "decode_device", "iter"), "second_round": ("decode", "decode_device", "iter"), "in_parts": ("parts",),
              "collects_redo": ("iter",)}[what]
    for route in routes:
        be = _ViewBackend(script, known=call.files[1:]).install(monkeypatch)
        monkeypatch.setitem(sys.modules, "torch", _torch_stand_in(be))
        dec = _decoder("xmajor")
        try:
            with pytest.raises(CorruptedJpeg, match=rf"^image {named}: Failed to decode image \({text}"):
                if route == "decode":
                    dec.decode(call.files, **kw)
                elif route == "decode_device":
                    dec.decode_device(call.files, parts=1, **kw)
                elif route == "parts":
                    dec.decode_device(call.files, parts=3, **kw)
                else:
                    list(dec.decode_device_iter([call.files], **{k: (iter([v]) if k in VC.PER_BATCH else v) for k, v in kw.items()}))
            records = be.take_records()
            holders = [files_of(r.rec, call.files) for r in records if named in files_of(r.rec, call.files)]
            assert holders, (route, "no plan held the damaged file")
            # (the message match above is what tells the three numberings apart: the file is named - 1 among the files that are read,
            # and in the plan that reported it it sits in front of both)
            assert holders[-1].index(named) < named - 1, (route, "the file sits at a named position in the plan that reported it", holders)
            if what in ("second_round", "collects_redo"):
                assert len(holders) >= 2, (route, "the damage was not found in a second round", holders)
            assert all(p.closed for p in be.plans), (route, "a plan stayed open behind the exception")
        finally:
            dec.close()


def test_an_affine_refusal_names_the_output_and_the_file_in_the_callers_numbering(monkeypatch, call):
    """a corner beyond 32768 for ONE view of a second-round file: `output k (file i)`, k the view's position in the call and i the
    file's position in the caller's list"""
    tail = positions(call.entries, "tail")[1]
    v = [v for v in call.views if v.file == tail + 1][1]
    for cname in ("affine_nearest", "affine_bicubic_orient"):
        kw = VC.call_kwargs(call, cname)
        kw["affine"] = list(kw["affine"])
        kw["affine"][v.k] = (1.0, 0.0, 40000.0, 0.0, 1.0, 0.0)
        be = _ViewBackend(_script(call.entries), known=call.files[1:]).install(monkeypatch)
        monkeypatch.setitem(sys.modules, "torch", _torch_stand_in(be))
        dec = _decoder("xmajor")
        try:
            for route in (dec.decode, dec.decode_device):
                with pytest.raises(ValueError, match=rf"^affine: output {v.k} \(file {v.file}\): a corner of the output has a source coordinate"):
                    route(call.files, **kw)
            assert not be.plans, "a plan was made for a call that is refused"
        finally:
            dec.close()


def test_a_perspective_refusal_and_a_bad_chain_name_the_output_in_the_callers_numbering(monkeypatch, call):
    """a coefficient that is not finite for ONE view of a second-round file: `output k (file i)` as an affine refusal names them; a
    chain that cannot be for that view: `output k`; no plan is made for either call"""
    tail = positions(call.entries, "tail")[1]
    v = [v for v in call.views if v.file == tail + 1][1]
    cases = [("perspective_bicubic_orient", "perspective", (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, float("inf"), 0.0),
              rf"^perspective: output {v.k} \(file {v.file}\): a coefficient is not finite"),
             ("perspective_nearest_colour_L", "perspective", (1.0, 0.0, float("nan"), 0.0, 1.0, 0.0, 0.0, 0.0),
              rf"^perspective: output {v.k} \(file {v.file}\): a coefficient is not finite"),
             ("colour_f16", "color_ops", (("posterize", 9),), rf"^color_ops: output {v.k}: posterize takes 1\.\.8 bits"),
             ("perspective_nearest_colour_L", "color_ops", (("invert",), ("posterize", 9)), rf"^color_ops: output {v.k}: posterize takes 1\.\.8 bits")]
    for cname, name, bad, text in cases:
        kw = VC.call_kwargs(call, cname)
        kw[name] = list(kw[name])
        kw[name][v.k] = bad
        be = _ViewBackend(_script(call.entries), known=call.files[1:]).install(monkeypatch)
        monkeypatch.setitem(sys.modules, "torch", _torch_stand_in(be))
        dec = _decoder("xmajor")
        try:
            for route in (dec.decode, dec.decode_device):
                with pytest.raises(ValueError, match=text):
                    route(call.files, **kw)
            assert not be.plans, "a plan was made for a call that is refused"
        finally:
            dec.close()


def test_the_stand_in_refuses_a_window_that_does_not_lie_inside_its_oriented_image(monkeypatch):
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    e = call_files()[0]                               # 200 x 120
    _ViewBackend().install(monkeypatch)
    dec = BatchDecoder(device=0)
    prep = prepare_batch([e.raw], B.MJ_LAYOUT_XMAJOR, 0)
    keep = {"prep": prep, "n_images": 1}
    B.Plan(dec.ctx, prep.to_c(), keep, size=VC.SIZE, views=[(0, (80, 0, 120, 120))])
    B.Plan(dec.ctx, prep.to_c(), keep, size=VC.SIZE, views=[(0, (0, 80, 120, 120))], orientation=[6])
    for kw in (dict(views=[(0, (0, 80, 120, 120))]), dict(views=[(0, (80, 0, 120, 120))], orientation=[6]), dict(views=[(0, (0, 0, 0, 4))])):
        with pytest.raises(B.BackendError, match="not inside"):
            B.Plan(dec.ctx, prep.to_c(), keep, size=VC.SIZE, **kw)
    dec.close()
