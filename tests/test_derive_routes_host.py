"""also= on every route without a GPU: BatchDecoder.decode, decode_device (one call, two parts) and decode_device_iter with the
stand-ins of tests/test_view_routes_host.py for `_binding.Context`, `_binding.Plan` and torch.  A derived plan is, to the stand-in, a
plan of its own keywords over the same batch — it computes its outputs with the models from what IT was given —, so what is held
here is the host's part alone: which group makes the plan that decodes and which derive from it, which files, views, flags, places
and slots every plan of every group gets through `_Request.narrow`, into which tensor it writes, and that a file is in one
decoding plan per round however many groups name it."""
import sys

import numpy as np
import pytest

from routes_common import with_com
from test_request_routes_host import _torch_stand_in
from test_view_routes_host import _ViewBackend

SIZE, SMALL, TINY = (24, 16), (12, 10), (7, 9)
NAMES = ("128x64_420_dri3", "50x70_grey_dri4", "64x48_422_pil", "prog_70x50_420_pil", "128x64_420_pil_rst", "100x36_420_dri7")


def _files():
    from conftest import GOLDEN
    raws = [(GOLDEN / "files" / f"{n}.jpg").read_bytes() for n in NAMES]
    raws[4] = with_com(raws[4])             # (the GPU marker scan hands this one back: a second round)
    return raws + [b"not a jpeg"]


CALL = dict(size=SIZE, mode="RGB", resample="bicubic", mirror=[True, False, False, True, True, False, True],
            views=[(4, (100, 30, 28, 34)), (0, None), (1, (0, 0, 50, 70)), (3, (2, 3, 60, 40)), (0, (3, 5, 61, 40)), (2, (5, 7, 33, 20)), (4, None)])
ALSO = [dict(size=SMALL, views=[(5, None), (4, (3, 5, 61, 40)), (0, (64, 0, 7, 64)), (5, (1, 2, 90, 30)), (3, None), (4, (1, 1, 9, 9))],
             mirror=[False, True, True, False, False, True], dtype="float16", normalize=((0.4, 0.5, 0.6), (0.2, 0.3, 0.4))),
        dict(size=TINY, views=[2, 0, 4], resample="box", resize_to=[(9, 5), (4, 12), (7, 9)], place=[(-1, 2), (1, -2), (0, 0)], fill=(1, 2, 3),
             color_ops=[None, [("invert",)], [("posterize", 3)]])]


class _Installed:
    def __init__(self, monkeypatch, files, script):
        from pyjpegdecoder_amd import _binding as B
        self.be = _ViewBackend(script, known=list(dict.fromkeys(f for f in files if f != b"not a jpeg"))).install(monkeypatch)
        be = self.be
        be.derived = []

        def derive(plan, prep, **kw):
            child = B.Plan(None, prep.to_c(), {"prep": prep, "n_images": len(prep.parsed)}, **kw)
            assert not plan.closed and prep is plan_prep[id(plan)], "derived from a closed plan, or with another batch than the parent's"
            be.derived.append((plan, child))
            return child
        plan_prep = {}
        made = B.Plan.__init__

        def init(plan, ctx, batch_c, keepalive, **kw):
            made(plan, ctx, batch_c, keepalive, **kw)
            plan_prep[id(plan)] = keepalive["prep"]
        monkeypatch.setattr(B.Plan, "__init__", init)
        monkeypatch.setattr(B.Plan, "derive", derive, raising=False)
        monkeypatch.setitem(sys.modules, "torch", _torch_stand_in(be))


def _as_array(t):
    return t if isinstance(t, np.ndarray) else t.a


def _alone(dec, files, call, group, how):
    from pyjpegdecoder_amd.batch import ALSO_CALL_WIDE
    kw = {k: v for k, v in call.items() if k in ALSO_CALL_WIDE} if group is not call else {}
    kw.update(group)
    return _as_array(getattr(dec, how)(files, **kw))


def _check(got, dec, files, how="decode_device", call=CALL, also=ALSO):
    assert isinstance(got, tuple) and len(got) == 1 + len(also)
    for g, (element, group) in enumerate(zip(got, [call] + list(also))):
        want = _alone(dec, files, call, group, how)
        a = _as_array(element)
        assert a.shape == want.shape and a.dtype == want.dtype and np.array_equal(a.view(np.uint8), want.view(np.uint8)), g


def _check_plans(inst, files):
    """every round decodes a file in ONE plan; derived plans hang on open parents of the same batch and are all closed"""
    be = inst.be
    derived = {id(c) for _, c in be.derived}
    decoding = [p for p in be.plans if id(p) not in derived]
    first_round, seen = [], set()
    for p in decoding:                        # (a second round decodes its files again: by then they were seen)
        fresh = [r for r in p.raws if r not in seen]
        first_round += fresh
        seen.update(p.raws)
    assert sorted(first_round) == sorted(set(files[:-1])), "a file was decoded in two plans of one round, or not at all"
    assert b"not a jpeg" not in seen
    assert be.derived and all(p.closed for p in be.plans)
    for parent, child in be.derived:
        assert child.raws == parent.raws and child.size != parent.size or child.kw["views"] != parent.kw["views"]


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
def test_decode_with_extra_groups(monkeypatch, layout):
    from pyjpegdecoder_amd import BatchDecoder
    files = _files()
    inst = _Installed(monkeypatch, files, {files[4]: "tail"})
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        got = dec.decode(files, also=ALSO, **CALL)
        _check_plans(inst, files)
        assert all(isinstance(a, np.ndarray) for a in got) and [a.shape[0] for a in got] == [7, 6, 3] and got[1].dtype == np.float16
        _check(got, dec, files, "decode")
    finally:
        dec.close()


@pytest.mark.parametrize("route", ["one_call_native", "one_call_python", "two_parts", "iter"])
@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
def test_decode_device_with_extra_groups(monkeypatch, layout, route):
    from pyjpegdecoder_amd import BatchDecoder
    files = _files()
    inst = _Installed(monkeypatch, files, {files[4]: "tail"})
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1, native_host=route != "one_call_python")
    try:
        if route == "iter":
            per = {k: v for k, v in CALL.items() if k not in ("views", "mirror")}
            (got,) = list(dec.decode_device_iter([files], views=[CALL["views"]], mirror=[CALL["mirror"]], also=[ALSO], **per))
        else:
            got = dec.decode_device(files, parts=2 if route == "two_parts" else 1, also=ALSO, **CALL)
        _check_plans(inst, files)
        assert [_as_array(t).shape[0] for t in got] == [7, 6, 3]
        _check(got, dec, files)
    finally:
        dec.close()


def test_one_kind_of_file_named_by_every_group_is_one_decoding_plan(monkeypatch):
    """the multi-crop case: every group names every file, so a batch is ONE plan that decodes and one derived plan per extra group"""
    from pyjpegdecoder_amd import BatchDecoder
    files = [_files()[i] for i in (0, 5, 0, 5)]                 # (a group without views names every file of the call)
    call = dict(size=SIZE, views=[(k % 4, (k, k, 30, 20)) for k in range(8)], mirror=[k % 3 == 0 for k in range(8)])
    also = [dict(size=SMALL, views=[(3 - k % 4, (2 * k, k, 40, 16)) for k in range(12)]), dict(size=TINY, mirror=[False, True, True, False])]
    inst = _Installed(monkeypatch, files, {})
    dec = BatchDecoder(device=0, layout="rowmajor", segment="gpu", gpu_segment_min_files=1)
    try:
        got = dec.decode_device(files, also=also, **call)
        derived = {id(c) for _, c in inst.be.derived}
        assert len(inst.be.plans) == 3 and len(derived) == 2 and len({id(p) for p, _ in inst.be.derived}) == 1
        _check(got, dec, files, call=call, also=also)
    finally:
        dec.close()
