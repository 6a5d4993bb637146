"""erase= on the routes where a file goes round again, on the MI355X: routes_common.call_files() — files of several kinds, hence
several plans into one tensor, files the GPU marker scan hands back and files whose synchronisation rounds are kept from settling,
hence second rounds that rewrite their slots — through decode_device in one piece and in three parts, decode_device_iter, decode, and
an also= call whose groups carry different boxes.  Every output is the same route's output without erase= with the model
(tools/erase_model.py) applied; the plans made are those of the call without it."""
import numpy as np
import pytest

from erase_cases import box_cases, model_outputs, same_bits, storage, with_values
from routes_common import ITER_BATCHES, NORMALIZE, SIZE, assert_second_rounds, call_files, record_of

pytestmark = pytest.mark.gpu

TWO_LAYOUTS = ("xmajor", "planar_rowmajor")
SMALL = (24, 16)


@pytest.fixture(scope="module")
def entries():
    return call_files()


@pytest.fixture
def unsettled(tune):
    """as tests/test_request_routes.py: the synchronisation form wherever it can be taken, and nothing that lets it settle"""
    for name, value in (("MJ_HUFFMAN", "sync"), ("MJ_SYNC_WARM", "0"), ("MJ_SYNC_CHUNK", "256"), ("MJ_SYNC_ROUNDS", "0")):
        tune(name, value)


@pytest.fixture
def plans(monkeypatch):
    """`_binding.Plan` wrapped: every plan a decoder makes is noted (routes_common.PlanRecord) before it is created"""
    from pyjpegdecoder_amd import _binding as B

    class Recorder:
        def __init__(self):
            self.records = []

        def take(self):
            out, self.records = self.records, []
            return out
    rec = Recorder()

    class RecordingPlan(B.Plan):
        def __init__(self, ctx, batch_c, keepalive, rois=None, size=None, slots=None, output=None, **kw):
            rec.records.append(record_of(batch_c, keepalive, slots))
            super().__init__(ctx, batch_c, keepalive, rois=rois, size=size, slots=slots, output=output, **kw)

    monkeypatch.setattr(B, "Plan", RecordingPlan)
    return rec


def boxes_for(n, size, dtype, seed, skip=1):
    """one entry per output: the box list's cases in turn, every fourth output (from ``skip``) without a box"""
    cases = box_cases(*size)
    names = list(cases)
    return [None if k % 4 == skip else with_values(cases[names[(k + seed) % len(names)]], 3, dtype, seed + k, kinds=("values", "number", "per_component")[k % 3:] + ("values",))
            for k in range(n)]


def check(got, base, erase, layout, dtype, what):
    got, base = storage(got), storage(base)
    want = model_outputs(base, erase, layout, dtype)
    assert got.shape == want.shape
    for k in range(len(want)):
        assert same_bits(got[k], want[k]), (what, layout, "output", k)
        assert (erase[k] is None) == same_bits(got[k], base[k]), (what, layout, "output", k, "erased or not")


def same_plans(a, b):
    return [(r.n_images, r.flags, r.slots, r.files) for r in a] == [(r.n_images, r.flags, r.slots, r.files) for r in b]


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode_device(entries, unsettled, plans, layout, parts):
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    erase = boxes_for(len(raws), SIZE, "float16", 1)
    assert all(erase[i] is not None for i, e in enumerate(entries) if e.kind in ("tail", "unconverged"))
    kw = dict(size=SIZE, dtype="float16", normalize=NORMALIZE, mirror=[e.mirror for e in entries], parts=parts)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = dec.decode_device(raws, **kw)
        without = plans.take()
        got = dec.decode_device(raws, erase=erase, **kw)
        made = plans.take()
        check(got, base, erase, layout, "float16", ("decode_device", parts))
        assert_second_rounds(made, entries, True, ("erase", layout, parts), one_plan_each=parts == 1)
        assert same_plans(made, without)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode_device_iter(entries, unsettled, plans, layout):
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    erase = boxes_for(len(raws), SIZE, "bfloat16", 2, skip=2)
    batches = [[raws[i] for i in b] for b in ITER_BATCHES]
    per_batch = [[erase[i] for i in b] for b in ITER_BATCHES]
    kw = dict(size=SIZE, dtype="bfloat16", mirror=[[entries[i].mirror for i in b] for b in ITER_BATCHES])
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = list(dec.decode_device_iter(batches, **kw))
        without = plans.take()
        got = list(dec.decode_device_iter(batches, erase=per_batch, **kw))
        made = plans.take()
        assert len(got) == len(batches) and same_plans(made, without)
        for k, b in enumerate(ITER_BATCHES):
            assert len(got[k]) == len(b)
            if b:
                check(got[k], base[k], per_batch[k], layout, "bfloat16", ("iter", k))
        with pytest.raises(ValueError, match="erase yields fewer entries than there are batches"):
            list(dec.decode_device_iter(batches[:2], erase=per_batch[:1], **dict(kw, mirror=None)))
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode(entries, unsettled, plans, layout):
    """the NumPy route, through the library as well: the values live in a block of the HIP runtime's own"""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    erase = boxes_for(len(raws), SIZE, "float32", 3, skip=0)
    kw = dict(size=SIZE, dtype="float32", normalize=NORMALIZE)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = dec.decode(raws, **kw)
        without = plans.take()
        got = dec.decode(raws, erase=erase, **kw)
        made = plans.take()
        assert isinstance(got, np.ndarray)
        check(got, base, erase, layout, "float32", "decode")
        assert_second_rounds(made, entries, False, ("erase", "decode", layout))
        assert same_plans(made, without)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_two_groups_with_different_boxes(entries, unsettled, plans, layout):
    """also=: the derived plans erase their own outputs, second rounds included; a group without boxes stays as it was"""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    first, second = boxes_for(len(raws), SIZE, "float16", 4), boxes_for(len(raws), SMALL, "uint8", 5, skip=3)
    kw = dict(size=SIZE, dtype="float16", normalize=NORMALIZE, parts=1)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = dec.decode_device(raws, also=[dict(size=SMALL, dtype="uint8", normalize=None), dict(size=SMALL, dtype="uint8", normalize=None)], **kw)
        without = plans.take()
        got = dec.decode_device(raws, erase=first, also=[dict(size=SMALL, dtype="uint8", normalize=None, erase=second),
                                                         dict(size=SMALL, dtype="uint8", normalize=None)], **kw)
        made = plans.take()
        assert len(got) == 3 and same_plans(made, without)
        check(got[0], base[0], first, layout, "float16", "also: the call's group")
        check(got[1], base[1], second, layout, "uint8", "also: the extra group")
        assert same_bits(storage(got[2]), storage(base[2]))
    finally:
        dec.close()
