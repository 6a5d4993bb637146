"""mix= on the routes where a call is more than one plan, on the MI355X: routes_common.call_files() — files of several kinds, hence
several plans into one tensor, files the GPU marker scan hands back and files whose synchronisation rounds are kept from settling,
hence second rounds that rewrite their slots — through decode_device in one piece and in parts, decode_device_iter, decode, and an
also= call whose extra group has a mix of its own at another size.  Every output is the same route's output without mix= with the
model (tools/mix_model.py) applied: the mix runs once, behind every plan, so a partner written by a second round is read as the
second round left it.  The plans made are those of the call without the argument."""
import numpy as np
import pytest

from mix_cases import LAMS, model_mix, pairings, same_bits, single_boxes, storage
from routes_common import ITER_BATCHES, NORMALIZE, SIZE, assert_second_rounds, call_files
from test_erase_routes import plans, same_plans, unsettled  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TWO_LAYOUTS = ("xmajor", "planar_rowmajor")
SMALL = (24, 16)


@pytest.fixture(scope="module")
def entries():
    return call_files()


def mix_for(n, size, partners, seed, floats=True):
    """one entry per output: mixup / cutmix / None in turn (cutmix for mixup where the output is uint8)"""
    boxes = list(single_boxes(*size).values())
    out = []
    for k in range(n):
        kind = ("mixup", "cutmix", None)[(k + seed) % 3]
        if kind is None:
            out.append(None)
        elif kind == "mixup" and floats:
            out.append(("mixup", partners[k], LAMS[(k + seed) % len(LAMS)]))
        else:
            out.append(("cutmix", partners[k], boxes[(k + seed) % len(boxes)]))
    return out


def check(got, base, mix, layout, dtype, what):
    got, base = storage(got), storage(base)
    want = model_mix(base, mix, layout, dtype)
    assert got.shape == want.shape
    for k in range(len(want)):
        assert same_bits(got[k], want[k]), (what, layout, "output", k, mix[k])
    assert not same_bits(got, base), what


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode_device(entries, unsettled, plans, layout, parts):
    """the roll pairing: every file that goes round again is the partner of the file behind it"""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    n = len(raws)
    mix = mix_for(n, SIZE, pairings(n)["roll"], 0)
    again = [i for i, e in enumerate(entries) if e.kind in ("tail", "unconverged")]
    assert again and any(mix[(i + 1) % n] is not None for i in again)
    kw = dict(size=SIZE, dtype="float16", normalize=NORMALIZE, mirror=[e.mirror for e in entries], parts=parts)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = dec.decode_device(raws, **kw)
        without = plans.take()
        got = dec.decode_device(raws, mix=mix, **kw)
        made = plans.take()
        check(got, base, mix, layout, "float16", ("decode_device", parts))
        assert_second_rounds(made, entries, True, ("mix", layout, parts), one_plan_each=parts == 1)
        assert same_plans(made, without)
    finally:
        dec.close()


def test_parts_on_a_short_list(entries):
    """parts=2 over four files: the partner of the first part's first output is the second part's last"""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries if e.kind == "ordinary"][:4]
    assert len(raws) == 4
    mix = [("mixup", 3, 0.3), ("cutmix", 0, (3, 2, 20, 11)), None, ("mixup", 2, 0.8)]
    kw = dict(size=SIZE, dtype="float32", parts=2)
    dec = BatchDecoder(device=0, layout="rowmajor")
    try:
        check(dec.decode_device(raws, mix=mix, **kw), dec.decode_device(raws, **kw), mix, "rowmajor", "float32", "parts=2")
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode_device_iter(entries, unsettled, plans, layout):
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    batches = [[raws[i] for i in b] for b in ITER_BATCHES]
    per_batch = [mix_for(len(b), SIZE, pairings(len(b))["flip" if k & 1 else "roll"], k) if len(b) else None for k, b in enumerate(ITER_BATCHES)]
    kw = dict(size=SIZE, dtype="bfloat16", mirror=[[entries[i].mirror for i in b] for b in ITER_BATCHES])
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = list(dec.decode_device_iter(batches, **kw))
        without = plans.take()
        got = list(dec.decode_device_iter(batches, mix=per_batch, **kw))
        made = plans.take()
        assert len(got) == len(batches) and same_plans(made, without)
        for k, b in enumerate(ITER_BATCHES):
            assert len(got[k]) == len(b)
            if b:
                check(got[k], base[k], per_batch[k], layout, "bfloat16", ("iter", k))
        with pytest.raises(ValueError, match="mix yields fewer entries than there are batches"):
            list(dec.decode_device_iter(batches[:2], mix=per_batch[:1], **dict(kw, mirror=None)))
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode_equals_decode_device(entries, unsettled, plans, layout):
    """the NumPy route, through the library as well: uploaded, mixed by mj_mix, downloaded"""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    n = len(raws)
    mix = mix_for(n, SIZE, pairings(n)["cycle3"], 1)
    kw = dict(size=SIZE, dtype="float32", normalize=NORMALIZE)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = dec.decode(raws, **kw)
        without = plans.take()
        got = dec.decode(raws, mix=mix, **kw)
        made = plans.take()
        assert isinstance(got, np.ndarray)
        check(got, base, mix, layout, "float32", "decode")
        assert_second_rounds(made, entries, False, ("mix", "decode", layout))
        assert same_plans(made, without)
        on_device = dec.decode_device(raws, mix=mix, parts=1, **kw)
        assert same_bits(storage(on_device), got)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_an_extra_group_with_a_mix_of_its_own(entries, unsettled, plans, layout):
    """also=: the call's group and an extra group at another size and element type are each mixed within themselves, with different
    pairings; a group without the key stays as it was"""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    n = len(raws)
    first = mix_for(n, SIZE, pairings(n)["roll"], 2)
    second = mix_for(n, SMALL, pairings(n)["flip"], 0, floats=False)
    kw = dict(size=SIZE, dtype="float16", normalize=NORMALIZE, parts=1)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = dec.decode_device(raws, also=[dict(size=SMALL, dtype="uint8", normalize=None), dict(size=SMALL, dtype="uint8", normalize=None)], **kw)
        without = plans.take()
        got = dec.decode_device(raws, mix=first, also=[dict(size=SMALL, dtype="uint8", normalize=None, mix=second),
                                                       dict(size=SMALL, dtype="uint8", normalize=None)], **kw)
        made = plans.take()
        assert len(got) == 3 and same_plans(made, without)
        check(got[0], base[0], first, layout, "float16", "also: the call's group")
        check(got[1], base[1], second, layout, "uint8", "also: the extra group")
        assert same_bits(storage(got[2]), storage(base[2]))
    finally:
        dec.close()
