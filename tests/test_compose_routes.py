"""compose= on the routes where a call is more than one plan, on the MI355X: routes_common.call_files() — files of several kinds, hence
several plans into one tile tensor, files the GPU marker scan hands back and files whose synchronisation rounds are kept from
settling, hence second rounds that rewrite their slots — through decode_device in one piece and in parts, decode_device_iter, decode,
and an also= call whose extra group has a compose of its own at another size while the primary has none.  Every result is the same
route's output without compose= with the model (tools/compose_model.py) applied: the compose runs once, behind every plan, so a tile
written by a second round is read as the second round left it.  The plans made are those of the call without the argument."""
import numpy as np
import pytest

from compose_cases import full_form, model_compose, same_bits, storage
from routes_common import ITER_BATCHES, NORMALIZE, SIZE, assert_second_rounds, call_files
from test_erase_routes import plans, same_plans, unsettled  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TWO_LAYOUTS = ("xmajor", "planar_rowmajor")
CANVAS = (56, 44)
SMALL, SMALL_CANVAS = (24, 16), (37, 23)
FILL = (7, 99, 201)


@pytest.fixture(scope="module")
def entries():
    return call_files()


def compose_for(n, tile, canvas, seed):
    """``compose=`` for ``n`` tiles of size ``tile``: mosaics of four around centres that move with the canvas's number (mosaic_tiles),
    every output a source of one of them, then a canvas with a strip of every output — a later strip over the one before"""
    from pyjpegdecoder_amd import mosaic_tiles
    (tw, th), (W, H) = tile, canvas
    outputs = []
    for m in range((n + 3) // 4):
        centre = (W // 2 - 6 + 3 * ((m + seed) % 5), H // 2 + 4 - 2 * ((m + seed) % 4))
        outputs.append([((4 * m + i) % n, at, win) for i, at, win in mosaic_tiles(canvas, centre, [(tw - (i + m) % 3, th - (i + seed) % 2) for i in range(4)])])
    outputs.append([(s, (-2 + 4 * s, 3 * (s % 3) - 1), (s % (tw - 8), 1, 8, th - 2)) for s in range(n)])
    return dict(size=canvas, fill=FILL, outputs=outputs)


def fill_elements(dtype, normalize, like):
    """FILL as the outputs store such a pixel: the bytes, or the bit patterns of the normalised values (tools/normalize_model.py)"""
    from tools import normalize_model
    if dtype == "uint8":
        return np.array(FILL, dtype=np.uint8)
    mean, std = normalize if normalize is not None else ((0.0,) * 3, (1.0,) * 3)
    bits = [normalize_model.table_bits(dtype, mean[c], std[c])[FILL[c]] for c in range(3)]
    return np.array(bits, dtype={2: np.uint16, 4: np.uint32}[like.dtype.itemsize]).view(like.dtype)


def check(got, base, compose, tile, layout, dtype, normalize, what):
    got, base = storage(got), storage(base)
    want = model_compose(base, full_form(compose["outputs"], *tile), compose["size"], layout, fill_elements(dtype, normalize, base))
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    for m in range(len(want)):
        assert same_bits(got[m], want[m]), (what, layout, "output", m)


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode_device(entries, unsettled, plans, layout, parts):
    """every file that goes round again is a tile of a mosaic and of the strip canvas"""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    n = len(raws)
    compose = compose_for(n, SIZE, CANVAS, 0)
    named = {s for tiles in compose["outputs"] for s, _, _ in tiles}
    assert named == set(range(n))
    kw = dict(size=SIZE, dtype="float16", normalize=NORMALIZE, mirror=[e.mirror for e in entries], parts=parts)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = dec.decode_device(raws, **kw)
        without = plans.take()
        got = dec.decode_device(raws, compose=compose, **kw)
        made = plans.take()
        assert len(got) == len(compose["outputs"])
        check(got, base, compose, SIZE, layout, "float16", NORMALIZE, ("decode_device", parts))
        assert_second_rounds(made, entries, True, ("compose", layout, parts), one_plan_each=parts == 1)
        assert same_plans(made, without)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode_device_iter(entries, unsettled, plans, layout):
    """one dict per batch, None for the empty one; an iterable that runs out before the batches do is refused"""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    batches = [[raws[i] for i in b] for b in ITER_BATCHES]
    per_batch = [compose_for(len(b), SIZE, CANVAS, k) if len(b) else None for k, b in enumerate(ITER_BATCHES)]
    kw = dict(size=SIZE, dtype="bfloat16", mirror=[[entries[i].mirror for i in b] for b in ITER_BATCHES])
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = list(dec.decode_device_iter(batches, **kw))
        without = plans.take()
        got = list(dec.decode_device_iter(batches, compose=per_batch, **kw))
        made = plans.take()
        assert len(got) == len(batches) and same_plans(made, without)
        for k, b in enumerate(ITER_BATCHES):
            if b:
                assert len(got[k]) == len(per_batch[k]["outputs"])
                check(got[k], base[k], per_batch[k], SIZE, layout, "bfloat16", None, ("iter", k))
            else:
                assert len(got[k]) == 0
        with pytest.raises(ValueError, match="compose yields fewer entries than there are batches"):
            list(dec.decode_device_iter(batches[:2], compose=per_batch[:1], **dict(kw, mirror=None)))
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_decode_equals_decode_device(entries, unsettled, plans, layout):
    """the NumPy route, through the library as well: uploaded, composed by mj_compose, downloaded"""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    compose = compose_for(len(raws), SIZE, CANVAS, 1)
    kw = dict(size=SIZE, dtype="float32", normalize=NORMALIZE)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = dec.decode(raws, **kw)
        without = plans.take()
        got = dec.decode(raws, compose=compose, **kw)
        made = plans.take()
        assert isinstance(got, np.ndarray)
        check(got, base, compose, SIZE, layout, "float32", NORMALIZE, "decode")
        assert_second_rounds(made, entries, False, ("compose", "decode", layout))
        assert same_plans(made, without)
        on_device = dec.decode_device(raws, compose=compose, parts=1, **kw)
        assert same_bits(storage(on_device), got)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", TWO_LAYOUTS)
def test_an_extra_group_with_a_compose_of_its_own(entries, unsettled, plans, layout):
    """also=: the primary group has no compose and stays as it was; an extra group at another size and element type is composed to
    another canvas size; a second extra group without the key stays as it was"""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [e.raw for e in entries]
    compose = compose_for(len(raws), SMALL, SMALL_CANVAS, 2)
    kw = dict(size=SIZE, dtype="float16", normalize=NORMALIZE, parts=1)
    dec = BatchDecoder(device=0, layout=layout, segment="gpu", gpu_segment_min_files=1)
    try:
        base = dec.decode_device(raws, also=[dict(size=SMALL, dtype="uint8", normalize=None), dict(size=SMALL, dtype="uint8", normalize=None)], **kw)
        without = plans.take()
        got = dec.decode_device(raws, also=[dict(size=SMALL, dtype="uint8", normalize=None, compose=compose),
                                            dict(size=SMALL, dtype="uint8", normalize=None)], **kw)
        made = plans.take()
        assert len(got) == 3 and same_plans(made, without)
        assert same_bits(storage(got[0]), storage(base[0]))
        check(got[1], base[1], compose, SMALL, layout, "uint8", None, "also: the extra group")
        assert same_bits(storage(got[2]), storage(base[2]))
    finally:
        dec.close()
