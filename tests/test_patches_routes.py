"""patches= through the decoders on the MI355X, on the tests' small golden files: every result is the library's own output of the same
call without patches= with the model (tools/patch_model.py) applied, in all four layouts — the launch runs once per group, behind
every plan, behind erase, mix and compose.  Bit patterns; no tolerance anywhere."""
import numpy as np
import pytest

from patch_cases import LAYOUTS, model_patchify, same_bits, storage
from test_colour import C411, GREY, KINDS, ODD, raw

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TILE, CANVAS = (40, 28), (56, 44)
SPEC = dict(patch=2, merge=2, repeat=2)                         # Qwen's form at a small size: 4 divides 40, 28, 56 and 44
SIZES = [(32, 20), (40, 28), (20, 28), (36, 24)]               # per-file resize_to: multiples of 4
_DEC = {}


@pytest.fixture(scope="module", autouse=True)
def decoders():
    yield
    for dec in _DEC.values():
        dec.close()
    _DEC.clear()


def decoder(layout):
    if layout not in _DEC:
        from pyjpegdecoder_amd import BatchDecoder
        _DEC[layout] = BatchDecoder(device=0, layout=layout)
    return _DEC[layout]


def held_to_the_model(layout, names, spec, what, call="decode_device", **kw):
    """the call (``kw``) with patches= against the model applied to the same call without it.  Returns (without, with) as storage."""
    dec = decoder(layout)
    files = [raw(n) for n in names]
    kw = dict(dict(size=TILE, mode="RGB"), **kw)
    fn = getattr(dec, call)
    base = storage(fn(files, **kw))
    got = storage(fn(files, patches=spec, **kw))
    want = model_patchify(base, spec, layout)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert same_bits(got, want), (what, layout)
    return base, got


@pytest.mark.parametrize("layout", LAYOUTS)
def test_grey_and_colour_files_are_two_plans(layout):
    """four kinds of file under mode="RGB" and under mode="L": several plans into one tensor, packed by one launch; float16
    normalised, and the bytes; both orders; padded"""
    held_to_the_model(layout, KINDS, SPEC, "RGB float16", dtype="float16", normalize=(MEAN, STD))
    held_to_the_model(layout, KINDS, dict(patch=4, order="hwc"), "RGB uint8 hwc")
    base, got = held_to_the_model(layout, KINDS, dict(patch=4, merge=1, length=100), "padded", dtype="float32")
    assert got.shape == (4, 100, 48) and not got[:, 70:].any()
    held_to_the_model(layout, KINDS, dict(patch=2, merge=2), "L", mode="L", dtype="bfloat16")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_file_at_its_own_size(layout):
    """the use it is for: resize_to per file, place=(0, 0), and the windows that go with them; patch_grids gives the row offsets"""
    from pyjpegdecoder_amd import patch_grids
    spec = dict(SPEC, windows=[(0, 0, w, h) for w, h in SIZES])
    base, got = held_to_the_model(layout, KINDS, spec, "resize_to", resize_to=SIZES, place=[(0, 0)] * 4, resample="bicubic", dtype="bfloat16",
                                  normalize=(MEAN, STD))
    grids, cu = patch_grids(spec, 4, TILE)
    assert [tuple(g) for g in grids] == [(h // 2, w // 2) for w, h in SIZES] and cu[-1] == len(got) and got.shape[1] == 3 * 2 * 2 * 2
    # source 2's rows are its window alone
    alone = model_patchify(base[2:3], dict(SPEC, windows=[spec["windows"][2]]), layout)
    assert same_bits(got[cu[2]:cu[3]], alone)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_behind_views_erase_and_mix(layout):
    views = [(0, (0, 0, 40, 30)), (0, (25, 15, 40, 30)), (1, (8, 8, 48, 48)), (0, (10, 5, 50, 40))]
    held_to_the_model(layout, [ODD, GREY], dict(SPEC, windows=[None, (4, 4, 32, 20), None, (1, 3, 8, 24)]), "views", views=views, dtype="float16")
    erase = [(2, 2, 30, 20, 1.5), None, [(0, 0, 5, 5, [0.25, -0.5, 3.0]), (20, 10, 14, 12)], None]
    erased, got = held_to_the_model(layout, KINDS, SPEC, "erase", erase=erase, dtype="float16")
    plain, other = held_to_the_model(layout, KINDS, SPEC, "no erase", dtype="float16")
    assert not same_bits(erased[0], plain[0]) and not same_bits(got, other)
    mix = [("cutmix", 1, (4, 4, 20, 12)), None, ("mixup", 3, 0.25), ("cutmix", 0, (0, 0, 40, 28))]
    mixed, got = held_to_the_model(layout, KINDS, SPEC, "mix", mix=mix, dtype="float32")
    assert not same_bits(mixed[0], storage(decoder(layout).decode_device([raw(n) for n in KINDS], size=TILE, mode="RGB", dtype="float32"))[0])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_behind_compose_the_sources_are_the_canvases(layout):
    compose = dict(size=CANVAS, fill=(114, 7, 200), outputs=[[(0, (-10, -8)), (1, (30, -8)), (2, (-10, 20)), (3, (30, 20), (5, 3, 26, 24))], [(0, (8, 8))], []])
    base, got = held_to_the_model(layout, KINDS, dict(SPEC, windows=[None, (8, 8, 40, 28), (3, 5, 4, 36)]), "compose", compose=compose, dtype="float16")
    assert base.shape[0] == 3 and len(got) == (56 // 2) * (44 // 2) + 20 * 14 + 2 * 18
    with pytest.raises(ValueError, match="patches: windows has 4 entries for 3 sources"):
        decoder(layout).decode_device([raw(n) for n in KINDS], size=TILE, mode="RGB", compose=compose, patches=dict(SPEC, windows=[None] * 4))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_an_extra_group_with_patches_of_its_own(layout):
    """also=: the primary group has no patches and stays as it was; an extra group at another size and element type is packed"""
    dec = decoder(layout)
    files = [raw(n) for n in KINDS]
    kw = dict(size=TILE, mode="RGB", dtype="float16", normalize=(MEAN, STD))
    small = dict(size=(24, 16), dtype="uint8", normalize=None)
    base = dec.decode_device(files, also=[small, small], **kw)
    spec = dict(patch=4, merge=2, order="hwc", length=30)
    got = dec.decode_device(files, also=[dict(small, patches=spec), small], **kw)
    assert len(got) == 3 and same_bits(storage(got[0]), storage(base[0])) and same_bits(storage(got[2]), storage(base[2]))
    want = model_patchify(storage(base[1]), spec, layout)
    assert want.shape == (4, 30, 48) and not want[:, 24:].any() and same_bits(storage(got[1]), want)
    # and the other way round: the primary packed, the extra group as it was
    got = dec.decode_device(files, patches=SPEC, also=[small], **kw)
    assert same_bits(storage(got[0]), model_patchify(storage(base[0]), SPEC, layout)) and same_bits(storage(got[1]), storage(base[1]))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_in_parts_through_decode_and_through_the_iterator(layout):
    held_to_the_model(layout, KINDS * 2, SPEC, "parts", parts=2, dtype="float16")
    base, got = held_to_the_model(layout, KINDS, SPEC, "decode", call="decode", dtype="float32", normalize=(MEAN, STD))
    assert isinstance(got, np.ndarray)
    on_device = decoder(layout).decode_device([raw(n) for n in KINDS], size=TILE, mode="RGB", dtype="float32", normalize=(MEAN, STD), patches=SPEC)
    assert same_bits(storage(on_device), got)
    dec = decoder(layout)
    batches = [[raw(n) for n in KINDS], [raw(ODD), raw(GREY)], [raw(C411)]]
    specs = [SPEC, None, dict(patch=4, order="hwc", windows=[(4, 4, 32, 24)])]
    kw = dict(size=TILE, mode="RGB", dtype="bfloat16")
    base = list(dec.decode_device_iter(batches, **kw))
    got = list(dec.decode_device_iter(batches, patches=specs, **kw))
    assert len(got) == 3 and same_bits(storage(got[1]), storage(base[1]))
    for k in (0, 2):
        assert same_bits(storage(got[k]), model_patchify(storage(base[k]), specs[k], layout)), ("iter", k)
    with pytest.raises(ValueError, match="patches yields fewer entries than there are batches"):
        list(dec.decode_device_iter(batches[:2], patches=specs[:1], **kw))
    with pytest.raises(ValueError, match="patches must be None or an iterable"):
        list(dec.decode_device_iter(batches, patches=SPEC, **kw))


def test_without_patches_the_call_is_as_it_was(monkeypatch):
    """patches=None: no patchify launch and no second tensor — the tensor the plans wrote is the one handed out"""
    from pyjpegdecoder_amd import _binding as B
    dec = decoder("rowmajor")
    files = [raw(n) for n in KINDS]
    kw = dict(size=TILE, mode="RGB")
    base = storage(dec.decode_device(files, **kw))
    launches = []
    real = B.Context.patchify
    monkeypatch.setattr(B.Context, "patchify", lambda self, *a, **k: (launches.append(a), real(self, *a, **k))[1])
    assert same_bits(storage(dec.decode_device(files, patches=None, **kw)), base)
    assert same_bits(storage(dec.decode_device(files, patches=None, also=[dict(size=(8, 8), patches=None)], **kw)[0]), base)
    assert same_bits(dec.decode(files, patches=None, **kw), base)
    assert not launches
    got = dec.decode_device(files, patches=dict(patch=4), **kw)
    assert len(launches) == 1 and tuple(got.shape) == (4 * 70, 48)


def test_on_a_stream_of_the_callers():
    """the launch goes on torch's current stream: a caller's stream, and what is queued behind it there sees the result"""
    import torch
    layout = "planar_rowmajor"
    dec = decoder(layout)
    files = [raw(n) for n in KINDS]
    kw = dict(size=TILE, mode="RGB", dtype="float32")
    base = storage(dec.decode_device(files, **kw))
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        got = dec.decode_device(files, patches=SPEC, **kw)
        twice = got * 2
    s.synchronize()
    want = model_patchify(base, SPEC, layout)
    assert same_bits(storage(got), want) and same_bits(storage(twice), want * 2)


def test_what_the_call_refuses_before_any_file_is_read():
    dec = decoder("rowmajor")
    not_files = [b"not a jpeg", b"nor this"]
    for kw, msg in [(dict(patches=SPEC), "patches needs size"),
                    (dict(patches=[SPEC], size=(8, 8)), "patches must be None or a dict"),
                    (dict(patches=dict(SPEC, size=4), size=(8, 8)), "patches: unknown key 'size'"),
                    (dict(patches=dict(patch=3), size=(8, 8)), r"patches: source 0: the whole 8 x 8 canvas is not a multiple of patch \* merge = 3"),
                    (dict(patches=dict(SPEC, windows=[None]), size=(8, 8)), "patches: windows has 1 entries for 2 sources"),
                    (dict(patches=dict(SPEC, windows=[None, (0, 0, 12, 4)]), size=(8, 8)), r"patches: source 1: window \(0, 0, 12, 4\) is not inside the 8 x 8 canvas"),
                    (dict(patches=dict(SPEC, length=3), size=(8, 8)), "patches: source 0: 16 tokens, more than length 3"),
                    (dict(patches=dict(patch=64, merge=2), size=(128, 128), mode="RGB", dtype="float32"), "patches: a merge block of 196608 bytes"),
                    (dict(size=(8, 8), also=[dict(size=(6, 4), patches=SPEC)]), r"also\[0\]: patches: source 0: the whole 6 x 4 canvas is not a multiple")]:
        with pytest.raises(ValueError, match=msg):
            dec.decode_device(not_files, **kw)
        with pytest.raises(ValueError, match=msg):
            dec.decode(not_files, **kw)
    with pytest.raises(ValueError, match="patches and return_seams do not go together|size and return_seams do not go together"):
        dec.decode(not_files, patches=SPEC, size=(8, 8), return_seams=True)
