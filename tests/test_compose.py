"""compose= on the MI355X (mj_compose; BatchDecoder.decode_device(size=..., compose=...)): several outputs of a call pasted onto one
canvas.  At the C ABI the whole case list (tests/compose_cases.py) over device arrays of random bits, against tools/compose_model.py
— which tests/test_compose_host.py holds to Pillow's Image.paste — and against the host twin; through decode_device the model
applied to the library's own output of the same call without compose=.  Bit patterns, in every layout; no tolerance anywhere."""
import numpy as np
import pytest

from compose_cases import BITS, DTYPES, LAYOUTS, all_cases, fill_for, full_form, model_compose, random_bits, same_bits, shape_of, storage
from test_colour import C411, GREY, KINDS, ODD, raw

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TILE, CANVAS = (40, 28), (56, 44)          # routes_common.SIZE, and the composed size
CASES = all_cases()
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


# ---- at the C ABI ----------------------------------------------------------------------------------------------------------
def launch(dec, layout, dtype, C, pre, ssize, dsize, fill, outputs, front=(0, 0)):
    """Context.compose from ``pre`` (host, bit patterns) into a sentinel-filled buffer; ``front``: bytes in front of src and dst inside
    their buffers.  Returns the composed array; the sentinels around it are checked, and that src is as it was."""
    import torch
    es = pre.dtype.itemsize
    nbytes = len(outputs) * dsize[0] * dsize[1] * C * es
    fs, fd = front
    src = torch.full((fs + pre.nbytes + 61,), 0x5A, dtype=torch.uint8, device="cuda:0")
    dst = torch.full((fd + nbytes + 61,), 0xA5, dtype=torch.uint8, device="cuda:0")
    src[fs:fs + pre.nbytes] = torch.from_numpy(np.ascontiguousarray(pre).reshape(-1).view(np.uint8)).to("cuda:0")
    torch.cuda.synchronize()
    dec.ctx.compose(src.data_ptr() + fs, dst.data_ptr() + fd, LAYOUTS.index(layout), dtype, C, ssize, len(pre), dsize, fill, outputs)
    torch.cuda.synchronize()                # (the context's stream is not torch's: wait for the device)
    got = dst.cpu().numpy()
    assert (got[:fd] == 0xA5).all() and (got[fd + nbytes:] == 0xA5).all(), ("a sentinel was written", front)
    kept = src.cpu().numpy()
    assert (kept[:fs] == 0x5A).all() and same_bits(kept[fs:fs + pre.nbytes], np.ascontiguousarray(pre).reshape(-1).view(np.uint8))
    return got[fd:fd + nbytes].copy().view(pre.dtype).reshape((len(outputs),) + shape_of(layout, dsize[0], dsize[1], C))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_case_list_on_the_device(layout, C, dtype):
    """every case from 256-byte-aligned arrays, and with src and dst one element past a 16-byte boundary (and one and two elements:
    not congruent), so that every line has a head and a tail of lone elements; against the model and against mj_host_compose"""
    from pyjpegdecoder_amd import _binding as B
    dec = decoder(layout)
    es = np.dtype(BITS[dtype]).itemsize
    fronts = [(0, 0), (64 + es, 64 + es), (64 + es, 64 + 2 * es)]
    for name, ssize, dsize, outputs, three in CASES:
        pre = np.array(random_bits(dtype, layout, ssize[0], ssize[1], C))
        fill = fill_for(es, C, three)
        want = model_compose(pre, outputs, dsize, layout, fill)
        twin = B.host_compose(pre, LAYOUTS.index(layout), dtype, C, ssize, dsize, fill, outputs).reshape(want.shape)
        assert same_bits(twin, want), (name, "host twin")
        for front in fronts:
            got = launch(dec, layout, dtype, C, pre, ssize, dsize, fill, outputs, front)
            for m in range(len(outputs)):
                assert same_bits(got[m], want[m]), (name, layout, C, dtype, dsize, front, "output", m)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_canvas_of_many_jobs(layout):
    """a 300 x 200 float32 canvas from 64 sources of 37 x 25 in a grid whose tiles overlap and run over the right edge — 720 KB, many
    jobs —, beside a canvas that is one fill rectangle of many jobs; then 150 x 120 sources, whose rectangles are several jobs each"""
    dec = decoder(layout)
    fill = fill_for(4, 3, True)
    pre = np.array(random_bits("float32", layout, 37, 25, 3, n=64))
    grid = [(k, (-3 + 36 * (k % 8), 2 + 24 * (k // 8)), (0, 0, 37, 25)) for k in range(64)]
    outputs = [grid, [], grid[::-1][:40]]
    want = model_compose(pre, outputs, (300, 200), layout, fill)
    got = launch(dec, layout, "float32", 3, pre, (37, 25), (300, 200), fill, outputs, (64 + 4, 64 + 8))
    for m in range(len(outputs)):
        assert same_bits(got[m], want[m]), (layout, "output", m)
    assert not same_bits(got[0], got[2])
    big = np.array(random_bits("float32", layout, 150, 120, 3, n=3))
    outputs = [[(0, (-10, -7)), (1, (120, 60)), (2, (155, 90), (5, 3, 140, 110))], [(2, (0, 0)), (2, (150, 0)), (1, (0, 120)), (0, (150, 80))]]
    outputs = full_form(outputs, 150, 120)
    want = model_compose(big, outputs, (300, 200), layout, fill)
    got = launch(dec, layout, "float32", 3, big, (150, 120), (300, 200), fill, outputs)
    for m in range(len(outputs)):
        assert same_bits(got[m], want[m]), (layout, "large tiles, output", m)


def test_two_calls_in_a_row_on_two_streams():
    """different tiles, different streams, back to back: the second call must not rewrite the job list under the first launch"""
    import torch
    layout, dtype, C = "rowmajor", "float16", 3
    dec = decoder(layout)
    name, ssize, dsize, first, _ = next(c for c in CASES if c[0] == "chain")
    second = next(c for c in CASES if c[0] == "chain_reversed" and c[1] == ssize)[3]
    pre = np.array(random_bits(dtype, layout, ssize[0], ssize[1], C))
    fill = fill_for(2, C, True)
    src = torch.from_numpy(pre.view(np.int16)).to("cuda:0")
    a = torch.zeros((1,) + shape_of(layout, dsize[0], dsize[1], C), dtype=torch.int16, device="cuda:0")
    b = torch.zeros_like(a)
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    args = (LAYOUTS.index(layout), dtype, C, ssize, len(pre), dsize, fill)
    dec.ctx.compose(src.data_ptr(), a.data_ptr(), *args, first, stream=s1.cuda_stream)
    dec.ctx.compose(src.data_ptr(), b.data_ptr(), *args, second, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert same_bits(a.cpu().numpy().view(np.uint16), model_compose(pre, first, dsize, layout, fill))
    assert same_bits(b.cpu().numpy().view(np.uint16), model_compose(pre, second, dsize, layout, fill))


def test_what_mj_compose_refuses():
    import torch
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.errors import BackendError
    dec = decoder("rowmajor")
    src = torch.zeros((2, 9, 13, 3), dtype=torch.float32, device="cuda:0")
    dst = torch.zeros((1, 14, 21, 3), dtype=torch.float32, device="cuda:0")

    def compose(outputs, s=None, d=None, layout=1, dtype="float32", C=3, ssize=(13, 9), n=2, dsize=(21, 14)):
        dec.ctx.compose(src.data_ptr() if s is None else s, dst.data_ptr() if d is None else d, layout, dtype, C, ssize, n, dsize, (1, 2, 3), outputs)
    for outputs, msg in [([[(2, (0, 0), (0, 0, 1, 1))]], "mj_compose: tile 0 .output 0, source 2.*no such source"),
                         ([[(0, (0, 0), (0, 0, 1, 1)), (1, (0, 0), (0, 0, 0, 1))]], "tile 1 .*a width or height below 1"),
                         ([[(0, (0, 0), (1, 0, 13, 9))]], "tile 0 .*the window is not inside the source canvas"),
                         ([[(0, (1 << 20, 0), (0, 0, 1, 1))]], "tile 0 .*an offset of 2.20 or more"),
                         ([[(0, (0, 0), (0, 0, 1, 1))] * 65], "tile 64 .*more than 64 tiles in one output")]:
        with pytest.raises(BackendError, match=msg):
            compose(outputs)
    ok = [[(0, (0, 0), (0, 0, 13, 9))]]
    for kw, msg in [(dict(d=src.data_ptr()), "src and dst overlap"), (dict(d=src.data_ptr() + 64), "src and dst overlap"), (dict(s=src.data_ptr() + 2), "not aligned to its 4-byte elements"),
                    (dict(layout=4), "layout 4"), (dict(C=2), "2 components"), (dict(dsize=(0, 14)), "outputs of 0 x 14"), (dict(ssize=(13, 65536)), "sources of 13 x 65536"),
                    (dict(n=0), "0 sources")]:
        with pytest.raises(BackendError, match=msg):
            compose(ok, **kw)
    # a refused call launched nothing
    torch.cuda.synchronize()
    assert not dst.any().item()


# ---- through decode_device --------------------------------------------------------------------------------------------------
def output_kw(dtype, mode="RGB"):
    if dtype == "uint8":
        return {}
    if dtype != "float16":
        return dict(dtype=dtype)
    return dict(dtype=dtype, normalize=(MEAN, STD) if mode == "RGB" else (0.449, 0.226))


def padding_element(layout, fill, mode, dtype):
    """what a call of this element type writes as fill= padding: a border element, per component, of a 100 x 36 file contained in the
    40 x 28 canvas (rows 0..6 are border)"""
    from tools.erase_model import chw_view
    out = storage(decoder(layout).decode_device([raw(C411)], size=TILE, resize_to="contain", fill=fill, mode=mode, **output_kw(dtype, mode)))
    border = chw_view(out[0], layout)
    assert (border[:, :7, :] == border[:, :1, :1]).all()
    return border[:, 0, 0].copy()


# a mosaic of the four files around (30, 20), a second output with a crop of output 2 pasted into output 0 off the edge, a row of all
MOSAIC = [[(0, (-10, -8)), (1, (30, -8)), (2, (-10, 20)), (3, (30, 20), (5, 3, 26, 24))],
          [(0, (8, 8)), (2, (40, 30), (10, 5, 25, 20))],
          [(3, (0, 0), (0, 0, 14, 28)), (2, (14, 0), (0, 0, 14, 28)), (1, (28, 0), (0, 0, 14, 28)), (0, (42, 0), (0, 0, 14, 28)), (1, (20, 30), (20, 14, 20, 14))]]


def held_to_the_model(layout, names, outputs, dtype, own_fill=None, mode="RGB", what=None, **kw):
    """the call (``kw``) with compose= against the model applied to the same call without it; the expected fill elements are what a
    call of this element type writes as padding for the bytes ``own_fill`` (else the call's fill=, else 0).  Returns (without, with)."""
    dec = decoder(layout)
    files = [raw(n) for n in names]
    kw = dict(kw, size=TILE, mode=mode, **output_kw(dtype, mode))
    base = storage(dec.decode_device(files, **kw))
    got = storage(dec.decode_device(files, compose=dict(size=CANVAS, outputs=outputs, **({} if own_fill is None else {"fill": own_fill})), **kw))
    C = 3 if mode == "RGB" else 1
    expect = own_fill if own_fill is not None else kw["fill"] if kw.get("fill") is not None else (0,) * C
    elements = padding_element(layout, expect, mode, dtype)
    want = model_compose(base, full_form(outputs, *TILE), CANVAS, layout, elements)
    assert got.shape == want.shape == (len(outputs),) + shape_of(layout, CANVAS[0], CANVAS[1], C) and got.dtype == want.dtype
    for m in range(len(want)):
        assert same_bits(got[m], want[m]), (what, layout, dtype, mode, "output", m)
    return base, got


@pytest.mark.parametrize("dtype", ["uint8", "float16"])
@pytest.mark.parametrize("mode", ["RGB", "L"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_four_kinds_of_file_into_mosaics(layout, mode, dtype):
    """several plans into one tile tensor, so that a canvas's tiles are several plans' outputs; the fill from compose=, from the call's
    fill= and absent"""
    C = 3 if mode == "RGB" else 1
    own = (114, 7, 200)[:C]
    held_to_the_model(layout, KINDS, MOSAIC, dtype, own_fill=own, mode=mode, what="compose's fill")
    held_to_the_model(layout, KINDS, MOSAIC, dtype, mode=mode, what="no fill")
    call = (31, 140, 250)[:C]
    held_to_the_model(layout, KINDS, MOSAIC, dtype, mode=mode, what="the call's fill", resize_to=[(30, 20), (40, 28), (20, 28), (36, 24)],
                      place=[(0, 0)] * 4, fill=call)
    if C == 3:
        held_to_the_model(layout, KINDS, MOSAIC, dtype, own_fill=9, mode=mode, what="one byte for all")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_behind_everything_else(layout):
    """with views= — two crops of one file in one mosaic —, with mirror= on some tiles — windows are in the mirrored tile's
    coordinates —, with erase= on a tile — the erased box travels with the tile — and with color_ops="""
    views = [(0, (0, 0, 40, 30)), (0, (25, 15, 40, 30)), (1, (8, 8, 48, 48)), (0, (10, 5, 50, 40))]
    held_to_the_model(layout, [ODD, GREY], MOSAIC, "float16", own_fill=(1, 2, 3), what="views", views=views)
    base, got = held_to_the_model(layout, KINDS, MOSAIC, "uint8", what="mirror", mirror=[True, False, True, False])
    plain = storage(decoder(layout).decode_device([raw(n) for n in KINDS], size=TILE, mode="RGB"))
    assert not same_bits(base[0], plain[0]) and same_bits(base[1], plain[1])
    erase = [(2, 2, 30, 20, 1.5), None, [(0, 0, 5, 5, [0.25, -0.5, 3.0]), (20, 10, 14, 12)], None]
    base, got = held_to_the_model(layout, KINDS, MOSAIC, "float16", what="erase", erase=erase)
    unerased, plain = held_to_the_model(layout, KINDS, MOSAIC, "float16", what="no erase")
    assert not same_bits(base[0], unerased[0]) and not same_bits(got[1], plain[1])
    held_to_the_model(layout, KINDS, MOSAIC, "float16", own_fill=(114, 114, 114), what="color_ops", mirror=[False, True, False, True],
                      color_ops=[[("contrast", 1.4)], None, [("equalize",), ("gaussian_blur", 1.0)], [("adjust_hue", 0.2)]])


def test_without_compose_the_call_is_as_it_was(monkeypatch):
    """compose=None: no compose launch and no second tensor — the tensor the plans wrote is the one handed out"""
    from pyjpegdecoder_amd import _binding as B
    dec = decoder("rowmajor")
    files = [raw(n) for n in KINDS]
    kw = dict(size=TILE, mode="RGB")
    base = storage(dec.decode_device(files, **kw))
    launches = []
    real = B.Context.compose
    monkeypatch.setattr(B.Context, "compose", lambda self, *a, **k: (launches.append(a), real(self, *a, **k))[1])
    assert same_bits(storage(dec.decode_device(files, compose=None, **kw)), base)
    assert same_bits(storage(dec.decode_device(files, compose=None, also=[dict(size=(8, 8), compose=None)], **kw)[0]), base)
    assert not launches
    got = dec.decode_device(files, compose=dict(size=CANVAS, outputs=[[]]), **kw)
    assert len(launches) == 1 and tuple(got.shape) == (1, 44, 56, 3) and not got.any().item()


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
        got = dec.decode_device(files, compose=dict(size=CANVAS, outputs=MOSAIC), **kw)
        twice = got * 2
    s.synchronize()
    want = model_compose(base, full_form(MOSAIC, *TILE), CANVAS, layout, np.zeros(3, dtype=np.float32))
    assert same_bits(storage(got), want) and same_bits(storage(twice), want * 2)


def test_what_the_call_refuses_before_any_file_is_read():
    dec = decoder("rowmajor")
    not_files = [b"not a jpeg", b"nor this"]
    ok = dict(size=(20, 20), outputs=[[(0, (1, 1))]])
    for kw, msg in [(dict(compose=ok), "compose needs size"),
                    (dict(compose=ok, size=(8, 8), mix=[("cutmix", 1, (0, 0, 1, 1)), None]), "compose and mix do not go together"),
                    (dict(compose=[ok], size=(8, 8)), "compose must be None or a dict"),
                    (dict(compose=dict(ok, outputs=[[(2, (0, 0))]]), size=(8, 8)), "compose: output 0, tile 0: source 2 is not"),
                    (dict(compose=dict(ok, outputs=[[(0, (0, 0)), (1, (0, 0), (0, 0, 9, 1))]]), size=(8, 8)), "compose: output 0, tile 1: window .* is not inside the 8 x 8 tile canvas"),
                    (dict(compose=dict(ok, fill=(1, 2)), size=(8, 8), mode="RGB"), "compose: fill must be None, one byte or one per output component"),
                    (dict(size=(8, 8), also=[dict(size=(4, 4), compose=dict(size=(9, 9), outputs=[[(0, (0, 0), (0, 0, 5, 5))]]))]),
                     r"also\[0\]: compose: output 0, tile 0: window .* is not inside the 4 x 4 tile canvas")]:
        with pytest.raises(ValueError, match=msg):
            dec.decode_device(not_files, **kw)
        with pytest.raises(ValueError, match=msg):
            dec.decode(not_files, **kw)
    with pytest.raises(ValueError, match="compose and return_seams do not go together|size and return_seams do not go together"):
        dec.decode(not_files, compose=ok, size=(8, 8), return_seams=True)
