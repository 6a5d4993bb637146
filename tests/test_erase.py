"""erase= on the MI355X (mj_plan_set_erase; BatchDecoder.decode_device(size=..., erase=...)): boxes of the finished outputs
overwritten.  The expected elements of every case are tools/erase_model.py — which tests/test_erase_host.py holds to torch's slice
assignment, bit for bit — applied to the library's own output of the same call without erase=.  Bit patterns, in every layout."""
import numpy as np
import pytest

from erase_cases import DTYPES, LAYOUTS, box_cases, model_outputs, same_bits, storage, with_values
from test_colour import C411, C440, GREY, KINDS, ODD, raw

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
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


def held_to_the_model(layout, names, erase, el="uint8", what=None, **kw):
    """the call (``kw``) with erase= against the model applied to the same call without it — ``el``: the output's element type by name —;
    returns (without, with) in storage types"""
    dec = decoder(layout)
    files = [raw(n) for n in names]
    base = storage(dec.decode_device(files, **kw))
    got = storage(dec.decode_device(files, erase=erase, **kw))
    want = model_outputs(base, erase, layout, el)
    assert got.shape == want.shape and got.dtype == want.dtype
    for k in range(len(want)):
        assert same_bits(got[k], want[k]), (what, layout, el, "output", k)
    assert not same_bits(got, base), (what, "the boxes change nothing")
    return base, got


def output_kw(dtype):
    if dtype == "uint8":
        return {}
    return dict(dtype=dtype, normalize=(MEAN, STD)) if dtype == "float16" else dict(dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_four_kinds_of_file_in_every_dtype(layout, dtype):
    """several plans into one tensor (slots): boxes in the first and the last slot, an output with none between outputs with some,
    constants, per-component values and (C, h, w) values from NumPy and from a tensor on the GPU; no two boxes of an output meet, so
    every plan erases in ONE launch"""
    import torch
    W, H = 40, 28
    cases = box_cases(W, H)
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, size=(3, 5, 7)).astype(np.uint8) if dtype == "uint8" else rng.standard_normal((3, 5, 7)).astype(np.float32)
    on_gpu = torch.from_numpy(noise).to("cuda:0")
    erase = [with_values(cases["disjoint"], 3, dtype, 1),
             None,
             (5, 4, 7, 5, on_gpu),                                               # (one box, not a list)
             with_values(cases["corner_br"] + cases["corner_tl"] + cases["1xh"], 3, dtype, 2, kinds=("values", "per_component", "number"))]
    base, got = held_to_the_model(layout, KINDS, erase, dtype, size=(W, H), mode="RGB", **output_kw(dtype))
    assert same_bits(got[1], base[1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_box_list(layout):
    """every box of the host test's list, one per output (views of one file), values included; the overlapping pairs force one
    launch per box ordinal, and their two orders differ"""
    for (W, H), dtype in (((23, 17), "float16"), ((24, 16), "uint8"), ((40, 28), "float32")):
        cases = box_cases(W, H)
        names = list(cases)
        erase = [with_values(cases[n], 3, dtype, 10 + k, kinds=("values", "number", "per_component")[k % 3:] + ("values",)) for k, n in enumerate(names)]
        base, got = held_to_the_model(layout, [ODD], erase, dtype, what=(W, H), size=(W, H), views=[0] * len(names), **output_kw(dtype))
        # the same values in both orders of the overlapping pair
        a, b = with_values(cases["overlap"], 3, dtype, 5, kinds=("values",))
        _, two = held_to_the_model(layout, [ODD], [[a, b], [b, a]], dtype, what="orders", size=(W, H), views=[0, 0], **output_kw(dtype))
        assert not same_bits(two[0], two[1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_component(layout):
    W, H = 23, 17
    cases = box_cases(W, H)
    for dtype in ("uint8", "bfloat16"):
        erase = [with_values(cases["odd_x_odd_width"] + cases["corner_bl"], 1, dtype, 1, kinds=("values", "per_component")), None,
                 with_values(cases["overlap"], 1, dtype, 2), with_values(cases["whole"], 1, dtype, 3, kinds=("values",))]
        held_to_the_model(layout, KINDS, erase, dtype, size=(W, H), mode="L", **output_kw(dtype))
    # grey files in their own mode
    held_to_the_model(layout, [GREY, GREY], [(1, 1, 5, 3, 9), [(0, 0, 2, 2, [7])]], "uint8", size=(W, H))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_behind_everything_else(layout):
    """with mirror= — the boxes are not mirrored —, with color_ops= — the last store is the colour launch's —, with resize_to= and
    fill= — boxes over fill —, and with several views per file with different boxes"""
    W, H = 24, 16
    cases = box_cases(W, H)
    boxes = [with_values(cases["corner_tr"] + cases["odd_x_odd_width"], 3, "float16", 1), None, with_values(cases["wx1"], 3, "float16", 2),
             with_values(cases["disjoint"], 3, "float16", 3, kinds=("values",))]
    f16 = dict(dtype="float16", normalize=(MEAN, STD))
    base, got = held_to_the_model(layout, KINDS, boxes, "float16", "mirror", size=(W, H), mode="RGB", mirror=[True, False, True, True], **f16)
    plain = storage(decoder(layout).decode_device([raw(n) for n in KINDS], size=(W, H), mode="RGB", **f16))
    assert not same_bits(base[0], plain[0])                                      # (the flag does something, and the model's box stayed where it was)
    held_to_the_model(layout, KINDS, boxes, "float16", "color_ops", size=(W, H), mode="RGB", mirror=[False, True, False, True],
                      color_ops=[[("contrast", 1.4)], None, [("equalize",), ("gaussian_blur", 1.0)], [("adjust_hue", 0.2)]], **f16)
    u8 = [with_values(cases["corner_tl"] + cases["corner_br"], 3, "uint8", 4), with_values(cases["whole"], 3, "uint8", 5, kinds=("values",)), None,
          with_values(cases["1x1"], 3, "uint8", 6)]
    held_to_the_model(layout, KINDS, u8, "uint8", "places", size=(W, H), mode="RGB", resize_to=[(12, 8), (30, 10), (24, 16), (8, 20)],
                      place=[(0, 0), (-3, 3), (0, 0), (10, -2)], fill=(114, 7, 200))
    views = [(0, (3, 5, 40, 30)), (1, None), (0, None), (1, (10, 10, 30, 30)), (0, (20, 0, 30, 50))]
    per_view = [with_values(cases["corner_bl"], 3, "float32", 7), with_values(cases["overlap"], 3, "float32", 8), None,
                with_values(cases["1xh"], 3, "float32", 9, kinds=("values",)), with_values(cases["corner_tr"], 3, "float32", 10)]
    held_to_the_model(layout, [ODD, C440], per_view, "float32", "views", size=(W, H), views=views, dtype="float32", mirror=[False, True, True, False, True])


def test_nothing_to_erase_is_the_call_without_the_argument():
    dec = decoder("rowmajor")
    files = [raw(n) for n in KINDS]
    kw = dict(size=(24, 16), mode="RGB")
    base = storage(dec.decode_device(files, **kw))
    for none in (None, [None] * 4, [None, [], (), None]):
        assert same_bits(storage(dec.decode_device(files, erase=none, **kw)), base), none


# ---- at the C ABI ----------------------------------------------------------------------------------------------------------
def _plan(dec, names, layout_id, **kw):
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    prep = prepare_batch([raw(n) for n in names], layout_id, 0)
    return B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(names)}, **kw)


@pytest.mark.parametrize("dtype", ("uint8", "float16", "float32"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_only_the_boxes_are_written(layout, dtype):
    """execute into a pointer inside a larger sentinel-filled buffer — element-aligned, not 16-byte aligned —, a box in the
    bottom-right corner of the last slot: the sentinels stay"""
    import torch
    from pyjpegdecoder_amd import _binding as B
    W, H, names = 23, 17, [ODD, ODD, ODD]
    dec = decoder(layout)
    plan = _plan(dec, names, LAYOUTS.index(layout), size=(W, H), output=(dtype, None, None, None))
    try:
        es = B.DTYPE_BYTES[dtype]
        nbytes, front = int(plan.info.rgb_bytes), 64 + 3 * es
        assert nbytes == 3 * W * H * 3 * es
        buf = torch.full((front + nbytes + 61,), 0xA5, dtype=torch.uint8, device="cuda:0")
        plan.execute(0, buf.data_ptr() + front)
        plan.sync()
        base = buf.cpu().numpy().copy()
        v = 200 if dtype == "uint8" else -1.75
        rects = [(2, W - 3, H - 2, 3, 2, v), (0, 0, 0, W, 1, v), (2, 0, 0, 1, 1, v)]
        plan.set_erase(rects)
        plan.execute(0, buf.data_ptr() + front)
        plan.sync()
        got = buf.cpu().numpy()
        assert (got[:front] == 0xA5).all() and (got[front + nbytes:] == 0xA5).all(), "a sentinel was written"
        st = np.dtype(dtype)
        shape = (3,) + ((W, H) if layout in ("xmajor", "planar") else (H, W))
        shape = shape[:1] + ((3,) + shape[1:] if layout.startswith("planar") else shape[1:] + (3,))
        outs = base[front:front + nbytes].view(st).reshape(shape)
        want = model_outputs(outs, [[(0, 0, W, 1, v)], None, [(W - 3, H - 2, 3, 2, v), (0, 0, 1, 1, v)]], layout, dtype)
        assert same_bits(got[front:front + nbytes].view(st).reshape(shape), want)
    finally:
        plan.close()


@pytest.mark.parametrize("layout", ("xmajor", "planar_rowmajor"))
def test_set_changed_and_cleared_on_the_graph_path(layout):
    """the same plan on one stream into one buffer — the third execute of a row replays a captured graph —, with boxes set, then
    changed (values too), then taken off with n = 0: right every time"""
    import torch
    W, H, names = 24, 16, [C411, C411]
    dec = decoder(layout)
    plan = _plan(dec, names, LAYOUTS.index(layout), size=(W, H), output=("float16", None, None, None))
    try:
        buf = torch.zeros(int(plan.info.rgb_bytes) // 2, dtype=torch.float16, device="cuda:0")
        shape = (2,) + (((3, W, H) if layout == "planar" else (3, H, W)) if layout.startswith("planar") else ((W, H, 3) if layout == "xmajor" else (H, W, 3)))

        def three_times(boxes):
            outs = []
            for _ in range(3):
                buf.zero_()
                torch.cuda.synchronize()
                plan.execute(0, buf.data_ptr())
                plan.sync()
                outs.append(buf.cpu().numpy().reshape(shape).copy())
            return outs
        base = three_times(None)
        assert same_bits(base[0], base[1]) and same_bits(base[0], base[2])
        vals = torch.arange(3 * 4 * 5, dtype=torch.float16, device="cuda:0")
        first = [(0, 1, 1, 5, 4, ("values", 0)), (1, 20, 12, 4, 4, 0.5)]
        plan.set_erase(first, vals.data_ptr(), keep=vals)
        want = model_outputs(base[0], [[(1, 1, 5, 4, vals.cpu().numpy().reshape(3, 4, 5))], [(20, 12, 4, 4, 0.5)]], layout, "float16")
        for k, out in enumerate(three_times(first)):
            assert same_bits(out, want), ("set", k)
        vals2 = torch.arange(100, 100 + 3 * 2 * 3, dtype=torch.float16, device="cuda:0")
        plan.set_erase([(1, 0, 0, 3, 2, ("values", 0)), (1, 2, 1, 6, 6, [1.0, 2.0, 3.0])], vals2.data_ptr(), keep=vals2)
        want = model_outputs(base[0], [None, [(0, 0, 3, 2, vals2.cpu().numpy().reshape(3, 2, 3)), (2, 1, 6, 6, [1.0, 2.0, 3.0])]], layout, "float16")
        for k, out in enumerate(three_times(None)):
            assert same_bits(out, want), ("changed", k)
        plan.set_erase([])
        for k, out in enumerate(three_times(None)):
            assert same_bits(out, base[0]), ("cleared", k)
        ms, nbytes = None, None
        plan.set_erase(first, vals.data_ptr(), keep=vals)
        ms, nbytes = plan.time_erase(3)
        assert ms > 0 and nbytes == (5 * 4 + 4 * 4) * 3 * 2
    finally:
        plan.close()


def test_what_set_erase_refuses():
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.errors import BackendError
    dec = decoder("rowmajor")
    sized = _plan(dec, [ODD, ODD], B.MJ_LAYOUT_ROWMAJOR, size=(10, 8))
    plain = _plan(dec, [ODD], B.MJ_LAYOUT_ROWMAJOR)
    floats = _plan(dec, [ODD], B.MJ_LAYOUT_ROWMAJOR, size=(10, 8), output=("float32", None, None, None))
    try:
        with pytest.raises(BackendError, match="mj_plan_set_erase: erase needs a size"):
            plain.set_erase([(0, 0, 0, 1, 1, 0)])
        for rect, msg in [((2, 0, 0, 1, 1, 0), "box 0 .output 2, .*no such output"), ((-1, 0, 0, 1, 1, 0), "no such output"),
                          ((0, 0, 0, 0, 1, 0), "a width or height below 1"), ((0, 8, 0, 3, 1, 0), "not inside the canvas"),
                          ((0, 0, 7, 1, 2, 0), "not inside the canvas"), ((1, -1, 0, 2, 2, 0), "not inside the canvas"),
                          ((0, 0, 0, 1, 1, 2.5), "not an integer 0..255"), ((0, 0, 0, 1, 1, 300), "not an integer 0..255"),
                          ((0, 0, 0, 1, 1, ("values", 0)), "a box of values without values"), (B.EraseRectC(0, 0, 0, 1, 1, 5), "a kind that is neither")]:
            with pytest.raises(BackendError, match=msg):
                sized.set_erase([rect])
        with pytest.raises(BackendError, match="box 1 .*a negative offset"):
            sized.set_erase([(0, 0, 0, 1, 1, 1), (0, 0, 0, 1, 1, ("values", -4))], 4096)
        for bad in (float("nan"), float("-inf")):
            with pytest.raises(BackendError, match="a value that is not finite"):
                floats.set_erase([(0, 0, 0, 1, 1, bad)])
        lib = dec.ctx.lib
        assert lib.mj_plan_set_erase(sized.handle, -1, None, None) == B.MJ_ERR_INVALID and b"n = -1" in lib.mj_last_error(dec.ctx.handle)
        assert lib.mj_plan_set_erase(sized.handle, 1, None, None) == B.MJ_ERR_INVALID and b"rects is NULL" in lib.mj_last_error(dec.ctx.handle)
        with pytest.raises(BackendError, match="no erase set"):
            sized.time_erase(1)
        # a refused call leaves the plan as it was: it still executes, unerased
        sized.execute()
        sized.sync()
        a = sized.read()["rgb"]
        sized.set_erase([(1, 0, 0, 10, 8, 7)])
        sized.execute()
        sized.sync()
        b = sized.read()["rgb"]
        assert np.array_equal(a[:240], b[:240]) and (b[240:] == 7).all()
    finally:
        for p in (sized, plain, floats):
            p.close()
