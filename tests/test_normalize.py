"""Model-ready output on the MI355X (mj_plan_request.output; decode / decode_device / decode_device_iter with dtype=,
normalize=, mirror=): every element is, bit for bit, tools/normalize_model.py — which tests/test_normalize_host.py pins to
torch's CPU chain — applied to tools/resize_model.py's resize of the oracle's pixels, laid out per layout and flipped along the
width where mirrored.  Comparisons are on the raw bits (uint16 / uint32 views), never a tolerance."""
import numpy as np
import pytest

from conftest import GOLDEN, oracle_rgb_all
from test_resize import SIZES, expect
from test_roi import LAYOUTS, _fixture_files, mcu_size, window_kinds

pytestmark = pytest.mark.gpu

FLOAT_DTYPES = ("float32", "float16", "bfloat16")
# per component and all different: a swapped channel shows
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MEAN2, STD2 = (0.1, 0.5, 0.9), (0.5, 0.25, 2.0)


def bits_of(t) -> np.ndarray:
    """A result (torch tensor on the GPU, or NumPy array) as its bit patterns on the host."""
    import torch
    if isinstance(t, np.ndarray):
        return t if t.dtype == np.uint8 else t.view({2: np.uint16, 4: np.uint32}[t.dtype.itemsize])
    if t.dtype == torch.uint8:
        return t.cpu().numpy()
    if t.element_size() == 2:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def width_axis(layout: str, ndim: int) -> int:
    """Which axis of ONE image of this layout runs along the width."""
    return (0 if layout in ("xmajor", "planar") else 1) + (1 if layout.startswith("planar") and ndim == 3 else 0)


def model_bits(u8: np.ndarray, layout: str, dtype: str, mean=None, std=None, mirror: bool = False) -> np.ndarray:
    """The expectation for one image: `u8` is the resized image as a decoder of this layout returns it (test_resize.expect)."""
    from tools import normalize_model
    if dtype == "uint8":
        out = u8
    else:
        nc = 3 if u8.ndim == 3 else 1
        m = [0.0] * nc if mean is None else list(mean)[:nc]
        s = [1.0] * nc if std is None else list(std)[:nc]
        tabs = [normalize_model.table_bits(dtype, m[c], s[c]) for c in range(nc)]
        if nc == 1:
            out = tabs[0][u8]
        elif layout.startswith("planar"):
            out = np.stack([tabs[c][u8[c]] for c in range(3)], axis=0)
        else:
            out = np.stack([tabs[c][u8[..., c]] for c in range(3)], axis=-1)
    if mirror:
        out = np.flip(out, axis=width_axis(layout, u8.ndim))
    return np.ascontiguousarray(out)


@pytest.fixture(scope="module")
def fixtures():
    from oracle import oracle
    files = _fixture_files()
    out = [(name, raw, oracle.decode(raw)["rgb"], mcu_size(raw)) for name, raw in files]
    return {nc: [f for f in out if (f[2].ndim == 3) == (nc == 3)] for nc in (1, 3)}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_fixture_every_size_every_float_dtype_whole_and_windows(fixtures, layout):
    """Every fixture file x the sizes of test_resize.SIZES x whole images and every window kind x float32 / float16 (decode, the
    NumPy route) and bfloat16 (decode_device), normalised with a mean and std per component."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    done = 0
    try:
        for nc, group in fixtures.items():
            assert group
            raws = [f[1] for f in group]
            kinds = [window_kinds(f[2].shape[0], f[2].shape[1], *f[3]) for f in group]
            norm = (MEAN, STD) if nc == 3 else (MEAN[:1], STD[:1])
            for dtype in FLOAT_DTYPES:
                for sname, size in SIZES.items():
                    for kind in [None] + list(kinds[0]):
                        wins = None if kind is None else [k[kind] for k in kinds]
                        if dtype == "bfloat16":
                            got = dec.decode_device(raws, rois=wins, size=size, dtype=torch.bfloat16, normalize=norm)
                            assert isinstance(got, torch.Tensor) and got.dtype == torch.bfloat16 and got.is_cuda
                        else:
                            got = dec.decode(raws, rois=wins, size=size, dtype=dtype, normalize=norm)
                            assert isinstance(got, np.ndarray) and got.dtype == np.dtype(dtype)
                        assert tuple(got.shape) == (len(group),) + dec._shape(size[0], size[1], nc), (sname, kind)
                        host = bits_of(got)
                        for i, (name, _, full, _) in enumerate(group):
                            win = (0, 0, full.shape[0], full.shape[1]) if wins is None else wins[i]
                            want = model_bits(expect(name, full, win, size, layout), layout, dtype, *norm)
                            assert host[i].dtype == want.dtype and np.array_equal(host[i], want), (name, dtype, sname, kind, win)
                            done += 1
        assert done == sum(len(g) for g in fixtures.values()) * 3 * len(SIZES) * 11
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mirror_flags_mixed_in_one_call(fixtures, layout):
    """Per-file flags that mix True and False in one call — uint8 and float16, odd and even output widths and width 1 — and
    mirror=True is np.flip of mirror=False of the same call."""
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    done = 0
    try:
        for nc, group in fixtures.items():
            raws = [f[1] for f in group]
            flags = [(i % 3) != 1 for i in range(len(group))]
            assert any(flags) and not all(flags)
            norm = (MEAN2, STD2) if nc == 3 else (MEAN2[:1], STD2[:1])
            for dtype in ("uint8", "float16"):
                kw = dict(dtype=dtype) if dtype == "uint8" else dict(dtype=dtype, normalize=norm)
                for size in ((13, 9), (12, 10), (1, 7), (301, 5), (224, 224)):
                    got = bits_of(dec.decode(raws, size=size, mirror=flags, **kw))
                    plain = bits_of(dec.decode(raws, size=size, mirror=False, **kw))
                    every = bits_of(dec.decode_device(raws, size=size, mirror=True, **kw))
                    assert got.shape == plain.shape == every.shape == (len(group),) + dec._shape(size[0], size[1], nc)
                    ax = 1 + width_axis(layout, got.ndim - 1)
                    assert got.shape[ax] == size[0]
                    assert np.array_equal(every, np.flip(plain, axis=ax)), (dtype, size)
                    for i, (name, _, full, _) in enumerate(group):
                        u8 = expect(name, full, (0, 0, full.shape[0], full.shape[1]), size, layout)
                        want = model_bits(u8, layout, dtype, *(norm if dtype != "uint8" else (None, None)), mirror=flags[i])
                        assert np.array_equal(got[i], want), (name, dtype, size, flags[i])
                        assert np.array_equal(plain[i], model_bits(u8, layout, dtype, *(norm if dtype != "uint8" else (None, None))))
                        done += 1
        assert done == sum(len(g) for g in fixtures.values()) * 2 * 5
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_float_output_without_normalize_is_the_uint8_output_over_255(fixtures, layout):
    """dtype=float32 alone: times 255, in float32, the uint8 output of the same call exactly; float16: after rounding to the
    nearest integer.  The resized bytes are untouched by the conversion."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0, layout=layout)
    done = 0
    try:
        for nc, group in fixtures.items():
            raws = [f[1] for f in group]
            for size in ((13, 9), (301, 257), (64, 64)):
                u8 = dec.decode_device(raws, size=size)
                f32 = dec.decode_device(raws, size=size, dtype="float32")
                f16 = dec.decode_device(raws, size=size, dtype=torch.float16)
                bf16 = dec.decode_device(raws, size=size, dtype="bfloat16")
                assert (u8.dtype, f32.dtype, f16.dtype, bf16.dtype) == (torch.uint8, torch.float32, torch.float16, torch.bfloat16)
                assert f32.shape == u8.shape == f16.shape == bf16.shape
                assert torch.equal(f32 * 255.0, u8.to(torch.float32))
                assert torch.equal(torch.round(f16.to(torch.float32) * 255.0), u8.to(torch.float32))
                # (what the chain users run today gives on the CPU, whose division by 255 is the correctly rounded one, for all three)
                chain = u8.cpu().to(torch.float32).div(255)
                assert torch.equal(f32.cpu(), chain) and torch.equal(f16.cpu(), chain.to(torch.float16))
                assert torch.equal(bf16.cpu(), chain.to(torch.bfloat16))
                done += 1
        assert done == 2 * 3
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
@pytest.mark.parametrize("segment", ["host", "gpu"])
def test_mixed_kinds_into_one_float_tensor_flags_follow_their_files(segment, layout):
    """Different image sizes, sampling layouts, baseline and progressive, with and without restart markers, one call: one float
    tensor in input order, mirror flags mixed — every plan (one per kind) gets the flags of ITS files."""
    import torch
    from oracle import oracle
    from pyjpegdecoder_amd import BatchDecoder
    from tools import synth
    g = np.load(GOLDEN / "odd_layouts.npz")
    odd = sorted(k for k in g.files if k.endswith(".jpg"))[0]
    files = [synth.synth_jpeg(41, 200, 120, 85, "420", 13), synth.synth_jpeg(44, 96, 64, 85, "444", 0),
             synth.synth_jpeg(42, 333, 77, 85, "420", 0), (GOLDEN / "files" / "prog_70x50_420_pil.jpg").read_bytes(),
             g[odd].tobytes(), synth.synth_jpeg(43, 200, 120, 85, "420", 7), (GOLDEN / "files" / "64x48_422_pil.jpg").read_bytes(),
             synth.synth_jpeg(45, 640, 480, 90, "422", 40), synth.synth_jpeg(46, 1920, 1080, 85, "420", 120)]
    fulls = [oracle.decode(r)["rgb"] for r in files]
    wins = [(37, 21, 90, 50), None, (150, 10, 5, 3), (10, 9, 33, 21), None, None, (17, 3, 40, 40), None, (736, 316, 448, 448)]
    flags = [True, False, False, True, True, False, True, False, True]
    size = (224, 224)
    done = 0
    for min_files in (64, 1):                    # a handful of files on the host-parsed route, or the native front end + GPU scan
        dec = BatchDecoder(device=0, layout=layout, segment=segment, gpu_segment_min_files=min_files)
        shape = dec._shape(224, 224, 3)
        try:
            for rois in (None, wins):
                for dtype in ("float16", "float32"):
                    got = dec.decode_device(files, rois=rois, size=size, dtype=dtype, normalize=(MEAN, STD), mirror=flags)
                    assert isinstance(got, torch.Tensor) and got.dtype == getattr(torch, dtype) and got.is_cuda
                    assert tuple(got.shape) == (len(files),) + shape
                    host = bits_of(got)
                    arr = bits_of(dec.decode(files, rois=rois, size=size, dtype=dtype, normalize=(MEAN, STD), mirror=flags))
                    for i, full in enumerate(fulls):
                        win = (rois[i] if rois is not None else None) or (0, 0, full.shape[0], full.shape[1])
                        want = model_bits(expect(("mixed", i), full, win, size, layout), layout, dtype, MEAN, STD, flags[i])
                        assert np.array_equal(host[i], want), (segment, min_files, dtype, i)
                        assert np.array_equal(arr[i], want), (segment, min_files, dtype, i)
                        done += 1
            # several batches, the flags batch by batch (one list, one bool, one list)
            per_batch = list(dec.decode_device_iter([files[:4], files[4:6], files[6:]], size=size, dtype=torch.bfloat16, normalize=(MEAN2, STD2),
                                                    mirror=[flags[:4], True, flags[6:]]))
            assert [tuple(t.shape) for t in per_batch] == [(4,) + shape, (2,) + shape, (3,) + shape]
            assert all(t.dtype == torch.bfloat16 for t in per_batch)
            both = bits_of(torch.cat(per_batch))
            used = flags[:4] + [True, True] + flags[6:]
            for i, full in enumerate(fulls):
                u8 = expect(("mixed", i), full, (0, 0, full.shape[0], full.shape[1]), size, layout)
                assert np.array_equal(both[i], model_bits(u8, layout, "bfloat16", MEAN2, STD2, used[i])), i
                done += 1
            # one bool for every batch, uint8
            outs = list(dec.decode_device_iter([files[:5], files[5:]], size=size, mirror=True))
            both = bits_of(torch.cat(outs))
            assert both.dtype == np.uint8
            for i, full in enumerate(fulls):
                u8 = expect(("mixed", i), full, (0, 0, full.shape[0], full.shape[1]), size, layout)
                assert np.array_equal(both[i], model_bits(u8, layout, "uint8", mirror=True)), i
                done += 1
        finally:
            dec.close()
    assert done == 2 * (2 * 2 * 9 + 9 + 9)


@pytest.mark.parametrize("layout", ["rowmajor", "planar"])
def test_a_call_large_enough_to_go_in_parts(layout):
    """640 files through decode_device's default route go as two parts (plans of 256 files or more): flags and slots of every
    part are those of its files."""
    import torch
    from oracle import oracle
    from pyjpegdecoder_amd import BatchDecoder
    from tools import synth
    distinct, n, size = 16, 640, (40, 24)
    raws = [synth.synth_jpeg(700 + k, 96 + 16 * (k % 3), 64, 85, "420", 6) for k in range(distinct)]
    fulls = [oracle.decode(r)["rgb"] for r in raws]
    pick = [(7 * i + i // distinct) % distinct for i in range(n)]
    files = [raws[d] for d in pick]
    flags = [((i * 2654435761) >> 7) & 1 == 1 for i in range(n)]
    assert 200 < sum(flags) < 440
    dec = BatchDecoder(device=0, layout=layout)
    try:
        assert dec.native_host and dec._gpu_segment_for(files) and min(4, n // 256) == 2
        got = dec.decode_device(files, size=size, dtype="float16", normalize=(MEAN, STD), mirror=flags)
        assert got.dtype == torch.float16 and tuple(got.shape) == (n,) + dec._shape(size[0], size[1], 3)
        host = bits_of(got)
        one = bits_of(dec.decode_device(files, size=size, dtype="float16", normalize=(MEAN, STD), mirror=flags, parts=1))
    finally:
        dec.close()
    assert np.array_equal(host, one)
    want = {}
    for i in range(n):
        key = (pick[i], flags[i])
        if key not in want:
            full = fulls[pick[i]]
            u8 = expect(("parts", pick[i]), full, (0, 0, full.shape[0], full.shape[1]), size, layout)
            want[key] = model_bits(u8, layout, "float16", MEAN, STD, flags[i])
        assert np.array_equal(host[i], want[key]), i
    assert len(want) == 2 * distinct


@pytest.mark.parametrize("layout,dtype", [("planar_rowmajor", "float16"), ("xmajor", "bfloat16")])
def test_at_size_1024_x_1080p_to_224_model_ready(layout, dtype):
    """1 024 x 1080p 4:2:0 (the 256 distinct files of test_resize's at-size test) to 224 x 224, normalised, mixed mirror flags,
    as the NCHW float16 batch and x-major bfloat16: every distinct image — both ways round — against the expectation."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from tools import synth
    W, H, n, distinct = 1920, 1080, 1024, 256
    blob, offs = synth.synth_batch(distinct, 8800, W, H, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(distinct)]
    pick = [(5 * i + i // distinct) % distinct for i in range(n)]
    files = [raws[d] for d in pick]
    flags = [(i // distinct) % 2 == 1 for i in range(n)]          # every distinct file twice plain and twice mirrored
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode_device(files, size=(224, 224), dtype=dtype, normalize=(MEAN, STD), mirror=flags)
        assert got.dtype == getattr(torch, dtype) and tuple(got.shape) == (n,) + dec._shape(224, 224, 3)
        host = bits_of(got)
    finally:
        dec.close()
    fulls = oracle_rgb_all(raws)
    seen = set()
    for i in range(n):
        d = pick[i]
        u8 = expect(("at_size", d), fulls[d], (0, 0, W, H), (224, 224), layout)
        assert np.array_equal(host[i], model_bits(u8, layout, dtype, MEAN, STD, flags[i])), (i, d, flags[i])
        seen.add((d, flags[i]))
    assert len(seen) == 2 * distinct


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_sentinels_and_slots_of_wider_elements(layout, dtype):
    """A pre-filled output, plans that own only some slots: the other slots and the bytes behind the array keep the pattern to the
    byte — the element size enters every offset."""
    import torch
    from oracle import oracle
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth
    files = [synth.synth_jpeg(31 + k, 200, 120, 85, "420", ri) for k, ri in enumerate((13, 7, 0))]
    fulls = [oracle.decode(r)["rgb"] for r in files]
    es = B.DTYPE_BYTES[dtype]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for size in ((24, 40), (131, 9)):
            per = size[0] * size[1] * 3 * es
            n_slots = 5
            buf = torch.full((n_slots * per + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            slot_of = {0: 3, 1: 0, 2: 4}                  # slots 1 and 2 belong to no plan
            flag_of = {0: True, 1: False, 2: True}
            for group in ([0, 1], [2]):                   # (files with and without restart markers are separate plans)
                sub = [files[i] for i in group]
                prep = prepare_batch(sub, dec.layout, 0, [parse_jpeg(f, headers_only=True) for f in sub])
                plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(sub)}, size=size,
                              slots=([slot_of[i] for i in group], n_slots), output=(dtype, MEAN, STD, [flag_of[i] for i in group]))
                try:
                    assert plan.info.rgb_bytes == n_slots * per        # bytes of the chosen type
                    plan.fill_source(0xC3)
                    plan.execute(0, buf.data_ptr())
                    plan.sync()
                    assert not plan.read(rgb=False)["status"].any()
                finally:
                    plan.close()
            host = buf.cpu().numpy()
            assert (host[n_slots * per:] == 0xA5).all(), "bytes written behind the output"
            for s in (1, 2):
                assert (host[s * per:(s + 1) * per] == 0xA5).all(), "a slot of no plan was written"
            for i, s in slot_of.items():
                u8 = expect(("sentinel", i), fulls[i], (0, 0, 200, 120), size, layout)
                want = model_bits(u8, layout, dtype, MEAN, STD, flag_of[i])
                got = host[s * per:(s + 1) * per].view(want.dtype).reshape(want.shape)
                assert np.array_equal(got, want), (i, layout, dtype, size)
    finally:
        dec.close()


def test_arguments_are_checked_through_every_entry_point_and_empty_lists_have_the_dtype():
    import ctypes
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth
    files = [synth.synth_jpeg(51, 200, 120, 85, "420", 13), synth.synth_jpeg(52, 200, 120, 85, "420", 13)]
    grey = (GOLDEN / "files" / "50x70_grey_dri4.jpg").read_bytes()
    dec = BatchDecoder(device=0)
    try:
        calls = (dec.decode, dec.decode_device, lambda f, **kw: next(dec.decode_device_iter([f], **kw)))
        for call in calls:
            for kw in (dict(dtype="float32"), dict(normalize=(MEAN, STD)), dict(mirror=True)):
                with pytest.raises(ValueError, match="size"):
                    call(files, **kw)
            with pytest.raises(ValueError, match="uint8"):
                call(files, size=(8, 8), dtype="uint8", normalize=(MEAN, STD))
            with pytest.raises(ValueError, match="std"):
                call(files, size=(8, 8), normalize=(MEAN, (0.2, 0.0, 0.2)))
            with pytest.raises(ValueError, match="entries"):
                call(files, size=(8, 8), normalize=(MEAN[:2], STD))
            with pytest.raises(ValueError, match="entries"):
                call([grey], size=(8, 8), normalize=(MEAN, STD))
            with pytest.raises(ValueError, match="dtype"):
                call(files, size=(8, 8), dtype="float64")
        for call in (dec.decode, dec.decode_device):
            with pytest.raises(ValueError, match="mirror"):
                call(files, size=(8, 8), mirror=[True])
        with pytest.raises(ValueError, match="mirror"):
            next(dec.decode_device_iter([files], size=(8, 8), mirror=[[True]]))
        with pytest.raises(ValueError, match="decode_device"):
            dec.decode(files, size=(8, 8), dtype=torch.bfloat16)
        # normalize alone means float32; greyscale takes one value (or a scalar)
        assert dec.decode(files, size=(8, 6), normalize=(MEAN, STD)).dtype == np.float32
        assert dec.decode_device([grey], size=(8, 6), normalize=(0.5, [0.25])).dtype == torch.float32
        # no files: an empty batch of the colour shape and the asked type, from every entry point
        assert dec.decode([], size=(8, 6), dtype="float16").dtype == np.float16
        assert dec.decode([], size=(8, 6), dtype="float16", mirror=True).shape == (0, 8, 6, 3)
        t = dec.decode_device([], size=(8, 6), dtype="bfloat16", normalize=(MEAN, STD))
        assert t.dtype == torch.bfloat16 and tuple(t.shape) == (0, 8, 6, 3)
        outs = list(dec.decode_device_iter([[], files], size=(8, 6), dtype="float32", mirror=False))
        assert [tuple(t.shape) for t in outs] == [(0, 8, 6, 3), (2, 8, 6, 3)] and all(t.dtype == torch.float32 for t in outs)
        # the C entry point, with a context: the output description is refused with its message; NULL output is the plain plan
        L = dec.ctx.lib
        prep = prepare_batch(files)
        bc = prep.to_c()
        h = ctypes.c_void_p()
        d = B.OutputDescC()
        d.dtype, d.normalize = B.MJ_DTYPE_F16, 1
        d.mean[:], d.std[:] = (0.0, 0.0, 0.0), (1.0, -1.0, 1.0)
        from routes_common import create_with
        assert create_with(L, dec.ctx.handle, bc, h, out_width=8, out_height=8, output=d) == B.MJ_ERR_INVALID
        assert b"std" in L.mj_last_error(dec.ctx.handle)
        d.dtype = 9
        assert create_with(L, dec.ctx.handle, bc, h, out_width=8, out_height=8, output=d) == B.MJ_ERR_INVALID
        assert b"dtype" in L.mj_last_error(dec.ctx.handle)
        assert create_with(L, dec.ctx.handle, bc, h, out_width=0, out_height=8, output=None) == B.MJ_ERR_INVALID
        assert b"output size" in L.mj_last_error(dec.ctx.handle)
        assert create_with(L, dec.ctx.handle, bc, h, out_width=8, out_height=8, output=None) == B.MJ_OK
        info = B.PlanInfoC()
        L.mj_plan_get_info(h, ctypes.byref(info))
        L.mj_plan_destroy(h)
        assert info.rgb_bytes == 2 * 8 * 8 * 3
    finally:
        dec.close()
