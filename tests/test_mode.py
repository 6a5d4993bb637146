"""Output colour mode on the MI355X (mj_plan_request.mode with and without a size, BatchDecoder's ``mode=``): every output
is tools/mode_model.py, then orient_model.py, then resize_model.py, then normalize_model.py applied to the ORACLE's pixels —
never to the library's own output.  tests/test_mode_host.py pins mode_model to Pillow's convert() on the CPU."""
import numpy as np
import pytest

from conftest import GOLDEN, oracle_rgb_all
from test_orientation import ODD_SIZES, tagged
from test_resize import as_layout
from test_roi import LAYOUTS, mcu_size, window_kinds

pytestmark = pytest.mark.gpu

MODES = ("RGB", "L")
GREY = ("64x64_grey_pil", "50x70_grey_dri4", "prog_64x64_grey_pil")
# one file of every class of colour file — and the noise file, for pixel variety.  (Chosen so that every class meets the conditions
# of test_the_conditions_...: smooth files' L mostly IS their Y plane, so the 4:1:1 and the progressive file are the noisier ones.)
COLOUR = {"64x64_420_pil": "4:2:0", "64x48_422_pil": "4:2:2", "48x80_440": "4:4:0", "100x36_411_dri3": "4:1:1", "40x40_444_dri5": "4:4:4",
          "ni_37x29_444_dri4": "non-interleaved", "prog_96x80_420_noise_pil": "progressive", "96x64_420_q100_noise": "4:2:0"}
# the odd sizes (tools.synth): (subsampling, restart interval) — two colour, two greyscale
ODD_KINDS = (("420", 0), ("grey", 0), ("444", 3), ("grey", 2))
CLASS_OF = dict(COLOUR, synth_70x50_420="4:2:0", synth_37x29_444="4:4:4")

_cache = {}


def want(f, mode, layout, o=1, win=None, size=None, filter="bilinear", out=None, mirror=False, resize_first=False):
    """The models' result for fixture ``f`` = (name, raw, oracle pixels (W, H[, 3]), MCU size), in the decoder's layout.  ``win``: of the
    oriented image.  ``out``: (dtype, mean, std).  ``resize_first``: the WRONG order (resize, then convert), for the sharpness
    conditions.  The part up to the resize is computed once per argument set and left unchanged: the layouts share it."""
    from tools import mode_model, normalize_model, orient_model, resize_model
    k = (f[0], mode, o, win, size, filter, resize_first)
    if k not in _cache:
        a = np.ascontiguousarray(f[2].swapaxes(0, 1))
        if not resize_first:
            a = mode_model.convert(a, mode)
        a = orient_model.orient(a, o)
        if win is not None:
            x, y, w, h = win
            a = np.ascontiguousarray(a[y:y + h, x:x + w])
        if size is not None:
            a = resize_model.resize(a, size, filter)
        if resize_first:
            a = mode_model.convert(a, mode)
        a = np.ascontiguousarray(a)
        a.setflags(write=False)
        _cache[k] = a
    a = _cache[k]
    if mirror:
        a = a[:, ::-1]
    if out is not None:
        a = normalize_model.normalize(np.ascontiguousarray(a), *out)
    return as_layout(a, layout)


@pytest.fixture(scope="module")
def fixtures():
    """(name, raw, oracle pixels, MCU size), greyscale and colour interleaved: g, c, c, g, c, c, ..."""
    from tools import synth
    named = [(n, (GOLDEN / "files" / f"{n}.jpg").read_bytes()) for n in GREY + tuple(COLOUR)]
    for k, ((w, h), (sub, ri)) in enumerate(zip(ODD_SIZES, ODD_KINDS)):
        named.append((f"synth_{w}x{h}_{sub}", synth.synth_jpeg(700 + k, w, h, 85, sub, ri)))
    fulls = oracle_rgb_all([raw for _, raw in named])
    fs = [(n, raw, full, mcu_size(raw)) for (n, raw), full in zip(named, fulls)]
    grey, colour = [f for f in fs if f[2].ndim == 2], [f for f in fs if f[2].ndim == 3]
    assert len(grey) == 5 and len(colour) == 10
    mixed = []
    while grey or colour:
        mixed += grey[:1] + colour[:2]
        grey, colour = grey[1:], colour[2:]
    assert [f[2].ndim for f in mixed[:4]] == [2, 3, 3, 2]
    return mixed


def test_the_conditions_that_keep_a_plausible_wrong_implementation_out(fixtures):
    """The expected "L" bytes of the colour fixtures differ from (a) the truncating formula, without the + 32768, (b) the
    oracle's Y plane and (c), at a size, resize-then-convert: in at least one byte per class of colour file (for (a) and (c): per
    file), and in at least 1 % of the bytes overall."""
    from oracle import oracle
    colour = [f for f in fixtures if f[2].ndim == 3]
    assert len(colour) == 10 and {f[2].shape[:2] for f in fixtures} >= set(ODD_SIZES)
    diff = {"truncating": [0, 0], "y_plane": [0, 0], "resize_first": [0, 0]}
    y_by_class = {c: 0 for c in CLASS_OF.values()}
    assert len(y_by_class) == 7
    for f in colour:
        l = want(f, "L", "rowmajor")
        rgb = f[2].swapaxes(0, 1).astype(np.uint32)
        trunc = ((19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2]) >> 16).astype(np.uint8)
        y = np.clip(oracle.decode(f[1])["planes"][..., 0].swapaxes(0, 1), 0, 255).astype(np.uint8)
        per = {"truncating": [(l != trunc).sum(), l.size], "y_plane": [(l != y).sum(), l.size], "resize_first": [0, 0]}
        for size in SIZES:
            for flt in FILTERS:
                a, b = want(f, "L", "rowmajor", size=size, filter=flt), want(f, "L", "rowmajor", size=size, filter=flt, resize_first=True)
                per["resize_first"][0] += (a != b).sum()
                per["resize_first"][1] += a.size
        y_by_class[CLASS_OF[f[0]]] += per["y_plane"][0]
        for what, (d, n) in per.items():
            assert d >= 1 or what == "y_plane", (f[0], what)
            diff[what][0] += d
            diff[what][1] += n
    assert all(d >= 1 for d in y_by_class.values()), y_by_class
    for what, (d, n) in diff.items():
        assert d >= 0.01 * n, (what, d, n)
    # and "RGB" of a greyscale file is three equal components, which the three tables of test 3 then tell apart
    g = want(fixtures[0], "RGB", "rowmajor")
    assert g.shape[-1] == 3 and np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 0], g[..., 2])


def shape_of(dec, f, mode, o=1, win=None):
    w, h = (win[2], win[3]) if win is not None else (f[2].shape[:2][::-1] if o >= 5 else f[2].shape[:2])
    return dec._shape(w, h, 3 if mode == "RGB" else 1)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_own_size_every_fixture_every_orientation_and_a_window(fixtures, mode, layout):
    from pyjpegdecoder_amd import BatchDecoder
    raws = [f[1] for f in fixtures]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode(raws, mode=mode)
        for f, img in zip(fixtures, got):
            assert img.shape == shape_of(dec, f, mode) and np.array_equal(img, want(f, mode, layout)), f[0]
        for o in range(1, 9):
            got = dec.decode(raws, orientation=o, mode=mode)
            for f, img in zip(fixtures, got):
                assert img.shape == shape_of(dec, f, mode, o) and np.array_equal(img, want(f, mode, layout, o)), (f[0], o)
        for o in (1, 6):
            wins = []
            for f in fixtures:
                w, h = f[2].shape[:2][::-1] if o >= 5 else f[2].shape[:2]
                wins.append(window_kinds(w, h, *(f[3][::-1] if o >= 5 else f[3]))["inner"])
            for call in (dec.decode, dec.decode_device):
                got = call(raws, rois=wins, orientation=o, mode=mode)
                for f, win, img in zip(fixtures, wins, got):
                    img = img if isinstance(img, np.ndarray) else img.cpu().numpy()
                    assert img.shape == shape_of(dec, f, mode, o, win) and np.array_equal(img, want(f, mode, layout, o, win)), (f[0], o, win)
    finally:
        dec.close()


@pytest.fixture(scope="module")
def wide():
    """a greyscale and a colour file wide enough for several tiles along the width: (name, raw, oracle pixels, MCU size)"""
    from tools import synth
    named = [("synth_4400x200_grey", synth.synth_jpeg(720, 4400, 200, 85, "grey", 0)), ("synth_4400x200_420", synth.synth_jpeg(721, 4400, 200, 85, "420", 0))]
    return [(n, raw, full, mcu_size(raw)) for (n, raw), full in zip(named, oracle_rgb_all([raw for _, raw in named]))]


SIZES = ((33, 21), (150, 131))          # one shrinks every fixture, one enlarges every fixture
FILTERS = ("bilinear", "bicubic")       # (bicubic: the signed instances)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_sized_a_mixed_list_is_one_array_correct_slot_by_slot(fixtures, mode, layout):
    from pyjpegdecoder_amd import BatchDecoder
    raws = [f[1] for f in fixtures]
    nc = 3 if mode == "RGB" else 1
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for size in SIZES:
            for flt in FILTERS:
                got = dec.decode(raws, size=size, resample=flt, mode=mode)
                assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (len(raws),) + dec._shape(size[0], size[1], nc)
                for i, f in enumerate(fixtures):
                    assert np.array_equal(got[i], want(f, mode, layout, size=size, filter=flt)), (f[0], size, flt)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("flt", FILTERS)
def test_sized_several_ragged_tiles_slots_sentinels_and_a_poisoned_source(fixtures, wide, flt, mode, layout):
    """4400 x 200 sources (and 64- and 96-wide ones beside them) to (1501, 37): every converting plan is cut into more than one
    tile along both axes, the last of them ragged — a row-major plan gives up columns only while a tile's source row segment is
    2 KB long, an x-major one when its columns of T outgrow LDS; the plans of the two kinds fill their slots (g, c, c, g) of one
    buffer whose other bytes stay what they were, whatever the intermediate buffer held before."""
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    by_name = {f[0]: f for f in fixtures}
    groups = {1: [wide[0], by_name["64x64_grey_pil"]], 3: [by_name["96x64_420_q100_noise"], wide[1]]}
    slots = {1: [0, 3], 3: [1, 2]}
    size, n_slots = (1501, 37), 5
    nc = 3 if mode == "RGB" else 1
    per = size[0] * size[1] * nc
    dec = BatchDecoder(device=0, layout=layout)
    try:
        buf = torch.full((n_slots * per + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for native, group in groups.items():
            prep = prepare_batch([f[1] for f in group], dec.layout, 0)
            kw = {"mode": mode} if native != nc else {}
            plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": len(group)}, size=size, slots=(slots[native], n_slots),
                          filter=None if flt == "bilinear" else flt, **kw)
            try:
                assert plan.info.rgb_bytes == n_slots * per
                shape = plan.resize_shape()
                if kw:
                    assert shape["tiles_x"] > 1 and shape["tiles_y"] > 1 and size[0] % shape["tile_cols"] and size[1] % shape["tile_rows"], shape
                    assert plan.image_offsets(1)[1] == slots[native][1] * per
                assert shape["signed"] == (flt == "bicubic") and 0 < shape["lds_bytes"] <= 64 * 1024
                plan.fill_source(0xC3)
                plan.execute(0, buf.data_ptr())
                plan.sync()
                assert not plan.read(rgb=False)["status"].any()
            finally:
                plan.close()
        host = buf.cpu().numpy()
        assert (host[n_slots * per:] == 0xA5).all(), "bytes written behind the output"
        assert (host[4 * per:5 * per] == 0xA5).all(), "a slot of no plan was written"
        for native, group in groups.items():
            for f, s in zip(group, slots[native]):
                w = want(f, mode, layout, size=size, filter=flt)
                assert np.array_equal(host[s * per:(s + 1) * per].reshape(w.shape), w), (f[0], s)
    finally:
        dec.close()


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.mark.parametrize("layout", ["planar_rowmajor", "xmajor"])
def test_model_ready_float16_three_tables_and_mixed_mirror_flags(fixtures, layout):
    from routes_common import bits_of
    from pyjpegdecoder_amd import BatchDecoder
    raws = [f[1] for f in fixtures]
    mirror = [bool((i // 2) % 2) for i in range(len(raws))]
    size = (40, 28)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for call in (dec.decode, dec.decode_device):
            bits = bits_of(call(raws, size=size, dtype="float16", normalize=(MEAN, STD), mirror=mirror, mode="RGB"))
            assert bits.shape == (len(raws),) + dec._shape(size[0], size[1], 3)
            for i, f in enumerate(fixtures):
                assert np.array_equal(bits[i], want(f, "RGB", layout, size=size, out=("float16", MEAN, STD), mirror=mirror[i])), (f[0], mirror[i])
            # a greyscale file's three channels: one byte through three different tables
            c_axis = 0 if layout.startswith("planar") else -1
            ch = np.moveaxis(bits[0], c_axis, 0)
            assert fixtures[0][2].ndim == 2 and not np.array_equal(ch[0], ch[1]) and not np.array_equal(ch[1], ch[2])
            bits = bits_of(call(raws, size=size, dtype="float16", normalize=(0.45, 0.225), mirror=mirror, mode="L"))
            assert bits.shape == (len(raws),) + dec._shape(size[0], size[1], 1)
            for i, f in enumerate(fixtures):
                assert np.array_equal(bits[i], want(f, "L", layout, size=size, out=("float16", 0.45, 0.225), mirror=mirror[i])), (f[0], mirror[i])
        with pytest.raises(ValueError, match="normalize: mean has 3 entries for files of 1 component"):
            dec.decode_device(raws, size=size, dtype="float16", normalize=(MEAN, STD), mode="L")
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_oriented_and_sized(fixtures, mode, layout):
    """Orientations 2, 3, 6 and 8 on the mixed list (5..8 read their source the other layout's way), both filters."""
    from pyjpegdecoder_amd import BatchDecoder
    raws = [f[1] for f in fixtures]
    size = (33, 21)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for shift in range(2):
            turns = [(2, 3, 6, 8)[(i + 2 * shift + i // 3) % 4] for i in range(len(raws))]
            flt = FILTERS[shift]
            got = dec.decode_device(raws, size=size, orientation=turns, resample=flt, mode=mode).cpu().numpy()
            for i, f in enumerate(fixtures):
                assert np.array_equal(got[i], want(f, mode, layout, turns[i], size=size, filter=flt)), (f[0], turns[i], flt)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["rowmajor", "planar"])
@pytest.mark.parametrize("mode", MODES)
def test_routes_tensor_iterator_and_parts(fixtures, mode, layout):
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    raws = [f[1] for f in fixtures]
    size, nc = (33, 21), 3 if mode == "RGB" else 1
    for min_files in (64, 1):                    # the host-parsed route, or the native front end + GPU marker scan
        dec = BatchDecoder(device=0, layout=layout, gpu_segment_min_files=min_files)
        shape = dec._shape(size[0], size[1], nc)
        try:
            def check(host, fs, what):
                for i, f in enumerate(fs):
                    assert np.array_equal(host[i], want(f, mode, layout, size=size)), (what, f[0])
            got = dec.decode_device(raws, size=size, mode=mode)
            assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and tuple(got.shape) == (len(raws),) + shape
            check(got.cpu().numpy(), fixtures, "decode_device")
            check(dec.decode_device(raws, size=size, mode=mode, parts=2).cpu().numpy(), fixtures, "parts")
            cut = (0, 4, 9, len(raws))
            per_batch = list(dec.decode_device_iter([raws[a:b] for a, b in zip(cut, cut[1:])], depth=2, size=size, mode=mode))
            assert [tuple(t.shape) for t in per_batch] == [(b - a,) + shape for a, b in zip(cut, cut[1:])]
            check(torch.cat(per_batch).cpu().numpy(), fixtures, "iter")
            # own sizes: lists of tensors
            own = dec.decode_device(raws, mode=mode, parts=2)
            for f, t in zip(fixtures, own):
                assert np.array_equal(t.cpu().numpy(), want(f, mode, layout)), ("own parts", f[0])
            own = [t for part in dec.decode_device_iter([raws[:5], raws[5:]], depth=2, mode=mode) for t in part]
            for f, t in zip(fixtures, own):
                assert np.array_equal(t.cpu().numpy(), want(f, mode, layout)), ("own iter", f[0])
        finally:
            dec.close()


def test_the_loader_call_one_nchw_tensor(fixtures):
    """decode_device(mixed files, size=(224, 224), mode="RGB", dtype, normalize, mirror, orientation="exif", resample="bicubic")
    on a planar_rowmajor decoder: the one NCHW tensor, bit for bit the models' result."""
    import torch
    from routes_common import bits_of
    from pyjpegdecoder_amd import BatchDecoder
    turns = [(1, 6, 3, 8, 2, 1, 5)[i % 7] for i in range(len(fixtures))]
    raws = [tagged(f[1], o) if o != 1 else f[1] for f, o in zip(fixtures, turns)]
    mirror = [i % 3 == 1 for i in range(len(raws))]
    size, layout = (224, 224), "planar_rowmajor"
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode_device(raws, size=size, mode="RGB", dtype=torch.float16, normalize=(MEAN, STD), mirror=mirror, orientation="exif",
                                resample="bicubic")
        assert got.dtype == torch.float16 and tuple(got.shape) == (len(raws), 3, 224, 224)
        bits = bits_of(got)
        for i, f in enumerate(fixtures):
            w = want(f, "RGB", layout, turns[i], size=size, filter="bicubic", out=("float16", MEAN, STD), mirror=mirror[i])
            assert np.array_equal(bits[i], w), (f[0], turns[i], mirror[i])
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["xmajor", "planar_rowmajor"])
def test_no_conversion_needed_is_a_call_without_the_argument(fixtures, layout):
    """mode="RGB" on colour files and mode="L" on greyscale files: identical bytes, from plans cut as those of a call without mode
    (the same entry points made them: MJ_MODE_NATIVE and the batch's own count return the plan of the function without the argument)."""
    import ctypes
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    size = (33, 21)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for mode, nd in (("RGB", 3), ("L", 2)):
            group = [f for f in fixtures if f[2].ndim == nd]
            raws = [f[1] for f in group]
            for kw in ({}, {"size": size}, {"size": size, "resample": "bicubic"}, {"orientation": 6}):
                plain, moded = dec.decode(raws, **kw), dec.decode(raws, mode=mode, **kw)
                assert len(plain) == len(moded) and all(np.array_equal(a, b) for a, b in zip(plain, moded)), (mode, kw)
            a = dec.decode_device(raws, size=size).cpu().numpy()
            assert np.array_equal(a, dec.decode_device(raws, size=size, mode=mode).cpu().numpy())
            assert np.array_equal(a[0], want(group[0], None, layout, size=size))
            prep = prepare_batch(raws[:1], dec.layout, 0)
            shapes, infos = [], []
            for m in (None, B.MJ_MODE_NATIVE, mode):
                plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 1}, size=size, mode=m)
                try:
                    shapes.append(plan.resize_shape())
                    infos.append(int(plan.info.rgb_bytes))
                finally:
                    plan.close()
            assert shapes[0] == shapes[1] == shapes[2] and infos[0] == infos[1] == infos[2]
            # the C ABI's own refusal of a mode that is none of MJ_MODE_*
            h, bc, lib = ctypes.c_void_p(), prep.to_c(), dec.ctx.lib
            from routes_common import create_with
            assert create_with(lib, dec.ctx.handle, bc, h, out_width=8, out_height=8, mode=2) == B.MJ_ERR_INVALID
            assert create_with(lib, dec.ctx.handle, bc, h, mode=2) == B.MJ_ERR_INVALID
            assert not h.value and b"mode 2 is none of MJ_MODE_" in lib.mj_last_error(dec.ctx.handle)
    finally:
        dec.close()
