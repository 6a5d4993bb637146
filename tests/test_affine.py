"""The affine transform on the MI355X (mj_plan_request.affine, BatchDecoder.decode / decode_device / decode_device_iter(size=...,
affine=...)): rotate, shear and translate in front of the window and the resize.  The expected bytes of every case are
tools/affine_model.py — which tests/test_affine_host.py holds to Pillow's Image.transform, bit for bit — applied to the library's
own plain decode of the file, then the models of the steps behind it (tools/views_model.py: window, resize, place, mirror;
tools/normalize_model.py).  Byte for byte, in every layout."""
import math

import numpy as np
import pytest

from conftest import GOLDEN
from test_resize import as_layout
from test_roi import LAYOUTS

pytestmark = pytest.mark.gpu

FILTERS = ("nearest", "bilinear", "bicubic")
ODD, GREY, C411, C440, C420 = "70x50_420_pil_opt", "64x64_grey_pil", "100x36_411_dri3", "48x80_440", "64x64_420_pil"
DIMS = {ODD: (70, 50), GREY: (64, 64), C411: (100, 36), C440: (48, 80), C420: (64, 64)}
FILL = (7, 99, 200)
_PLAIN = {}


def raw(name):
    return (GOLDEN / "files" / f"{name}.jpg").read_bytes()


def plain(name):
    """the library's own plain decode of the file, row-major, in the file's components: computed once, never changed"""
    if name not in _PLAIN:
        from pyjpegdecoder_amd import BatchDecoder
        dec = BatchDecoder(device=0, layout="rowmajor")
        try:
            (img,) = dec.decode([raw(name)])
        finally:
            dec.close()
        img = img[:, :, 0] if img.ndim == 3 and img.shape[2] == 1 else img
        img.setflags(write=False)
        _PLAIN[name] = img
    return _PLAIN[name]


def rotate_shear(size, degrees=30.0, shear=0.2, shift=(0.0, 0.0)):
    """output -> input: a rotation by `degrees` about the centre with a shear along x, then a shift"""
    w, h = size
    t = math.radians(degrees)
    a0, a1, a3, a4 = math.cos(t), math.sin(t) + shear, -math.sin(t), math.cos(t)
    cx, cy = w / 2.0, h / 2.0
    return (a0, a1, cx - a0 * cx - a1 * cy + shift[0], a3, a4, cy - a3 * cx - a4 * cy + shift[1])


def want(name, layout, a, size, **kw):
    from tools import affine_model
    return as_layout(affine_model.expected(plain(name), a, kw.pop("window", None), size, **kw), layout)


def host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_identity_is_the_call_without_the_argument(layout):
    from pyjpegdecoder_amd import BatchDecoder
    files = [raw(ODD), raw(C411), raw(C440)]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        base = host(dec.decode_device(files, size=(40, 28)))
        for resample in FILTERS:
            got = host(dec.decode_device(files, size=(40, 28), affine=(1, 0, 0, 0, 1, 0), affine_resample=resample, affine_fill=FILL))
            assert got.shape == base.shape and np.array_equal(got, base), resample
        # an output whose matrix is None is the output of the call without the argument; the other one is not
        got = host(dec.decode_device(files, size=(40, 28), affine=[None, rotate_shear(DIMS[C411]), None], affine_resample="bilinear"))
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2]) and not np.array_equal(got[1], base[1])
    finally:
        dec.close()


@pytest.mark.parametrize("resample", FILTERS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rotation_with_shear_of_four_kinds_of_file(layout, resample):
    from pyjpegdecoder_amd import BatchDecoder
    names = [ODD, GREY, C411, C440, C420]
    mats = [rotate_shear(DIMS[n], 30.0 + 2 * k, 0.2 - 0.1 * k, (k, -k)) for k, n in enumerate(names)]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for size in ((24, 16), (120, 96)):          # smaller and larger than the images
            kw = dict(size=size, mode="RGB", affine=mats, affine_resample=resample, affine_fill=FILL)
            got = host(dec.decode_device([raw(n) for n in names], **kw))
            for k, n in enumerate(names):
                exp = want(n, layout, mats[k], size, resample=resample, affine_fill=FILL, mode="RGB")
                assert np.array_equal(got[k], exp), (n, size)
            if layout == "rowmajor" and resample == "bicubic":
                assert np.array_equal(dec.decode([raw(n) for n in names], **kw), got)
                kw.pop("affine")
                (one, two) = list(dec.decode_device_iter([[raw(n) for n in names], [raw(ODD)]], affine=[mats, mats[0]], **kw))
                assert np.array_equal(host(one), got) and np.array_equal(host(two)[0], got[0])
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("xmajor", "planar_rowmajor"))
def test_fill_pixels_go_through_the_output_table(layout):
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from tools import normalize_model
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    names = [ODD, C440]
    # most of the image leaves its frame
    mats = [rotate_shear(DIMS[n], 12.0, 0.0, (0.7 * DIMS[n][0], -0.55 * DIMS[n][1])) for n in names]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode_device([raw(n) for n in names], size=(32, 24), affine=mats, affine_resample="bilinear", affine_fill=FILL, dtype=torch.float16,
                                normalize=(mean, std))
        assert got.dtype == torch.float16
        bits = got.cpu().view(torch.int16).numpy().view(np.uint16)
        for k, n in enumerate(names):
            from tools import affine_model
            rm = affine_model.expected(plain(n), mats[k], None, (32, 24), resample="bilinear", affine_fill=FILL)
            assert (rm.reshape(-1, 3) == np.array(FILL, np.uint8)).all(axis=1).mean() > 0.5          # (mostly fill)
            assert np.array_equal(bits[k], as_layout(normalize_model.normalize(rm, "float16", mean, std), layout)), n
    finally:
        dec.close()


@pytest.mark.parametrize("resample", ("nearest", "bicubic"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_convert_then_orient_then_transform(layout, resample):
    from pyjpegdecoder_amd import BatchDecoder
    names, orient = [ODD, C411, C440], [3, 6, 5]
    odims = [DIMS[ODD], DIMS[C411][::-1], DIMS[C440][::-1]]
    mats = [rotate_shear(d, -25.0, 0.15, (1.5, -2.0)) for d in odims]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        kw = dict(size=(40, 28), orientation=orient, affine=mats, affine_resample=resample, affine_fill=FILL)
        got = host(dec.decode_device([raw(n) for n in names], **kw))
        for k, n in enumerate(names):
            assert np.array_equal(got[k], want(n, layout, mats[k], (40, 28), resample=resample, affine_fill=FILL, orientation=orient[k])), (n, orient[k])
        # mode="L" on colour files (every tap converted before it is interpolated), mode="RGB" on the grey one
        kw.update(mode="L", affine_fill=55)
        got = host(dec.decode_device([raw(n) for n in names], **kw))
        for k, n in enumerate(names):
            assert np.array_equal(got[k], want(n, layout, mats[k], (40, 28), resample=resample, affine_fill=55, orientation=orient[k], mode="L")), (n, "L")
        m = rotate_shear(DIMS[GREY], 40.0, -0.1)
        got = host(dec.decode_device([raw(GREY)], size=(40, 28), mode="RGB", orientation=8, affine=m, affine_resample=resample, affine_fill=FILL))
        assert np.array_equal(got[0], want(GREY, layout, m, (40, 28), resample=resample, affine_fill=FILL, orientation=8, mode="RGB"))
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_windows_are_windows_of_the_transformed_image(layout):
    from pyjpegdecoder_amd import BatchDecoder
    names = [ODD, C420, C411]
    # windows at the corners: their bicubic taps and the out-of-frame test meet the image's edge
    rois = [(0, 0, 31, 22), (64 - 29, 64 - 33, 29, 33), (100 - 17, 0, 17, 36)]
    mats = [rotate_shear(DIMS[n], 8.0, 0.05, (-3.0, 2.0)) for n in names]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for resample in ("bicubic", "nearest"):
            kw = dict(size=(24, 16), rois=rois, affine=mats, affine_resample=resample, affine_fill=FILL, resample="bicubic")
            got = host(dec.decode_device([raw(n) for n in names], **kw))
            for k, n in enumerate(names):
                assert np.array_equal(got[k], want(n, layout, mats[k], (24, 16), window=rois[k], resample=resample, affine_fill=FILL, filter="bicubic")), (n, resample)
        # resize_to= (the shorter side to 20, centre crop on a 16 x 16 canvas) and mirror=
        from pyjpegdecoder_amd.batch import centred, resized_size
        kw = dict(size=(16, 16), resize_to=20, mirror=[True, False, True], affine=mats, affine_resample="bilinear", affine_fill=FILL)
        got = host(dec.decode_device([raw(n) for n in names], **kw))
        for k, n in enumerate(names):
            target = resized_size(20, DIMS[n][0], DIMS[n][1], (16, 16))
            exp = want(n, layout, mats[k], (16, 16), resample="bilinear", affine_fill=FILL, resized=target, xy=centred(20, target, (16, 16)), mirror=kw["mirror"][k])
            assert np.array_equal(got[k], exp), (n, target)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_view_has_its_own_matrix(layout):
    from pyjpegdecoder_amd import BatchDecoder
    m1, m2 = rotate_shear(DIMS[ODD], 30.0, 0.2), rotate_shear(DIMS[ODD], -50.0, 0.0, (4.0, 1.0))
    w1, w2 = (5, 3, 40, 30), (33, 11, 37, 39)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        kw = dict(size=(24, 16), affine_resample="bilinear", affine_fill=FILL)
        got = host(dec.decode_device([raw(ODD)], views=[(0, w1), (0, w2), 0], affine=[m1, m2, None], **kw))
        for k, (m, w) in enumerate(((m1, w1), (m2, w2))):
            one = host(dec.decode_device([raw(ODD)], rois=[w], affine=m, **kw))
            assert np.array_equal(got[k], one[0]), k
            assert np.array_equal(got[k], want(ODD, layout, m, (24, 16), window=w, resample="bilinear", affine_fill=FILL)), k
        assert np.array_equal(got[2], host(dec.decode_device([raw(ODD)], size=(24, 16)))[0])
    finally:
        dec.close()


def test_refusals_name_what_is_wrong():
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0)
    try:
        with pytest.raises(ValueError, match="affine needs size"):
            dec.decode_device([raw(ODD)], affine=(1, 0, 0, 0, 1, 0))
        with pytest.raises(ValueError, match="affine and reducing_gap do not go together yet"):
            dec.decode_device([raw(ODD)], size=(24, 16), affine=(1, 0, 0, 0, 1, 0), reducing_gap=2.0)
        with pytest.raises(ValueError, match=r"affine: output 0 \(file 0\): a corner of the output has a source coordinate"):
            dec.decode_device([raw(ODD)], size=(24, 16), affine=(1, 0, 40000, 0, 1, 0))
        with pytest.raises(ValueError, match="affine has 2 entries for 1 outputs"):
            dec.decode([raw(ODD)], size=(24, 16), affine=[None, (1, 0, 0, 0, 1, 0)])
    finally:
        dec.close()
