"""The perspective transform on the MI355X (MJ_AFFINE_PERSPECTIVE in mj_plan_request.affine, BatchDecoder.decode / decode_device /
decode_device_iter(size=..., perspective=...)): torchvision's RandomPerspective in front of the window and the resize.  The expected
bytes of every case are tools/perspective_model.py — which tests/test_perspective_host.py holds to Pillow's Image.transform, bit for
bit — applied to the library's own plain decode of the file, then the models of the steps behind it (tools/views_model.py: window,
resize, place, mirror; tools/normalize_model.py; tools/colour_model.py).  Byte for byte, in every layout.

The files are the smallest that reach every tile path of the launch (64 x 16 tiles): 100 x 36 spans two tiles along the fast axis
and three across, with a row tail; 70 x 50 has tails on both axes.  The pole and the huge coordinates are defined arithmetic — fill —,
the same that tools/perspective_host_check.cpp runs on the host under the sanitizers."""
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
IDENT = (1, 0, 0, 0, 1, 0, 0, 0)
_PLAIN = {}


def raw(name):
    return (GOLDEN / "files" / f"{name}.jpg").read_bytes()


def plain(name, folder="files"):
    """the library's own plain decode of the file, row-major, in the file's components: computed once, never changed"""
    if (name, folder) not in _PLAIN:
        from pyjpegdecoder_amd import BatchDecoder
        dec = BatchDecoder(device=0, layout="rowmajor")
        try:
            (img,) = dec.decode([(GOLDEN / folder / f"{name}.jpg").read_bytes()])
        finally:
            dec.close()
        img = img[:, :, 0] if img.ndim == 3 and img.shape[2] == 1 else img
        img.setflags(write=False)
        _PLAIN[(name, folder)] = img
    return _PLAIN[(name, folder)]


def keystone(size, k=0):
    """about 35 % fill; all four image edges fall inside the frame, so the repeated-row and clipped-column taps run (k: another per file)"""
    from pyjpegdecoder_amd import perspective_coeffs
    w, h = size
    ends = [((0.1 + 0.01 * k) * w, 0.15 * h), (0.95 * w, (0.05 + 0.01 * k) * h), (0.85 * w, 0.9 * h), (0.05 * w, (0.8 - 0.01 * k) * h)]
    return perspective_coeffs([(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)], ends)


def pole(size, k=0):
    """the pole line crosses the frame at x = 0.6 w (k: a little further on): denominator -0.65 at the far corners, 74 % fill"""
    return (1, 0, 0, 0, 1, 0, -1 / ((0.6 + 0.01 * k) * size[0]), 0)


def away(size):
    """most of the image leaves its frame: 84 % fill at full size"""
    w, h = size
    return (1, 0, 0.7 * w, 0, 1, -0.55 * h, 0.001, 0.0005)


def want(name, layout, c, size, **kw):
    from tools import perspective_model
    return as_layout(perspective_model.expected(plain(name), c, kw.pop("window", None), size, **kw), layout)


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
            got = host(dec.decode_device(files, size=(40, 28), perspective=IDENT, affine_resample=resample, affine_fill=FILL))
            assert got.shape == base.shape and np.array_equal(got, base), resample
        # an output whose entry is None — here between two transformed ones — is the output of the call without the argument
        got = host(dec.decode_device(files, size=(40, 28), perspective=[keystone(DIMS[ODD]), None, pole(DIMS[C440])], affine_resample="bilinear"))
        assert np.array_equal(got[1], base[1]) and not np.array_equal(got[0], base[0]) and not np.array_equal(got[2], base[2])
        # ... and a call whose entries are all None is that call
        assert np.array_equal(host(dec.decode_device(files, size=(40, 28), perspective=[None, None, None])), base)
    finally:
        dec.close()


@pytest.mark.parametrize("resample", FILTERS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_keystone_and_pole_of_five_kinds_of_file(layout, resample):
    from pyjpegdecoder_amd import BatchDecoder
    names = [ODD, GREY, C411, C440, C420]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for geometry in (keystone, pole):
            coeffs = [geometry(DIMS[n], k) for k, n in enumerate(names)]
            for size in ((24, 16), (120, 96)):          # smaller and larger than the images
                kw = dict(size=size, mode="RGB", perspective=coeffs, affine_resample=resample, affine_fill=FILL)
                got = host(dec.decode_device([raw(n) for n in names], **kw))
                for k, n in enumerate(names):
                    exp = want(n, layout, coeffs[k], size, resample=resample, affine_fill=FILL, mode="RGB")
                    assert np.array_equal(got[k], exp), (geometry.__name__, n, size)
                if layout == "rowmajor" and resample == "bicubic" and size == (24, 16):
                    assert np.array_equal(dec.decode([raw(n) for n in names], **kw), got)
                    kw.pop("perspective")
                    (one, two) = list(dec.decode_device_iter([[raw(n) for n in names], [raw(ODD)]], perspective=[coeffs, coeffs[0]], **kw))
                    assert np.array_equal(host(one), got) and np.array_equal(host(two)[0], got[0])
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ("xmajor", "planar_rowmajor"))
def test_fill_pixels_go_through_the_output_table(layout):
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from tools import normalize_model, perspective_model
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    names = [ODD, C440]
    coeffs = [away(DIMS[n]) for n in names]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        got = dec.decode_device([raw(n) for n in names], size=(32, 24), perspective=coeffs, affine_resample="bilinear", affine_fill=FILL,
                                dtype=torch.float16, normalize=(mean, std))
        assert got.dtype == torch.float16
        bits = got.cpu().view(torch.int16).numpy().view(np.uint16)
        for k, n in enumerate(names):
            rm = perspective_model.expected(plain(n), coeffs[k], None, (32, 24), resample="bilinear", affine_fill=FILL)
            assert (rm.reshape(-1, 3) == np.array(FILL, np.uint8)).all(axis=1).mean() > 0.5          # (mostly fill: a condition on the input)
            assert np.array_equal(bits[k], as_layout(normalize_model.normalize(rm, "float16", mean, std), layout)), n
    finally:
        dec.close()


@pytest.mark.parametrize("resample", ("nearest", "bicubic"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_convert_then_orient_then_transform(layout, resample):
    from pyjpegdecoder_amd import BatchDecoder
    names, orient = [ODD, C411, C440], [3, 6, 5]
    odims = [DIMS[ODD], DIMS[C411][::-1], DIMS[C440][::-1]]
    coeffs = [keystone(d, k) for k, d in enumerate(odims)]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        kw = dict(size=(40, 28), orientation=orient, perspective=coeffs, affine_resample=resample, affine_fill=FILL)
        got = host(dec.decode_device([raw(n) for n in names], **kw))
        for k, n in enumerate(names):
            assert np.array_equal(got[k], want(n, layout, coeffs[k], (40, 28), resample=resample, affine_fill=FILL, orientation=orient[k])), (n, orient[k])
        # mode="L" on colour files (every tap converted before it is interpolated), mode="RGB" on the grey one
        kw.update(mode="L", affine_fill=55)
        got = host(dec.decode_device([raw(n) for n in names], **kw))
        for k, n in enumerate(names):
            assert np.array_equal(got[k], want(n, layout, coeffs[k], (40, 28), resample=resample, affine_fill=55, orientation=orient[k], mode="L")), (n, "L")
        c = pole(DIMS[GREY])
        got = host(dec.decode_device([raw(GREY)], size=(40, 28), mode="RGB", orientation=8, perspective=c, affine_resample=resample, affine_fill=FILL))
        assert np.array_equal(got[0], want(GREY, layout, c, (40, 28), resample=resample, affine_fill=FILL, orientation=8, mode="RGB"))
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_windows_are_windows_of_the_transformed_image(layout):
    from pyjpegdecoder_amd import BatchDecoder
    names = [ODD, C420, C411, C440]
    # windows at the four corners of the frame: their bicubic taps and the inside test meet the image's edge
    rois = [(0, 0, 31, 22), (64 - 29, 64 - 33, 29, 33), (100 - 17, 0, 17, 36), (0, 80 - 21, 25, 21)]
    coeffs = [keystone(DIMS[n], k) for k, n in enumerate(names)]
    dec = BatchDecoder(device=0, layout=layout)
    try:
        for resample in ("bicubic", "nearest"):
            kw = dict(size=(24, 16), rois=rois, perspective=coeffs, affine_resample=resample, affine_fill=FILL, resample="bicubic")
            got = host(dec.decode_device([raw(n) for n in names], **kw))
            for k, n in enumerate(names):
                exp = want(n, layout, coeffs[k], (24, 16), window=rois[k], resample=resample, affine_fill=FILL, filter="bicubic")
                assert np.array_equal(got[k], exp), (n, resample)
        # resize_to= (the shorter side to 20, centre crop on a 16 x 16 canvas) and mixed mirror=
        from pyjpegdecoder_amd.batch import centred, resized_size
        kw = dict(size=(16, 16), resize_to=20, mirror=[True, False, True, False], perspective=coeffs, affine_resample="bilinear", affine_fill=FILL)
        got = host(dec.decode_device([raw(n) for n in names], **kw))
        for k, n in enumerate(names):
            target = resized_size(20, DIMS[n][0], DIMS[n][1], (16, 16))
            exp = want(n, layout, coeffs[k], (16, 16), resample="bilinear", affine_fill=FILL, resized=target, xy=centred(20, target, (16, 16)), mirror=kw["mirror"][k])
            assert np.array_equal(got[k], exp), (n, target)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_view_has_its_own_coefficients(layout):
    from pyjpegdecoder_amd import BatchDecoder
    c1, c2 = keystone(DIMS[ODD]), pole(DIMS[ODD])
    w1, w2 = (5, 3, 40, 30), (33, 11, 37, 39)
    dec = BatchDecoder(device=0, layout=layout)
    try:
        kw = dict(size=(24, 16), affine_resample="bilinear", affine_fill=FILL)
        got = host(dec.decode_device([raw(ODD)], views=[(0, w1), (0, w2), 0], perspective=[c1, c2, None], **kw))
        for k, (c, w) in enumerate(((c1, w1), (c2, w2))):
            one = host(dec.decode_device([raw(ODD)], rois=[w], perspective=c, **kw))
            assert np.array_equal(got[k], one[0]), k
            assert np.array_equal(got[k], want(ODD, layout, c, (24, 16), window=w, resample="bilinear", affine_fill=FILL)), k
        assert np.array_equal(got[2], host(dec.decode_device([raw(ODD)], size=(24, 16)))[0])
    finally:
        dec.close()


def test_colour_ops_behind_a_keystone_see_the_fill():
    """contrast's mean and the blur's neighbourhoods are those of the canvas, fill pixels included"""
    from pyjpegdecoder_amd import BatchDecoder
    from tools import colour_model, perspective_model
    names = [ODD, C411]
    coeffs = [keystone(DIMS[n], k) for k, n in enumerate(names)]
    chain = [("contrast", 1.3), ("gaussian_blur", 1.0)]
    dec = BatchDecoder(device=0, layout="rowmajor")
    try:
        got = host(dec.decode_device([raw(n) for n in names], size=(40, 28), perspective=coeffs, affine_resample="bilinear", affine_fill=FILL, color_ops=chain))
        for k, n in enumerate(names):
            canvas = perspective_model.expected(plain(n), coeffs[k], None, (40, 28), resample="bilinear", affine_fill=FILL)
            assert np.array_equal(got[k], colour_model.apply_chain(canvas, chain)), n
    finally:
        dec.close()


@pytest.mark.parametrize("kind", ("444", "grey"))
def test_bicubic_keystone_of_the_checker_clamps_at_both_ends(kind):
    from pyjpegdecoder_amd import BatchDecoder
    from tools import perspective_model
    name = f"checker_48x40_{kind}"
    src = plain(name, "affine")
    c, fill = keystone((48, 40)), (FILL if src.ndim == 3 else 55)
    exp = perspective_model.transform(src, c, "bicubic", fill)
    X, Y = np.meshgrid(np.arange(48), np.arange(40))
    xin, yin = perspective_model.source_coords(c, X, Y)
    inside = (xin >= 0) & (xin < 48) & (yin >= 0) & (yin < 40)
    assert (exp[inside] == 0).any() and (exp[inside] == 255).any()      # (bytes of 0 and of 255 that are not fill)
    dec = BatchDecoder(device=0, layout="rowmajor")
    try:
        # (a box resize to the image's own size is the identity: the transformed image itself)
        got = host(dec.decode_device([(GOLDEN / "affine" / f"{name}.jpg").read_bytes()], size=(48, 40), resample="box", perspective=c,
                                     affine_resample="bicubic", affine_fill=fill))
        assert np.array_equal(got[0].reshape(exp.shape), exp)
    finally:
        dec.close()


def test_refusals_name_what_is_wrong():
    from pyjpegdecoder_amd import BatchDecoder
    dec = BatchDecoder(device=0)
    try:
        with pytest.raises(ValueError, match="perspective needs size"):
            dec.decode_device([raw(ODD)], perspective=IDENT)
        with pytest.raises(ValueError, match="perspective and reducing_gap do not go together yet"):
            dec.decode_device([raw(ODD)], size=(24, 16), perspective=IDENT, reducing_gap=2.0)
        with pytest.raises(ValueError, match="affine and perspective do not go together"):
            dec.decode_device([raw(ODD)], size=(24, 16), perspective=IDENT, affine=(1, 0, 0, 0, 1, 0))
        with pytest.raises(ValueError, match=r"perspective: output 1 \(file 1\): a coefficient is not finite"):
            dec.decode_device([raw(ODD), raw(C411)], size=(24, 16), perspective=[None, (1, 0, 0, 0, 1, 0, float("nan"), 0)])
        with pytest.raises(ValueError, match="perspective has 2 entries for 1 outputs"):
            dec.decode([raw(ODD)], size=(24, 16), perspective=[None, IDENT])
        with pytest.raises(ValueError, match="perspective yields fewer entries than there are batches"):
            list(dec.decode_device_iter([[raw(ODD)], [raw(ODD)]], size=(24, 16), perspective=iter([[IDENT]])))
    finally:
        dec.close()
