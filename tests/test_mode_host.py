"""The output colour mode on the CPU: tools/mode_model.py (the definition) and mj_host_convert_mode (the host twin of the
kernels' conversion) against Pillow's Image.convert over every input there is, what normalize_mode takes and refuses, and that a
call without ``mode=`` is what it was."""
import numpy as np
import pytest

from conftest import GOLDEN


def all_rgb() -> np.ndarray:
    """every 8-bit RGB triple, (2^24, 3) uint8"""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8)


@pytest.fixture(scope="module")
def triples():
    a = all_rgb()
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def pillow_l(triples):
    """Pillow's convert("L") of every triple"""
    Image = pytest.importorskip("PIL.Image")
    out = np.asarray(Image.fromarray(triples.reshape(4096, 4096, 3), "RGB").convert("L")).reshape(-1).copy()
    out.setflags(write=False)
    return out


def test_model_l_is_pillows_over_all_triples(triples, pillow_l):
    from tools import mode_model
    got = mode_model.convert(triples, "L")
    assert got.shape == (1 << 24,) and got.dtype == np.uint8
    assert np.array_equal(got, pillow_l)


def test_host_twin_l_is_pillows_over_all_triples(triples, pillow_l):
    from pyjpegdecoder_amd import _binding as B
    got = B.convert_mode(triples, "L")
    assert got.shape == (1 << 24,) and got.dtype == np.uint8
    assert np.array_equal(got, pillow_l)


def test_l_is_not_the_truncating_formula(triples, pillow_l):
    """(what the + 32768 is worth: a model or a kernel without it would not pass the two tests above)"""
    t = triples.astype(np.uint32)
    trunc = ((19595 * t[:, 0] + 38470 * t[:, 1] + 7471 * t[:, 2]) >> 16).astype(np.uint8)
    assert (trunc != pillow_l).mean() > 0.4


def test_rgb_of_every_grey_value_model_and_host_twin():
    from tools import mode_model
    from pyjpegdecoder_amd import _binding as B
    Image = pytest.importorskip("PIL.Image")
    grey = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = np.asarray(Image.fromarray(grey, "L").convert("RGB"))
    assert want.shape == (16, 16, 3)
    assert np.array_equal(mode_model.convert(grey, "RGB"), want)
    assert np.array_equal(B.convert_mode(grey, "RGB"), want)
    assert np.array_equal(B.convert_mode(grey, B.MJ_MODE_RGB), want)


def test_modes_that_change_nothing_and_bad_arguments():
    import ctypes
    from tools import mode_model
    from pyjpegdecoder_amd import _binding as B
    rng = np.random.default_rng(5)
    colour, grey = rng.integers(0, 256, (7, 5, 3), dtype=np.uint8), rng.integers(0, 256, (7, 5), dtype=np.uint8)
    for conv in (mode_model.convert, B.convert_mode):
        assert np.array_equal(conv(colour, "RGB"), colour) and np.array_equal(conv(colour, None), colour)
        assert np.array_equal(conv(grey, "L"), grey) and np.array_equal(conv(grey, None), grey)
        with pytest.raises(ValueError):
            conv(grey, "CMYK")
    assert (B.MJ_MODE_NATIVE, B.MJ_MODE_L, B.MJ_MODE_RGB) == (0, 1, 3) and B.MODES == mode_model.MODES
    L = B.load_library()
    out = np.zeros(64, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.mj_host_convert_mode(2, p(grey), 1, 4, p(out)) == B.MJ_ERR_INVALID         # no such mode
    assert L.mj_host_convert_mode(B.MJ_MODE_L, p(grey), 2, 4, p(out)) == B.MJ_ERR_INVALID      # no such source
    assert L.mj_host_convert_mode(B.MJ_MODE_L, None, 3, 4, p(out)) == B.MJ_ERR_INVALID
    assert L.mj_host_convert_mode(B.MJ_MODE_L, None, 3, 0, None) == B.MJ_OK
    assert "mj_host_convert_mode" in B.EXPORTS and hasattr(L, "mj_host_convert_mode")


def test_normalize_mode_accepts_and_refuses():
    from pyjpegdecoder_amd.batch import normalize_mode
    assert normalize_mode(None) is None and normalize_mode("RGB") == "RGB" and normalize_mode("L") == "L"
    for bad in ("rgb", "l", "RGBA", "YCbCr", "1", "", 1, 3, 0, True, b"L", ("L",), ["RGB"], 1.0):
        with pytest.raises(ValueError, match="mode must be"):
            normalize_mode(bad)


def test_requests_carry_the_mode_and_pass_it_only_to_plans_that_convert():
    from pyjpegdecoder_amd.batch import _Request
    req = _Request([b"a", b"b", b"c"], None, (4, 6), mode="RGB")
    assert req.ncomp == 3 and req.narrow([2, 0]).mode == "RGB"
    assert req.plan_kwargs(1)["mode"] == "RGB" and "mode" not in req.plan_kwargs(3)
    grey = _Request([b"a"], None, None, mode="L")
    assert grey.ncomp == 1 and grey.plan_kwargs(3)["mode"] == "L" and "mode" not in grey.plan_kwargs(1)
    # files of the mode's own count: the arguments of a call without the argument
    assert req.plan_kwargs(3) == _Request([b"a", b"b", b"c"], None, (4, 6)).plan_kwargs()
    plain = _Request([b"a"], None, (4, 6))
    assert plain.mode is None and plain.ncomp is None and "mode" not in plain.plan_kwargs(1) and "mode" not in plain.plan_kwargs()


def test_a_call_without_mode_still_refuses_a_mixed_list_under_size():
    """mode=None is today's behaviour, the error and its text included; what needs no GPU is checked before any GPU work."""
    from pyjpegdecoder_amd.batch import BatchDecoder, one_component_count
    with pytest.raises(ValueError) as e:
        one_component_count([3, 3, 1])
    assert str(e.value) == ("file 2: 1 colour component(s) where file 0 has 3: greyscale and colour files do not share one array; "
                            "decode them in separate calls")
    files = [(GOLDEN / "files" / n).read_bytes() for n in ("64x64_420_pil.jpg", "64x64_grey_pil.jpg")]
    dec = BatchDecoder.__new__(BatchDecoder)          # (no context: these checks come before anything touches the GPU)
    dec.layout, dec.gpu_segment, dec.gpu_segment_min_files, dec.base_flags = 0, True, 8, 0
    for call in (dec.decode, dec.decode_device):
        with pytest.raises(ValueError, match="file 1: 1 colour component.*decode them in separate calls"):
            call(files, size=(8, 8))
        with pytest.raises(ValueError, match="file 1: 1 colour component.*decode them in separate calls"):
            call(files, size=(8, 8), mode=None)
        with pytest.raises(ValueError, match="mode must be"):
            call(files, size=(8, 8), mode="rgb")
    with pytest.raises(ValueError, match="mode must be"):
        next(dec.decode_device_iter([files], size=(8, 8), mode="YCbCr"))
    with pytest.raises(ValueError, match="mode and return_seams"):
        dec.decode(files, return_seams=True, mode="RGB")
    # normalize is checked against the mode's count, not the files'
    with pytest.raises(ValueError, match="normalize: mean has 3 entries for files of 1 component"):
        dec.decode(files, size=(8, 8), mode="L", dtype="float32", normalize=((0.1, 0.2, 0.3), 1.0))
