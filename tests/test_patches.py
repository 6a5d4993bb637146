"""patches= on the MI355X at the C ABI (mj_patchify): the whole case list (tests/patch_cases.py) over device arrays of random bits,
against tools/patch_model.py — which tests/test_patches_host.py holds to torch's reshape / permute — and against the host twin.
Bit patterns, in every layout and element type; no tolerance anywhere.  Through the decoders: tests/test_patches_routes.py."""
import numpy as np
import pytest

from patch_cases import BITS, DTYPES, LAYOUTS, all_cases, full_windows, many_jobs_cases, model_patchify, random_bits, same_bits

pytestmark = pytest.mark.gpu

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


def launch(dec, layout, dtype, C, pre, size, spec, shape, front=(0, 0)):
    """Context.patchify from ``pre`` (host, bit patterns) into a sentinel-filled buffer that holds exactly ``shape`` between its
    guards; ``front``: bytes in front of src and dst inside their buffers.  Returns the token array; the sentinels around it are
    checked, and that src is as it was."""
    import torch
    nbytes = int(np.prod(shape)) * pre.dtype.itemsize
    fs, fd = front
    src = torch.full((fs + pre.nbytes + 61,), 0x5A, dtype=torch.uint8, device="cuda:0")
    dst = torch.full((fd + nbytes + 61,), 0xA5, dtype=torch.uint8, device="cuda:0")
    flat = np.ascontiguousarray(pre).reshape(-1).view(np.uint8)
    src[fs:fs + pre.nbytes] = torch.from_numpy(flat).to("cuda:0")
    torch.cuda.synchronize()
    dec.ctx.patchify(src.data_ptr() + fs, dst.data_ptr() + fd, LAYOUTS.index(layout), dtype, C, size, len(pre), spec)
    torch.cuda.synchronize()                # (the context's stream is not torch's: wait for the device)
    got = dst.cpu().numpy()
    assert (got[:fd] == 0xA5).all() and (got[fd + nbytes:] == 0xA5).all(), ("a sentinel was written", front)
    kept = src.cpu().numpy()
    assert (kept[:fs] == 0x5A).all() and (kept[fs + pre.nbytes:] == 0x5A).all() and same_bits(kept[fs:fs + pre.nbytes], flat)
    return got[fd:fd + nbytes].copy().view(pre.dtype).reshape(shape)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_case_list_on_the_device(layout, dtype):
    """every case from 256-byte-aligned arrays, and with src and dst one element past a 16-byte boundary (and one and two elements:
    not congruent), so that every job's range has a head and a tail of lone elements; against the model and mj_host_patchify"""
    from pyjpegdecoder_amd import _binding as B
    dec = decoder(layout)
    es = np.dtype(BITS[dtype]).itemsize
    fronts = [(0, 0), (64 + es, 64 + es), (64 + es, 64 + 2 * es)]
    for name, size, C, spec in CASES:
        pre = np.array(random_bits(dtype, layout, size[0], size[1], C))
        want = model_patchify(pre, spec, layout)
        full = full_windows(spec, size)
        twin = B.host_patchify(pre, LAYOUTS.index(layout), dtype, C, size, full)
        assert same_bits(twin.reshape(want.shape), want), (name, "host twin")
        for front in fronts:
            got = launch(dec, layout, dtype, C, pre, size, full, want.shape, front)
            assert same_bits(got, want), (name, layout, dtype, front)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_many_jobs_and_the_largest_block(layout):
    """one source whose single band is 1.4 MB — many jobs whatever a job holds —, one of a hundred bands, and merge blocks of
    exactly 65536 bytes, the most a job's range (and the LDS image) can be; src and dst at non-congruent places"""
    dec = decoder(layout)
    for name, size, C, dtype, spec in many_jobs_cases():
        es = np.dtype(BITS[dtype]).itemsize
        pre = np.array(random_bits(dtype, layout, size[0], size[1], C, n=1))
        want = model_patchify(pre, spec, layout)
        got = launch(dec, layout, dtype, C, pre, size, spec, want.shape, (64 + es, 64 + 2 * es))
        assert same_bits(got, want), (name, layout)


def test_two_calls_in_a_row_on_two_streams():
    """different windows, different streams, back to back: the second call must not rewrite the job list under the first launch"""
    import torch
    layout, dtype, C, size = "rowmajor", "float16", 3, (48, 36)
    dec = decoder(layout)
    first = dict(patch=2, merge=2, repeat=2, windows=[(0, 0, 48, 36), (4, 4, 40, 28), (8, 0, 4, 36), (0, 8, 48, 4), (4, 4, 40, 28)])
    second = dict(patch=2, merge=2, repeat=2, windows=[(4, 4, 40, 28), (0, 0, 48, 36), (0, 8, 48, 4), (1, 3, 40, 28), (8, 0, 4, 36)])
    pre = np.array(random_bits(dtype, layout, size[0], size[1], C))
    wants = [model_patchify(pre, spec, layout) for spec in (first, second)]
    assert wants[0].shape == wants[1].shape and not same_bits(*wants)
    src = torch.from_numpy(pre.view(np.int16)).to("cuda:0")
    a = torch.zeros(wants[0].shape, dtype=torch.int16, device="cuda:0")
    b = torch.zeros_like(a)
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    args = (LAYOUTS.index(layout), dtype, C, size, len(pre))
    dec.ctx.patchify(src.data_ptr(), a.data_ptr(), *args, first, stream=s1.cuda_stream)
    dec.ctx.patchify(src.data_ptr(), b.data_ptr(), *args, second, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert same_bits(a.cpu().numpy().view(np.uint16), wants[0])
    assert same_bits(b.cpu().numpy().view(np.uint16), wants[1])


def test_what_mj_patchify_refuses():
    import torch
    from pyjpegdecoder_amd.errors import BackendError
    dec = decoder("rowmajor")
    src = torch.zeros((2, 12, 16, 3), dtype=torch.float32, device="cuda:0")
    dst = torch.zeros((2 * 6 * 8, 3 * 4), dtype=torch.float32, device="cuda:0")

    def patchify(spec, s=None, d=None, layout=1, dtype="float32", C=3, size=(16, 12), n=2):
        dec.ctx.patchify(src.data_ptr() if s is None else s, dst.data_ptr() if d is None else d, layout, dtype, C, size, n, spec)
    ok = dict(patch=2)
    for spec, msg in [(dict(patch=0), "mj_patchify: patch 0 is not 1..64"), (dict(patch=65), "patch 65 is not 1..64"), (dict(patch=2, merge=9), "merge 9 is not 1..8"),
                      (dict(patch=2, repeat=5), "repeat 5 is not 1..4"), (dict(patch=2, repeat=2, order="hwc"), "order hwc needs repeat 1"),
                      (dict(patch=2, length=-1), "length -1 is below 0"),
                      (dict(patch=2, windows=[(0, 0, 16, 12), (2, 0, 16, 12)]), "source 1 .window 2, 0, 16 x 12.: the window is not inside the source canvas"),
                      (dict(patch=2, windows=[(0, 0, 16, 12), (0, 0, 0, 12)]), "source 1 .*a width or height below 1"),
                      (dict(patch=2, merge=2, windows=[(0, 0, 16, 12), (1, 1, 6, 8)]), "source 1 .window 1, 1, 6 x 8.: width and height must be multiples of patch . merge = 4"),
                      (dict(patch=5), "source 0 .the whole canvas 0, 0, 16 x 12.: width and height must be multiples of patch . merge = 5"),
                      (dict(patch=2, length=47), "source 0 .*48 tokens, more than length 47"),
                      (dict(patch=64, merge=3), "a merge block of 442368 bytes .*more than 65536")]:
        with pytest.raises(BackendError, match=msg):
            patchify(spec)
    for kw, msg in [(dict(d=src.data_ptr()), "src and dst overlap"), (dict(d=src.data_ptr() + 64), "src and dst overlap"), (dict(s=src.data_ptr() + 2), "not aligned to its 4-byte elements"),
                    (dict(d=dst.data_ptr() + 1), "not aligned to its 4-byte elements"), (dict(s=0), "NULL argument"), (dict(layout=4), "layout 4"), (dict(C=2), "2 components"),
                    (dict(size=(16, 65536)), "sources of 16 x 65536"), (dict(n=0), "0 sources")]:
        with pytest.raises(BackendError, match=msg):
            patchify(ok, **kw)
    # a refused call launched nothing
    torch.cuda.synchronize()
    assert not dst.any().item()
