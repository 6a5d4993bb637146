"""Model-ready output (dtype / normalize / mirror of a decode to a fixed size), the parts that need no GPU: the NumPy model of
the element function (tools/normalize_model.py) is torch's CPU chain `.to(float32).div(255).sub_(mean).div_(std).to(dtype)` bit
for bit; the library's table (mj_host_normalize_table) is the model's; the argument rules raise before any GPU work; the C
entry point refuses a bad output description without a device; the new struct has its ctypes twin's layout."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FLOAT_DTYPES = ("float32", "float16", "bfloat16")


def pairs():
    """(mean, std) of one component: ImageNet's three, (0, 1), (0.5, 0.5), stds small enough that float16 (and one that
    bfloat16 / float32) overflow to infinity, the extremes, and 300 seeded random pairs."""
    out = list(zip(*IMAGENET)) + [(0.0, 1.0), (0.5, 0.5), (0.0, 1e-6), (0.25, 1e-5), (0.0, 1e-39), (0.9, 3e-39), (1.0, 1.0),
                                  (-1.0, 1e4), (0.0, 1.0 / 255), (0.1, 1e30)]
    rng = np.random.default_rng(9090)
    for k in range(300):
        mean = float(rng.uniform(-1.0, 2.0))
        std = float(10.0 ** rng.uniform(-7, 2)) if k % 3 == 0 else float(rng.uniform(0.01, 1.0))
        out.append((mean, std))
    return out


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


def torch_bits(dtype, mean, std):
    """the chain users run today, on the CPU, for the 256 bytes of one component: bit patterns"""
    import torch
    v = torch.arange(256, dtype=torch.uint8)
    y = v.to(torch.float32).div(255).sub_(torch.tensor(mean, dtype=torch.float32)).div_(torch.tensor(std, dtype=torch.float32))
    if dtype == "float32":
        return y.view(torch.int32).numpy().view(np.uint32)
    return y.to(getattr(torch, dtype)).view(torch.int16).numpy().view(np.uint16)


def test_model_is_torchs_cpu_chain_bit_for_bit():
    from tools import normalize_model
    cases = pairs()
    assert len(cases) == 313
    bad, overflow16 = [], 0
    for mean, std in cases:
        for dtype in FLOAT_DTYPES:
            got, want = normalize_model.table_bits(dtype, mean, std), torch_bits(dtype, mean, std)
            assert got.dtype == want.dtype and got.shape == (256,)
            if not np.array_equal(got, want):
                bad.append((mean, std, dtype))
            if dtype == "float16" and (got & 0x7FFF == 0x7C00).any():
                overflow16 += 1
    assert not bad, f"{len(bad)} of {3 * len(cases)} tables differ from torch, first {bad[:5]}"
    assert overflow16 >= 3                       # (the small stds did reach float16's infinity)
    # torchvision's own formulation for a whole image: to_tensor is .div(255), Normalize is .sub_(mean[:, None, None]).div_(std[...])
    import torch
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    t = torch.from_numpy(img).permute(2, 0, 1).to(torch.float32).div(255)
    m, s = (torch.tensor(x, dtype=torch.float32).view(3, 1, 1) for x in IMAGENET)
    want = t.sub_(m).div_(s).permute(1, 2, 0).contiguous()
    for dtype in FLOAT_DTYPES:
        got = normalize_model.normalize(img, dtype, *IMAGENET)
        w = want.view(torch.int32).numpy().view(np.uint32) if dtype == "float32" else \
            want.to(getattr(torch, dtype)).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got, w), dtype
    # without normalize: value / 255, and float32 times 255 is the byte again
    y = normalize_model.table_f32()
    assert np.array_equal((y * np.float32(255)).astype(np.float32), np.arange(256, dtype=np.float32))
    assert np.array_equal(np.rint(normalize_model.table_bits("float16").view(np.float16).astype(np.float32) * np.float32(255)),
                          np.arange(256, dtype=np.float32))


def test_library_table_is_the_models(lib):
    from pyjpegdecoder_amd import _binding as B
    from tools import normalize_model
    done = 0
    for mean, std in pairs():
        for dtype in FLOAT_DTYPES:
            got = B.normalize_table(dtype, mean, std)
            want = normalize_model.table_bits(dtype, mean, std)
            assert got.dtype == want.dtype and np.array_equal(got, want), (mean, std, dtype)
            done += 1
    assert done == 313 * 3
    # float16's subnormals and its rounding at the top come out of the library's own conversion: the values around them
    for mean, std in ((0.0, 2.0 ** 14), (0.0, 2.0 ** 17), (0.0, 60000.0), (0.0, 1.0 / 65519.9), (0.0, 1.0 / 65520.1), (0.5, 2.0 ** 20)):
        assert np.array_equal(B.normalize_table("float16", mean, std), normalize_model.table_bits("float16", mean, std)), (mean, std)
    buf = np.zeros(256, dtype=np.uint32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.mj_host_normalize_table(B.MJ_DTYPE_F32, 0.0, 1.0, p) == B.MJ_OK
    for dtype, mean, std in ((B.MJ_DTYPE_U8, 0.0, 1.0), (7, 0.0, 1.0), (-1, 0.0, 1.0), (B.MJ_DTYPE_F32, 0.0, 0.0), (B.MJ_DTYPE_F16, 0.0, -1.0),
                             (B.MJ_DTYPE_F32, 0.0, float("nan")), (B.MJ_DTYPE_BF16, 0.0, float("inf")), (B.MJ_DTYPE_F32, float("nan"), 1.0),
                             (B.MJ_DTYPE_F32, float("-inf"), 1.0)):
        assert lib.mj_host_normalize_table(dtype, mean, std, p) == B.MJ_ERR_INVALID, (dtype, mean, std)
    assert lib.mj_host_normalize_table(B.MJ_DTYPE_F32, 0.0, 1.0, None) == B.MJ_ERR_INVALID


def test_argument_rules_need_no_gpu():
    """Every ValueError of dtype / normalize / mirror, from the plain function decode / decode_device / decode_device_iter call
    before any GPU work."""
    import torch
    from pyjpegdecoder_amd.batch import OutputSpec, dtype_name, normalize_output
    size = (8, 6)
    # nothing asked: nothing returned, with or without size — the plain path
    assert normalize_output(None, None, None, None) is None and normalize_output(None, None, None, size, 4, 3) is None
    assert normalize_output("uint8", None, None, size, 4, 3) is None
    # no size
    for kw in (dict(dtype="float32"), dict(normalize=IMAGENET), dict(mirror=True), dict(mirror=[True, False]), dict(dtype="uint8")):
        args = dict(dtype=None, normalize=None, mirror=None)
        args.update(kw)
        with pytest.raises(ValueError, match="size"):
            normalize_output(args["dtype"], args["normalize"], args["mirror"], None, 2, 3)
    # dtype names and objects
    for given, name in (("float32", "float32"), (torch.float16, "float16"), (torch.bfloat16, "bfloat16"), (np.float32, "float32"),
                        (np.dtype("float16"), "float16"), (torch.uint8, "uint8"), (np.uint8, "uint8"), ("bfloat16", "bfloat16")):
        assert dtype_name(given) == name
    for bad in ("float64", torch.float64, np.int8, "half", 16, torch.int32):
        with pytest.raises(ValueError, match="dtype"):
            normalize_output(bad, None, None, size, 2, 3)
    with pytest.raises(ValueError, match="decode_device"):
        normalize_output("bfloat16", None, None, size, 2, 3, host=True)
    with pytest.raises(ValueError, match="decode_device"):
        normalize_output(torch.bfloat16, IMAGENET, None, size, host=True)
    assert normalize_output("bfloat16", None, None, size, 2, 3).dtype == "bfloat16"
    # normalize
    with pytest.raises(ValueError, match="uint8"):
        normalize_output("uint8", IMAGENET, None, size, 2, 3)
    spec = normalize_output(None, IMAGENET, None, size, 2, 3)
    assert spec == OutputSpec("float32", IMAGENET[0], IMAGENET[1], None)
    assert normalize_output("float16", (0.5, 0.25), None, size, 2, 3) == OutputSpec("float16", (0.5,) * 3, (0.25,) * 3, None)
    assert normalize_output("float16", (0.5, [0.25]), None, size, 2, 1) == OutputSpec("float16", (0.5,), (0.25,), None)
    assert normalize_output("float32", None, None, size, 2, 3) == OutputSpec("float32", None, None, None)
    for bad in ((IMAGENET[0], IMAGENET[1][:2]), (IMAGENET[0][:1], IMAGENET[1]), ((0.1, 0.2, 0.3, 0.4), 1.0), ([], 1.0)):
        with pytest.raises(ValueError, match="entries"):
            normalize_output("float32", bad, None, size, 2, 3)
    with pytest.raises(ValueError, match="entries"):
        normalize_output("float32", IMAGENET, None, size, 2, 1)             # greyscale files, three values
    for bad in (0.5, (0.5,), (0.5, 0.5, 0.5), "ab", ("a", 1.0), (None, 1.0)):
        with pytest.raises(ValueError, match="normalize"):
            normalize_output("float32", bad, None, size, 2, 3)
    for std in (0.0, -0.5, float("nan"), float("inf"), 1e-50, (0.2, 0.0, 0.2), (0.2, 0.2, float("nan"))):
        with pytest.raises(ValueError, match="std"):
            normalize_output("float32", (0.5, std), None, size, 2, 3)
    for mean in (float("nan"), float("inf"), 1e39, (0.0, float("-inf"), 0.0)):
        with pytest.raises(ValueError, match="mean"):
            normalize_output("float32", (mean, 1.0), None, size, 2, 3)
    # mirror
    assert normalize_output(None, None, True, size, 3, 3) == OutputSpec("uint8", None, None, [True] * 3)
    assert normalize_output(None, None, [True, False, np.bool_(True)], size, 3, 3).mirror == [True, False, True]
    assert normalize_output("float16", None, np.array([False, True]), size, 2, 3).mirror == [False, True]
    assert normalize_output("float16", None, torch.tensor([False, True]), size, 2, 3).mirror == [False, True]
    for bad, n in (([True, False], 3), ([], 1), ([True] * 4, 3)):
        with pytest.raises(ValueError, match="mirror"):
            normalize_output(None, None, bad, size, n, 3)
    for bad in ("yes", 1, [True, "no"], [0.5, 1.0], [2, 0]):
        with pytest.raises(ValueError, match="mirror"):
            normalize_output(None, None, bad, size, 2, 3)
    # flags follow their files
    spec = normalize_output("float32", IMAGENET, [True, False, False, True, True], size, 5, 3)
    assert spec.for_files([4, 1, 0]).mirror == [True, False, True]
    assert spec.plan_output([1, 3]) == ("float32", IMAGENET[0], IMAGENET[1], [False, True])
    assert spec.numpy_dtype == np.float32 and spec.torch_dtype == torch.float32


def test_a_narrowed_request_takes_its_files_arguments_along():
    """batch._Request.narrow: a request for files 1 and 3 of five carries exactly their windows, slots and mirror flags, and
    gives _binding.Plan the keyword arguments the per-site slices gave; a request without windows, slots or flags keeps None."""
    from pyjpegdecoder_amd.batch import _Request, normalize_output
    files = [bytes([k]) * (k + 1) for k in range(5)]
    wins = [(k, 2 * k, 8 + k, 9 + k) for k in range(5)]
    slots = [7, 0, 5, 2, 6]
    mirror = [True, False, False, True, True]
    dest = np.empty((9, 4, 6, 3), dtype=np.float32)
    spec = normalize_output("float32", IMAGENET, mirror, (4, 6), 5, 3)
    idxs = [1, 3]
    sub = _Request(files, wins, (4, 6), spec, dest, slots).narrow(idxs)
    assert sub.files == [files[1], files[3]] and sub.wins == [wins[1], wins[3]] and sub.slots == [0, 2]
    assert sub.output.mirror == [False, True] and sub.size == (4, 6) and sub.dest is dest
    assert sub.plan_kwargs() == {"rois": [wins[i] for i in idxs], "size": (4, 6), "slots": ([slots[i] for i in idxs], 9),
                                 "output": ("float32", IMAGENET[0], IMAGENET[1], [mirror[i] for i in idxs])}
    assert _Request(files, wins, (4, 6), spec, dest, slots).narrow(np.array([4, 0])).slots == [6, 7]    # (indices from NumPy too)
    bare = _Request(files).narrow(idxs)
    assert bare.files == [files[1], files[3]] and (bare.wins, bare.size, bare.output, bare.dest, bare.slots) == (None,) * 5
    assert bare.plan_kwargs() == {"rois": None, "size": None, "slots": None, "output": None}
    unflagged = _Request(files, None, (4, 6), normalize_output("float16", None, None, (4, 6), 5, 3)).narrow(idxs)
    assert unflagged.output.mirror is None and unflagged.plan_kwargs()["output"] == ("float16", None, None, None)


def test_entry_point_refuses_a_bad_output_without_a_device(lib):
    """mj_plan_create_with looks at the output description before the context: MJ_ERR_INVALID with a message (no
    context: mj_last_error(NULL)'s) for a dtype that is none of the four, normalize with MJ_DTYPE_U8, a std <= 0 or not finite, a
    mean not finite."""
    from pyjpegdecoder_amd import _binding as B
    from routes_common import create_with
    h = ctypes.c_void_p()

    def call(dtype, normalize, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
        d = B.OutputDescC()
        d.dtype, d.normalize = dtype, normalize
        d.mean[:] = mean
        d.std[:] = std
        rc = create_with(lib, None, None, h, out_width=8, out_height=8, output=d)
        return rc, lib.mj_last_error(None)
    for dtype in (4, -1, 99):
        rc, msg = call(dtype, 0)
        assert rc == B.MJ_ERR_INVALID and b"dtype" in msg, msg
    rc, msg = call(B.MJ_DTYPE_U8, 1)
    assert rc == B.MJ_ERR_INVALID and b"normalize" in msg, msg
    for std in ((0.2, 0.0, 0.2), (-1.0, 1.0, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        for dtype in (B.MJ_DTYPE_F16, B.MJ_DTYPE_BF16, B.MJ_DTYPE_F32):
            rc, msg = call(dtype, 1, std=std)
            assert rc == B.MJ_ERR_INVALID and b"std" in msg, (std, msg)
    for mean in ((float("nan"), 0.0, 0.0), (0.0, 0.0, float("inf"))):
        rc, msg = call(B.MJ_DTYPE_F32, 1, mean=mean)
        assert rc == B.MJ_ERR_INVALID and b"mean" in msg, (mean, msg)
    # (without normalize, mean and std are not looked at)
    create_with(lib, None, None, h)
    rc, msg = call(B.MJ_DTYPE_F32, 0, std=(0.0, 0.0, 0.0))
    assert rc == B.MJ_ERR_INVALID and b"std" not in msg.split(b"output:")[-1]
    # the Python binding refuses an output without a size
    with pytest.raises(ValueError, match="size"):
        B.Plan(None, None, None, output=("float32", None, None, None))


def test_output_desc_layout_and_prototypes_match_the_binding(lib, tmp_path):
    from pyjpegdecoder_amd import _binding as B
    for name in ("mj_host_normalize_table",):
        assert name in B.EXPORTS and hasattr(lib, name), name
    assert (B.MJ_DTYPE_U8, B.MJ_DTYPE_F16, B.MJ_DTYPE_BF16, B.MJ_DTYPE_F32) == (0, 1, 2, 3)
    gcc = shutil.which("gcc")
    assert gcc is not None, "the header is held to a C compiler"
    fields = [f for f, _ in B.OutputDescC._fields_]
    flags = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include")]
    # the prototypes the binding assumes, assigned from the header's declarations (a mismatch is a compile error)
    proto = tmp_path / "proto.c"
    proto.write_text("""
#include "mijpeg.h"
int main(void) {
  int (*b)(int32_t, float, float, void *) = mj_host_normalize_table;
  (void)b;
  return 0;
}
""")
    subprocess.run([gcc] + flags + ["-c", str(proto), "-o", str(tmp_path / "proto.o")], check=True)
    # the struct: size and offsets as the C compiler lays it out against the ctypes twin's
    src = tmp_path / "layout.c"
    src.write_text("\n".join(
        ['#include <stdio.h>', '#include <stddef.h>', '#include "mijpeg.h"', 'int main(void) {', '  printf("%zu", sizeof(mj_output_desc));'] +
        [f'  printf(" %zu", offsetof(mj_output_desc, {f}));' for f in fields] +
        ['  printf(" %d %d %d %d\\n", MJ_DTYPE_U8, MJ_DTYPE_F16, MJ_DTYPE_BF16, MJ_DTYPE_F32);', '  return 0;', '}']))
    exe = tmp_path / "layout"
    subprocess.run([gcc] + flags + [str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(B.OutputDescC)] + [getattr(B.OutputDescC, f).offset for f in fields] + [0, 1, 2, 3]
    assert got == want, (got, want)
