"""The model-ready output of `decode(..., size=, dtype=, normalize=, mirror=)`, as a small NumPy model: what torchvision's
`Normalize(mean, std)(to_tensor(img))` followed by torch's `.to(dtype)` does to a resized byte.  Tests hold the library's
table (mj_host_normalize_table) and the GPU's elements to this model, and the model to torch's CPU ops
(tests/test_normalize_host.py) — bit patterns, not tolerances.

For a byte v (0..255) of component c, every operation a float32 one, each correctly rounded:

    t   = fl32(float32(v) / float32(255))                       to_tensor
    y32 = fl32(fl32(t - fl32(mean[c])) / fl32(std[c]))           Normalize; the float32 output
    float16 / bfloat16 = y32 rounded to nearest even             .to(dtype)

It depends on (c, v) only: 256 values per component."""
import numpy as np

DTYPES = ("float32", "float16", "bfloat16")


def bfloat16_bits(y32: np.ndarray) -> np.ndarray:
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even (finite values and infinities)."""
    bits = np.ascontiguousarray(y32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def table_f32(mean: float = 0.0, std: float = 1.0) -> np.ndarray:
    """y32 of one component for v = 0..255 (float32[256])."""
    m, s, d = np.float32(mean), np.float32(std), np.float32(255)
    out = np.empty(256, dtype=np.float32)
    with np.errstate(over="ignore"):
        for v in range(256):
            t = np.float32(v) / d
            out[v] = (t - m) / s              # (NumPy float32 scalars: every operation rounds to float32)
    return out


def table_bits(dtype: str, mean: float = 0.0, std: float = 1.0) -> np.ndarray:
    """The 256 elements of one component as bit patterns: uint32 for "float32", uint16 for "float16" / "bfloat16"."""
    y = table_f32(mean, std)
    if dtype == "float32":
        return y.view(np.uint32).copy()
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return y.astype(np.float16).view(np.uint16).copy()
    if dtype == "bfloat16":
        return bfloat16_bits(y)
    raise ValueError(f"no float dtype {dtype!r}")


def normalize(img: np.ndarray, dtype: str, mean=None, std=None) -> np.ndarray:
    """img: uint8 (..., C) with the components last, or (...) greyscale with mean / std scalars.  Returns the bit patterns
    (uint32 / uint16) of the same shape.  mean / std: None (0 and 1), one float, or one per component."""
    img = np.asarray(img, dtype=np.uint8)
    per = np.ndim(mean) > 0 or np.ndim(std) > 0
    if not per:
        return table_bits(dtype, 0.0 if mean is None else mean, 1.0 if std is None else std)[img]
    C = img.shape[-1]
    mean = np.broadcast_to(np.asarray(0.0 if mean is None else mean, dtype=np.float64), (C,))
    std = np.broadcast_to(np.asarray(1.0 if std is None else std, dtype=np.float64), (C,))
    return np.stack([table_bits(dtype, mean[c], std[c])[img[..., c]] for c in range(C)], axis=-1)
