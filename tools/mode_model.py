"""The output colour mode of `decode(..., mode=)`, restated in NumPy: the definition the GPU path is held to
(tests/test_mode*.py, which also pin it to Pillow's ``Image.convert``).

``convert(a, mode)`` is what Pillow's ``img.convert(mode)`` does to 8-bit pixels:

    "L"    a colour pixel (R, G, B) becomes (19595 R + 38470 G + 7471 B + 32768) >> 16 — ITU-R 601-2 luma in 16-bit fixed
           point with the rounding half added (the three weights sum to 65536, so grey stays what it was); greyscale is unchanged
    "RGB"  a greyscale value goes into all three components; colour is unchanged
    None   the pixels as they are

The conversion applies to the DECODED pixels, in front of everything else a call does: the result of a call is
``exif_transpose(img.convert(mode)).resize(size, filter)``, then the output table, then the mirror (tools/orient_model.py,
resize_model.py, normalize_model.py).  For "L" the place matters — the resize rounds each component to a byte, and the luma of
rounded bytes is not the rounded luma — so resize-then-convert is another image.
"""
import numpy as np

MODES = {"L": 1, "RGB": 3}       # Pillow's name -> components of the output


def luma(r, g, b) -> np.ndarray:
    """Pillow's L of 8-bit R, G, B (arrays of one shape, any integer type): uint8."""
    r, g, b = (np.asarray(v).astype(np.uint32) for v in (r, g, b))
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).astype(np.uint8)


def convert(a: np.ndarray, mode) -> np.ndarray:
    """uint8 pixels ``a`` — (..., 3) colour with the components last, or any other shape greyscale — in ``mode``: (...) for
    "L", (..., 3) for "RGB", ``a`` itself for None.  ValueError for anything else."""
    a = np.asarray(a, dtype=np.uint8)
    if mode is None:
        return a
    if mode not in MODES:
        raise ValueError(f"mode must be None, 'L' or 'RGB', not {mode!r}")
    colour = a.ndim >= 2 and a.shape[-1] == 3
    if mode == "L":
        return luma(a[..., 0], a[..., 1], a[..., 2]) if colour else a
    return a if colour else np.ascontiguousarray(np.repeat(a[..., None], 3, axis=-1))
