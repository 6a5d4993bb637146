"""EXIF orientation, restated in NumPy: the definition the GPU path is held to (tests/test_orientation*.py).

``orient(a, o)`` is what Pillow's ``ImageOps.exif_transpose`` does to an image whose Orientation tag is ``o``:

    1 identity            2 FLIP_LEFT_RIGHT     3 ROTATE_180          4 FLIP_TOP_BOTTOM
    5 TRANSPOSE           6 ROTATE_270          7 TRANSVERSE          8 ROTATE_90

for a row-major ``(H, W[, C])`` array.  5..8 exchange width and height.  Every one of them is: transpose first (5..8), then
reverse the columns (2, 3, 6, 7) and / or the rows (3, 4, 7, 8) — ``bits(o)``, which is how the library's kernels take them.
"""
import numpy as np

_BITS = {1: 0, 2: 1, 3: 3, 4: 2, 5: 4, 6: 5, 7: 7, 8: 6}      # bit 0: columns reversed, bit 1: rows reversed, bit 2: transposed first


def bits(o: int) -> int:
    if o not in _BITS:
        raise ValueError(f"orientation must be 1..8, not {o!r}")
    return _BITS[o]


def transposing(o: int) -> bool:
    """Does orientation ``o`` exchange width and height?"""
    return bool(bits(o) & 4)


def orient(a: np.ndarray, o: int) -> np.ndarray:
    """The row-major image ``a`` (H, W[, C]) as orientation ``o`` shows it."""
    b = bits(o)
    a = np.asarray(a)
    if b & 4:
        a = np.swapaxes(a, 0, 1)
    if b & 1:
        a = a[:, ::-1]
    if b & 2:
        a = a[::-1]
    return np.ascontiguousarray(a)


def oriented_size(o: int, width: int, height: int):
    """(width, height) of the oriented image of a stored ``width`` x ``height`` one."""
    return (height, width) if transposing(o) else (width, height)


def stored_window(o: int, width: int, height: int, window):
    """The window (x, y, w, h) of the STORED ``width`` x ``height`` image that window ``window`` = (x, y, w, h) of the oriented
    image shows: ``orient(a, o)[y:y+h, x:x+w] == orient(a[stored window], o)``."""
    x, y, w, h = (int(v) for v in window)
    b = bits(o)
    wo, ho = oriented_size(o, width, height)
    if b & 1:
        x = wo - x - w
    if b & 2:
        y = ho - y - h
    return (y, x, h, w) if b & 4 else (x, y, w, h)
