"""The rule of ``erase=`` (mj_plan_set_erase), restated in NumPy for one output in any of the four layouts.

torchvision's ``F.erase(img, i, j, h, w, v)`` is ``img[..., i:i+h, j:j+w] = v`` on a (C, H, W) tensor.  Here a box is
``(x, y, width, height[, value])`` with x along the width, applied to the finished output — after the mirror, in the output's
element type —, box after box, so a later box wins where two overlap.

``value``: absent or a number — every component gets it, converted as ``torch.tensor(value)`` assigned into the tensor does: to
float32 first, then to the output's type, each with one rounding to nearest even; a sequence of C numbers — one per component,
converted the same way; an array of shape (C, height, width) — one value per element, converted from ITS type with one rounding
(``v.to(dtype)``).  A uint8 output takes integers 0..255 and uint8 arrays only.

Arrays are in their storage type: uint8, float16, float32, and for bfloat16 the uint16 bit patterns (``dtype="bfloat16"`` says so;
NumPy has no such type).  No torch, no library: this is what the tests hold both against.
"""
from __future__ import annotations

import numpy as np

LAYOUTS = ("xmajor", "rowmajor", "planar", "planar_rowmajor")


def bfloat16_bits(a: np.ndarray) -> np.ndarray:
    """uint16 bit patterns of ``a`` (float16, float32 or float64) rounded ONCE, to nearest even, to bfloat16"""
    a = np.asarray(a)
    if a.dtype == np.float64:
        # one rounding from float64: to float32 rounding to odd (a sticky last bit), which the second rounding then sees through
        with np.errstate(over="ignore"):
            f = a.astype(np.float32)
        inexact = np.isfinite(f) & (f.astype(np.float64) != a)
        beyond = inexact & (np.abs(f.astype(np.float64)) > np.abs(a))
        f = np.where(beyond, np.nextafter(f, np.float32(0)), f).astype(np.float32)       # truncated toward zero
        bits = f.view(np.uint32) | inexact.astype(np.uint32)
    else:
        bits = a.astype(np.float32).view(np.uint32)
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    rounded = ((bits.astype(np.uint64) + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(nan, ((bits >> 16) | 0x40).astype(np.uint16), rounded)


def to_storage(a, dtype: str) -> np.ndarray:
    """``a`` (an array of numbers of any NumPy type) as elements of the output type ``dtype``, one rounding"""
    a = np.asarray(a)
    if dtype == "uint8":
        if a.dtype != np.uint8 and not np.array_equal(a, np.clip(np.round(a), 0, 255)):
            raise ValueError("a uint8 output takes integers 0..255")
        return a.astype(np.uint8)
    if dtype == "bfloat16":
        return bfloat16_bits(a)
    with np.errstate(over="ignore"):
        return a.astype(np.dtype(dtype))


def chw_view(out: np.ndarray, layout: str) -> np.ndarray:
    """the (C, H, W) view of one output in ``layout`` (a one-component output has no component axis)"""
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}")
    if out.ndim == 2:
        return (out if layout in ("rowmajor", "planar_rowmajor") else out.T)[None]
    return {"xmajor": out.transpose(2, 1, 0), "rowmajor": out.transpose(2, 0, 1), "planar": out.transpose(0, 2, 1),
            "planar_rowmajor": out}[layout]


def box_value(value, C: int, h: int, w: int, dtype: str) -> np.ndarray:
    """the (C, h, w) block of storage elements a box's value stands for"""
    if value is None:
        value = 0
    v = np.asarray(value) if not isinstance(value, np.ndarray) else value
    if v.ndim == 0 or v.ndim == 1:
        # numbers: float32 first (torch.tensor(value)), then the output's type
        if v.ndim == 1 and v.shape[0] != C:
            raise ValueError(f"{v.shape[0]} values for {C} component(s)")
        if dtype != "uint8":
            with np.errstate(over="ignore"):
                v = v.astype(np.float64).astype(np.float32)
        per = to_storage(v.reshape(-1), dtype)
        return np.broadcast_to(per.reshape(-1, 1, 1), (C, h, w))
    if v.shape != (C, h, w):
        raise ValueError(f"values of shape {v.shape} for a box of {(C, h, w)}")
    if dtype == "uint8" and v.dtype != np.uint8:
        raise ValueError("a uint8 output takes uint8 arrays")
    return to_storage(v, dtype)


def erase(out: np.ndarray, boxes, layout: str, dtype: str = None) -> np.ndarray:
    """``out`` — one output in ``layout``, storage type — with ``boxes`` (None, one box or a list of boxes) applied in order; a copy"""
    res = np.array(out, copy=True)
    if boxes is None:
        return res
    if isinstance(boxes, tuple):
        boxes = [boxes]
    dtype = dtype or res.dtype.name
    img = chw_view(res, layout)
    C, H, W = img.shape
    for b in boxes:
        x, y, w, h = (int(t) for t in b[:4])
        if w < 1 or h < 1 or x < 0 or y < 0 or x + w > W or y + h > H:
            raise ValueError(f"box {b[:4]} not inside {W} x {H}")
        img[:, y:y + h, x:x + w] = box_value(b[4] if len(b) > 4 else None, C, h, w, dtype)
    return res
