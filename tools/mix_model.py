"""The rule of ``mix=`` (mj_mix), restated in NumPy for the outputs of one call in any of the four layouts.

MixUp and CutMix as torchvision's and timm's collate functions do them, on the finished outputs — behind the mirror, the element
type and ``erase=``.  One entry per output: None, ``("mixup", partner, lam)`` or ``("cutmix", partner, (x, y, width, height))``;
``partner`` is the index of an output of the same call (it may be the output itself), and EVERY output reads the array as it
stands before any mixing — the mixing is simultaneous, as it is where the collate functions mix from a ``roll`` / ``flip`` copy.

cutmix: ``out[k] = pre[k]`` with elements ``[..., y:y+height, x:x+width]`` replaced by ``pre[partner]``'s; any element type.

mixup (float types): with ``ws = float32(lam)`` and ``wp = float32(1.0 - lam)`` — the subtraction in double, then ONE rounding —,
element-wise ``out = T(f32(T(f32(pre[partner]) * wp)) + f32(T(f32(pre[k]) * ws)))``, T rounding to nearest even into the element
type and every float32 operation rounded on its own.  That is what ``pre.roll(1, 0).mul(1.0 - lam).add_(pre.mul(lam))`` and timm's
``x.flip(0).mul_(1. - lam)`` / ``x.mul_(lam).add_(..)`` compute with torch's CPU ops, bit for bit, in float32, float16 and
bfloat16 (tests/test_mix_host.py): torch computes a half-precision product or sum in float32 and rounds it once.  ``partner == k``
still runs the arithmetic.  A NaN result is some NaN.

Arrays are in their storage type: uint8, float16, float32, and for bfloat16 the uint16 bit patterns (``dtype="bfloat16"`` says so).
No torch, no library: this is what the tests hold both against.
"""
from __future__ import annotations

import math

import numpy as np

from tools.erase_model import LAYOUTS, bfloat16_bits, chw_view

__all__ = ["LAYOUTS", "mix", "mixup_elements", "weights"]


def weights(lam: float):
    """(ws, wp): the output's own weight and its partner's, as float32"""
    lam = float(lam)
    if not math.isfinite(lam) or not 0.0 <= lam <= 1.0:
        raise ValueError(f"lam {lam!r} is not a finite number in 0..1")
    return np.float32(lam), np.float32(1.0 - lam)


def _to_f32(a: np.ndarray, dtype: str) -> np.ndarray:
    if dtype == "bfloat16":
        return np.left_shift(a.astype(np.uint32), 16).view(np.float32)
    return a.astype(np.float32)


def _to_storage(f: np.ndarray, dtype: str) -> np.ndarray:
    if dtype == "bfloat16":
        return bfloat16_bits(f)
    with np.errstate(over="ignore"):
        return f.astype(np.dtype(dtype))


def mixup_elements(own: np.ndarray, partner: np.ndarray, lam: float, dtype: str) -> np.ndarray:
    """the three operations on storage arrays of the float type ``dtype``"""
    if dtype not in ("float16", "float32", "bfloat16"):
        raise ValueError(f"mixup needs a float element type, not {dtype}")
    ws, wp = weights(lam)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        a = _to_f32(_to_storage(_to_f32(partner, dtype) * wp, dtype), dtype)
        b = _to_f32(_to_storage(_to_f32(own, dtype) * ws, dtype), dtype)
        return _to_storage(a + b, dtype)


def mix(pre: np.ndarray, entries, layout: str, dtype: str = None) -> np.ndarray:
    """``pre`` — the outputs of a call in ``layout``, storage type, outputs along the first axis — with ``entries`` applied, one per
    output; a new array"""
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}")
    pre = np.asarray(pre)
    dtype = dtype or pre.dtype.name
    n = pre.shape[0]
    if len(entries) != n:
        raise ValueError(f"{len(entries)} entries for {n} outputs")
    out = np.array(pre, copy=True)
    for k, e in enumerate(entries):
        if e is None:
            continue
        op, partner = e[0], e[1]
        if not (isinstance(partner, (int, np.integer)) and 0 <= int(partner) < n):
            raise ValueError(f"output {k}: partner {partner!r} is not an output 0..{n - 1}")
        if op == "mixup":
            out[k] = mixup_elements(pre[k], pre[int(partner)], e[2], dtype)
        elif op == "cutmix":
            x, y, w, h = (int(t) for t in e[2])
            img, src = chw_view(out[k], layout), chw_view(pre[int(partner)], layout)
            _, H, W = img.shape
            if w < 1 or h < 1 or x < 0 or y < 0 or x + w > W or y + h > H:
                raise ValueError(f"output {k}: box {(x, y, w, h)} not inside {W} x {H}")
            img[:, y:y + h, x:x + w] = src[:, y:y + h, x:x + w]
        else:
            raise ValueError(f"output {k}: unknown op {op!r}")
    return out
