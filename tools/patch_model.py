"""The rule of ``patches=`` (mj_patchify), restated in NumPy for the outputs of one call in any of the four layouts.

The finished outputs — behind erase, mix or compose — cut into P x P patches and packed as the token rows of a native-resolution
vision encoder.  Source k's window ``(x, y, width, height)`` (None: its whole canvas), as ``img`` = (C, h, w), has gh = h / P by
gw = w / P patches; with m = ``merge`` and t = ``repeat``

    row  = cu[k] + ((py // m) * (gw // m) + px // m) * m * m + (py % m) * m + px % m       # patch (py, px) of source k
    chw:  out[row, ((c * t + r) * P + j) * P + i] = img[c, py * P + j, px * P + i]          for r in 0 .. t - 1
    hwc:  out[row, (j * P + i) * C + c]           = img[c, py * P + j, px * P + i]

whatever the layout of the arrays.  ``length`` None: the packed form, one (T, D) array, cu[k] the tokens of the sources before k.
``length`` L: the padded form (N, L, D), cu[k] = k * L, the rows behind a source's tokens zero.  Elements are copied as they are
(bit patterns); arrays are in their storage type: uint8, float16, float32, and for bfloat16 the uint16 bit patterns.  This knows
nothing of the jobs the library cuts the output into.  No torch, no library: what the tests hold both against.
"""
from __future__ import annotations

import numpy as np

from tools.erase_model import LAYOUTS, chw_view

__all__ = ["LAYOUTS", "patchify", "token_rows", "tokens_of"]


def token_rows(gh: int, gw: int, m: int) -> np.ndarray:
    """(gh, gw): the row, within its source, of patch (py, px) — merge blocks of m x m patches in raster order, raster inside one"""
    py, px = np.meshgrid(np.arange(gh), np.arange(gw), indexing="ij")
    return ((py // m) * (gw // m) + px // m) * m * m + (py % m) * m + px % m


def tokens_of(img: np.ndarray, P: int, m: int = 1, t: int = 1, order: str = "chw") -> np.ndarray:
    """the (gh * gw, D) token rows of one window ``img`` = (C, h, w)"""
    C, h, w = img.shape
    if order not in ("chw", "hwc") or (order == "hwc" and t != 1):
        raise ValueError(f"order {order!r} with repeat {t}")
    if h % (P * m) or w % (P * m) or h < 1 or w < 1:
        raise ValueError(f"a {w} x {h} window is no multiple of patch * merge = {P * m}")
    gh, gw = h // P, w // P
    cut = img.reshape(C, gh, P, gw, P)                                  # [c, py, j, px, i]
    if order == "chw":
        tok = np.broadcast_to(cut.transpose(1, 3, 0, 2, 4)[:, :, :, None], (gh, gw, C, t, P, P))
    else:
        tok = cut.transpose(1, 3, 2, 4, 0)                              # [py, px, j, i, c]
    out = np.empty((gh * gw, C * t * P * P), dtype=img.dtype)
    out[token_rows(gh, gw, m).reshape(-1)] = tok.reshape(gh * gw, -1)
    return out


def patchify(pre: np.ndarray, spec: dict, layout: str) -> np.ndarray:
    """``pre`` — the outputs of a call in ``layout``, storage type, outputs along the first axis — as the token rows of ``spec``
    (``patch``, and ``merge``, ``repeat``, ``order``, ``windows``, ``length`` with their defaults); a new array"""
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}")
    pre = np.asarray(pre)
    P, m, t = int(spec["patch"]), int(spec.get("merge", 1)), int(spec.get("repeat", 1))
    order, length, windows = spec.get("order", "chw"), spec.get("length"), spec.get("windows")
    if windows is not None and len(windows) != len(pre):
        raise ValueError(f"{len(windows)} windows for {len(pre)} sources")
    rows = []
    for k in range(len(pre)):
        img = chw_view(pre[k], layout)
        C, H, W = img.shape
        x, y, w, h = (0, 0, W, H) if windows is None or windows[k] is None else (int(v) for v in windows[k])
        if x < 0 or y < 0 or w < 1 or h < 1 or x + w > W or y + h > H:
            raise ValueError(f"source {k}: window {(x, y, w, h)} not inside {W} x {H}")
        rows.append(tokens_of(img[:, y:y + h, x:x + w], P, m, t, order))
    if length is None:
        return np.concatenate(rows, axis=0)
    out = np.zeros((len(pre), int(length), rows[0].shape[1]), dtype=pre.dtype)
    for k, r in enumerate(rows):
        if len(r) > length:
            raise ValueError(f"source {k}: {len(r)} tokens, more than length {length}")
        out[k, :len(r)] = r
    return out
