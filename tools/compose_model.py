"""The rule of ``compose=`` (mj_compose), restated in NumPy for the outputs of one call in any of the four layouts.

Several finished outputs — behind the mirror, the element type and ``erase=`` — pasted onto one canvas: Mosaic, image grids, a crop
of one sample in another at another place.  ``outputs`` has one list of tiles per composed canvas, applied in order, so a later
tile wins where two overlap; a tile is ``(source, (dx, dy))`` or ``(source, (dx, dy), (sx, sy, w, h))``: the window (default: the
whole tile canvas, x along the width) of output ``source`` with its top-left corner at ``(dx, dy)`` of the composed canvas, which
may be negative or beyond it.  The paste is clipped to the canvas as ``Image.paste`` clips it; a tile wholly outside pastes nothing.

    out[m] = full(canvas, fill)
    for (s, (dx, dy), (sx, sy, w, h)) in outputs[m]:
        out[m][..., dy:dy+h, dx:dx+w] = pre[s][..., sy:sy+h, sx:sx+w]          # both sides clipped to the canvas

Elements are copied as they are (bit patterns), so the rule is the same in every element type; ``fill`` is one ELEMENT per
component, in the array's storage type — what a fill byte becomes under ``dtype=`` / ``normalize=`` is the caller's business.
Arrays are in their storage type: uint8, float16, float32, and for bfloat16 the uint16 bit patterns.  This pastes tile by tile and
knows nothing of the rectangles the library resolves the tiles into.  No torch, no library: what the tests hold both against.
"""
from __future__ import annotations

import numpy as np

from tools.erase_model import LAYOUTS, chw_view

__all__ = ["LAYOUTS", "compose", "canvas_shape"]


def canvas_shape(layout: str, W: int, H: int, C: int, grey_axis: bool):
    """one canvas's shape in ``layout`` (``grey_axis``: False where a one-component output has no component axis)"""
    wh = (W, H) if layout in ("xmajor", "planar") else (H, W)
    if C == 1 and not grey_axis:
        return wh
    return (C,) + wh if layout.startswith("planar") else wh + (C,)


def compose(pre: np.ndarray, outputs, size, layout: str, fill=0) -> np.ndarray:
    """``pre`` — the outputs of a call in ``layout``, storage type, outputs along the first axis — composed onto ``len(outputs)``
    canvases of ``size`` = (W, H); ``fill``: one element for all components or one per component; a new array"""
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}")
    pre = np.asarray(pre)
    W, H = (int(v) for v in size)
    first = chw_view(pre[0], layout)
    C, SH, SW = first.shape
    out = np.empty((len(outputs),) + canvas_shape(layout, W, H, C, pre[0].ndim == 3), dtype=pre.dtype)
    fills = np.broadcast_to(np.asarray(fill, dtype=pre.dtype).reshape(-1), (C,)) if np.ndim(fill) else np.full((C,), fill, dtype=pre.dtype)
    for m, tiles in enumerate(outputs):
        canvas = chw_view(out[m], layout)
        canvas[...] = fills.reshape(C, 1, 1)
        for tile in tiles:
            s, (dx, dy) = int(tile[0]), (int(v) for v in tile[1])
            sx, sy, w, h = (int(v) for v in tile[2]) if len(tile) > 2 else (0, 0, SW, SH)
            if not 0 <= s < len(pre):
                raise ValueError(f"output {m}: source {s} is not an output 0..{len(pre) - 1}")
            if w < 1 or h < 1 or sx < 0 or sy < 0 or sx + w > SW or sy + h > SH:
                raise ValueError(f"output {m}: window {(sx, sy, w, h)} not inside {SW} x {SH}")
            x0, y0, x1, y1 = max(dx, 0), max(dy, 0), min(dx + w, W), min(dy + h, H)
            if x0 >= x1 or y0 >= y1:
                continue
            src = chw_view(pre[s], layout)
            canvas[:, y0:y1, x0:x1] = src[:, sy + (y0 - dy):sy + (y1 - dy), sx + (x0 - dx):sx + (x1 - dx)]
    return out
