"""What the erase tests share (tests/test_erase_host.py on the CPU, tests/test_erase.py and tests/test_erase_routes.py on the MI355X):
the box list, the values that go with it, and the storage views (bit patterns) both sides are compared in."""
import numpy as np

LAYOUTS = ("xmajor", "rowmajor", "planar", "planar_rowmajor")          # by MJ_LAYOUT_* value
DTYPES = ("uint8", "float16", "float32", "bfloat16")
STORAGE = {"uint8": np.uint8, "float16": np.float16, "float32": np.float32, "bfloat16": np.uint16}


def box_cases(W: int, H: int):
    """{name: the boxes (x, y, width, height) of ONE output} on a W x H canvas"""
    return {
        "1x1": [(4, 3, 1, 1)],
        "1xh": [(3, 2, 1, H - 4)],
        "wx1": [(2, 3, W - 4, 1)],
        "whole": [(0, 0, W, H)],
        "corner_tl": [(0, 0, 3, 2)],
        "corner_tr": [(W - 3, 0, 3, 2)],
        "corner_bl": [(0, H - 2, 3, 2)],
        "corner_br": [(W - 3, H - 2, 3, 2)],
        "odd_x_odd_width": [(5, 4, 7, 5)],
        "disjoint": [(1, 1, 4, 3), (10, 8, 5, 4)],
        "overlap": [(2, 2, 8, 6), (6, 5, 9, 7)],
        "overlap_reversed": [(6, 5, 9, 7), (2, 2, 8, 6)],
    }


def shape_of(layout: str, W: int, H: int, C: int):
    """one output's shape as a decoder of ``layout`` returns it (a one-component output has no component axis)"""
    wh = (W, H) if layout in ("xmajor", "planar") else (H, W)
    if C == 1:
        return wh
    return (C,) + wh if layout.startswith("planar") else wh + (C,)


def value_for(j: int, C: int, w: int, h: int, dtype: str, rng, kind: str):
    """box j's value of ``kind``: "number", "per_component" or "values" ((C, h, w): uint8 for a uint8 output, else float32)"""
    if kind == "number":
        return (37 + 11 * j) if dtype == "uint8" else 0.1 * (j + 1) - 0.25
    if kind == "per_component":
        return [(200 - 30 * c - j) for c in range(C)] if dtype == "uint8" else [0.3 * c - 0.1 * j + 0.123456789 for c in range(C)]
    if dtype == "uint8":
        return rng.integers(0, 256, size=(C, h, w)).astype(np.uint8)
    return rng.standard_normal(size=(C, h, w)).astype(np.float32)


def with_values(boxes, C: int, dtype: str, seed: int, kinds=("number", "per_component", "values")):
    """the boxes with values: box j gets kind j mod len(kinds)"""
    rng = np.random.default_rng(seed)
    return [(x, y, w, h, value_for(j, C, w, h, dtype, rng, kinds[j % len(kinds)])) for j, (x, y, w, h) in enumerate(boxes)]


def storage(t, dtype: str = None) -> np.ndarray:
    """a result — NumPy array, or torch tensor wherever it lives — in its storage type: uint8, float16, float32, or the uint16 bit
    patterns of bfloat16"""
    if isinstance(t, np.ndarray):
        return t
    import torch
    t = t.detach().cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """equal as bit patterns (floats: -0.0 is not 0.0, a NaN equals itself)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def model_outputs(base: np.ndarray, erase, layout: str, dtype: str) -> np.ndarray:
    """the model applied output by output to ``base`` (storage type), the call's result without ``erase``"""
    from tools import erase_model
    out = np.array(base, copy=True)
    for k, boxes in enumerate(erase):
        if boxes:
            boxes = [boxes] if isinstance(boxes, tuple) else boxes
            conv = [b[:4] + ((storage(b[4]),) if len(b) > 4 and hasattr(b[4], "shape") else b[4:]) for b in boxes]
            # (values that are bfloat16 tensors come as bit patterns: put them back through float32, which holds them exactly)
            conv = [b[:4] + ((np.left_shift(b[4].astype(np.uint32), 16).view(np.float32),) if len(b) > 4 and isinstance(b[4], np.ndarray) and b[4].dtype == np.uint16 else b[4:])
                    for b in conv]
            out[k] = erase_model.erase(out[k], conv, layout, dtype)
    return out
