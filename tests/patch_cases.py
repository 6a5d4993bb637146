"""What the patches tests share (tests/test_patches_host.py on the CPU, tests/test_patches.py and tests/test_patches_routes.py on the
MI355X): the canvases, the specs, arrays of random bits, and the model by import.

A case is (name, (W, H), C, spec) and goes with every layout and element type.  Canvases are 48 x 36 and 45 x 33 — odd, so that a
whole canvas is no multiple of anything but 1 and 3 there —, every case has N_SOURCES = 5 sources.  All are a few KB; the
many-jobs cases, of one source each, are up to 1.4 MB."""
import numpy as np

from compose_cases import BITS, DTYPES, random_bits, shape_of  # noqa: F401
from erase_cases import LAYOUTS, same_bits, storage  # noqa: F401

CANVASES = ((48, 36), (45, 33))
N_SOURCES = 5
PATCHES = (1, 2, 3, 14, 16)
MERGES = (1, 2, 3)
# (repeat, order) in turn over the grid: "hwc" goes with repeat 1 only
FORMS = ((1, "chw"), (2, "chw"), (1, "hwc"))


def five_windows(W: int, H: int, u: int):
    """five windows of multiples of ``u`` = patch * merge on a W x H canvas: one at the odd origin (5, 3) as large as fits, a single
    merge block, a single band, a single block column, and the first once more — two sources with the same window.  None where not
    even one block fits the canvas."""
    if u > W or u > H:
        return None
    ox, oy = (5, 3) if u <= W - 5 and u <= H - 3 else (0, 0)
    big = (ox, oy, (W - ox) // u * u, (H - oy) // u * u)
    at = lambda x, y: (x if x + u <= W else 0, y if y + u <= H else 0)                      # noqa: E731
    bx, by = at(3, 1)
    cx, cy = at(2, 0)
    return [big, at(1, 2) + (u, u), (bx, by, (W - bx) // u * u, u), (cx, cy, u, (H - cy) // u * u), big]


def tokens_in(spec, size):
    """tokens per source of a spec on a canvas of ``size``"""
    P = spec["patch"]
    wins = spec.get("windows") or [None] * N_SOURCES
    return [(size[0] // P) * (size[1] // P) if w is None else (w[2] // P) * (w[3] // P) for w in wins]


def all_cases():
    """[(name, (W, H), C, spec)]"""
    out, idx = [], 0
    # the base grid: every patch x merge that fits, on both canvases; repeat, order and the component count in turn
    for W, H in CANVASES:
        for P in PATCHES:
            for m in MERGES:
                wins = five_windows(W, H, P * m)
                if wins is None:                        # (14 x 3 and 16 x 3 are taller than both canvases)
                    continue
                t, order = FORMS[idx % 3]
                C = (1, 3)[(idx // 3 + idx) % 2]
                out.append((f"grid_{W}x{H}_p{P}_m{m}_t{t}_{order}_c{C}", (W, H), C, dict(patch=P, merge=m, repeat=t, order=order, windows=wins)))
                idx += 1
    # whole canvases: windows None, and a None among windows
    for P, m, t, order, C in [(1, 1, 1, "chw", 3), (2, 2, 2, "chw", 1), (3, 1, 1, "hwc", 3), (4, 3, 1, "chw", 3), (6, 2, 1, "hwc", 1), (12, 1, 2, "chw", 3)]:
        out.append((f"whole_p{P}_m{m}_t{t}_{order}_c{C}", (48, 36), C, dict(patch=P, merge=m, repeat=t, order=order)))
    out.append(("whole_odd_canvas_p3", (45, 33), 3, dict(patch=3, merge=1, order="hwc", windows=None)))
    out.append(("none_among_windows", (48, 36), 3, dict(patch=2, merge=3, repeat=2, windows=[None, (5, 3, 12, 6), None, (1, 1, 6, 30), (42, 30, 6, 6)])))
    # token rows whose byte length is no multiple of 16 in uint8: 27, 196 and 588 bytes, rows at every alignment
    for P, C, order in [(3, 3, "chw"), (3, 3, "hwc"), (14, 1, "chw"), (14, 3, "chw"), (14, 3, "hwc")]:
        out.append((f"row_bytes_p{P}_c{C}_{order}", (45, 33), C, dict(patch=P, order=order, windows=five_windows(45, 33, P))))
    # padded: length the longest source's (one source has no pad rows), and well above it
    for P, m, t, order, C in [(2, 2, 1, "chw", 3), (3, 1, 1, "hwc", 3), (14, 1, 2, "chw", 1)]:
        spec = dict(patch=P, merge=m, repeat=t, order=order, windows=five_windows(45, 33, P * m))
        longest = max(tokens_in(spec, (45, 33)))
        out.append((f"padded_exact_p{P}_m{m}_{order}", (45, 33), C, dict(spec, length=longest)))
        out.append((f"padded_long_p{P}_m{m}_{order}", (45, 33), C, dict(spec, length=longest * 2 + 37)))
    out.append(("padded_whole", (48, 36), 1, dict(patch=4, merge=3, length=200)))
    # Qwen2-VL's real shape: patch 14, merge 2, repeat 2; 56 x 84 windows (3 x 2 merge blocks)
    out.append(("qwen", (61, 90), 3, dict(patch=14, merge=2, repeat=2, windows=[(0, 0, 56, 84), (5, 3, 56, 84), (4, 6, 56, 56), (1, 0, 28, 84), (5, 3, 56, 84)])))
    return out


def many_jobs_cases():
    """[(name, (W, H), C, dtype, spec)], one source each: a band of 1.4 MB, which is many jobs whatever a job holds; many bands; and
    a merge block of exactly 65536 bytes, the most a job's range can be"""
    return [("wide", (4201, 29), 3, "float32", dict(patch=14, merge=2, windows=[(1, 1, 4200, 28)])),
            ("tall", (29, 2801), 3, "float32", dict(patch=14, merge=2, windows=[(1, 1, 28, 2800)])),
            ("largest_block", (131, 130), 1, "float32", dict(patch=64, merge=2, windows=[(3, 1, 128, 128)])),
            ("largest_block_hwc_u8", (257, 258), 1, "uint8", dict(patch=64, merge=4, order="hwc", windows=[(1, 2, 256, 256)]))]


def model_patchify(pre: np.ndarray, spec, layout: str) -> np.ndarray:
    from tools import patch_model
    return patch_model.patchify(pre, spec, layout)


def full_windows(spec, size, n: int = N_SOURCES):
    """the spec with every window written out (None: the whole canvas), as the C calls take it"""
    wins = spec.get("windows")
    if wins is None:
        return dict(spec)
    return dict(spec, windows=[(0, 0, size[0], size[1]) if w is None else tuple(w) for w in wins])
