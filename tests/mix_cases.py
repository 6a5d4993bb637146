"""What the mix tests share (tests/test_mix_host.py on the CPU, tests/test_mix.py and tests/test_mix_routes.py on the MI355X): the
pairings, the lam values, the boxes, and — by import — the storage views (bit patterns) both sides are compared in."""
import numpy as np

from erase_cases import DTYPES, LAYOUTS, STORAGE, box_cases, same_bits, shape_of, storage  # noqa: F401

FLOATS = ("float16", "float32", "bfloat16")


def beta_draw() -> float:
    """one Beta(0.8, 0.8) draw, timm's mixup_alpha = 0.8 (a fixed seed: the same number every run)"""
    return float(np.random.default_rng(8).beta(0.8, 0.8))


# 1e-5 puts float16 products into the subnormal range
LAMS = (0.0, 1.0, 0.3, 0.5, beta_draw(), 1e-5)


def pairings(n: int):
    """{name: partner of output k, for k in 0..n-1}: torchvision's roll(1, 0), timm's flip(0), every output its own partner, and a
    permutation with a 3-cycle (n >= 4: 0 -> 2 -> 1 -> 0, the rest swapped pairwise or fixed)"""
    cyc = list(range(n))
    if n >= 3:
        cyc[0], cyc[2], cyc[1] = 2, 1, 0
    for k in range(3, n - 1, 2):
        cyc[k], cyc[k + 1] = k + 1, k
    return {"roll": [(k - 1) % n for k in range(n)], "flip": [n - 1 - k for k in range(n)], "self": list(range(n)), "cycle3": cyc}


def single_boxes(W: int, H: int):
    """{name: (x, y, width, height)}: box_cases' single boxes"""
    return {name: boxes[0] for name, boxes in box_cases(W, H).items() if len(boxes) == 1}


def entries_for(n: int, partners, W: int, H: int, dtype: str, seed: int = 0):
    """one entry per output, kinds in turn — mixup / None / cutmix / mixup … (cutmix in the place of mixup for a uint8 output) —,
    lam values and boxes taken in turn from LAMS and the single boxes"""
    boxes = list(single_boxes(W, H).values())
    out = []
    for k in range(n):
        kind = ("mixup", None, "cutmix", "mixup")[k % 4]
        if kind is None:
            out.append(None)
        elif kind == "mixup" and dtype != "uint8":
            out.append(("mixup", partners[k], LAMS[(k + seed + 2) % len(LAMS)]))
        else:
            out.append(("cutmix", partners[k], boxes[(k + seed) % len(boxes)]))
    return out


def model_mix(base: np.ndarray, entries, layout: str, dtype: str) -> np.ndarray:
    from tools import mix_model
    return mix_model.mix(base, entries, layout, dtype)
