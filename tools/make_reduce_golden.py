"""Writes tests/golden/reduce_blocks.npz with Pillow: small random images, the arguments and what Pillow made of them —
Image.reduce((fx, fy)) and Image.resize(size, filter, reducing_gap=g) — so that tools/reduce_model.py stays pinned where Pillow is
not installed (tests/test_reduce_host.py).  Run once; the file is committed.

    python -m tools.make_reduce_golden
"""
from pathlib import Path

import numpy as np

from tools import reduce_model

FILTERS = ("bilinear", "box", "hamming", "bicubic", "lanczos")


def main():
    from PIL import Image
    pil = {"bilinear": Image.BILINEAR, "box": Image.BOX, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
    rng = np.random.default_rng(20250215)
    out = {}
    reduce_args = []
    for k, (w, h, nc, fx, fy) in enumerate(((37, 29, 3, 4, 4), (70, 50, 3, 4, 3), (64, 31, 1, 2, 2), (50, 41, 1, 7, 1), (33, 65, 3, 1, 5),
                                             (128, 17, 3, 32, 16), (61, 47, 1, 3, 3), (300, 5, 1, 291, 2), (25, 26, 3, 5, 13))):
        a = rng.integers(0, 256, (h, w, 3) if nc == 3 else (h, w), dtype=np.uint8)
        out[f"reduce_in_{k}"] = a
        out[f"reduce_out_{k}"] = np.asarray(Image.fromarray(a).reduce((fx, fy)))
        reduce_args.append((fx, fy))
    out["reduce_args"] = np.asarray(reduce_args, dtype=np.int32)
    resize_args = []
    k = 0
    for f, name in enumerate(FILTERS):
        for gap in (1.0, 1.5, 2.0, 3.0):
            w, h = int(rng.integers(30, 90)), int(rng.integers(30, 90))
            ow, oh = int(rng.integers(2, 7)), int(rng.integers(2, 7))
            nc = 3 if (k % 2) else 1
            fx, fy = reduce_model.reduce_factors(w, h, ow, oh, gap)
            assert (fx > 1 or fy > 1) and not reduce_model.tall(-(-w // fx), -(-h // fy), oh)
            a = rng.integers(0, 256, (h, w, 3) if nc == 3 else (h, w), dtype=np.uint8)
            out[f"resize_in_{k}"] = a
            out[f"resize_out_{k}"] = np.asarray(Image.fromarray(a).resize((ow, oh), pil[name], reducing_gap=gap))
            resize_args.append((ow, oh, f, gap))
            k += 1
    out["resize_args"] = np.asarray(resize_args, dtype=np.float64)
    path = Path(__file__).resolve().parent.parent / "tests" / "golden" / "reduce_blocks.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
