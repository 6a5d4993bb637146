"""Writes the two checkerboard fixtures of tests/test_affine_paths*.py under tests/golden/affine/:

    checker_48x40_444.jpg     three components, no subsampling
    checker_48x40_grey.jpg    one component

Each is a 48 x 40 black and white checkerboard of 8 x 8-pixel cells — the cells are the JPEG blocks, so at quality 100 every
decoded value lies at 0 or at 255 within the quantisation's rounding — which a bicubic transform overshoots on both sides at every
cell edge: the input that makes the transform's clamp to 0 and 255 busy in ONE component too, where photographic files almost
never clamp.  Written with Pillow (12.2 wrote the committed files); the tests decode them with the oracle and hold the pixels to
"at least 40 % at most 3, at least 40 % at least 252", so a rewrite with another encoder that keeps that is as good.

    python tools/make_affine_fixtures.py
"""
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "affine"
W, H, CELL = 48, 40, 8


def checkerboard() -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    return (((x // CELL + y // CELL) & 1) * 255).astype(np.uint8)


def main():
    from PIL import Image
    OUT.mkdir(parents=True, exist_ok=True)
    board = checkerboard()
    Image.fromarray(np.stack([board] * 3, axis=-1)).save(OUT / "checker_48x40_444.jpg", quality=100, subsampling=0)
    Image.fromarray(board).save(OUT / "checker_48x40_grey.jpg", quality=100)
    for p in sorted(OUT.glob("*.jpg")):
        print(p.name, p.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
