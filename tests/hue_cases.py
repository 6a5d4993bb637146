"""What tests/test_hue_host.py (no GPU) and tests/test_hue.py (MI355X) share: a file made at run time whose canvas takes adjust_hue
(csrc/mijpeg_internal.h: colour_rgb_to_hsv, colour_hsv_to_rgb) down every branch of its arithmetic, and the census that says which
branches a canvas reaches.

The file is tests/colour_cases.craft's kind: 4:4:4, quantisation tables that are all 8, DC-only blocks — every 8 x 8 block is flat.
Its twenty blocks are (Y, Cb, Cr) levels chosen so that the decoded blocks are the three primaries, the three secondaries (each a
tie of two components at the maximum), the colours half-way between them (the odd sextants of the hue circle), ties at the maximum
and at the minimum away from the corners of the cube, near-greys one step off the grey axis, black, white and a grey.  At the file's own size the default resize is the identity, so the canvas IS the
block pattern.  The host file holds the file to these colours with Pillow's decode and the census to the model; the GPU file asserts
the census over the library's own canvases before it compares anything.  Neither a test file nor a conftest: nothing here is
collected."""
import numpy as np

import colour_cases

# name -> ((Y, Cb, Cr) levels of the block, the RGB the block decodes to)
BLOCKS = {
    "red": ((76, 84, 255), (254, 0, 0)), "green": ((120, 0, 0), (0, 255, 0)), "blue": ((29, 255, 107), (0, 0, 254)),
    "yellow": ((226, 0, 149), (255, 255, 0)), "cyan": ((179, 171, 0), (0, 255, 255)), "magenta": ((77, 229, 255), (255, 0, 255)),
    "orange": ((142, 0, 209), (255, 128, 0)), "chartreuse": ((183, 0, 89), (128, 255, 0)), "azure": ((72, 231, 0), (0, 128, 255)),
    "rose": ((77, 157, 255), (255, 0, 128)),
    "tie_rg_max": ((182, 48, 141), (200, 200, 40)), "tie_gb_max": ((152, 155, 48), (40, 200, 200)), "tie_rb_max": ((106, 181, 195), (200, 40, 200)),
    "tie_rg_min": ((58, 208, 115), (40, 40, 200)),
    "near_grey_b": ((128, 129, 128), (128, 128, 130)), "near_grey_r": ((128, 128, 129), (129, 127, 128)), "near_grey_dark": ((3, 127, 128), (3, 3, 1)),
    "black": ((0, 128, 128), (0, 0, 0)), "white": ((255, 128, 128), (255, 255, 255)), "grey": ((128, 128, 128), (128, 128, 128)),
}
SIZE = (40, 32)                 # five by four blocks
_file = []


def raw() -> bytes:
    """the crafted file"""
    if not _file:
        ycc = [v[0] for v in BLOCKS.values()]
        _file.append(colour_cases.craft(np.array([c[0] for c in ycc]).reshape(4, 5), True, [(c[1], c[2]) for c in ycc]))
    return _file[0]


def intended() -> np.ndarray:
    """the canvas the file is meant to be, row-major (32, 40, 3)"""
    rgb = np.array([v[1] for v in BLOCKS.values()], dtype=np.uint8).reshape(4, 5, 3)
    return np.kron(rgb, np.ones((8, 8, 1), dtype=np.uint8))


CLASSES = frozenset(["max == min", "r is max", "g is max", "b is max", "r == g == max", "g == b == max", "r == b == max"] +
                    [f"i % 6 == {k}" for k in range(6)])


def census(canvases, shift: int) -> set:
    """the classes of CLASSES that the pixels of these row-major (H, W, 3) canvases reach under adjust_hue with this shift: the
    branches of the first conversion by the bytes, those of the second by the model's H and S bytes after the shift"""
    from tools import colour_model
    px = np.concatenate([np.asarray(c).reshape(-1, 3) for c in canvases]).astype(np.int32)
    r, g, b = px[:, 0], px[:, 1], px[:, 2]
    mx, mn = px.max(axis=1), px.min(axis=1)
    found = set()
    colour = mx != mn
    for name, hit in (("max == min", ~colour), ("r is max", colour & (r == mx)), ("g is max", colour & (r != mx) & (g == mx)),
                      ("b is max", colour & (r != mx) & (g != mx)), ("r == g == max", colour & (r == mx) & (g == mx)),
                      ("g == b == max", colour & (g == mx) & (b == mx)), ("r == b == max", colour & (r == mx) & (b == mx))):
        if hit.any():
            found.add(name)
    hsv = colour_model.rgb_to_hsv(px.astype(np.uint8))
    assert ((hsv[:, 1] == 0) == ~colour).all()          # (S is 0 for the greys alone: the second conversion's first branch is "max == min")
    h = ((hsv[:, 0].astype(np.int32) + shift) & 255)[hsv[:, 1] != 0]
    for k in np.unique(np.floor(h.astype(np.float32).astype(np.float64) * 6.0 / 255.0).astype(np.int64) % 6):
        found.add(f"i % 6 == {int(k)}")
    return found
