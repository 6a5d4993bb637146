"""Aspect-preserving sizing, restated from the libraries (NumPy only): every image is resized to a size of ITS OWN, and the
resized image is placed at an offset on a canvas of one fixed size; canvas pixels it does not cover hold a fill value.

    kind int s       torchvision's Resize(s) then center_crop: the shorter side becomes s, the longer int(s * long / short)
                     (Python arithmetic: an integer product, one true division, truncation); per axis an image at least as
                     large as the canvas is cropped at int(round((r - c) / 2.0)) — Python's round, half to even — and a
                     smaller one padded with (c - r) // 2 in front.
    kind (w, h)      that resized size for every file, centred as for an int.
    kind "contain"   Pillow's ImageOps.contain / ImageOps.pad with centering 0.5: the image fits inside the canvas — the other
                     side is round(h / w * W) or round(w / h * H), float ratios, half to even — and sits at
                     round((c - r) * 0.5) along the axis that differs.

place() is tools/resize_model.py's resize pasted on the canvas.  tests/test_place_host.py pins all of it to Pillow.
"""
import numpy as np

try:
    from . import resize_model
except ImportError:          # run as a script from tools/
    import resize_model


def resized_size(kind, w: int, h: int, canvas):
    """(width, height) an image of w x h is resized to under ``kind`` on a canvas (width, height).  A side of 0 is returned as
    it comes out: the caller refuses it, naming the file."""
    w, h = int(w), int(h)
    if isinstance(kind, str):
        if kind != "contain":
            raise ValueError(f"kind must be an int, (width, height) or 'contain', not {kind!r}")
        cw, ch = int(canvas[0]), int(canvas[1])
        im_ratio, dest_ratio = w / h, cw / ch
        if im_ratio == dest_ratio:
            return cw, ch
        if im_ratio >= dest_ratio:
            return cw, round(h / w * cw)
        return round(w / h * ch), ch
    if isinstance(kind, (tuple, list)):
        return int(kind[0]), int(kind[1])
    s = int(kind)
    short, long = sorted((w, h))
    new_short, new_long = s, int(s * long / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


def centred(kind, resized, canvas):
    """(x, y) of the resized image's top-left on the canvas under ``kind``'s centring rule."""
    out = []
    for r, c in zip(resized, canvas):
        r, c = int(r), int(c)
        if kind == "contain":
            out.append(round((c - r) * 0.5))
        elif r >= c:
            out.append(-int(round((r - c) / 2.0)))
        else:
            out.append((c - r) // 2)
    return tuple(out)


def place(img_rm: np.ndarray, resized, xy, canvas, fill=0, filter: str = "bilinear") -> np.ndarray:
    """img_rm: uint8 (H, W) or (H, W, C), row-major.  Returns the canvas (height, width[, C]): ``fill`` (one byte, or one per
    component) everywhere but where resize(img_rm, resized, filter) lies with its top-left at xy = (x, y) — either may be
    negative (the image is cropped there) or positive (padded)."""
    img_rm = np.asarray(img_rm, dtype=np.uint8)
    rw, rh = int(resized[0]), int(resized[1])
    cw, ch = int(canvas[0]), int(canvas[1])
    x, y = int(xy[0]), int(xy[1])
    small = resize_model.resize(img_rm, (rw, rh), filter)
    out = np.empty((ch, cw) + img_rm.shape[2:], dtype=np.uint8)
    out[...] = np.asarray(fill, dtype=np.uint8)
    x0, x1, y0, y1 = max(x, 0), min(x + rw, cw), max(y, 0), min(y + rh, ch)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = small[y0 - y:y1 - y, x0 - x:x1 - x]
    return out
