"""What `decode(..., size=..., views=[...])` computes, restated: the meaning of a call with views in terms of calls without them,
and in terms of Pillow.

A call with views names its OUTPUTS: output k is a window of file i_k.  It is, byte for byte, output 0 of the call on the one
file `files[i_k]` with `rois=[window_k]`, the k-th entry of every per-output argument (`mirror`, the list forms of `resize_to` and
`place`), the file's own entry of every per-file argument (`orientation`) and every other argument as given: `equivalent_calls`.
The library decodes every file once and runs one resize record per view; the equivalent calls decode a file once per view.  That
is the whole difference, and it is not one of bytes.

In Pillow's terms (`expected`, a NumPy model on the pixels a plain decode gives — tools/orient_model.py, mode_model.py,
reduce_model.py and place_model.py hold the pieces to Pillow themselves):

    exif_transpose(img.convert(mode)).crop(window).resize(target, filter[, reducing_gap=g])

placed on the canvas `size` (target = `size` without `resize_to`), mirrored if `mirror[k]`.  Taps stop at the window's edge — this
is crop().resize(), not resize(box=) — and under `reducing_gap` the factors come from the window's size and the cell grid starts
at the window's origin.  The output table (dtype, normalize) applies to the finished bytes as ever (tools/normalize_model.py).

`pillow_expression` is the same thing through Pillow itself, for tests that have it."""
import numpy as np

from tools import mode_model, orient_model, place_model, reduce_model

_PER_OUTPUT = ("mirror", "resize_to", "place")       # list forms: one entry per view
_PER_FILE = ("orientation",)                         # list forms: one entry per file


def normal_views(views, dims):
    """[(file, (x, y, width, height))] of a `views` argument; dims: every file's (width, height) as its orientation shows it"""
    out = []
    for v in views:
        i, r = (v, None) if isinstance(v, (int, np.integer)) else v
        out.append((int(i), tuple(int(t) for t in r) if r is not None else (0, 0) + tuple(dims[int(i)])))
    return out


def equivalent_calls(files, views, **kwargs):
    """One (files, kwargs) per output: the call without views whose output 0 is output k of `decode(files, views=views, **kwargs)`.
    kwargs: the call's other keyword arguments (`size` among them).  Per-output lists give their k-th entry, per-file lists the
    entry of the view's file; a bare file index or a None window makes `rois=None`."""
    calls = []
    for k, v in enumerate(views):
        i, r = (v, None) if isinstance(v, (int, np.integer)) else v
        kw = dict(kwargs)
        for name in _PER_OUTPUT:
            if isinstance(kw.get(name), list):
                kw[name] = [kw[name][k]]
        for name in _PER_FILE:
            if isinstance(kw.get(name), (list, tuple)):
                kw[name] = [kw[name][int(i)]]
        kw["rois"] = [tuple(r)] if r is not None else None
        calls.append(([files[int(i)]], kw))
    return calls


def expected(pixels_rm: np.ndarray, window, size, filter: str = "bilinear", orientation: int = 1, mode=None, reducing_gap=None,
             mirror: bool = False, resized=None, xy=(0, 0), fill=0) -> np.ndarray:
    """One view's bytes, row-major (height, width[, C]): `pixels_rm` are the file's pixels as a plain decode gives them (stored
    order, the file's own components); window None: the whole oriented image.  resized / xy / fill: the view's place on the canvas
    `size` (None: stretched over all of it)."""
    a = orient_model.orient(mode_model.convert(pixels_rm, mode), orientation)
    if window is not None:
        x, y, w, h = window
        a = a[y:y + h, x:x + w]
    target = tuple(resized) if resized is not None else tuple(size)
    if reducing_gap is not None:
        out = reduce_model.resize(a, target, filter, reducing_gap)
        if target != tuple(size) or tuple(xy) != (0, 0):
            canvas = np.empty((size[1], size[0]) + out.shape[2:], dtype=np.uint8)
            canvas[...] = np.asarray(fill, dtype=np.uint8)
            x0, y0 = xy
            ys, xs = slice(max(0, y0), min(size[1], y0 + target[1])), slice(max(0, x0), min(size[0], x0 + target[0]))
            canvas[ys, xs] = out[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0]
            out = canvas
    else:
        out = place_model.place(a, target, xy, size, fill, filter)
    return out[:, ::-1] if mirror else out


def pillow_expression(img, window, size, filter: str = "bilinear", orientation: int = 1, mode=None, reducing_gap=None, mirror: bool = False):
    """exif_transpose(img.convert(mode)).crop(window).resize(size, filter[, reducing_gap=g]) of a PIL image, then the mirror — as
    a NumPy array.  (orientation is applied as the transpose exif_transpose would apply for that tag.)"""
    from PIL import Image
    turns = {2: Image.Transpose.FLIP_LEFT_RIGHT, 3: Image.Transpose.ROTATE_180, 4: Image.Transpose.FLIP_TOP_BOTTOM, 5: Image.Transpose.TRANSPOSE,
             6: Image.Transpose.ROTATE_270, 7: Image.Transpose.TRANSVERSE, 8: Image.Transpose.ROTATE_90}
    if mode is not None:
        img = img.convert(mode)
    if orientation in turns:
        img = img.transpose(turns[orientation])
    if window is not None:
        x, y, w, h = window
        img = img.crop((x, y, x + w, y + h))
    img = img.resize(tuple(size), getattr(Image.Resampling, filter.upper()), reducing_gap=reducing_gap)
    out = np.asarray(img)
    return out[:, ::-1] if mirror else out
