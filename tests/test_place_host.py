"""Aspect-preserving sizing (resize_to= / place= / fill=), the parts that need no GPU: tools/place_model.py's rules are the
libraries' — the pinned cases of torchvision's Resize + center_crop and of Pillow's ImageOps.contain / pad — and its canvases are
Pillow's, byte for byte, for every source size 1..40 x 1..40 and the golden files' sizes; the package's own rules
(batch.resized_size / centred / normalize_places) are the model's; the three keywords are checked before any GPU work; the new
entry point is exported, declared as plain C, and mj_place has the layout the binding assumes."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_index

FILTERS = ("bilinear", "box", "hamming", "bicubic", "lanczos")
CANVASES = ((32, 32), (64, 64), (7, 5))

# (source, s, resized, canvas, origin): torchvision's Resize(s) then center_crop
PINNED_INT = (((1920, 1080), 256, (455, 256), (224, 224), (-116, -16)),
              ((500, 375), 256, (341, 256), (224, 224), (-58, -16)),        # half to even, not -59
              ((100, 36), 20, (55, 20), (32, 32), (-12, 6)))
# (source, canvas, resized, origin): Pillow's ImageOps.contain / pad, centring 0.5
PINNED_CONTAIN = (((1920, 1080), (224, 224), (224, 126), (0, 49)),
                  ((100, 36), (64, 64), (64, 23), (0, 20)))


def _sizes():
    """every (w, h) in 1..40 x 1..40, then the golden files' sizes"""
    out = [(w, h) for w in range(1, 41) for h in range(1, 41)]
    out += sorted({(m["image_width"], m["image_height"]) for m in golden_index().values()} - set(out))
    return out


def test_pinned_cases_model_and_package():
    from tools import place_model
    from pyjpegdecoder_amd import batch
    for impl in (place_model, batch):
        for (w, h), s, resized, canvas, origin in PINNED_INT:
            assert impl.resized_size(s, w, h, canvas) == resized
            assert tuple(impl.centred(s, resized, canvas)) == origin
            assert tuple(impl.centred(resized, resized, canvas)) == origin          # (w, h): centred as for an int
        for (w, h), canvas, resized, origin in PINNED_CONTAIN:
            assert impl.resized_size("contain", w, h, canvas) == resized
            assert tuple(impl.centred("contain", resized, canvas)) == origin
    assert batch.normalize_places(256, None, (224, 224), [(1920, 1080), (500, 375)]) == [(455, 256, -116, -16), (341, 256, -58, -16)]
    assert batch.normalize_places("contain", None, (64, 64), [(100, 36)]) == [(64, 23, 0, 20)]


def test_package_rules_are_the_models():
    from tools import place_model
    from pyjpegdecoder_amd import batch
    for canvas in CANVASES:
        for (w, h) in _sizes():
            for kind in (min(canvas), 20, "contain", (canvas[0] + 3, max(1, canvas[1] - 2))):
                r = place_model.resized_size(kind, w, h, canvas)
                assert batch.resized_size(kind, w, h, canvas) == r, (kind, w, h, canvas)
                if min(r) >= 1:
                    assert tuple(batch.centred(kind, r, canvas)) == tuple(place_model.centred(kind, r, canvas)), (kind, w, h, canvas)


def _image(rng, w, h, c):
    return rng.integers(0, 256, (h, w, 3) if c == 3 else (h, w), dtype=np.uint8)


@pytest.mark.parametrize("canvas", CANVASES)
@pytest.mark.parametrize("filter", FILTERS)
def test_contain_is_imageops_pad(filter, canvas):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageOps
    from tools import place_model
    pil = getattr(Image.Resampling, filter.upper())
    rng = np.random.default_rng(5)
    checked = padded = 0
    for k, (w, h) in enumerate(_sizes()):
        c = 3 if k % 2 else 1
        fill = (114, 7, 200) if c == 3 else 114
        r = place_model.resized_size("contain", w, h, canvas)
        if min(r) < 1:          # (Pillow refuses a side of 0 too; the package raises ValueError naming the file)
            continue
        a = _image(rng, w, h, c)
        want = np.asarray(ImageOps.pad(Image.fromarray(a), canvas, pil, color=fill))
        got = place_model.place(a, r, place_model.centred("contain", r, canvas), canvas, fill, filter)
        assert got.shape == want.shape and np.array_equal(got, want), ((w, h), canvas, r)
        checked += 1
        padded += r != canvas
    assert checked >= 1500 and padded >= 1000


@pytest.mark.parametrize("canvas", CANVASES)
@pytest.mark.parametrize("filter", FILTERS)
def test_int_and_explicit_kinds_are_pillow_resize_pasted(filter, canvas):
    """img.resize(r, filter) pasted on (or cropped to) a canvas of the fill colour at the model's offset: Image.paste clips."""
    Image = pytest.importorskip("PIL.Image")
    from tools import place_model
    pil = getattr(Image.Resampling, filter.upper())
    rng = np.random.default_rng(6)
    crop_both = pad_both = mixed = 0
    for k, (w, h) in enumerate(_sizes()):
        if max(w, h) > 128 and k % 2:          # (the two large golden sizes: one kind each is enough)
            continue
        c = 3 if k % 2 else 1
        fill = (9, 250, 77) if c == 3 else 31
        a = _image(rng, w, h, c)
        kinds = [(min(canvas) + k % 5, None), ((canvas[0] + 3, max(1, canvas[1] - 2)), None), ((1 + k % 11, 1 + k % 7), (k % 9 - 4, 3 - k % 5))]
        for kind, xy in kinds[k % 3:k % 3 + 2]:
            r = place_model.resized_size(kind, w, h, canvas)
            if min(r) < 1 or max(r) > 4096:
                continue
            xy = xy if xy is not None else place_model.centred(kind, r, canvas)
            if xy[0] >= canvas[0] or xy[1] >= canvas[1] or xy[0] + r[0] <= 0 or xy[1] + r[1] <= 0:
                continue
            want = Image.new("RGB" if c == 3 else "L", canvas, fill)
            want.paste(Image.fromarray(a).resize(r, pil), tuple(xy))
            got = place_model.place(a, r, xy, canvas, fill, filter)
            assert np.array_equal(got, np.asarray(want)), ((w, h), kind, r, xy, canvas)
            cx, cy = xy[0] < 0 or xy[0] + r[0] > canvas[0], xy[1] < 0 or xy[1] + r[1] > canvas[1]
            px, py = xy[0] > 0 or xy[0] + r[0] < canvas[0], xy[1] > 0 or xy[1] + r[1] < canvas[1]
            crop_both += cx and cy
            pad_both += px and py and not cx and not cy
            mixed += (cx and py and not cy) or (cy and px and not cx)
    assert crop_both and pad_both and mixed, (crop_both, pad_both, mixed)


def test_int_kind_is_torchvision_resize_center_crop():
    pytest.importorskip("torchvision")
    Image = pytest.importorskip("PIL.Image")
    from torchvision import transforms as T
    from tools import place_model
    rng = np.random.default_rng(8)
    for (w, h), s, canvas in (((100, 36), 20, (32, 32)), ((50, 70), 40, (32, 32)), ((37, 29), 33, (32, 32)), ((96, 24), 20, (32, 32))):
        a = _image(rng, w, h, 3)
        want = np.asarray(T.CenterCrop((canvas[1], canvas[0]))(T.Resize(s, interpolation=T.InterpolationMode.BICUBIC)(Image.fromarray(a))))
        r = place_model.resized_size(s, w, h, canvas)
        got = place_model.place(a, r, place_model.centred(s, r, canvas), canvas, 0, "bicubic")
        assert np.array_equal(got, want), ((w, h), s)


def test_keywords_are_checked_without_a_gpu():
    from pyjpegdecoder_amd.batch import normalize_fill, normalize_places
    size = (32, 32)
    dims = [(100, 36), (48, 80)]
    assert normalize_places(None, None, size, dims) is None
    assert normalize_places(size, None, size, dims) is None                 # stretched over the canvas: a call without the arguments
    assert normalize_places([20, "contain"], [None, (1, -2)], size, dims) == [(55, 20, -12, 6), (19, 32, 1, -2)]
    assert normalize_places((40, 20), (3, 4), size, dims) == [(40, 20, 3, 4)] * 2
    for bad_kw, match in (
            (dict(resize_to=20, place=None, size=None), "needs size"),
            (dict(resize_to=None, place=(0, 0), size=size), "place needs resize_to"),
            (dict(resize_to=0, place=None, size=size), "resize_to must be"),
            (dict(resize_to=True, place=None, size=size), "resize_to must be"),
            (dict(resize_to="cover", place=None, size=size), "resize_to must be"),
            (dict(resize_to=(20, 0), place=None, size=size), "resize_to must be"),
            (dict(resize_to=2.5, place=None, size=size), "resize_to must be"),
            (dict(resize_to=[20, 1.5], place=None, size=size), "resize_to must be"),
            (dict(resize_to=20, place=(1, 2, 3), size=size), "place must be"),
            (dict(resize_to=20, place=(1.0, 2), size=size), "place must be"),
            (dict(resize_to=20, place=(70000, 0), size=size), "place must be"),
            (dict(resize_to=20, place=[(0, 0), 5], size=size), "place must be")):
        with pytest.raises(ValueError, match=match):
            normalize_places(bad_kw["resize_to"], bad_kw["place"], bad_kw["size"])
    with pytest.raises(ValueError, match="resize_to has 3 entries for 2 files"):
        normalize_places([20, 20, 20], None, size, dims)
    with pytest.raises(ValueError, match="place has 1 entries for 2 files"):
        normalize_places(20, [(0, 0)], size, dims)
    with pytest.raises(ValueError, match="file 1: .*does not meet"):
        normalize_places((8, 8), [None, (32, 0)], size, dims)
    with pytest.raises(ValueError, match="file 7: .*does not meet"):
        normalize_places((8, 8), [None, (-8, 0)], size, dims, index=[3, 7])
    with pytest.raises(ValueError, match="file 0: .*1..65535"):
        normalize_places("contain", None, (64, 64), [(200, 1)])            # round(1 / 200 * 64) == 0
    assert normalize_fill(None, None) is None
    assert normalize_fill(7, 20, 3) == (7, 7, 7) and normalize_fill((1, 2, 3), 20, 3) == (1, 2, 3) and normalize_fill(255, "contain", 1) == (255,)
    for fill, rt, nc, match in ((7, None, 3, "fill needs resize_to"), (256, 20, 3, "0..255"), (-1, 20, 1, "0..255"), ((1, 2), 20, 3, "fill must be"),
                                ((1, 2, 3), 20, 1, "fill must be"), (1.5, 20, 3, "fill must be"), ("red", 20, 3, "fill must be")):
        with pytest.raises(ValueError, match=match):
            normalize_fill(fill, rt, nc)


def test_entry_point_is_exported_and_mj_place_has_the_bindings_layout(tmp_path):
    from pyjpegdecoder_amd import _binding as B
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mijpeg.h"', 'int main(void) {', '  printf("%zu", sizeof(mj_place));']
    lines += [f'  printf(" %zu", offsetof(mj_place, {name}));' for name, _ in B.PlaceC._fields_]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(B.PlaceC)] + [getattr(B.PlaceC, name).offset for name, _ in B.PlaceC._fields_]
