"""Region-of-interest decode, host side: the `rois` normaliser of BatchDecoder and the C layout of mj_roi.  CPU only."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


def test_rois_none_means_whole_images():
    from pyjpegdecoder_amd.batch import normalize_rois
    assert normalize_rois(None, [(10, 20), (30, 40)]) is None


def test_one_window_is_broadcast_to_every_file():
    from pyjpegdecoder_amd.batch import normalize_rois
    assert normalize_rois((1, 2, 3, 4), [(10, 20), (30, 40)]) == [(1, 2, 3, 4), (1, 2, 3, 4)]
    assert normalize_rois([1, 2, 3, 4], [(10, 20)] * 3) == [(1, 2, 3, 4)] * 3
    assert normalize_rois(np.array([0, 0, 5, 5]), [(10, 20)]) == [(0, 0, 5, 5)]


def test_per_file_windows_and_none_entries():
    from pyjpegdecoder_amd.batch import normalize_rois
    got = normalize_rois([None, (0, 1, 2, 3), None, (9, 19, 1, 1)], [(10, 20), (30, 40), (7, 8), (10, 20)])
    assert got == [(0, 0, 10, 20), (0, 1, 2, 3), (0, 0, 7, 8), (9, 19, 1, 1)]
    # four files, four windows: a list of tuples is per file, not one window
    assert normalize_rois([(0, 0, 1, 1)] * 4, [(2, 2)] * 4) == [(0, 0, 1, 1)] * 4


@pytest.mark.parametrize("win, what", [
    ((0, 0, 0, 5), "empty"), ((0, 0, 5, 0), "empty"), ((-1, 0, 2, 2), "not inside"), ((0, -1, 2, 2), "not inside"),
    ((9, 0, 2, 2), "not inside"), ((0, 19, 2, 2), "not inside"), ((0, 0, 11, 20), "not inside"), ((0, 0, 10, 21), "not inside"),
])
def test_windows_outside_the_image_name_the_file(win, what):
    from pyjpegdecoder_amd.batch import normalize_rois
    with pytest.raises(ValueError, match=r"file 1: .*" + what):
        normalize_rois([None, win], [(30, 30), (10, 20)])


def test_malformed_rois_raise_value_error():
    from pyjpegdecoder_amd.batch import normalize_rois
    with pytest.raises(ValueError, match="3 entries for 2 files"):
        normalize_rois([None, None, None], [(10, 10), (10, 10)])
    with pytest.raises(ValueError, match="file 0"):
        normalize_rois([(0, 0, 1), None], [(10, 10), (10, 10)])
    with pytest.raises(ValueError, match="file 1"):
        normalize_rois([None, (0.5, 0, 1, 1)], [(10, 10), (10, 10)])
    with pytest.raises(ValueError):
        normalize_rois(7, [(10, 10)])


def test_header_dimensions_of_every_golden_file():
    """The windows are checked against the frame header before any GPU work: the quick reader agrees with the parser."""
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import _image_dims
    for f in sorted((GOLDEN / "files").glob("*.jpg")):
        raw = f.read_bytes()
        p = parse_jpeg(raw)
        assert _image_dims(raw) == (p.image_width, p.image_height), f.name


def test_mj_roi_layout_matches_the_binding(tmp_path):
    from pyjpegdecoder_amd import _binding as B
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mijpeg.h"', 'int main(void) {',
             '  printf("%zu", sizeof(mj_roi));']
    for fname, _ in B.RoiC._fields_:
        lines.append(f'  printf(" %zu", offsetof(mj_roi, {fname}));')
    lines += ['  printf("\\n");', '  return 0;', '}']
    src = tmp_path / "roi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "roi"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(B.RoiC)] + [getattr(B.RoiC, f).offset for f, _ in B.RoiC._fields_]


def test_decode_rejects_rois_with_seams_before_touching_the_gpu():
    """The check comes first: no context is needed to see the error (the decoder object is built without __init__)."""
    from pyjpegdecoder_amd.batch import BatchDecoder
    dec = BatchDecoder.__new__(BatchDecoder)
    with pytest.raises(ValueError, match="return_seams"):
        dec.decode([b""], rois=(0, 0, 1, 1), return_seams=True)
