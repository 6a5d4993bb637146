"""The one plan request on the host (no GPU): include/mijpeg.h's mj_plan_request and the two entry points against the binding's
ctypes twin, and _binding.plan_request — the one place Plan's keywords become the request's fields."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

KEYWORDS = {
    "rois": [(0, 0, 4, 4), (1, 2, 3, 4)],
    "size": (17, 5),
    "slots": ([3, 1], 6),
    "output": ("float16", (0.5, 0.25, 0.125), (1.0, 2.0, 4.0), [0, 1]),
    "orientation": [6, 3],
    "filter": "lanczos",
    "mode": "L",
    "places": [(17, 5, 0, 0), (9, 7, -2, 3)],
    "fill": (7, 8, 9),
}
# what a keyword cannot be given without
NEEDS = {"slots": ("size",), "output": ("size",), "filter": ("size",), "places": ("size",), "fill": ("size", "places")}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


def test_the_request_and_both_entry_points_are_declared_as_the_binding_assumes(lib, tmp_path):
    from pyjpegdecoder_amd import _binding as B
    for name in ("mj_plan_create_with", "mj_plan_create"):
        assert name in B.EXPORTS and hasattr(lib, name), name
    assert [n for n in B.EXPORTS if n.startswith("mj_plan_create")] == ["mj_plan_create", "mj_plan_create_with"]
    gcc = shutil.which("gcc")
    assert gcc is not None, "the header is held to a C compiler"
    flags = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include")]
    # the prototypes, assigned from the header's declarations (a mismatch is a compile error)
    proto = tmp_path / "proto.c"
    proto.write_text("""
#include "mijpeg.h"
int main(void) {
  int (*a)(mj_context *, const mj_batch *, const mj_plan_request *, mj_plan **) = mj_plan_create_with;
  int (*b)(mj_context *, const mj_batch *, mj_plan **) = mj_plan_create;
  mj_plan_request zeroed = {0};
  (void)a; (void)b; (void)zeroed;
  return 0;
}
""")
    subprocess.run([gcc] + flags + ["-c", str(proto), "-o", str(tmp_path / "proto.o")], check=True)
    # the struct: size and offsets as the C compiler lays it out against the ctypes twin's
    fields = [f for f, _ in B.PlanRequestC._fields_]
    assert fields == ["rois", "orientations", "mode", "out_width", "out_height", "slots", "n_slots", "output", "filter", "places", "fill"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(
        ['#include <stdio.h>', '#include <stddef.h>', '#include "mijpeg.h"', 'int main(void) {', '  printf("%zu", sizeof(mj_plan_request));'] +
        [f'  printf(" %zu", offsetof(mj_plan_request, {f}));' for f in fields] + ['  printf("\\n");', '  return 0;', '}']))
    exe = tmp_path / "layout"
    subprocess.run([gcc] + flags + [str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(B.PlanRequestC)] + [getattr(B.PlanRequestC, f).offset for f in fields]


def check_request(r, keep, given):
    """every field of request `r` holds what the keywords `given` say, and nothing where they say nothing"""
    from pyjpegdecoder_amd import _binding as B

    def bytes_at(addr, n):
        return list(ctypes.string_at(addr, n))
    assert bool(r.rois) == ("rois" in given)
    if "rois" in given:
        assert [(w.x, w.y, w.width, w.height) for w in (r.rois[0], r.rois[1])] == given["rois"]
    assert bool(r.orientations) == ("orientation" in given)
    if "orientation" in given:
        assert bytes_at(r.orientations, 2) == given["orientation"]
    assert r.mode == (B.MJ_MODE_L if "mode" in given else B.MJ_MODE_NATIVE)
    assert (r.out_width, r.out_height) == (given["size"] if "size" in given else (0, 0))
    assert bool(r.slots) == ("slots" in given) and r.n_slots == (6 if "slots" in given else 0)
    if "slots" in given:
        assert list(np.frombuffer(ctypes.string_at(r.slots, 8), dtype=np.int32)) == given["slots"][0]
    assert bool(r.output) == ("output" in given)
    if "output" in given:
        o = r.output.contents
        assert (o.dtype, o.normalize, list(o.mean), list(o.std)) == (B.MJ_DTYPE_F16, 1, [0.5, 0.25, 0.125], [1.0, 2.0, 4.0])
        assert o.mirror and bytes_at(o.mirror, 2) == given["output"][3] and o.mirror == keep["mirror"].ctypes.data
    assert r.filter == (B.MJ_FILTER_LANCZOS if "filter" in given else B.MJ_FILTER_BILINEAR)
    assert bool(r.places) == ("places" in given)
    if "places" in given:
        assert (r.places[1].width, r.places[1].height, r.places[1].x, r.places[1].y) == given["places"][1]
    assert bool(r.fill) == ("fill" in given)
    if "fill" in given:
        assert bytes_at(r.fill, 3) == list(given["fill"])


def test_plan_request_puts_every_keyword_where_it_belongs():
    from pyjpegdecoder_amd import _binding as B
    r, keep = B.plan_request(2)
    check_request(r, keep, {})
    assert bytes(r) == bytes(ctypes.sizeof(B.PlanRequestC)), "no keyword: the zeroed request"
    for name in KEYWORDS:
        given = {k: KEYWORDS[k] for k in (name,) + NEEDS.get(name, ())}
        r, keep = B.plan_request(2, **given)
        check_request(r, keep, given)
    r, keep = B.plan_request(2, **KEYWORDS)
    check_request(r, keep, KEYWORDS)
    # an output without mirror flags, and fewer fill bytes than components
    r, keep = B.plan_request(2, size=(8, 8), output=("float32", None, None, None), places=KEYWORDS["places"], fill=(200,))
    assert r.output.contents.dtype == B.MJ_DTYPE_F32 and r.output.contents.normalize == 0 and not r.output.contents.mirror
    assert list(ctypes.string_at(r.fill, 3)) == [200, 0, 0]


def test_plan_request_refuses_what_only_a_sized_or_placed_plan_has_and_lists_of_the_wrong_length():
    from pyjpegdecoder_amd import _binding as B
    with pytest.raises(ValueError, match="places.* need size"):
        B.plan_request(2, places=KEYWORDS["places"])
    with pytest.raises(ValueError, match="fill needs places"):
        B.plan_request(2, size=(8, 8), fill=(1, 2, 3))
    with pytest.raises(ValueError, match="filter.* need size"):
        B.plan_request(2, filter="box")
    with pytest.raises(ValueError, match="output need size"):
        B.plan_request(2, output=("float32", None, None, None))
    with pytest.raises(ValueError, match="places: 1 entries, not one for each of the 2 images"):
        B.plan_request(2, size=(8, 8), places=KEYWORDS["places"][:1])
    with pytest.raises(ValueError, match="orientation: 3 entries, not one for each of the 2 images"):
        B.plan_request(2, orientation=[1, 1, 1])
    with pytest.raises(ValueError, match="mirror: 1 entries, not one for each of the 2 images"):
        B.plan_request(2, size=(8, 8), output=("uint8", None, None, [1]))
    with pytest.raises(ValueError, match="filter must be"):
        B.plan_request(2, size=(8, 8), filter="nearest")
    with pytest.raises(ValueError, match="mode must be"):
        B.plan_request(2, mode="CMYK")
    # Plan refuses before it touches its context
    with pytest.raises(ValueError, match="size"):
        B.Plan(None, None, None, output=("float32", None, None, None))


def test_the_entry_point_refuses_a_bad_request_without_a_context(lib):
    from pyjpegdecoder_amd import _binding as B
    from routes_common import create_with
    h = ctypes.c_void_p()
    d = B.OutputDescC()
    d.dtype = 9
    assert create_with(lib, None, None, h, output=d) == B.MJ_ERR_INVALID
    assert b"mj_plan_create_with: output: dtype" in lib.mj_last_error(None)
    assert create_with(lib, None, None, h, out_width=8, out_height=8, output=d) == B.MJ_ERR_INVALID
    assert b"dtype" in lib.mj_last_error(None)
    assert create_with(lib, None, None, h, mode=2) == B.MJ_ERR_INVALID and b"mode 2 is none of MJ_MODE_" in lib.mj_last_error(None)
    assert create_with(lib, None, None, h, filter=5) == B.MJ_ERR_INVALID and b"filter 5 is none of MJ_FILTER_" in lib.mj_last_error(None)
    # nothing wrong with the request: the missing context is refused, by either entry point, and nothing is created
    assert lib.mj_plan_create_with(None, None, None, ctypes.byref(h)) == B.MJ_ERR_INVALID
    assert lib.mj_plan_create(None, None, ctypes.byref(h)) == B.MJ_ERR_INVALID
    assert not h.value
