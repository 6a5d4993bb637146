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
    "reducing_gap": 1.5,
    "views": [(1, (0, 1, 2, 3)), (0, None)],
    "affine": ([(1.0, 0.0, 2.0, 0.0, 1.0, 3.0), None], "bicubic", (4, 5, 6)),
    "perspective": ([None, (1.0, 0.0, 2.0, 0.0, 1.0, 3.0, 0.5, 0.25)], "nearest", (9,)),
    "colour": [[("brightness", 1.5), ("invert",)], None],
}
# what a keyword cannot be given without
NEEDS = {"slots": ("size",), "output": ("size",), "filter": ("size",), "places": ("size",), "fill": ("size", "places"),
         "reducing_gap": ("size",), "views": ("size",), "affine": ("size",), "perspective": ("size",), "colour": ("size",)}
# ... and what it cannot be given with (the request of every keyword leaves the second of a pair out; rois do not go with views)
ALL_BUT = ("perspective", "rois")
# every structure a request holds or points to: the header's name and the binding's twin
STRUCTS = {"mj_plan_request": "PlanRequestC", "mj_roi": "RoiC", "mj_place": "PlaceC", "mj_view": "ViewC", "mj_output_desc": "OutputDescC",
           "mj_affine": "AffineC", "mj_perspective": "PerspectiveC", "mj_colour_op": "ColourOpC", "mj_colour_chain": "ColourChainC"}


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
  /* every array is a plain field: no cast, no wrapper */
  mj_view views[2] = {{1, {0, 1, 2, 3}}, {0, {0, 0, 0, 0}}};
  mj_perspective coeffs[2] = {{{1, 0, 2, 0, 1, 3, 0.5, 0.25}}, {{0, 0, 0, 0, 0, 0, 0, 0}}};
  mj_colour_chain chains[2] = {{1, {{MJ_COLOUR_INVERT, 0}}}, {0, {{0, 0}}}};
  mj_plan_request r = {0};
  mj_plan *plan = 0;
  r.out_width = r.out_height = 8;
  r.views = views; r.n_views = 2;
  r.perspective = coeffs; r.transform_filter = MJ_AFFINE_BILINEAR;
  r.transform_fill[0] = 1; r.transform_fill[1] = 2; r.transform_fill[2] = 3;
  r.colour = chains;
  r.reducing_gap = 0;
  (void)a; (void)b; (void)zeroed;
  return a == 0 ? mj_plan_create_with(0, 0, &r, &plan) : 0;
}
""")
    subprocess.run([gcc] + flags + ["-c", str(proto), "-o", str(tmp_path / "proto.o")], check=True)
    # the structs: size and every field's offset as the C compiler lays them out against the ctypes twins'
    fields = [f for f, _ in B.PlanRequestC._fields_]
    assert fields == ["rois", "orientations", "mode", "out_width", "out_height", "transform_filter", "affine", "perspective", "slots", "n_slots",
                      "n_views", "views", "output", "filter", "reducing_gap", "places", "fill", "colour", "transform_fill"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mijpeg.h"', 'int main(void) {']
    for cname, twin in STRUCTS.items():
        lines += [f'  printf("%zu", sizeof({cname}));'] + [f'  printf(" %zu", offsetof({cname}, {f}));' for f, _ in getattr(B, twin)._fields_] + ['  printf("\\n");']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ['  return 0;', '}']))
    exe = tmp_path / "layout"
    subprocess.run([gcc] + flags + [str(src), "-o", str(exe)], check=True)
    got = [[int(x) for x in line.split()] for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert len(got) == len(STRUCTS)
    for (cname, twin), layout in zip(STRUCTS.items(), got):
        T = getattr(B, twin)
        assert layout == [ctypes.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_], cname
    # ... and no field the twin does not list hides between or behind them: the fields fill the request up to its alignment
    end = max(getattr(B.PlanRequestC, f).offset + getattr(B.PlanRequestC, f).size for f in fields)
    assert ctypes.sizeof(B.PlanRequestC) - end < ctypes.alignment(B.PlanRequestC)


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
    assert r.reducing_gap == (given["reducing_gap"] if "reducing_gap" in given else 0.0)
    assert bool(r.views) == ("views" in given) and r.n_views == (2 if "views" in given else 0)
    if "views" in given:
        assert [(v.image, (v.window.x, v.window.y, v.window.width, v.window.height)) for v in (r.views[0], r.views[1])] == [(1, (0, 1, 2, 3)), (0, (0, 0, 0, 0))]
    assert bool(r.affine) == ("affine" in given) and bool(r.perspective) == ("perspective" in given)
    if "affine" in given:
        assert [list(m.a) for m in (r.affine[0], r.affine[1])] == [list(given["affine"][0][0]), [0.0] * 6]
        assert r.transform_filter == B.MJ_AFFINE_BICUBIC and tuple(r.transform_fill) == (4, 5, 6)
    elif "perspective" in given:
        assert [list(m.a) for m in (r.perspective[0], r.perspective[1])] == [[0.0] * 8, list(given["perspective"][0][1])]
        assert r.transform_filter == B.MJ_AFFINE_NEAREST and tuple(r.transform_fill) == (9, 0, 0)
    else:
        assert r.transform_filter == 0 and bytes(r.transform_fill) == bytes(3)
    assert bool(r.colour) == ("colour" in given)
    if "colour" in given:
        c = r.colour[0]
        assert (c.n, c.op[0].kind, c.op[0].value, c.op[1].kind) == (2, B.COLOUR_OPS["brightness"], 1.5, B.COLOUR_OPS["invert"]) and r.colour[1].n == 0


def test_plan_request_puts_every_keyword_where_it_belongs():
    from pyjpegdecoder_amd import _binding as B
    r, keep = B.plan_request(2)
    check_request(r, keep, {})
    assert bytes(r) == bytes(ctypes.sizeof(B.PlanRequestC)), "no keyword: the zeroed request"
    for name in KEYWORDS:
        given = {k: KEYWORDS[k] for k in (name,) + NEEDS.get(name, ())}
        r, keep = B.plan_request(2, **given)
        check_request(r, keep, given)
    every = {k: v for k, v in KEYWORDS.items() if k not in ALL_BUT}
    r, keep = B.plan_request(2, **every)
    check_request(r, keep, every)
    assert sorted(keep) == sorted([{"orientation": "orientations"}.get(k, k) for k in every if k not in ("size", "filter", "mode", "reducing_gap")] + ["mirror"])
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
    for name in ("affine", "perspective"):
        with pytest.raises(ValueError, match=f"{name}: 1 entries, not one for each of the 2 images"):
            B.plan_request(2, size=(8, 8), **{name: (KEYWORDS[name][0][:1],) + KEYWORDS[name][1:]})
    with pytest.raises(ValueError, match="colour: 2 entries, not one for each of the 3 views"):
        B.plan_request(2, size=(8, 8), views=KEYWORDS["views"] + [(0, None)], colour=KEYWORDS["colour"])
    with pytest.raises(ValueError, match="affine and perspective do not go together"):
        B.plan_request(2, size=(8, 8), affine=KEYWORDS["affine"], perspective=KEYWORDS["perspective"])
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


def test_load_library_refuses_a_library_of_another_version(lib, monkeypatch):
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.errors import BackendError
    assert lib.mj_version() == B.MJ_VERSION
    monkeypatch.setattr(B, "MJ_VERSION", B.MJ_VERSION + 1)
    monkeypatch.setattr(B, "_lib", None)
    with pytest.raises(BackendError, match="rebuild"):
        B.load_library()
    assert B._lib is None, "a refused library is not kept"
    monkeypatch.undo()
    assert B.load_library() is lib
