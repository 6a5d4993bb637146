"""Derived plans and also= on the host (no GPU): include/mijpeg.h's mj_plan_derive against the binding, its refusals that need no
device, and the pure-Python layer of also= — normalize_also, the union selection, _Request.narrow with extra groups."""
import ctypes
import shutil
import subprocess

import pytest

from conftest import ROOT

SIZE, SMALL = (24, 16), (12, 10)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from pyjpegdecoder_amd import _binding as B
    if not B.LIB_PATH.exists():
        g.build()
    return B.load_library()


def test_the_entry_point_is_declared_as_the_binding_assumes(lib, tmp_path):
    from pyjpegdecoder_amd import _binding as B
    assert "mj_plan_derive" in B.EXPORTS and hasattr(lib, "mj_plan_derive")
    assert not "mj_plan_derive".startswith("mj_plan_create")
    gcc = shutil.which("gcc")
    assert gcc is not None, "the header is held to a C compiler"
    proto = tmp_path / "proto.c"
    proto.write_text("""
#include "mijpeg.h"
int main(void) {
  int (*d)(mj_plan *, const mj_batch *, const mj_plan_request *, mj_plan **) = mj_plan_derive;
  mj_plan_request r = {0};
  mj_plan *plan = 0;
  r.out_width = r.out_height = 8;
  return d == 0 ? mj_plan_derive(0, 0, &r, &plan) : 0;
}
""")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")],
                   check=True)


def test_the_abi_is_the_one_it_was_plus_one_function(lib):
    from pyjpegdecoder_amd import _binding as B
    assert lib.mj_version() == 2 and B.MJ_VERSION == 2
    assert [f for f, _ in B.PlanRequestC._fields_] == [
        "rois", "orientations", "mode", "out_width", "out_height", "transform_filter", "affine", "perspective", "slots", "n_slots",
        "n_views", "views", "output", "filter", "reducing_gap", "places", "fill", "colour", "transform_fill"]
    assert [n for n in B.EXPORTS if n.startswith("mj_plan_create")] == ["mj_plan_create", "mj_plan_create_with"]


def test_null_arguments_are_refused_without_a_device(lib):
    from pyjpegdecoder_amd import _binding as B
    r = B.PlanRequestC()
    r.out_width = r.out_height = 8
    b = B.BatchC()
    out = ctypes.c_void_p(1234)
    assert lib.mj_plan_derive(None, ctypes.byref(b), ctypes.byref(r), ctypes.byref(out)) == B.MJ_ERR_INVALID
    assert b"mj_plan_derive: NULL argument" in lib.mj_last_error(None)
    assert lib.mj_plan_derive(None, ctypes.byref(b), None, ctypes.byref(out)) == B.MJ_ERR_INVALID
    assert lib.mj_plan_derive(None, ctypes.byref(b), ctypes.byref(r), None) == B.MJ_ERR_INVALID
    assert lib.mj_plan_derive(None, None, None, None) == B.MJ_ERR_INVALID


# ---- also=: normalisation ----------------------------------------------------------------------------------------------------------

CALL = dict(dtype="float16", normalize=((0.5,) * 3, (0.25,) * 3), resample="bicubic", mode="RGB", reducing_gap=2.0, fill=(1, 2, 3),
            affine_resample="bilinear", affine_fill=(9, 9, 9))


def test_none_and_the_empty_list_are_a_call_without():
    from pyjpegdecoder_amd.batch import normalize_also
    assert normalize_also(None, CALL, SIZE) is None and normalize_also([], CALL, SIZE) is None and normalize_also((), CALL, None) is None


def test_call_wide_keys_are_inherited_and_per_output_keys_are_not():
    from pyjpegdecoder_amd.batch import ALSO_CALL_WIDE, ALSO_PER_OUTPUT, normalize_also
    call = dict(CALL, reducing_gap=None, views=[(0, None)], mirror=[True], resize_to=32, place=(1, 1), affine=(1, 0, 0, 0, 1, 0), color_ops=[("invert",)])
    (g,) = normalize_also([dict(size=SMALL)], call, SIZE)
    assert g["size"] == SMALL
    assert all(g[k] is None for k in ALSO_PER_OUTPUT), g                                 # never the call's
    for k in ("dtype", "normalize", "resample", "mode"):
        assert g[k] == call[k], k
    # what the call says about placing and transforming goes to the groups that place and transform
    assert g["fill"] is None and g["affine_resample"] is None and g["affine_fill"] is None
    (g,) = normalize_also([dict(size=SMALL, resize_to=8, perspective=(1, 0, 0, 0, 1, 0, 0, 0))], call, SIZE)
    assert g["fill"] == (1, 2, 3) and g["affine_resample"] == "bilinear" and g["affine_fill"] == (9, 9, 9) and g["affine"] is None
    # an entry's own word wins, None included
    (g,) = normalize_also([dict(size=list(SMALL), dtype=None, normalize=None, resample="box", mode=None, reducing_gap=3.0, mirror=True,
                                views=[0, (1, (0, 0, 2, 2))])], dict(call, reducing_gap=2.0), SIZE)
    assert (g["dtype"], g["normalize"], g["resample"], g["mode"], g["reducing_gap"], g["mirror"]) == (None, None, "box", None, 3.0, True)
    assert g["size"] == SMALL and g["views"] == [0, (1, (0, 0, 2, 2))]
    assert set(g) == {"size"} | set(ALSO_PER_OUTPUT) | set(ALSO_CALL_WIDE)
    two = normalize_also([dict(size=SMALL), dict(size=(7, 9), mode="L")], call, SIZE)
    assert [t["size"] for t in two] == [SMALL, (7, 9)] and [t["mode"] for t in two] == ["RGB", "L"]


@pytest.mark.parametrize("also, kw, message", [
    ([dict(size=SMALL), dict(size=SMALL, shape=3)], {}, r"also\[1\]: unknown key 'shape'"),
    ([dict(size=SMALL, rois=[(0, 0, 1, 1)])], {}, r"also\[0\]: rois is not a key of an entry: windows are views"),
    ([dict(size=SMALL, orientation=6)], {}, r"also\[0\]: orientation is not a key of an entry: it is per file and the call's"),
    ([dict(size=SMALL), dict(size=SMALL), dict(size=SMALL, return_seams=True)], {}, r"also\[2\]: return_seams is not a key of an entry"),
    ([dict(views=[0])], {}, r"also\[0\]: size is required"),
    ([dict(size=None)], {}, r"also\[0\]: size is required"),
    ([dict(size=SMALL), [("size", SMALL)]], {}, r"also\[1\]: an entry is a dict"),
    ([dict(size=SMALL), None], {}, r"also\[1\]: an entry is a dict"),
    ([dict(size=(0, 4))], {}, r"also\[0\]: size must be \(width, height\)"),
    ([dict(size=SMALL, resample="nearest")], {}, r"also\[0\]: resample: Pillow's NEAREST"),
    ([dict(size=SMALL, dtype="uint8", normalize=(0.5, 0.5))], {}, r"also\[0\]: normalize needs a float dtype"),
    ([dict(size=SMALL, place=(1, 1))], {}, r"also\[0\]: place needs resize_to"),
    ([dict(size=SMALL, color_ops=[("sepia",)])], {}, r"also\[0\]: color_ops: unknown op 'sepia'"),
    ([dict(size=SMALL, affine=(1, 0, 0, 0, 1, 0), reducing_gap=2.0)], {}, r"also\[0\]: affine and reducing_gap do not go together"),
    ([dict(size=SMALL, views=7)], {}, r"also\[0\]: views must be None or a list"),
    (dict(size=SMALL), {}, r"also must be None or a list with one dict per extra group"),
    ([dict(size=SMALL)], dict(size=None), r"also needs size="),
    ([dict(size=SMALL)], dict(rois=[(0, 0, 1, 1)]), r"also and rois do not go together"),
    ([dict(size=SMALL)], dict(return_seams=True), r"also and return_seams do not go together"),
])
def test_refusals_name_the_entry(also, kw, message):
    from pyjpegdecoder_amd.batch import normalize_also
    call = dict(dtype=None, normalize=None, resample=None, mode=None, reducing_gap=None, fill=None, affine_resample=None, affine_fill=None)
    with pytest.raises(ValueError, match=message):
        normalize_also(also, call, kw.get("size", SIZE), kw.get("rois"), kw.get("return_seams", False))


def test_bfloat16_is_refused_on_the_numpy_route_only():
    from pyjpegdecoder_amd.batch import normalize_also
    call = dict.fromkeys(("dtype", "normalize", "resample", "mode", "reducing_gap", "fill", "affine_resample", "affine_fill"))
    assert normalize_also([dict(size=SMALL, dtype="bfloat16")], call, SIZE)[0]["dtype"] == "bfloat16"
    with pytest.raises(ValueError, match=r"also\[0\]: dtype bfloat16: NumPy has no such type"):
        normalize_also([dict(size=SMALL, dtype="bfloat16")], call, SIZE, host=True)


# ---- the union selection and the merged request ------------------------------------------------------------------------------------

def test_the_union_selection_drops_a_file_no_group_names():
    from pyjpegdecoder_amd.batch import select_union_files
    files = [b"a", b"not a jpeg", b"c", b"d", b"not one either"]
    groups = [dict(size=SIZE, views=[(3, None), (0, (0, 0, 1, 1))]), dict(size=SMALL, views=[2, 0, 0])]
    assert select_union_files(files, groups) == [0, 2, 3]
    assert select_union_files(files, groups + [dict(size=(7, 9), views=None)]) == [0, 1, 2, 3, 4]       # (no views: every file)
    assert select_union_files(files, [dict(size=SIZE, views=[])]) == []
    with pytest.raises(ValueError, match="^view 1: file 5 is not one of the 5 files"):
        select_union_files(files, [dict(size=SIZE, views=[0, 5])])
    with pytest.raises(ValueError, match=r"^also\[1\]: view 0: file -1 is not one of the 5 files"):
        select_union_files(files, groups + [dict(size=SIZE, views=[-1])])


def _fake_build(files, orientation=None, size=None, views=None, mirror=None, **_):
    """one group alone, as _device_request would build it (no header is read: windows are left as given)"""
    from pyjpegdecoder_amd.batch import OutputSpec, _per_file_of, _Request, normalize_orientation, select_view_files
    sel = select_view_files(files, views, size)
    index = None
    if sel is not None:
        index, views = sel
        orientation = _per_file_of(orientation, len(files), index, "orientation")
        files = [files[i] for i in index]
    n = len(views) if views is not None else len(files)
    return _Request(files, None, size, OutputSpec("uint8", mirror=list(mirror)) if mirror is not None else None, None, list(range(n)), index,
                    normalize_orientation(orientation, files), views=views)


def test_groups_are_merged_over_the_files_some_group_names():
    from pyjpegdecoder_amd.batch import BatchDecoder
    files = [b"f0", b"junk", b"f2", b"f3", b"f4"]
    groups = [dict(size=SIZE, views=[(3, (0, 0, 5, 5)), (0, None)], mirror=[True, False]),
              dict(size=SMALL, views=[(4, None), (3, (1, 1, 2, 2)), (4, (2, 2, 3, 3))], mirror=[False, True, True])]
    req = BatchDecoder._merged_request(files, [1, 8, 1, 6, 3], groups, _fake_build)
    assert req.files == [b"f0", b"f3", b"f4"] and req.index == [0, 3, 4] and req.orient == [1, 6, 3]
    assert req.views == [(1, (0, 0, 5, 5)), (0, None)] and req.size == SIZE
    (extra,) = req.also
    assert extra.files == req.files and extra.index == req.index and extra.orient == req.orient and extra.also is None
    assert extra.views == [(2, None), (1, (1, 1, 2, 2)), (2, (2, 2, 3, 3))] and extra.size == SMALL
    assert [g.size for g in req.groups] == [SIZE, SMALL]
    # files sorted by orientation class AND by the groups that name them: file 0 primary only, 3 both, 4 extra only
    assert sorted(map(tuple, req.orient_classes())) == [(0,), (1,), (2,)]
    assert req.plan_keys() == [(0, True, False), (2, True, True), (1, False, True)]
    # upright files named by all groups stay one class
    same = BatchDecoder._merged_request(files, None, [dict(size=SIZE, views=[0, 2]), dict(size=SMALL, views=[2, 0, 0])], _fake_build)
    assert same.orient is None and same.orient_classes() == [[0, 1]]
    # an error in an extra group's arguments names the entry
    with pytest.raises(ValueError, match=r"also\[0\]: view 0: file 9 is not one of the 5 files"):
        BatchDecoder._merged_request(files, None, [dict(size=SIZE, views=[0]), dict(size=SMALL, views=[9])], _fake_build)


def test_narrow_narrows_every_group():
    from pyjpegdecoder_amd.batch import AffineSpec, OutputSpec, _Request
    files = [b"a", b"b", b"c", b"d"]
    m = (1.0, 0.0, 1.0, 0.0, 1.0, 2.0)
    one = _Request(files, None, SMALL, OutputSpec("uint8", mirror=[True, False, False, True, True]), "dest1", [4, 3, 2, 1, 0], None, [1, 6, 3, 1],
                   views=[(3, (0, 0, 1, 1)), (1, (0, 0, 2, 2)), (3, (0, 0, 3, 3)), (0, None), (1, (0, 0, 5, 5))],
                   places=[(1, 1, 0, 0), (2, 2, 0, 0), (3, 3, 0, 0), (4, 4, 0, 0), (5, 5, 0, 0)],
                   affine=AffineSpec([None, m, None, None, None], "bilinear", (0, 0, 0)), colour=[None, None, (("invert",),), None, None])
    two = _Request(files, None, (7, 9), OutputSpec("float16", mirror=[False, True]), "dest2", [0, 1], None, [1, 6, 3, 1], views=[(2, None), (2, (1, 1, 2, 2))])
    req = _Request(files, None, SIZE, None, "dest0", [0, 1, 2, 3], None, [1, 6, 3, 1], also=[one, two])
    sub = req.narrow([3, 1])
    assert sub.files == [b"d", b"b"] and sub.index == [3, 1] and sub.orient == [1, 6] and sub.slots == [3, 1] and sub.dest == "dest0"
    a, b = sub.also
    # each group's views re-indexed among the files, in their order; its slots, mirror flags, places, matrices and chains picked
    assert a.files == sub.files and a.index == sub.index and a.orient == sub.orient and a.size == SMALL and a.dest == "dest1"
    assert a.views == [(0, (0, 0, 1, 1)), (1, (0, 0, 2, 2)), (0, (0, 0, 3, 3)), (1, (0, 0, 5, 5))]
    assert a.slots == [4, 3, 2, 0] and a.output.mirror == [True, False, False, True]
    assert a.places == [(1, 1, 0, 0), (2, 2, 0, 0), (3, 3, 0, 0), (5, 5, 0, 0)]
    assert a.affine.matrices == [None, m, None, None] and a.colour == [None, None, (("invert",),), None]
    # a group with no output among the files comes out empty
    assert b.views == [] and b.slots == [] and b.output.mirror == [] and b.n_outputs == 0 and b.size == (7, 9) and b.dest == "dest2"
    # ... and where it has some, a group the others have left keeps its own
    c = req.narrow([2]).also
    assert c[0].views == [] and c[0].affine is None and c[0].colour is None
    assert c[1].views == [(0, None), (0, (1, 1, 2, 2))] and c[1].slots == [0, 1] and c[1].output.mirror == [False, True] and c[1].orient == [3]
    # narrowing twice is narrowing once
    assert req.narrow([3, 1, 0]).narrow([0, 1]) == sub


def test_a_request_without_also_is_what_it_was():
    from pyjpegdecoder_amd.batch import OutputSpec, _Request
    files = [b"a", b"b", b"c"]
    req = _Request(files, None, SIZE, OutputSpec("float16", (0.5,) * 3, (0.25,) * 3, [True, False, True]), None, [0, 1, 2], resample="lanczos")
    assert req.also is None and req.groups == [req]
    sub = req.narrow([2, 0])
    assert sub.also is None and sub == _Request([b"c", b"a"], None, SIZE, OutputSpec("float16", (0.5,) * 3, (0.25,) * 3, [True, True]), None, [2, 0], [2, 0],
                                                resample="lanczos")
    assert sub.plan_kwargs() == {"rois": None, "size": SIZE, "slots": None, "output": ("float16", (0.5,) * 3, (0.25,) * 3, [True, True]), "filter": "lanczos"}
    assert _Request(files).orient_classes() == [[0, 1, 2]] and _Request(files).plan_keys() is None
    assert _Request(files, None, SIZE, also=[]).narrow([1]).also == []
