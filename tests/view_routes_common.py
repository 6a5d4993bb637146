"""What the view-route tests share (tests/test_view_routes.py on the MI355X, tests/test_view_routes_host.py with a stand-in back
end): the call of tests/routes_common.py — files of every kind, some of which go round again — asked for as VIEWS, two or three per
file and interleaved, behind a leading entry that is no JPEG and that no view names; what is per view (window, mirror flag, matrix or
perspective coefficients, colour chain, place) and per file (orientation) under each combination of arguments; ONE expectation per view; and the reading of the plans a
call made against the call's views.  Not a test file: nothing here is collected.

The expectation of a view (`expect`) is the models' pipeline evaluated on the view's window only — tools/mode_model.convert,
orient_model.orient, affine_model.transform(window=) or perspective_model.transform(window=), place_model.place,
colour_model.apply_chain, the mirror, normalize_model.normalize — on the oracle's pixels; the stand-in plan of the host file
computes the same view with tools/affine_model.expected or tools/perspective_model.expected, which transform the whole image and
cut the window out, so that the two agree is itself held."""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from affine_cases import rotate_shear
from routes_common import CallFile, differ, files_of, positions
from test_resize import as_layout

SIZE = (40, 28)
NORMALIZE = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FILL, AFFINE_FILL = (114, 9, 201), (7, 99, 200)
JUNK = b"not a jpeg"
# by position in routes_common.call_files(): upright, flipping (2, 3, 4) and transposing (5 .. 8) files; the tail files (3, 6, 8)
# are upright, transposing and flipping, the unconverged ones (4, 10) flipping and transposing
ORIENT = [1, 3, 6, 1, 2, 8, 5, 1, 4, 1, 7, 1, 6]
UNTRANSFORMED = 9           # the file (a plan of its own) whose views all have no matrix: that plan carries no affine

COMBOS = {
    "views": dict(),
    "L_bicubic": dict(mode="L", resample="bicubic"),
    "places_f16": dict(places=True, dtype="float16", mirror=True),
    "affine_nearest": dict(affine="nearest"),
    "affine_bicubic_orient": dict(affine="bicubic", orientation=True, mirror=True),
    "colour_f16": dict(colour=True, dtype="float16", mirror=True),
    "perspective_bicubic_orient": dict(perspective="bicubic", orientation=True, mirror=True),
    "perspective_nearest_colour_L": dict(perspective="nearest", colour=True, mode="L"),
}
HIST_OPS, BLUR_OPS = ("contrast", "autocontrast", "equalize"), ("gaussian_blur", "box_blur")


@dataclass
class View:
    file: int                   # position in the caller's list (the leading non-JPEG counted)
    gi: int                     # what the view's values are derived from: the file's number (call_files() position) ...
    j: int                      # ... and which of the file's views this is
    k: int = 0                  # position among the call's views


@dataclass
class ViewCall:
    entries: List[CallFile]
    gis: List[int]
    files: List[bytes] = field(default_factory=list)
    views: List[View] = field(default_factory=list)


def make_call(entries: List[CallFile], gis: Optional[List[int]] = None) -> ViewCall:
    """entries as views: every file's first view in file order, the second views rotated by half the files, a third view of every
    even-numbered file rotated by one — no file's views are adjacent for three files and more"""
    gis = list(range(len(entries))) if gis is None else list(gis)
    n = len(entries)
    call = ViewCall(entries, gis, [JUNK] + [e.raw for e in entries])
    order = [(i, 0) for i in range(n)] + [((i + n // 2) % n, 1) for i in range(n)]
    order += [((i + 1) % n, 2) for i in range(n) if gis[(i + 1) % n] % 2 == 0]
    call.views = [View(i + 1, gis[i], j, k) for k, (i, j) in enumerate(order)]
    return call


def oriented_dims(call: ViewCall, v: View, combo: dict):
    w, h = call.entries[v.file - 1].full.shape[:2]
    return (h, w) if combo.get("orientation") and ORIENT[v.gi] >= 5 else (w, h)


def window_of(call: ViewCall, v: View, combo: dict):
    """the view's own window of its file's image as the combination shows it (third views: the whole image)"""
    W, H = oriented_dims(call, v, combo)
    g = v.gi
    if v.j == 0:
        return (W // 8 + g % 5, H // 8 + g % 4, W // 2, H // 2)
    if v.j == 1:
        return (W // 4 - g % 2, H // 4 + g % 3, W // 2 + g % 5, H // 2 - g % 3)
    return (0, 0, W, H)


def mirror_of(v: View) -> bool:
    return bool((v.gi + 2 * v.j + v.gi // 3) & 1)


def matrix_of(call: ViewCall, v: View, combo: dict):
    """the view's own matrix under the affine combinations: some None, under "nearest" some with a1 == a3 == 0 (index tables)"""
    if not combo.get("affine") or v.gi == UNTRANSFORMED:
        return None
    W, H = oriented_dims(call, v, combo)
    t = 3 * v.gi + v.j                  # one number per view of the whole call
    if combo["affine"] == "nearest":
        if t % 4 == 0:
            return None
        if t % 4 == 1:
            return (1.0 + 0.1 * (t % 5), 0.0, -0.06 * W + t % 3, 0.0, 0.8 + 0.05 * (t % 7), 0.04 * H - t % 4)
        return rotate_shear((W, H), 10.0 + 3.0 * t, 0.02 * (t % 5), (t % 3, -(t % 4)))
    if t % 5 == 0:
        return None
    return rotate_shear((W, H), -20.0 + 4.0 * t, 0.1, (t % 3, -(t % 4)))


def chain_of(v: View):
    """the view's own colour chain (a tuple of ops, as the request holds it) under the colour combinations: some None, the others
    pairwise different — every factor, threshold and radius is made from t —, one to four ops long, every kind of op among them;
    ("equalize",) stands first in some chains and second in others"""
    if v.gi == UNTRANSFORMED:
        return None
    t = 3 * v.gi + v.j
    m = t % 8
    if m == 0:
        return (("contrast", 0.6 + 0.03 * t), ("gaussian_blur", 0.9 + 0.05 * t))
    if m == 1:
        return (("equalize",), ("brightness", 0.7 + 0.02 * t))
    if m == 2:
        return (("box_blur", 0.25 + 0.1 * t), ("solarize", float(100 + t)), ("invert",))
    if m == 3:
        return None
    if m == 4:
        return (("sharpness", 0.5 + 0.05 * t), ("color", 0.3 + 0.04 * t), ("posterize", float(2 + t % 6)), ("autocontrast",))
    if m == 5:
        return (("brightness", 0.7 + 0.02 * t), ("equalize",))
    if m == 6:
        return (("gaussian_blur", 0.8 + 0.04 * t),)
    return (("autocontrast",), ("contrast", 1.9 - 0.03 * t), ("box_blur", 0.5 + 0.07 * t))


def coeffs_of(call: ViewCall, v: View, combo: dict):
    """the view's own perspective coefficients under the perspective combinations (some None): the corners of its file's oriented
    image drawn inwards by two to seven per cent of the side, every corner by its own amount, every view by its own"""
    if not combo.get("perspective") or v.gi == UNTRANSFORMED:
        return None
    from tools import perspective_model
    W, H = oriented_dims(call, v, combo)
    t = 3 * v.gi + v.j
    if t % (4 if combo["perspective"] == "nearest" else 5) == 0:
        return None
    ends = []
    for i, (x, y) in enumerate(perspective_model.corners(W, H)):
        fx, fy = 0.02 + 0.01 * ((t + 2 * i) % 5) + 0.0007 * t, 0.02 + 0.01 * ((3 * t + i) % 5) + 0.0005 * t
        ends.append((x + fx * W if x == 0 else x - fx * W, y + fy * H if y == 0 else y - fy * H))
    return perspective_model.coeffs(perspective_model.corners(W, H), ends)


def transform_fill(combo: dict):
    """affine_fill as the call passes it: one byte per output component"""
    return AFFINE_FILL[0] if combo.get("mode") == "L" else AFFINE_FILL


def place_of(v: View):
    """(width, height, x, y): the view's own resize_to and place on the canvas SIZE"""
    t = 3 * v.gi + v.j
    return (24 + (t % 5) * 3, 18 + (t % 4) * 2, -3 + t % 7, -2 + t % 5)


def call_kwargs(call: ViewCall, cname: str, entry_point: str = "decode_device") -> dict:
    combo = COMBOS[cname]
    kw = dict(size=SIZE, views=[(v.file, window_of(call, v, combo) if v.j < 2 else None) for v in call.views])
    if combo.get("mode"):
        kw["mode"] = combo["mode"]
    if combo.get("resample"):
        kw["resample"] = combo["resample"]
    if combo.get("mirror"):
        kw["mirror"] = [mirror_of(v) for v in call.views]
    if combo.get("dtype"):
        kw.update(dtype=combo["dtype"], normalize=NORMALIZE)
    if combo.get("places"):
        kw.update(resize_to=[place_of(v)[:2] for v in call.views], place=[place_of(v)[2:] for v in call.views], fill=FILL)
    if combo.get("affine"):
        kw.update(affine=[matrix_of(call, v, combo) for v in call.views], affine_resample=combo["affine"], affine_fill=AFFINE_FILL)
    if combo.get("perspective"):
        kw.update(perspective=[coeffs_of(call, v, combo) for v in call.views], affine_resample=combo["perspective"], affine_fill=transform_fill(combo))
    if combo.get("colour"):
        kw["color_ops"] = [chain_of(v) for v in call.views]
    if combo.get("orientation"):
        kw["orientation"] = [1] + [ORIENT[g] for g in call.gis]
    return kw


PER_BATCH = ("views", "mirror", "affine", "orientation", "color_ops", "perspective")         # what decode_device_iter takes batch by batch


def iter_kwargs(calls: List[ViewCall], cname: str) -> dict:
    """the keyword arguments of decode_device_iter for these batches: what is per view or per file as one iterator over the batches"""
    kws = [call_kwargs(c, cname) for c in calls]
    kw = {k: v for k, v in kws[0].items() if k not in PER_BATCH}
    for name in PER_BATCH:
        if name in kws[0]:
            kw[name] = iter([k[name] for k in kws])
    return kw


_rm = {}


def pixels_rm(e: CallFile) -> np.ndarray:
    if e.name not in _rm:
        _rm[e.name] = np.ascontiguousarray(e.full.swapaxes(0, 1))
    return _rm[e.name]


_expect = {}


def expect(call: ViewCall, v: View, cname: str, layout: str, window="own", matrix="own", place="own", mirror="own", chain="own",
           coeffs="own") -> np.ndarray:
    """One view's output under a combination: uint8 pixels or the bit patterns of float16.  window / matrix / place / mirror / chain /
    coeffs: the view's own, or another's — what a decoder that mixes views up would compute."""
    from tools import affine_model, colour_model, mode_model, normalize_model, orient_model, perspective_model, place_model
    combo = COMBOS[cname]
    e = call.entries[v.file - 1]
    win = window_of(call, v, combo) if window == "own" else window
    a = matrix_of(call, v, combo) if matrix == "own" else matrix
    pl = (place_of(v) if place == "own" else place) if combo.get("places") else SIZE + (0, 0)
    flip = (mirror_of(v) if mirror == "own" else mirror) if combo.get("mirror") else False
    c = coeffs_of(call, v, combo) if coeffs == "own" else coeffs
    ch = (chain_of(v) if chain == "own" else chain) if combo.get("colour") else None
    key = (e.name, cname, win, a, pl, c, ch)
    if key not in _expect:
        img = orient_model.orient(mode_model.convert(pixels_rm(e), combo.get("mode")), ORIENT[v.gi] if combo.get("orientation") else 1)
        x, y, w, h = win
        fill = AFFINE_FILL if img.ndim == 3 else AFFINE_FILL[0]
        if c is not None:
            part = perspective_model.transform(img, c, combo["perspective"], fill, win)
        elif a is not None:
            part = affine_model.transform(img, a, combo["affine"], fill, win)
        else:
            part = np.ascontiguousarray(img[y:y + h, x:x + w])
        out = place_model.place(part, pl[:2], pl[2:], SIZE, FILL if combo.get("places") else 0, combo.get("resample") or "bilinear")
        out = colour_model.apply_chain(out, ch)
        if combo.get("dtype"):
            out = normalize_model.normalize(out, combo["dtype"], *NORMALIZE)
        _expect[key] = out
    out = _expect[key]
    return as_layout(out[:, ::-1] if flip else out, layout)


def window_fits(call: ViewCall, v: View, combo: dict, win) -> bool:
    W, H = oriented_dims(call, v, combo)
    return win[0] + win[2] <= W and win[1] + win[3] <= H


def others_of(call: ViewCall, v: View) -> List[View]:
    """the view before it, the view after it, and a view of another file that is neither"""
    near = [call.views[k] for k in (v.k - 1, v.k + 1) if 0 <= k < len(call.views)]
    far = next(o for o in call.views[::-1] if o.file != v.file and o not in near)
    return near + [far]


def assert_expectations_tell_views_apart(call: ViewCall, cnames, layouts):
    """Without this the view-by-view comparison could pass for a decoder that mixes views up: the expectations of all views are
    pairwise different; each changes with its own flag; each changes when given the window, the matrix, the coefficients, the
    chain or the place of the view before it, of the view after it and of a view of another file — wherever that value is not its
    own, and where that window lies inside its image (elsewhere the plan is refused: no image comes of it)."""
    for cname in cnames:
        combo = COMBOS[cname]
        for layout in layouts:
            want = [expect(call, v, cname, layout) for v in call.views]
            for i in range(len(want)):
                for j in range(i):
                    assert differ(want[i], want[j]), (cname, layout, "views", j, i)
            for v in call.views:
                if combo.get("mirror"):
                    assert differ(want[v.k], expect(call, v, cname, layout, mirror=not mirror_of(v))), (cname, layout, v.k, "flag")
                for o in others_of(call, v):
                    win = window_of(call, o, combo)
                    if win != window_of(call, v, combo) and window_fits(call, v, combo, win):
                        assert differ(want[v.k], expect(call, v, cname, layout, window=win)), (cname, layout, v.k, "window of", o.k)
                    if combo.get("affine") and matrix_of(call, o, combo) != matrix_of(call, v, combo):
                        assert differ(want[v.k], expect(call, v, cname, layout, matrix=matrix_of(call, o, combo))), (cname, layout, v.k, "matrix of", o.k)
                    if combo.get("places"):
                        assert differ(want[v.k], expect(call, v, cname, layout, place=place_of(o))), (cname, layout, v.k, "place of", o.k)
                    if combo.get("colour") and chain_of(o) != chain_of(v):
                        assert differ(want[v.k], expect(call, v, cname, layout, chain=chain_of(o))), (cname, layout, v.k, "chain of", o.k)
                    if combo.get("perspective") and coeffs_of(call, o, combo) != coeffs_of(call, v, combo):
                        assert differ(want[v.k], expect(call, v, cname, layout, coeffs=coeffs_of(call, o, combo))), (cname, layout, v.k, "coefficients of", o.k)


def assert_the_call_is_interleaved(call: ViewCall):
    files = [v.file for v in call.views]
    assert all(a != b for a, b in zip(files, files[1:])), "views of one file are adjacent"
    assert 28 <= len(files) <= 36 and set(files) == set(range(1, len(call.files))) and call.files[0] == JUNK
    per_file = [files.count(f) for f in range(1, len(call.files))]
    assert set(per_file) == {2, 3}
    tail, unconverged = positions(call.entries, "tail"), positions(call.entries, "unconverged")
    for pos in (tail, unconverged):
        assert len({(ORIENT[call.gis[i]] != 1) + (ORIENT[call.gis[i]] >= 5) for i in pos}) >= 2, "all in one orientation class"
    assert {(o != 1) + (o >= 5) for o in ORIENT} == {0, 1, 2}
    for cname, combo in COMBOS.items():
        mats = [matrix_of(call, v, combo) for v in call.views]
        if combo.get("affine"):
            assert any(m is None for m in mats) and len({m for m in mats if m is not None}) == sum(m is not None for m in mats)
            assert all(m is None for m, v in zip(mats, call.views) if v.gi == UNTRANSFORMED)
        if combo.get("affine") == "nearest":
            assert sum(m is not None and m[1] == 0 and m[3] == 0 for m in mats) >= 5
        cs = [coeffs_of(call, v, combo) for v in call.views]
        if combo.get("perspective"):
            assert sum(c is None for c in cs) > sum(v.gi == UNTRANSFORMED for v in call.views), "no view of a transformed file without coefficients"
            assert len({c for c in cs if c is not None}) == sum(c is not None for c in cs) >= 20
            assert all(c is None for c, v in zip(cs, call.views) if v.gi == UNTRANSFORMED)
            assert all(mats[k] is None for k in range(len(mats)))
        else:
            assert all(c is None for c in cs)
    from tools import colour_model
    chains = [chain_of(v) for v in call.views]
    real = [c for c in chains if c is not None]
    assert all(c is None for c, v in zip(chains, call.views) if v.gi == UNTRANSFORMED)
    assert len(chains) - len(real) > sum(v.gi == UNTRANSFORMED for v in call.views), "no view of another file without a chain"
    assert len(set(real)) == len(real) >= 20 and {len(c) for c in real} == {1, 2, 3, 4}
    assert {op[0] for c in real for op in c} == set(colour_model.OPS), "an op kind that no chain of the call has"
    assert sum(any(op[0] in HIST_OPS for op in c) for c in real) >= 5
    radii = [op[1] for c in real for op in c if op[0] in BLUR_OPS]
    assert sum(any(op[0] in BLUR_OPS for op in c) for c in real) >= 5 and len(set(radii)) == len(radii)
    assert {c.index(("equalize",)) for c in real if ("equalize",) in c} == {0, 1}, "no op stands at two positions"
    flags = [mirror_of(v) for v in call.views]
    assert 10 <= sum(flags) <= len(flags) - 10
    assert len({place_of(v) for v in call.views}) == len(call.views)


def check_outputs(got, call: ViewCall, cname: str, layout: str, what):
    from routes_common import bits_of
    assert len(got) == len(call.views), what
    got = bits_of(got) if len(call.views) else got
    for v in call.views:
        want = expect(call, v, cname, layout)
        assert got[v.k].dtype == want.dtype and got[v.k].shape == want.shape, (what, v.k, got[v.k].shape, want.shape)
        assert np.array_equal(got[v.k], want), (what, "view", v.k, "of file", v.file)


# ---- reading the plans of a call ------------------------------------------------------------------------------------------------------
@dataclass
class ViewPlanRecord:
    rec: object                 # routes_common.PlanRecord
    kw: dict                    # the keywords the plan was given
    plan: object = None


@dataclass
class Bare:
    affine: int = 0
    perspective: int = 0
    colour: int = 0


def assert_bare_plans(bare: Bare, call: ViewCall, cname: str, what):
    """the call's file without a transformed view and without a chain made a plan: the checks that such a plan carries no affine, no
    perspective and no colour ran on something"""
    if UNTRANSFORMED in call.gis:
        for name in ("affine", "perspective", "colour"):
            assert getattr(bare, name) >= 1 or not COMBOS[cname].get(name), (what, f"no plan without {name}")


def assert_plans_hold_their_views(records: List[ViewPlanRecord], call: ViewCall, cname: str, on_device: bool, what):
    """every plan against the call: its slots are exactly the call positions of the views of its files, in view order; its views
    name plan-local files and those views' own windows; its matrices or coefficients, chains, places and mirror flags are those
    views' own; a plan whose views are all untransformed carries neither affine nor perspective, one whose views all have no chain
    no colour.  Returns Bare: how many plans carried no affine though the call had matrices, no perspective though it had
    coefficients, no colour though it had chains."""
    combo = COMBOS[cname]
    bare = Bare()
    for r in records:
        held = files_of(r.rec, call.files)                      # positions in the caller's list, in the plan's order
        assert 0 not in held
        mine = [v for v in call.views if v.file in held]
        kw = r.kw
        assert kw.get("rois") is None and kw["size"] == SIZE, what
        if on_device:
            assert kw["slots"] is not None and [int(s) for s in kw["slots"][0]] == [v.k for v in mine] and int(kw["slots"][1]) == len(call.views), (what, kw["slots"], [v.k for v in mine])
        else:
            assert kw.get("slots") is None
        assert [(held[f], tuple(w)) for f, w in kw["views"]] == [(v.file, window_of(call, v, combo)) for v in mine], (what, held, kw["views"])
        if combo.get("mirror") or combo.get("dtype"):
            flags = kw["output"][3]
            assert (list(flags) if flags is not None else None) == ([mirror_of(v) for v in mine] if combo.get("mirror") else None), what
        else:
            assert kw.get("output") is None
        if combo.get("places"):
            assert [tuple(p) for p in kw["places"]] == [place_of(v) for v in mine] and tuple(kw["fill"]) == FILL, what
        else:
            assert kw.get("places") is None
        if combo.get("orientation"):
            turns = kw.get("orientation") or [1] * len(held)
            assert list(turns) == [([1] + [ORIENT[g] for g in call.gis])[i] for i in held], (what, turns, held)
        mats = [matrix_of(call, v, combo) for v in mine]
        if all(m is None for m in mats):
            assert kw.get("affine") is None, (what, "a plan without a transformed view carries affine")
            bare.affine += bool(combo.get("affine"))
        else:
            assert list(kw["affine"][0]) == mats and kw["affine"][1] == combo["affine"] and tuple(kw["affine"][2]) == AFFINE_FILL, what
        cs = [coeffs_of(call, v, combo) for v in mine]
        if all(c is None for c in cs):
            assert kw.get("perspective") is None, (what, "a plan without a transformed view carries perspective")
            bare.perspective += bool(combo.get("perspective"))
        else:
            fill = AFFINE_FILL[:1] if combo.get("mode") == "L" else AFFINE_FILL
            assert kw.get("affine") is None, (what, "a plan of a perspective call carries affine")
            assert list(kw["perspective"][0]) == cs and kw["perspective"][1] == combo["perspective"] and tuple(kw["perspective"][2]) == fill, what
        chains = [chain_of(v) if combo.get("colour") else None for v in mine]
        if all(c is None for c in chains):
            assert kw.get("colour") is None, (what, "a plan whose views all have no chain carries colour")
            bare.colour += bool(combo.get("colour"))
        else:
            assert [tuple(c) if c is not None else None for c in kw["colour"]] == chains, (what, kw["colour"], chains)
    return bare
