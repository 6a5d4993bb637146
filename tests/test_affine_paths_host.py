"""The cases of tests/test_affine_paths.py, held on the CPU to what they are meant to reach (no GPU): with the model alone, on
the golden pixels, every table case has its runs of -1, every clamp case clamps on both sides, every edge case meets every edge
of the image — tests/affine_cases.census, with the thresholds of the cases' statement — and the expectation of every case differs
from that of each wrong variant of the transform it must tell apart (`variant`, a local restatement of
tools/affine_model.transform with one thing wrong).  A GPU run that passes then means something.

The variants and where they apply:
  tables_from_0, neighbour_tables   every table case (kind 1)
  no_clamp                          every bicubic case with a clamped value
  other_orientation                 every case, each of the other seven orientations — on the checker fixtures but those under which
                                    the ideal board gives the case the same bytes (the board is its own mirror image top to bottom,
                                    and its pattern of cells is its own transpose): at most three of the seven
                                    (the whole 512 x 512 transforms: two other orientations, for the time they take)
  luma_after                        photographic colour files as "L", bilinear and bicubic (the checkerboard's components are equal)
  fill_reversed                     three-component outputs with fill pixels
  origin_folded, fused,             a change of the LAST bit of a source coordinate (fix_truncates: of a fixed-point entry, NEAREST
  fix_truncates                     in fixed point).  It shows only where a coordinate lies within an ulp of a whole number, which
                                    a matrix of arbitrary entries does not produce in a few thousand pixels; the `tenths` matrices
                                    (affine_cases.tenths) do, for a fifth of their pixels.  So these are held on every `tenths`
                                    case — there is one among the tables, one per orientation call, one per tile plan and one
                                    per row-tail call — not on every case, and under bicubic (where the cubic at a distance within
                                    an ulp of 0 or 1 mostly rounds to the tap itself) only where they show.
The fused multiply-add is emulated with exact rational arithmetic (Python 3.10 has no math.fma)."""
from fractions import Fraction

import numpy as np
import pytest

import affine_cases as AC
from affine_cases import Case, buffer, case_census, census, pixels, source


def variant(c: Case, what: str, other: Case = None, orientation: int = None, px: np.ndarray = None) -> np.ndarray:
    """`buffer(c)` with one thing wrong.  tools/affine_model.transform restated, so that each step can be swapped."""
    from tools import mode_model
    from tools.affine_model import _cubic, scale_table
    if what == "luma_after":
        rgb = variant(Case(c.name, c.file, c.a, c.resample, c.window, c.orientation, None), "right")
        out = mode_model.convert(rgb, "L")
        out[(rgb == np.array(AC.FILL3, np.uint8)).all(axis=2)] = AC.FILL1         # (the fill is the call's, not a converted one)
        return out
    img = source(c, px, orientation=orientation)
    src = img.reshape(img.shape[0], img.shape[1], -1)
    h, w, C = src.shape
    x0, y0, ww, wh = c.window
    a = [float(v) for v in c.a]
    fill = c.fill if what != "fill_reversed" else c.fill[::-1]
    if what == "origin_folded":
        a[2], a[5] = a[0] * x0 + a[1] * y0 + a[2], a[3] * x0 + a[4] * y0 + a[5]
        x0 = y0 = 0
    out = np.empty((wh, ww, C), dtype=np.uint8)
    out[:] = np.broadcast_to(np.asarray(fill, dtype=np.uint8), (C,))
    X, Y = np.meshgrid(np.arange(x0, x0 + ww, dtype=np.int64), np.arange(y0, y0 + wh, dtype=np.int64))
    if c.resample == "nearest":
        if a[1] == 0 and a[3] == 0:
            if what == "tables_from_0":
                tx, ty = scale_table(a[0], a[2], w, ww), scale_table(a[4], a[5], h, wh)
            elif what == "neighbour_tables":
                b, (bx, by) = [float(v) for v in other.a], other.window[:2]
                tx, ty = scale_table(b[0], b[2], w, bx + ww)[bx:], scale_table(b[4], b[5], h, by + wh)[by:]
            else:
                tx, ty = scale_table(a[0], a[2], w, x0 + ww)[x0:], scale_table(a[4], a[5], h, y0 + wh)[y0:]
            sx, sy = tx[None, :].repeat(wh, 0), ty[:, None].repeat(ww, 1)
        else:
            fix = (lambda v: int(v * 65536.0 + 0.5)) if what == "fix_truncates" else (lambda v: int(np.floor(v * 65536.0 + 0.5)))
            A = [fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]
            wrap = lambda v: ((v + (1 << 31)) % (1 << 32)) - (1 << 31)          # noqa: E731
            sx, sy = wrap(A[2] + X * A[0] + Y * A[1]) >> 16, wrap(A[5] + X * A[3] + Y * A[4]) >> 16
        ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        out[ok] = src[sy[ok], sx[ok]]
        return out.reshape((wh, ww) + img.shape[2:])
    xc, yc = X + 0.5, Y + 0.5
    if what == "fused":
        # what a compiler that contracts makes of a0 * xc + a1 * yc + a2: fma(a1, yc, a0 * xc) + a2
        def line(p, q, r):
            Q = Fraction(q)
            first = p * xc
            return np.array([[float(Q * Fraction(float(yc[j, i])) + Fraction(float(first[j, i]))) for i in range(ww)] for j in range(wh)]) + r
        xin, yin = line(a[0], a[1], a[2]), line(a[3], a[4], a[5])
    else:
        xin, yin = a[0] * xc + a[1] * yc + a[2], a[3] * xc + a[4] * yc + a[5]
    ok = ~((xin < 0.0) | (xin >= w) | (yin < 0.0) | (yin >= h))
    xin, yin = xin[ok] - 0.5, yin[ok] - 0.5
    ix, iy = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - ix)[:, None], (yin - iy)[:, None]
    s = src.astype(np.float64)
    if c.resample == "bilinear":
        c0, c1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)

        def row(r):
            return s[r, c0] + (s[r, c1] - s[r, c0]) * dx
        v1 = row(np.clip(iy, 0, h - 1))
        v2 = np.where(((iy + 1 >= 0) & (iy + 1 < h))[:, None], row(np.clip(iy + 1, 0, h - 1)), v1)
        out[ok] = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)
    else:
        cols = [np.clip(ix + k, 0, w - 1) for k in (-1, 0, 1, 2)]

        def row(r):
            return _cubic(s[r, cols[0]], s[r, cols[1]], s[r, cols[2]], s[r, cols[3]], dx)
        v = [row(np.clip(iy - 1, 0, h - 1))]
        for k in (0, 1, 2):
            v.append(np.where(((iy + k >= 0) & (iy + k < h))[:, None], row(np.clip(iy + k, 0, h - 1)), v[-1]))
        t = _cubic(v[0], v[1], v[2], v[3], dy)
        if what == "no_clamp":
            out[ok] = (np.trunc(t).astype(np.int64) & 255).astype(np.uint8)
        else:
            out[ok] = np.where(t <= 0.0, 0, np.where(t >= 255.0, 255, np.trunc(np.clip(t, 0.0, 255.0)))).astype(np.uint8)
    return out.reshape((wh, ww) + img.shape[2:])


def differs(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape != b.shape or not np.array_equal(a, b)


def is_tenths(c: Case) -> bool:
    return c.a is not None and tuple(c.a[k] for k in (0, 1, 3, 4)) == (0.8, 0.6, -0.6, 0.8)


def assert_told_apart(cases, neighbours=True, orientations=range(1, 9)):
    """every case of one call against every variant that applies to it; returns the variants that were held"""
    held = set()
    table = [c for c in cases if c.a is not None and c.resample == "nearest" and c.a[1] == 0 and c.a[3] == 0]
    for c in cases:
        if c.a is None:
            continue
        right = buffer(c)
        assert np.array_equal(variant(c, "right"), right), (c.name, "the restatement is not the model")
        todo = []
        if c in table:
            todo.append(("tables_from_0", {}))
            if neighbours:
                k = table.index(c)
                todo += [("neighbour_tables", {"other": table[j]}) for j in (k - 1, k + 1) if 0 <= j < len(table)]
        if c.resample == "bicubic" and case_census(c)["below"] + case_census(c)["above"] > 0:
            todo.append(("no_clamp", {}))
        if c.resample != "nearest" and AC.COMPS[c.file] == 3 and c.mode == "L" and not c.file.startswith("checker_"):
            todo.append(("luma_after", {}))
        if c.ncomp == 3 and case_census(c)["fill"]:
            todo.append(("fill_reversed", {}))
        if is_tenths(c) and c.window[2] * c.window[3] <= 4096:
            todo.append(("origin_folded", {}))
            todo.append(("fused", {}) if c.resample != "nearest" else ("fix_truncates", {}))
        turns = [o for o in orientations if o != c.orientation]
        if c.file.startswith("checker_"):
            # the board is its own mirror image top to bottom (five rows of cells), and its cells' pattern is its own transpose:
            # an orientation under which the IDEAL board gives this case the same bytes cannot be told apart on the decoded one
            # either, and only such an orientation is left out — at most three of the seven
            ideal = AC.ideal_checker(c.file)
            turns = [o for o in turns if differs(variant(c, "right", orientation=o, px=ideal), variant(c, "right", px=ideal))]
            assert len(turns) >= 4, (c.name, turns)
        todo += [("other_orientation", {"orientation": o}) for o in turns]
        for what, kw in todo:
            wrong = variant(c, "right" if what == "other_orientation" else what, **kw)
            if c.resample == "bicubic" and what in ("origin_folded", "fused") and not differs(wrong, right):
                continue            # (the cubic at d within an ulp of 0 or 1 mostly rounds to the tap itself: held where it shows)
            assert differs(wrong, right), (c.name, what, kw.get("orientation"), getattr(kw.get("other"), "name", None))
            held.add(what)
    return held


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
def test_the_checker_fixtures_are_black_and_white():
    import json
    from conftest import GOLDEN
    index = json.loads((GOLDEN / "files" / "index.json").read_text())
    for name in (AC.CHECK3, AC.CHECK1):
        px = pixels(name)
        assert px.shape == ((40, 48, 3) if name == AC.CHECK3 else (40, 48)) and AC.path(name).stat().st_size < 4096
        assert (px <= 3).mean() >= 0.40 and (px >= 252).mean() >= 0.40, (name, (px <= 3).mean(), (px >= 252).mean())
        assert name not in index


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def test_table_cases_have_runs_of_minus_one_at_both_ends():
    """"a leading and a trailing run of -1 on at least one axis" is held for the two scale matrices on the WHOLE image, as the
    figures it was stated with were measured.  A 40 x 24 window cannot span their inside runs (56 columns, 32 rows), so of the
    plan's windows s1_lead / s2_lead meet the leading runs, s1_trail / s2_trail the trailing ones, and only s3_both — a stronger
    shrink — has both runs, on both axes, in one window."""
    cases = AC.table_cases()
    assert len(cases) >= 7 and len({c.window[:2] for c in cases}) == len(cases) and all(c.size == (AC.TW, AC.TH) for c in cases)
    by = {c.name: c for c in cases}
    px = pixels(AC.NOISE)
    # the two scale matrices on the whole image: a leading AND a trailing run on at least one axis, at least 30 % inside (s3
    # has both in its one window, below)
    for name, m in (("s1", AC.S1), ("s2", AC.S2)):
        n = census(px, m, "nearest")
        assert (n["x_lead"] > 0 and n["x_trail"] > 0) or (n["y_lead"] > 0 and n["y_trail"] > 0), (name, n)
        assert n["inside"] >= 0.30 * n["pixels"], (name, n)
    assert [census(px, AC.S1, "nearest")[k] for k in ("x_lead", "x_trail", "y_lead")] == [12, 28, 13]
    assert [census(px, AC.S2, "nearest")[k] for k in ("y_lead", "y_trail")] == [15, 17]
    # ... and over the windows the plan uses: each scale matrix meets its leading and its trailing run, every window is at
    # least 30 % inside, and one window (s3) has both runs on both axes at once
    n = {c.name: case_census(c) for c in cases if c.a is not None}
    for name in ("s1_lead", "s2_lead", "s1_trail", "s2_trail", "s3_both", "flip", "shift"):
        assert n[name]["inside"] >= 0.30 * n[name]["pixels"], (name, n[name])
    assert n["s1_lead"]["x_lead"] > 0 and n["s1_lead"]["y_lead"] > 0 and n["s1_trail"]["x_trail"] > 0
    assert n["s2_lead"]["y_lead"] > 0 and n["s2_trail"]["y_trail"] > 0
    assert all(n["s3_both"][k] > 0 for k in ("x_lead", "x_trail", "y_lead", "y_trail"))
    # the flip's table runs backwards and the shift's rows begin outside the image: neither can have runs at both ends of an
    # axis (their entries step by one), so they are held to what they are there for
    from tools.affine_model import scale_table
    tx = scale_table(-1.0, 96.0, 96, 96)
    assert tx.tolist() == list(range(95, -1, -1)) and n["flip"]["inside"] == n["flip"]["pixels"]
    assert n["shift"]["y_lead"] == 3 and n["shift"]["x_lead"] == n["shift"]["x_trail"] == 0
    # the two fixed-point views: negative sums (an arithmetic shift) in both, a negative entry in both
    for name in ("rotation", "tenths"):
        assert by[name].a[1] != 0 and n[name]["fill"] >= 3 and n[name]["inside"] >= 0.30 * n[name]["pixels"], (name, n[name])
    assert n["rotation"]["negative"] >= 3
    assert sum(c.a is None for c in cases) == 1 and sum(c.a == AC.S1 for c in cases) == 2 and by["s1_trail"].window[:2] != (0, 0)


def test_table_cases_tell_the_wrong_variants_apart():
    cases = AC.table_cases()
    held = assert_told_apart(cases)
    assert held >= {"tables_from_0", "neighbour_tables", "fix_truncates", "origin_folded", "other_orientation", "fill_reversed"}, held
    # reversed, every view gets other table offsets: the neighbours are then the other way round, which the above covers, and
    # all expectations are pairwise different, so a view that got another's record shows
    bufs = [buffer(c) for c in cases]
    assert all(differs(bufs[i], bufs[j]) for i in range(len(bufs)) for j in range(i))


# ---- the clamp -------------------------------------------------------------------------------------------------------------------------
def test_clamp_cases_clamp_on_both_sides():
    cases = AC.clamp_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        n = case_census(c)
        if c.file in (AC.Q98, AC.NOISE):
            # RGB noise: at least 1 % of the inside component values below 0 and 0.4 % above 255
            assert n["below"] >= 0.01 * n["values"] and n["above"] >= 0.004 * n["values"], (c.name, n)
        else:
            assert n["below"] >= 0.05 * n["values"] and n["above"] >= 0.05 * n["values"], (c.name, n)
    # one component: the three ways to it, each with the window the image and with a corner window
    assert {(c.file, c.mode) for c in cases if c.file.startswith("checker")} == {(AC.CHECK3, None), (AC.CHECK3, "L"), (AC.CHECK1, None), (AC.CHECK1, "RGB")}
    for f in (AC.Q98, AC.NOISE, AC.CHECK3, AC.CHECK1):
        mine = [c for c in cases if c.file == f]
        assert any(c.window == (0, 0) + AC.DIMS[f] for c in mine) and any(c.window[2] < AC.DIMS[f][0] and (c.window[0] == 0 or c.window[0] + c.window[2] == AC.DIMS[f][0]) for c in mine)


def test_clamp_cases_tell_the_wrong_variants_apart():
    held = assert_told_apart(AC.clamp_cases(), neighbours=False)
    assert held >= {"no_clamp", "other_orientation"}, held


# ---- orientations and edges --------------------------------------------------------------------------------------------------------
ORIENT_CALLS = [(f, r, m) for f in (AC.ODD, AC.GREY) for r in AC.FILTERS for m in (None, AC.other_mode(f))]


@pytest.mark.parametrize("file,resample,mode", ORIENT_CALLS, ids=[f"{f}-{r}-{m or 'own'}" for f, r, m in ORIENT_CALLS])
def test_orientation_cases_meet_every_edge_and_tell_the_variants_apart(file, resample, mode):
    cases = AC.orientation_cases(file, resample, mode)
    assert [c.orientation for c in cases] == list(range(1, 9)) and len({c.a for c in cases}) == 8
    for c in cases:
        ow, oh = AC.oriented(AC.DIMS[file], c.orientation)
        x, y, w, h = c.window
        assert x > 0 and y > 0 and x + w <= ow and y + h <= oh
        n = case_census(c)
        assert n["inside"] >= 0.30 * n["pixels"] and n["fill"] >= 3, (c.name, n)
    held = assert_told_apart(cases, neighbours=False)
    want = {"other_orientation"} | {"nearest": {"origin_folded", "fix_truncates"}, "bilinear": {"origin_folded", "fused"}, "bicubic": set()}[resample]
    want |= {"luma_after"} if (mode == "L" and resample != "nearest") else set()
    want |= {"fill_reversed"} if cases[0].ncomp == 3 else set()
    assert held >= want, (held, want)


@pytest.mark.parametrize("resample", ("bilinear", "bicubic"))
@pytest.mark.parametrize("file", (AC.ODD, AC.GREY))
def test_edge_cases_meet_every_edge_of_the_image(file, resample):
    """the cases that claim the image's edge, exactly as the GPU file runs them — every output the whole oriented image at its own
    size, orientations 1..4 in one call and 5..8 in another (and, bicubic, the clamp calls' rotations of the whole noise images):
    at least 3 pixels each with ix == -1, ix + 1 >= w, iy == -1, iy + 1 >= h"""
    groups = AC.edge_cases(file, resample)
    assert [[c.orientation for c in g] for g in groups] == [[1, 2, 3, 4], [5, 6, 7, 8]]
    claimed = [c for g in groups for c in g]
    if resample == "bicubic" and file == AC.ODD:
        claimed += [c for c in AC.clamp_cases() if c.name.endswith("_turn")]
        assert len(claimed) == 10
    for g in groups:
        assert len({c.size for c in g}) == 1 and all(c.window == (0, 0) + AC.oriented(AC.DIMS[file], c.orientation) for c in g)
    for c in claimed:
        n = case_census(c)
        assert min(n["ix_m1"], n["ix_hi"], n["iy_m1"], n["iy_hi"]) >= 3, (c.name, n)
        if resample == "bicubic":
            assert n["iy_hi2"] >= n["iy_hi"]
    for g in groups:
        assert "other_orientation" in assert_told_apart(g, neighbours=False)


# ---- tiles -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("rowmajor", "xmajor"))
def test_tile_cases_cover_the_grid_and_every_row_tail(layout):
    fast = 0 if layout == "rowmajor" else 1
    for resample in ("bilinear", "bicubic"):
        cases = AC.tile_cases(resample, layout)
        sizes = [c.size for c in cases]
        tiles = [((s[fast] + 63) // 64, (s[1 - fast] + 15) // 16) for s in sizes]
        # the whole image: 8 x 32 tiles; 1 x 1; exactly one tile; 2 x 2 tiles with one pixel in the second; a long thin one —
        # so most workgroups of the smaller windows take the early return, and the fast axis has more than two tiles
        assert tiles[0] == (8, 32) and sizes[1] == (1, 1) and tiles[2] == (1, 1) and sizes[2][fast] == 64 and sizes[2][1 - fast] == 16
        assert tiles[3] == (2, 2) and sizes[3][fast] == 65 and sizes[3][1 - fast] == 17 and sizes[4] == (300, 20)
        held = assert_told_apart(cases[1:], neighbours=False) | assert_told_apart(cases[:1], neighbours=False, orientations=(3, 6))
        assert held >= {"other_orientation"} | ({"origin_folded", "fused"} if resample == "bilinear" else set()), held
    seen3, seen1 = set(), set()
    for r in (1, 2, 3, 4):
        for mode, seen in ((None, seen3), ("L", seen1)):
            cases = AC.row_tail_cases(r, layout, mode)
            assert len(cases) == 3 and len({c.window[:2] for c in cases}) == 3
            for c in cases:
                x, y, w, h = c.window
                assert x + w <= 512 and y + h <= 512 and c.size[fast] == 64 + r and c.size[1 - fast] == 19
                seen.add(((c.size[fast] - 64) * c.ncomp) % 4)
                n = case_census(c)
                assert n["inside"] >= 0.30 * n["pixels"], (c.name, n)
            if r == 1:
                held = assert_told_apart(cases, neighbours=False)
                assert held >= {"other_orientation", "origin_folded", "fused"} | ({"luma_after"} if mode else set()), held
    # ne, the bytes of a row's last tile, at every remainder modulo 4 — for three components and for one
    assert seen3 == seen1 == {0, 1, 2, 3}


def test_the_models_resize_is_the_identity_at_the_windows_own_size():
    """what lets a call with size == window show every byte of the affine buffer"""
    from tools import resize_model
    rng = np.random.default_rng(7)
    sizes = {(AC.TW, AC.TH)} | {c.size for c in AC.clamp_cases()} | {c.size for f in (AC.ODD, AC.GREY) for c in AC.orientation_cases(f, "bilinear")}
    sizes |= {c.size for lay in ("rowmajor", "xmajor") for r in (1, 2, 3, 4) for c in AC.row_tail_cases(r, lay)}
    sizes |= {c.size for f in (AC.ODD, AC.GREY) for g in AC.edge_cases(f, "bilinear") for c in g}
    for w, h in sorted(sizes):
        for shape in ((h, w, 3), (h, w)):
            img = rng.integers(0, 256, shape, dtype=np.uint8)
            assert np.array_equal(resize_model.resize(img, (w, h)), img), (w, h)


def all_cases():
    """every case of tests/test_affine_paths.py, by name"""
    cases = AC.table_cases() + AC.clamp_cases()
    cases += [c for f, r, m in ORIENT_CALLS for c in AC.orientation_cases(f, r, m)]
    cases += [c for f in (AC.ODD, AC.GREY) for r in ("bilinear", "bicubic") for g in AC.edge_cases(f, r) for c in g]
    for layout in ("rowmajor", "xmajor"):
        tag = lambda c: Case(f"{c.name}_{layout}", c.file, c.a, c.resample, c.window, c.orientation, c.mode)          # noqa: E731
        cases += [tag(c) for r in ("bilinear", "bicubic") for c in AC.tile_cases(r, layout)]
        cases += [tag(c) for r in (1, 2, 3, 4) for m in (None, "L") for c in AC.row_tail_cases(r, layout, m)]
    assert len({c.name for c in cases}) == len(cases)
    return [c for c in cases if c.a is not None]


CENSUS_KEYS = ("pixels", "inside", "fill", "x_lead", "x_trail", "x_inside", "y_lead", "y_trail", "y_inside", "negative", "ix_m1", "ix_hi", "iy_m1",
               "iy_hi", "iy_hi2", "values", "below", "above")


def census_table():
    return ["case " + " ".join(CENSUS_KEYS)] + [c.name + " " + " ".join(str(case_census(c).get(k, "-")) for k in CENSUS_KEYS) for c in all_cases()]


def test_the_census_table_in_profiles_is_current():
    """profiles/affine_paths_census.txt holds what the committed cases reach (python tests/test_affine_paths_host.py rewrites it)"""
    from conftest import ROOT
    assert (ROOT / "profiles" / "affine_paths_census.txt").read_text().splitlines() == census_table()


if __name__ == "__main__":
    from conftest import ROOT
    (ROOT / "profiles" / "affine_paths_census.txt").write_text("\n".join(census_table()) + "\n")
