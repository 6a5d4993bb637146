"""patches= on the CPU: the rule (tools/patch_model.py) against torch's reshape / permute as transformers' Qwen2-VL image processor
and SigLIP 2's convert_image_to_patches write it (and against einops where it imports), the host twin mj_host_patchify against the
rule over the whole case list (tests/patch_cases.py), mj_host_patchify_count against patch_grids, every refusal of
normalize_patches and of the C ABI, the also= key, and smart_resize.  Bit patterns; no tolerance anywhere."""
import numpy as np
import pytest

from patch_cases import BITS, CANVASES, DTYPES, LAYOUTS, N_SOURCES, all_cases, full_windows, many_jobs_cases, model_patchify, random_bits, same_bits, tokens_in

CASES = all_cases()


def test_the_case_list_is_what_it_says():
    """every patch size, merge, repeat and order occurs; rows at every alignment; windows at odd origins, single blocks, bands and
    block columns, two sources with one window; whole canvases; both padded forms; and the random bits hold NaN patterns"""
    specs = [c[3] for c in CASES]
    assert {s["patch"] for s in specs} >= {1, 2, 3, 14, 16} and {s.get("merge", 1) for s in specs} == {1, 2, 3}
    assert {(s.get("repeat", 1), s.get("order", "chw")) for s in specs} == {(1, "chw"), (2, "chw"), (1, "hwc")}
    assert {c[2] for c in CASES} == {1, 3} and {c[1] for c in CASES} >= set(CANVASES)
    row_bytes = {c[2] * s.get("repeat", 1) * s["patch"] ** 2 for c, s in zip(CASES, specs)}
    assert {27, 196, 588} <= row_bytes
    assert any(s.get("windows") is None for s in specs) and any(s.get("windows") and None in s["windows"] for s in specs)
    for name, size, C, spec in CASES:
        wins = spec.get("windows")
        if name.startswith("grid_"):
            u = spec["patch"] * spec["merge"]
            assert wins[0] == wins[4] and wins[1][2:] == (u, u) and wins[2][3] == u and wins[3][2] == u, name
        if spec.get("length") is not None:
            assert max(tokens_in(spec, size)) <= spec["length"]
    exact = [c for c in CASES if c[0].startswith("padded_exact")]
    assert exact and all(max(tokens_in(c[3], c[1])) == c[3]["length"] > min(tokens_in(c[3], c[1])) for c in exact)
    assert any(w[0] % 2 and w[1] % 2 for c in CASES for w in (c[3].get("windows") or []) if w)
    f = random_bits("float32", "rowmajor", 48, 36, 3).view(np.float32)
    assert np.isnan(f).any() and np.isfinite(f).any()
    for name, size, C, dtype, spec in many_jobs_cases():
        x, y, w, h = spec["windows"][0]
        m, P = spec.get("merge", 1), spec["patch"]
        block = m * m * C * P * P * np.dtype(BITS[dtype]).itemsize
        assert block <= 65536 and (block == 65536) == name.startswith("largest_block"), name
    wide = many_jobs_cases()[0]
    assert wide[1][0] > 4200 and 4200 * 28 * 3 * 4 > 20 * 65536          # one band, a score of jobs at the very least


# ---- the rule is the processors' ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,m,t,gh,gw,C", [(14, 2, 2, 6, 4, 3), (2, 2, 2, 4, 6, 3), (3, 1, 1, 5, 7, 1), (2, 3, 1, 6, 3, 3), (1, 1, 2, 3, 2, 3), (16, 2, 1, 2, 2, 1)])
def test_the_chw_rule_is_qwen2_vls_expression(P, m, t, gh, gw, C):
    """images.reshape(B, C, gh // m, m, P, gw // m, m, P).permute(0, 2, 5, 3, 6, 1, 4, 7).unsqueeze(6).expand(..., t, ...).reshape(B, gh * gw,
    C * t * P * P): the flatten of transformers' Qwen2-VL image processor for a still image repeated along the temporal axis"""
    import torch
    from tools import patch_model
    B_ = 3
    img = np.random.default_rng(P * 100 + m).standard_normal((B_, C, gh * P, gw * P)).astype(np.float32)
    x = torch.from_numpy(img)
    want = (x.reshape(B_, C, gh // m, m, P, gw // m, m, P).permute(0, 2, 5, 3, 6, 1, 4, 7).unsqueeze(6)
            .expand(-1, -1, -1, -1, -1, -1, t, -1, -1).reshape(B_, gh * gw, C * t * P * P)).numpy()
    for b in range(B_):
        assert same_bits(patch_model.tokens_of(img[b], P, m, t, "chw"), want[b])
    got = patch_model.patchify(img if C == 3 else img[:, 0], dict(patch=P, merge=m, repeat=t), "planar_rowmajor")
    assert same_bits(got, want.reshape(B_ * gh * gw, -1))


@pytest.mark.parametrize("P,gh,gw,C", [(16, 3, 2, 3), (3, 5, 7, 3), (14, 2, 3, 1), (1, 4, 4, 3)])
def test_the_hwc_rule_is_siglip2s_expression(P, gh, gw, C):
    """image.reshape(C, gh, P, gw, P).permute(1, 3, 2, 4, 0).reshape(gh * gw, -1): convert_image_to_patches; padded, rows of zeros
    behind (pad_along_first_dim with value 0)"""
    import torch
    from tools import patch_model
    img = np.random.default_rng(P + gh).integers(0, 256, size=(C, gh * P, gw * P)).astype(np.uint8)
    want = torch.from_numpy(img).reshape(C, gh, P, gw, P).permute(1, 3, 2, 4, 0).reshape(gh * gw, -1).numpy()
    assert same_bits(patch_model.tokens_of(img, P, 1, 1, "hwc"), want)
    L = gh * gw + 5
    got = patch_model.patchify((img if C == 3 else img[0])[None], dict(patch=P, order="hwc", length=L), "planar_rowmajor")
    assert got.shape == (1, L, P * P * C) and same_bits(got[0, :gh * gw], want) and not got[0, gh * gw:].any()


@pytest.mark.parametrize("P,m,gh,gw", [(14, 2, 6, 4), (3, 3, 3, 6), (2, 1, 5, 3)])
def test_the_rule_is_an_einops_rearrange(P, m, gh, gw):
    einops = pytest.importorskip("einops")
    from tools import patch_model
    img = np.random.default_rng(7).standard_normal((3, gh * P, gw * P)).astype(np.float32)
    want = einops.rearrange(img, "c (by iy j) (bx ix i) -> (by bx iy ix) c j i", iy=m, ix=m, j=P, i=P)
    assert same_bits(patch_model.tokens_of(img, P, m, 1, "chw"), want.reshape(gh * gw, -1))
    want = einops.rearrange(img, "c (by iy j) (bx ix i) -> (by bx iy ix) j i c", iy=m, ix=m, j=P, i=P)
    assert same_bits(patch_model.tokens_of(img, P, m, 1, "hwc"), want.reshape(gh * gw, -1))


def test_the_model_in_the_four_layouts_is_one_model():
    """the same (C, H, W) content in every layout gives the same token rows"""
    from tools.erase_model import chw_view
    for name, size, C, spec in CASES[::3]:
        base = np.array(random_bits("float16", "planar_rowmajor", size[0], size[1], C))
        want = model_patchify(base, spec, "planar_rowmajor")
        for layout in LAYOUTS:
            pre = np.empty_like(np.array(random_bits("float16", layout, size[0], size[1], C)))
            for k in range(len(pre)):
                chw_view(pre[k], layout)[...] = chw_view(base[k], "planar_rowmajor")
            assert same_bits(model_patchify(pre, spec, layout), want), (name, layout)


# ---- the host twin ----------------------------------------------------------------------------------------------------------
def guarded(shape, dtype):
    """(the whole buffer, the exactly sized array inside it between two guards of 64 sentinel bytes)"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    buf = np.full(64 + n + 64, 0xA5, dtype=np.uint8)
    return buf, buf[64:64 + n].view(dtype).reshape(shape)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_host_twin_against_the_model(layout, dtype):
    """mj_host_patchify on exactly sized arrays of random bits, NaN patterns among them: every case; the guards around the
    destination and the source stay as they were"""
    from pyjpegdecoder_amd import _binding as B
    for name, size, C, spec in CASES:
        pre = np.array(random_bits(dtype, layout, size[0], size[1], C))
        kept = pre.copy()
        want = model_patchify(pre, spec, layout)
        buf, dst = guarded(want.shape, pre.dtype)
        B.host_patchify(pre, LAYOUTS.index(layout), dtype, C, size, full_windows(spec, size), dst=dst)
        assert same_bits(dst, want), (name, layout, dtype)
        assert (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all() and same_bits(pre, kept), name


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_host_twin_on_many_jobs(layout):
    from pyjpegdecoder_amd import _binding as B
    for name, size, C, dtype, spec in many_jobs_cases():
        pre = np.array(random_bits(dtype, layout, size[0], size[1], C, n=1))
        want = model_patchify(pre, spec, layout)
        buf, dst = guarded(want.shape, pre.dtype)
        B.host_patchify(pre, LAYOUTS.index(layout), dtype, C, size, spec, dst=dst)
        assert same_bits(dst, want) and (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all(), (name, layout)


def test_the_row_count_against_patch_grids():
    from pyjpegdecoder_amd import _binding as B, patch_grids
    for name, size, C, spec in CASES:
        grids, cu = patch_grids(spec, N_SOURCES, size)
        assert grids.shape == (N_SOURCES, 2) and cu.shape == (N_SOURCES + 1,) and cu[0] == 0
        assert list(grids[:, 0] * grids[:, 1]) == tokens_in(spec, size) == list(np.diff(cu)), name
        rows = B.host_patchify_count(1, "float16", C, size, N_SOURCES, full_windows(spec, size))
        assert rows == (cu[-1] if spec.get("length") is None else N_SOURCES * spec["length"]), name
        want = model_patchify(np.array(random_bits("uint8", "rowmajor", size[0], size[1], C)), spec, "rowmajor")
        assert int(np.prod(want.shape[:-1])) == rows and want.shape[-1] == C * spec.get("repeat", 1) * spec["patch"] ** 2


# ---- what is refused ----------------------------------------------------------------------------------------------------------
OK = dict(patch=2, merge=2)


@pytest.mark.parametrize("kw,msg", [
    (dict(patches=OK, size=None), "patches needs size"),
    (dict(patches=OK, return_seams=True), "patches and return_seams do not go together"),
    (dict(patches=[OK]), "patches must be None or a dict"),
    (dict(patches=dict(OK, stride=2)), "patches: unknown key 'stride'"),
    (dict(patches=dict(merge=2)), "patches: patch must be an integer 1..64, not None"),
    (dict(patches=dict(patch=0)), "patches: patch must be an integer 1..64, not 0"),
    (dict(patches=dict(patch=65)), "patches: patch must be an integer 1..64, not 65"),
    (dict(patches=dict(patch=2.0)), "patches: patch must be an integer 1..64, not 2.0"),
    (dict(patches=dict(patch=2, merge=9)), "patches: merge must be an integer 1..8, not 9"),
    (dict(patches=dict(patch=2, merge=0)), "patches: merge must be an integer 1..8, not 0"),
    (dict(patches=dict(patch=2, repeat=5)), "patches: repeat must be an integer 1..4, not 5"),
    (dict(patches=dict(patch=2, repeat="2")), "patches: repeat must be an integer 1..4, not '2'"),
    (dict(patches=dict(patch=2, order="cwh")), "patches: order must be 'chw' or 'hwc', not 'cwh'"),
    (dict(patches=dict(patch=2, order="hwc", repeat=2)), "patches: order 'hwc' needs repeat 1, not 2"),
    (dict(patches=dict(patch=2, length=0)), "patches: length must be None or an integer of at least 1, not 0"),
    (dict(patches=dict(patch=2, length=1.5)), "patches: length must be None or an integer of at least 1, not 1.5"),
    (dict(patches=dict(OK, windows=[(0, 0, 4, 4)]), n_outputs=2), "patches: windows has 1 entries for 2 sources"),
    (dict(patches=dict(OK, windows=(0, 0, 4, 4)), n_outputs=4), "patches: source 0: a window is None or four integers"),
    (dict(patches=dict(OK, windows=[None, (0, 0, 4)]), n_outputs=2), r"patches: source 1: a window is None or four integers \(x, y, width, height\), not \(0, 0, 4\)"),
    (dict(patches=dict(OK, windows=[None, (0, 0, 4, 4.0)]), n_outputs=2), "patches: source 1: a window is None or four integers"),
    (dict(patches=dict(OK, windows=[None, (42, 0, 8, 4)]), n_outputs=2), r"patches: source 1: window \(42, 0, 8, 4\) is not inside the 48 x 36 canvas"),
    (dict(patches=dict(OK, windows=[None, (-4, 0, 8, 4)]), n_outputs=2), r"patches: source 1: window \(-4, 0, 8, 4\) is not inside"),
    (dict(patches=dict(OK, windows=[None, (0, 0, 0, 4)]), n_outputs=2), r"patches: source 1: window \(0, 0, 0, 4\) is not inside"),
    (dict(patches=dict(OK, windows=[None, (1, 1, 6, 4)]), n_outputs=2), r"patches: source 1: window \(1, 1, 6, 4\) is not a multiple of patch \* merge = 4 per side"),
    (dict(patches=dict(patch=5), n_outputs=2), r"patches: source 0: the whole 48 x 36 canvas is not a multiple of patch \* merge = 5 per side"),
    (dict(patches=OK, size=(45, 33), n_outputs=2), r"patches: source 0: the whole 45 x 33 canvas is not a multiple of patch \* merge = 4"),
    (dict(patches=dict(OK, windows=[(0, 0, 4, 4), None]), size=(45, 33), n_outputs=2), r"patches: source 1: the whole 45 x 33 canvas is not a multiple"),
    (dict(patches=dict(OK, length=100, windows=[(0, 0, 4, 4), (0, 0, 24, 20)]), n_outputs=2), "patches: source 1: 120 tokens, more than length 100"),
    (dict(patches=dict(patch=64, merge=5), size=(320, 320)), "patches: a merge block of 102400 bytes"),
    (dict(patches=dict(patch=64, merge=2), size=(128, 128), ncomp=3, dtype="float32"), r"patches: a merge block of 196608 bytes \(merge 2, patch 64, repeat 1, 3 components of 4 bytes\), more than 65536"),
    (dict(patches=dict(OK, windows=[None] * 3), n_outputs=5, compose=dict(size=(8, 8), outputs=[[], []])), "patches: windows has 3 entries for 2 sources"),
    (dict(patches=OK, n_outputs=5, compose=dict(size=(9, 8), outputs=[[], []])), "patches: source 0: the whole 9 x 8 canvas is not a multiple"),
])
def test_what_normalize_patches_refuses(kw, msg):
    from pyjpegdecoder_amd import normalize_patches
    kw = dict(dict(size=(48, 36)), **kw)
    with pytest.raises(ValueError, match=msg):
        normalize_patches(**kw)


def test_what_normalize_patches_returns():
    from pyjpegdecoder_amd import normalize_patches
    assert normalize_patches(None, None) is None and normalize_patches(None, (48, 36), return_seams=True) is None
    assert normalize_patches(dict(patch=np.int64(4)), (48, 36), 3) == dict(patch=4, merge=1, repeat=1, order="chw", length=None, windows=None)
    got = normalize_patches(dict(patch=2, merge=3, repeat=2, length=np.int32(500), windows=[None, [6, 0, 12, 6]]), (48, 36), 2, 3, "bfloat16")
    assert got == dict(patch=2, merge=3, repeat=2, order="chw", length=500, windows=[(0, 0, 48, 36), (6, 0, 12, 6)])
    # under compose the sources are the composed canvases
    got = normalize_patches(dict(patch=5, windows=[None, (5, 5, 10, 5)]), (48, 36), 7, compose=dict(size=(20, 15), outputs=[[], []]))
    assert got["windows"] == [(0, 0, 20, 15), (5, 5, 10, 5)]
    # a block of exactly 65536 bytes is taken
    assert normalize_patches(dict(patch=64, merge=2), (128, 128), 1, 1, "float32")["patch"] == 64


def test_an_also_entry_has_its_own_patches():
    from pyjpegdecoder_amd.batch import ALSO_PER_OUTPUT, normalize_also
    assert "patches" in ALSO_PER_OUTPUT
    call = dict(size=(48, 36), patches=dict(patch=4))
    groups = normalize_also([dict(size=(8, 8), patches=dict(patch=2, merge=2)), dict(size=(10, 10))], call, (48, 36))
    assert groups[0]["patches"] == dict(patch=2, merge=2) and groups[1]["patches"] is None         # (never the call's)
    with pytest.raises(ValueError, match=r"also\[0\]: patches: source 0: the whole 10 x 8 canvas is not a multiple of patch \* merge = 4"):
        normalize_also([dict(size=(10, 8), patches=dict(patch=2, merge=2))], call, (48, 36))
    with pytest.raises(ValueError, match=r"also\[1\]: patches: unknown key 'p'"):
        normalize_also([dict(size=(8, 8)), dict(size=(8, 8), patches=dict(p=2))], call, (48, 36))
    groups = normalize_also([dict(size=(8, 8), compose=dict(size=(20, 12), outputs=[[(0, (1, 1))]]), patches=dict(patch=4, windows=[(4, 4, 16, 8)]))], call, (48, 36))
    assert groups[0]["patches"]["windows"] == [(4, 4, 16, 8)]


def test_what_the_c_abi_refuses():
    """mj_host_patchify and mj_host_patchify_count: MJ_ERR_INVALID with a message that names the source — and nothing is written"""
    from pyjpegdecoder_amd import _binding as B
    src = np.array(random_bits("float32", "rowmajor", 48, 36, 3)[:2])
    buf, dst = guarded((2 * 24 * 18, 12), np.uint32)

    def both(spec, msg, s=src, d=dst, layout=1, dtype="float32", C=3, size=(48, 36)):
        with pytest.raises(ValueError, match="mj_host_patchify: " + msg):
            B.host_patchify(s, layout, dtype, C, size, spec, dst=d)
        with pytest.raises(ValueError, match="mj_host_patchify_count: " + msg):
            B.host_patchify_count(layout, dtype, C, size, len(s), spec)
    both(dict(patch=0), "patch 0 is not 1..64")
    both(dict(patch=65), "patch 65 is not 1..64")
    both(dict(patch=2, merge=0), "merge 0 is not 1..8")
    both(dict(patch=2, merge=9), "merge 9 is not 1..8")
    both(dict(patch=2, repeat=0), "repeat 0 is not 1..4")
    both(dict(patch=2, repeat=5), "repeat 5 is not 1..4")
    both(dict(patch=2, repeat=2, order="hwc"), "order hwc needs repeat 1, not 2")
    both(dict(patch=2, length=-3), "length -3 is below 0")
    both(dict(patch=2, length=431), r"source 0 \(the whole canvas 0, 0, 48 x 36\): 432 tokens, more than length 431")
    both(dict(patch=5), r"source 0 \(the whole canvas 0, 0, 48 x 36\): width and height must be multiples of patch \* merge = 5")
    both(dict(patch=2, merge=2, windows=[(0, 0, 48, 36), (1, 1, 6, 4)]), r"source 1 \(window 1, 1, 6 x 4\): width and height must be multiples of patch \* merge = 4")
    both(dict(patch=2, windows=[(0, 0, 48, 36), (2, 0, 48, 36)]), r"source 1 \(window 2, 0, 48 x 36\): the window is not inside the source canvas")
    both(dict(patch=2, windows=[(0, 0, 48, 36), (0, -2, 48, 36)]), r"source 1 .*the window is not inside the source canvas")
    both(dict(patch=2, windows=[(0, 0, 48, 36), (0, 0, 48, 0)]), r"source 1 .*a width or height below 1")
    both(dict(patch=64, merge=3), r"a merge block of 442368 bytes \(merge 3, patch 64, repeat 1, 3 components of 4 bytes\), more than 65536")
    both(dict(patch=2), "layout 4, 3 components", layout=4)
    both(dict(patch=2), "layout 1, 2 components", C=2)
    both(dict(patch=2), "layout 1, 3 components, 2 sources of 0 x 36", size=(0, 36))
    both(dict(patch=2), "layout 1, 3 components, 2 sources of 48 x 65536", size=(48, 65536))
    both(dict(patch=2), "layout 1, 3 components, 0 sources", s=src[:0])
    with pytest.raises(ValueError, match="windows for 2 sources"):
        B.host_patchify(src, 1, "float32", 3, (48, 36), dict(patch=2, windows=[(0, 0, 48, 36)]), dst=dst)
    ok = dict(patch=2)
    L = B.load_library()
    for s, d, msg in [(None, dst, "NULL argument"), (src, None, "NULL argument"), (src, src, "src and dst overlap"),
                      (src, src.reshape(-1)[100:], "src and dst overlap")]:
        rc = L.mj_host_patchify(B._ptr(s), B._ptr(d), 1, B.DTYPES["float32"], 3, 48, 36, 2, 2, 1, 1, 0, 0, None)
        assert rc != B.MJ_OK and msg in L.mj_last_error(None).decode()
    odd = buf[66:66 + dst.nbytes]                       # (two bytes past a four-byte boundary)
    rc = L.mj_host_patchify(B._ptr(src), B._ptr(odd), 1, B.DTYPES["float32"], 3, 48, 36, 2, 2, 1, 1, 0, 0, None)
    assert rc != B.MJ_OK and "not aligned to its 4-byte elements" in L.mj_last_error(None).decode()
    assert L.mj_host_patchify_count(1, B.DTYPES["float32"], 3, 48, 36, 2, 2, 1, 1, 0, 0, None, None) != B.MJ_OK and "NULL argument" in L.mj_last_error(None).decode()
    assert L.mj_host_patchify(B._ptr(src), B._ptr(dst), 1, 7, 3, 48, 36, 2, 2, 1, 1, 0, 0, None) != B.MJ_OK and "dtype 7" in L.mj_last_error(None).decode()
    assert L.mj_host_patchify(B._ptr(src), B._ptr(dst), 1, B.DTYPES["float32"], 3, 48, 36, 2, 2, 1, 1, 2, 0, None) != B.MJ_OK and "order 2" in L.mj_last_error(None).decode()
    # a refused call wrote nothing
    assert (buf == 0xA5).all()
    B.host_patchify(src, 1, "float32", 3, (48, 36), ok, dst=dst)
    assert same_bits(dst, model_patchify(src, ok, "rowmajor")) and (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all()


def test_the_library_exports_the_calls():
    from pyjpegdecoder_amd import _binding as B
    L = B.load_library()
    for name in ("mj_patchify", "mj_patchify_time", "mj_host_patchify", "mj_host_patchify_count"):
        assert name in B.EXPORTS and hasattr(L, name)
    import pyjpegdecoder_amd
    for name in ("normalize_patches", "patch_grids", "smart_resize"):
        assert name in pyjpegdecoder_amd.__all__ and hasattr(pyjpegdecoder_amd, name)


# ---- smart_resize -------------------------------------------------------------------------------------------------------------
def test_smart_resize_hand_checked():
    from pyjpegdecoder_amd import smart_resize
    assert smart_resize(1080, 1920) == (728, 1316)
    assert smart_resize(40, 30) == (84, 56)
    assert smart_resize(500, 375) == (504, 364)
    assert smart_resize(1080, 1920, max_pixels=256 * 28 * 28) == (336, 588)


def test_smart_resize_keeps_its_bounds():
    """over a sweep of sizes: multiples of the factor, the product within the bounds, and the aspect ratio off by less than one
    factor step per side"""
    from pyjpegdecoder_amd import smart_resize
    for factor, lo, hi in [(28, 56 * 56, 14 * 14 * 4 * 1280), (28, 56 * 56, 256 * 28 * 28), (32, 64 * 64, 512 * 512)]:
        for h in list(range(20, 200, 7)) + [480, 777, 1080, 2160, 4000]:
            for w in list(range(20, 200, 11)) + [640, 1001, 1920, 3840]:
                H, W = smart_resize(h, w, factor, lo, hi)
                assert H % factor == 0 and W % factor == 0 and H >= factor and W >= factor
                assert lo <= H * W <= hi, (h, w, H, W)
    with pytest.raises(ValueError, match="aspect ratio"):
        smart_resize(10, 2001)
