"""The fast stage 2's rare pixel paths against the oracle, byte for byte, on every sampling layout and through every route
that runs the strip worker (csrc/reconstruct_fast_strips.h): the stage-2 kernel on written coefficients, whole files
through BatchDecoder, window plans (the WIN instance) and the fused launch's consumer wavefronts.

The inputs are the families of tests/stage2_families.py — B-tie brackets, the green patch threshold, the R edge and the
fp32 range, luma and output clamps, heavy-tailed blocks, one rare MCU in a benign strip — whose reach is asserted on the
CPU by tests/test_stage2_families_host.py from the oracle's own planes; the oracle's result of an image is computed once
per process and shared by all routes.  Needs a real MI355X: run with `-m gpu`."""
import numpy as np
import pytest

import stage2_families as F
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [(lay, fam) for lay in F.LAYOUTS for fam in F.families_of(lay)]
COLOUR_CASES = [(lay, fam) for lay, fam in CASES if lay != "grey"]
ORDERS = ("xmajor", "rowmajor")
ALL_ORDERS = ("xmajor", "rowmajor", "planar", "planar_rowmajor")

# Copies of a file in a fused-launch case.  The smallest count at which the plan of every image here reports MJ_FORM_FUSED is
# 1 (probed with plans of 1, 2, 4 ... 256 copies on an MI355X: form 97 = fused | resolved | lanes from one copy on; row-major
# 4:1:1 reports 33, the two launches, at every count; greyscale never takes the fused launch); 9 copies make several workgroups.
FUSED_COPIES = (1, 9)


@pytest.fixture(scope="module")
def decs():
    from pyjpegdecoder_amd import BatchDecoder
    d = {order: BatchDecoder(device=0, layout=order, segment="host") for order in ALL_ORDERS}
    yield d
    for x in d.values():
        x.close()


def _refs(layout, family):
    return [F.oracle_of(layout, family, k) for k in range(len(F.images(layout, family)))]


def expect(full: np.ndarray, order: str, win=None) -> np.ndarray:
    """The oracle's (W, H[, 3]) image — or a window (x, y, width, height) of it — laid out as a decoder of `order` returns it."""
    s = full if win is None else full[win[0]:win[0] + win[2], win[1]:win[1] + win[3]]
    if order in ("rowmajor", "planar_rowmajor"):
        s = s.swapaxes(0, 1)
    if order.startswith("planar") and s.ndim == 3:
        s = np.moveaxis(s, -1, 0)
    return np.ascontiguousarray(s)


def _where(got, want):
    bad = np.argwhere(got != want)
    return f"{bad.shape[0]} bytes differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


# ---- (a) Plan.write_coef + execute_stage2 --------------------------------------------------------------------------------
def _stage2(dec, img, flags):
    from pyjpegdecoder_amd import _binding as B
    _, plan = dec.plan([img.file()], flags)
    try:
        plan.write_coef(img.blocks)
        plan.execute_stage2()
        plan.sync()
        out = plan.read(rgb=True, planes=bool(flags & B.MJ_FLAG_KEEP_PLANES))
    finally:
        plan.close()
    assert not out["status"].any()
    return out


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("layout,family", CASES)
def test_written_coefficients_through_stage2(decs, layout, family, order):
    """flags = 0 is the production instance of k_reconstruct_fast; with MJ_FLAG_KEEP_PLANES the seam instance (all pixels through
    the exact routine) must give the oracle's planes and the production launch's bytes."""
    from pyjpegdecoder_amd import _binding as B
    from oracle import oracle
    dec = decs[order]
    for img, ref in zip(F.images(layout, family), _refs(layout, family)):
        want = oracle.reconstruct(ref["parsed"], img.blocks)
        fast = _stage2(dec, img, 0)["rgb"]
        w = expect(want["rgb"], order)
        assert np.array_equal(fast.reshape(w.shape), w), (img.name, _where(fast.reshape(w.shape), w))
        seam = _stage2(dec, img, B.MJ_FLAG_KEEP_PLANES)
        assert np.array_equal(seam["planes"].reshape(want["planes"].shape), want["planes"]), img.name
        assert np.array_equal(seam["rgb"], fast), img.name


# ---- (b) files through BatchDecoder.decode -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,family", CASES)
def test_files_through_the_decoder_in_every_output_order(decs, layout, family):
    files = [i.file() for i in F.images(layout, family)]
    refs = _refs(layout, family)
    for order in ALL_ORDERS:
        for img, ref, got in zip(F.images(layout, family), refs, decs[order].decode(files)):
            w = expect(ref["rgb"], order)
            assert got.shape == w.shape and np.array_equal(got, w), (order, img.name, _where(got, w))


@pytest.mark.parametrize("layout", list(F.LAYOUTS))
def test_two_odd_sized_images_in_one_plan(decs, layout):
    """The second image's output starts at an odd byte: no strip of it is staged."""
    from oracle import oracle
    pair = F.batch_pair(layout)
    files = [i.file() for i in pair]
    wants = [oracle.decode(f)["rgb"] for f in files]
    for order in ALL_ORDERS:
        for img, full, got in zip(pair, wants, decs[order].decode(files)):
            w = expect(full, order)
            assert got.shape == w.shape and np.array_equal(got, w), (order, img.family, _where(got, w))
        for img, full, got in zip(pair[::-1], wants[::-1], decs[order].decode(files[::-1])):
            w = expect(full, order)
            assert np.array_equal(got, w), (order, "reversed", img.family, _where(got, w))


# ---- (c) windows: the WIN instance ---------------------------------------------------------------------------------------
def windows_of(img):
    """Windows that start and end inside MCUs: top-left on a dword boundary of the run direction of both output orders (x and y
    multiples of 4: x * 3 and y * 3 are multiples of 4) and off it; narrower than 16 bytes of a column (5 rows: 15 bytes)
    and of a row (3 columns: 9 bytes); and straight through the image's planted MCUs (or its middle MCU)."""
    W, H = img.width, img.height
    mw, mh = F.mcu_px(img.layout)
    out = {"on_dword": (4, 4, W - 9, H - 11), "off_dword": (5, 3, W - 7, H - 8),
           "narrow_columns": (W // 2 + 1, 12, 3, H - 13), "narrow_rows": (12, H // 2 + 1, W - 13, 5)}
    cuts = img.planted[:4] or [(img.mcus[0] // 2, img.mcus[1] // 2)]
    for i, (mx, my) in enumerate(cuts):
        x0, y0 = min(mx * mw + mw // 2, W - 1), min(my * mh + mh // 2, H - 1)
        out[f"through_mcu_{i}"] = (x0, y0, min(37, W - x0), min(41, H - y0))
        x1, y1 = max(0, mx * mw + 3 - 30), max(0, my * mh + 3 - 30)             # ... and one that ENDS inside it
        out[f"into_mcu_{i}"] = (x1, y1, min(mx * mw + 3, W) - x1, min(my * mh + 3, H) - y1)
    return {k: v for k, v in out.items() if v[2] > 0 and v[3] > 0}


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("layout,family", CASES)
def test_windows(decs, layout, family, order):
    """windows_of: the per-lane byte copy of the window instance (no extent of these windows is a whole number of dwords), all
    images of the family in one call.  stage2_families.staged_windows: windows whose strips the instance STAGES — origin and
    extent multiples of 4, one image per call so that its output starts at byte 0 — with runs cut at the window's top and
    bottom and, in the green and planted images, the patch in LDS (test_stage2_families_host.py counts both)."""
    imgs, refs = F.images(layout, family), _refs(layout, family)
    files = [i.file() for i in imgs]
    wins = [windows_of(i) for i in imgs]
    for kind in sorted(set().union(*wins)):
        sel = [k for k in range(len(imgs)) if kind in wins[k]]
        got = decs[order].decode([files[k] for k in sel], rois=[wins[k][kind] for k in sel])
        for k, g in zip(sel, got):
            w = expect(refs[k]["rgb"], order, wins[k][kind])
            assert g.shape == w.shape and np.array_equal(g, w), (imgs[k].name, kind, wins[k][kind], _where(g, w))
    for img, ref, f in zip(imgs, refs, files):
        for kind, win in F.staged_windows(img).items():
            (g,) = decs[order].decode([f], rois=[win])
            w = expect(ref["rgb"], order, win)
            assert g.shape == w.shape and np.array_equal(g, w), (img.name, kind, win, _where(g, w))


# ---- (d) the fused launch's consumer wavefronts --------------------------------------------------------------------------
def _execute_poisoned(ctx, prep, n, torch, opts):
    """(rgb on the device, statuses, stage1_form) of three executes of a plan under library options, each into a zeroed buffer and
    with the coefficient store poisoned first: a consumer that reads a block before its producer wrote it must not find the
    previous execute's copy.  The three outputs must be one.  (What test_gpu_parity._decode_plan does for its batches.)"""
    from pyjpegdecoder_amd import _binding as B
    for k, v in opts:
        B.set_option(k, v)
    try:
        dev = torch.device("cuda", 0)
        d_blob = torch.from_numpy(prep.blob).to(dev)
        torch.cuda.synchronize()
        plan = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), {"prep": prep, "n_images": n})
        try:
            out = torch.zeros(plan.info.rgb_bytes, dtype=torch.uint8, device=dev)
            keep = None
            for k, poison in enumerate((0x5A, 0xC3, 0x7E)):
                out.zero_()
                torch.cuda.synchronize()                # (the fill runs on torch's stream, the plan on the context's)
                plan.fill_coef(poison)
                plan.execute(0, out.data_ptr())
                plan.sync()
                if keep is None:
                    keep = out.clone()
                else:
                    assert torch.equal(out, keep), f"execute {k} of the plan differs from its first"
            return keep, plan.read(rgb=False)["status"], plan.stage1_form()
        finally:
            plan.close()
    finally:
        for k, _ in opts:
            B.set_option(k, None)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("layout,family", COLOUR_CASES)
def test_fused_launch(decs, layout, family, order):
    """1 and 9 copies of the file (restart interval = one MCU row), the lane walk forced, the coefficient store poisoned
    before every execute (_execute_poisoned: three executes that must agree): the plan must report
    the fused form — except row-major 4:1:1, which fused_applies excludes and which must report the two launches — and every
    copy must be the oracle's image."""
    torch = pytest.importorskip("torch")
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.batch import prepare_batch
    dec = decs[order]
    for n, (img, ref) in ((n, ir) for n in FUSED_COPIES for ir in zip(F.images(layout, family), _refs(layout, family))):
        prep = prepare_batch([img.file()] * n, dec.layout, 0)
        out, st, form = _execute_poisoned(dec.ctx, prep, n, torch, [("MJ_HUFFMAN", "lanes")])
        assert form & 15 == B.MJ_FORM_LANES, form
        if layout == "411" and order == "rowmajor":
            assert not form & B.MJ_FORM_FUSED, form
        else:
            assert form & B.MJ_FORM_FUSED, (img.name, form)
        assert not st.any()
        got = out.view(n, -1)
        assert bool((got == got[0]).all()), img.name
        w = expect(ref["rgb"], order)
        g = got[0].cpu().numpy().reshape(w.shape)
        assert np.array_equal(g, w), (img.name, _where(g, w))
