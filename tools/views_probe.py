"""Views on the GPU box: what `decode_device(files, size=, views=)` costs beside the call that was there before — every file
listed once per view, with `rois=` — and whether the paths this change did not mean to touch run as they did.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan), per
layout (row-major and x-major).  One process; the comparison is always against ANOTHER build of the library (`--parent-lib
path/to/libmijpeg.so`, the parent commit's) loaded into the same process.  Every plan is executed once first; then `--reps`
rounds, every round one sample of every plan in turn (interleaved, so that a drifting clock meets all alike); per plan the median
and the spread (min .. max).  A sample of the launches: mj_plan_time_execute(iters=1) — the decode, front + main, HIP events on the
plan's stream — and mj_plan_time_resize(iters=1), the resize launch.  End to end: decode_device, wall clock around a synchronised
call (host assembly, upload, plan creation, every launch), `--e2e-reps` calls in turn after one that warms the caches.

    v2        two random-resized crops per file (torchvision's RandomResizedCrop parameters, scale 0.08..1, fixed seed) -> 224 x 224,
              bicubic, float16 normalised: the views call against the parent's call on every file listed twice with rois=
    v1_<a>    ONE crop per file of area fraction a (centred, the image's aspect) as a view against the same crop as rois= on the
              parent: where does decoding whole images and reading a window win over decoding the window?  (csrc/resize_plan.hip's
              placed_source_ranges records 6.4 / 6.1 ms whole against 11.1 / 8.9 ms windowed for a 44 % crop.)
    v8_96     eight crops per file, scale 0.05..0.4 -> 96 x 96: the second call of a 2 + 8 multi-crop (its first is v2)
    untouched the plain bilinear and bicubic resize launches and the reducing_gap=2.0 reduce launch, this build against the parent's,
              with a second parent plan beside the first: what two plans of ONE build differ by

    python tools/views_probe.py --parent-lib PATH [--n 1024] [--distinct 64] [--reps 12] [--layouts rowmajor,xmajor]
"""
from __future__ import annotations

import argparse
import json
import math
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.normalize_probe import other_build, summary  # noqa: E402

W, H = 1920, 1080
LAYOUTS = {"xmajor": 0, "rowmajor": 1}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def random_resized_crop(rng: random.Random, w: int, h: int, scale, ratio=(3 / 4, 4 / 3)):
    """torchvision's RandomResizedCrop.get_params with Python's generator: (x, y, width, height)"""
    area = w * h
    for _ in range(10):
        target = area * rng.uniform(*scale)
        r = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        cw, ch = int(round(math.sqrt(target * r))), int(round(math.sqrt(target / r)))
        if 0 < cw <= w and 0 < ch <= h:
            return rng.randint(0, w - cw), rng.randint(0, h - ch), cw, ch
    ch = min(h, int(round(w / min(max(w / h, ratio[0]), ratio[1]))))
    cw = min(w, int(round(ch * min(max(w / h, ratio[0]), ratio[1]))))
    return (w - cw) // 2, (h - ch) // 2, cw, ch


def centred_crop(w: int, h: int, fraction: float):
    s = math.sqrt(fraction)
    cw, ch = max(1, int(round(w * s))), max(1, int(round(h * s)))
    return (w - cw) // 2, (h - ch) // 2, cw, ch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--e2e-reps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,xmajor")
    ap.add_argument("--fractions", default="0.05,0.1,0.2,0.44,0.7,1.0")
    ap.add_argument("--parent-lib", required=True)
    args = ap.parse_args()

    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth

    dev = torch.device("cuda", 0)
    n, nd = args.n, args.distinct
    blob, offs = synth.synth_batch(nd, args.seed, W, H, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nd)]
    files = [raws[i % nd] for i in range(n)]
    parsed = [parse_jpeg(f, headers_only=True) for f in files]
    output = ("float16", MEAN, STD, None)

    def emit(**line):
        print(json.dumps(line), flush=True)

    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx, pctx = dec.ctx, other_build(B, args.parent_lib)
        pdec = BatchDecoder(device=0, layout=lname)          # the parent's build behind the same Python
        pdec.ctx.close()
        pdec.ctx = pctx

        def batch(v):
            """(prepared batch, its blob on the device) of every file listed v times in a row"""
            prep = prepare_batch([files[k // v] for k in range(n * v)], LAYOUTS[lname], 0, [parsed[k // v] for k in range(n * v)])
            d = torch.from_numpy(prep.blob).to(dev)
            torch.cuda.synchronize()
            return prep, d

        once, d_once = batch(1)

        def compare(label, v, crops, size, e2e=True):
            """views (this build, every file once) against rois on the files listed v times (the parent): crops[k] is view k, of file k // v"""
            rep, d_rep = (once, d_once) if v == 1 else batch(v)
            kw = dict(size=size, filter="bicubic", output=output)
            plans = {"views": B.Plan(ctx, once.to_c(d_once.data_ptr()), {"prep": once, "n_images": n}, views=[(k // v, crops[k]) for k in range(n * v)], **kw),
                     "parent_rois": B.Plan(pctx, rep.to_c(d_rep.data_ptr()), {"prep": rep, "n_images": n * v}, rois=crops, **kw)}
            try:
                out = {name: torch.empty((n * v,) + dec._shape(size[0], size[1], 3), dtype=torch.float16, device=dev) for name in plans}
                ok = True
                for name, plan in plans.items():
                    plan.execute(0, out[name].data_ptr())
                    plan.sync()
                    ok = ok and not plan.read(rgb=False)["status"].any()
                torch.cuda.synchronize()
                same = bool(torch.equal(out["views"].view(torch.int16), out["parent_rois"].view(torch.int16)))
                dec_ms, rs_ms = {name: [] for name in plans}, {name: [] for name in plans}
                for _ in range(args.reps):
                    for name, plan in plans.items():
                        front, main_ms = plan.time_execute(1, out[name].data_ptr())
                        dec_ms[name].append(front + main_ms)
                        rs_ms[name].append(plan.time_resize(1, out[name].data_ptr())[0])
                line = {"layout": lname, "point": label, "views_per_file": v, "size": list(size), "outputs": n * v, "status_ok": ok, "views_equal_parent_rois": same,
                        "crop_area_mean": round(sum(c[2] * c[3] for c in crops) / len(crops) / (W * H), 4),
                        "fused": {name: bool(plans[name].shape()[1]) for name in plans},
                        "source_bytes": {name: int(plans[name].time_resize(1, out[name].data_ptr())[1]) for name in plans}}
                for name in plans:
                    line[name + "_decode_ms"] = summary(dec_ms[name])
                    line[name + "_resize_ms"] = summary(rs_ms[name])
                    line[name + "_launches_ms"] = round(statistics.median(dec_ms[name]) + statistics.median(rs_ms[name]), 4)
            finally:
                for plan in plans.values():
                    plan.close()
            del out
            if e2e:
                t = {"views": [], "parent_rois": []}
                rep_files = [files[k // v] for k in range(n * v)]
                for r in range(args.e2e_reps + 1):
                    for name in t:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        if name == "views":
                            dec.decode_device(files, size=size, resample="bicubic", dtype="float16", normalize=(MEAN, STD), views=[(k // v, crops[k]) for k in range(n * v)])
                        else:
                            pdec.decode_device(rep_files, size=size, resample="bicubic", dtype="float16", normalize=(MEAN, STD), rois=crops)
                        torch.cuda.synchronize()
                        if r:
                            t[name].append((time.perf_counter() - t0) * 1e3)
                line["e2e_decode_device_ms"] = {name: summary(xs) for name, xs in t.items()}
            emit(**line)

        rng = random.Random(args.seed)
        compare("v2", 2, [random_resized_crop(rng, W, H, (0.08, 1.0)) for _ in range(2 * n)], (224, 224))
        for a in (float(x) for x in args.fractions.split(",")):
            compare(f"v1_{a:g}", 1, [centred_crop(W, H, a)] * n, (224, 224), e2e=a == 0.44)
        compare("v8_96", 8, [random_resized_crop(rng, W, H, (0.05, 0.4)) for _ in range(8 * n)], (96, 96))

        # the paths this change did not mean to touch: this build against the parent's, a second parent plan beside the first
        keep = {"prep": once, "n_images": n}
        for label, kw in (("bilinear", {}), ("bicubic", {"filter": "bicubic"}), ("gap2_bicubic", {"filter": "bicubic", "reducing_gap": 2.0})):
            plans = {"parent": B.Plan(pctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), **kw),
                     "parent_twin": B.Plan(pctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), **kw),
                     "this": B.Plan(ctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), **kw)}
            try:
                out = {name: torch.empty((n,) + dec._shape(224, 224, 3), dtype=torch.uint8, device=dev) for name in plans}
                for name, plan in plans.items():
                    plan.execute(0, out[name].data_ptr())
                    plan.sync()
                torch.cuda.synchronize()
                rs, rd = {name: [] for name in plans}, {name: [] for name in plans}
                for _ in range(2 * args.reps):
                    for name, plan in plans.items():
                        rs[name].append(plan.time_resize(1, out[name].data_ptr())[0])
                        if "reducing_gap" in kw:
                            rd[name].append(plan.time_reduce(1))
                line = {"layout": lname, "point": "untouched_" + label, "this_equals_parent": bool(torch.equal(out["this"], out["parent"]))}
                for name in plans:
                    line[name + "_resize_ms"] = summary(rs[name])
                    if rd[name]:
                        line[name + "_reduce_ms"] = summary(rd[name])
                which = rd if "reducing_gap" in kw else rs
                lo, hi = min(which["parent"] + which["parent_twin"]), max(which["parent"] + which["parent_twin"])
                line["this_median_inside_parents_spread"] = bool(lo <= statistics.median(which["this"]) <= hi)
                emit(**line)
            finally:
                for plan in plans.values():
                    plan.close()
            del out
        del d_once
        pctx.close()
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
