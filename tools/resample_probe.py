"""Resample filters on the GPU box: what the resize launch costs with each filter of `decode(..., size=, resample=)`, and that
the bilinear launch has not moved.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan) to
224 x 224, per layout (row-major and x-major).  One process; every plan executed once first (the resize launch reads what stage
2 left), then `--reps` rounds, every round one sample of every point in turn (interleaved, so that a drifting clock meets all
points alike); per point the median and the spread (min .. max) over the rounds.  A sample is mj_plan_time_resize(iters=1): one
warm launch, then one between two HIP events.

    bilinear_ms, box_ms, hamming_ms      the unsigned instances with each of the three non-negative tables (bilinear: the plan of a
                                         call without resample=)
    bicubic_ms, lanczos_ms               the signed instances: two and three times the taps per pixel on the same bytes
    bilinear_twin_ms                     a second bilinear plan of this build — the same code on other buffers: how far two plans
                                         of ONE build lie apart is what a difference between builds has to exceed
    bilinear_parent_ms, bilinear_parent_twin_ms   the same launch from another build of the library (`--parent-lib
                                         path/to/libmijpeg.so`, e.g. the parent commit's) loaded into the same process: the same
                                         instances, so the times should agree within the twins' spread
    copy_ms                              what the library's plain 16-bytes-per-lane copy (mj_device_copy_rate) takes for the bytes the
                                         launch reads and writes: the floor every filter's time stands beside
    shape                                mj_debug_resize_shape of every plan: tile, tiles per image, LDS per workgroup, taps

and whether every filter's first images equal tools/resize_model.py applied to the plain decode (a call without size=) of the
same files.

    python tools/resample_probe.py [--n 1024] [--distinct 64] [--reps 16] [--layouts rowmajor,xmajor] [--parent-lib PATH] [--parent-first]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.normalize_probe import other_build, summary  # noqa: E402

W, H, SIZE = 1920, 1080, (224, 224)
LAYOUTS = {"xmajor": 0, "rowmajor": 1, "planar": 2, "planar_rowmajor": 3}
FILTERS = ("bilinear", "box", "hamming", "bicubic", "lanczos")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,xmajor")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--check-images", type=int, default=2)
    ap.add_argument("--parent-first", action="store_true",
                    help="create, execute and sample the other build's plans in front of this build's (which build's buffers are "
                         "allocated first is the one thing besides the code that differs between the two)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import resize_model, synth

    dev = torch.device("cuda", 0)
    n, nd = args.n, args.distinct
    blob, offs = synth.synth_batch(nd, args.seed, W, H, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nd)]
    files = [raws[i % nd] for i in range(n)]
    parsed = [parse_jpeg(f, headers_only=True) for f in files]
    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx = dec.ctx
        pctx = other_build(B, args.parent_lib) if args.parent_lib else None
        prep = prepare_batch(files, LAYOUTS[lname], 0, parsed)
        d_blob = torch.from_numpy(prep.blob).to(dev)
        torch.cuda.synchronize()
        keep = {"prep": prep, "n_images": n}
        # (bilinear: no filter argument — the plan and the entry point of a call without resample=)
        plans = {}
        if pctx is not None and args.parent_first:
            plans["bilinear_parent"] = B.Plan(pctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE)
            plans["bilinear_parent_twin"] = B.Plan(pctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE)
        for f in FILTERS:
            plans[f] = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE, filter=None if f == "bilinear" else f)
        plans["bilinear_twin"] = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE)
        if pctx is not None and not args.parent_first:
            plans["bilinear_parent"] = B.Plan(pctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE)
            plans["bilinear_parent_twin"] = B.Plan(pctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE)
        try:
            shape = (n,) + dec._shape(SIZE[0], SIZE[1], 3)
            out = {name: torch.empty(shape, dtype=torch.uint8, device=dev) for name in plans}
            ok = True
            for name, plan in plans.items():
                assert plan.info.rgb_bytes == out[name].numel()
                plan.execute(0, out[name].data_ptr())
                plan.sync()
                ok = ok and not plan.read(rgb=False)["status"].any()
            torch.cuda.synchronize()
            # every filter's first images against the model of the plain decode of the same files
            k = min(args.check_images, nd)
            full = dec.decode(raws[:k])
            equal = {}
            for f in FILTERS:
                same = True
                for i in range(k):
                    a = full[i]
                    if lname.startswith("planar"):
                        a = np.moveaxis(a, 0, -1)
                    if lname in ("xmajor", "planar"):
                        a = a.swapaxes(0, 1)
                    want = resize_model.resize(np.ascontiguousarray(a), SIZE, f)
                    got = out[f][i].cpu().numpy()
                    if lname.startswith("planar"):
                        got = np.moveaxis(got, 0, -1)
                    if lname in ("xmajor", "planar"):
                        got = got.swapaxes(0, 1)
                    same = same and bool(np.array_equal(got, want))
                equal[f] = same
            same_parent = bool(torch.equal(out["bilinear"], out["bilinear_parent"])) if pctx is not None else None
            samples = {name: [] for name in plans}
            for _ in range(args.reps):
                for name, plan in plans.items():
                    samples[name].append(plan.time_resize(1, out[name].data_ptr())[0])
            src_bytes = plans["bilinear"].time_resize(1, out["bilinear"].data_ptr())[1]
            out_bytes = int(plans["bilinear"].info.rgb_bytes)
            copy_tbs = ctx.copy_rate_gbs(1 << 30, 5) / 1e3
            med = {name: statistics.median(xs) for name, xs in samples.items()}
            line = {"layout": lname, "parent_first": bool(args.parent_first), "images": n, "distinct": nd, "size": list(SIZE), "source_bytes": int(src_bytes), "output_bytes": out_bytes,
                    "copy_tbs": round(copy_tbs, 3), "copy_ms": round((int(src_bytes) + out_bytes) / (copy_tbs * 1e12) * 1e3, 4)}
            for name in plans:
                line[name + "_ms"] = summary(samples[name])
            for f in FILTERS[1:]:
                line[f + "_over_bilinear"] = round(med[f] / med["bilinear"], 3)
            line["shape"] = {f: plans[f].resize_shape() for f in FILTERS}
            line.update(status_ok=ok, equals_model_first_images=equal, parent_bilinear_equals_this_build=same_parent)
            if pctx is not None:
                twins = abs(med["bilinear"] - med["bilinear_twin"])
                line["bilinear_minus_parent_ms"] = round(med["bilinear"] - med["bilinear_parent"], 4)
                line["twin_gap_ms"] = round(max(twins, abs(med["bilinear_parent"] - med["bilinear_parent_twin"])), 4)
            print(json.dumps(line), flush=True)
        finally:
            for plan in plans.values():
                plan.close()
        del out, d_blob
        if pctx is not None:
            pctx.close()
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
