"""The two-step resize on the GPU box: what `decode(..., size=, reducing_gap=)` costs beside the single step.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan) to
224 x 224, per layout (row-major and x-major) and per filter (bilinear, bicubic, Lanczos).  One process; every plan executed once
first, then `--reps` rounds, every round one sample of every point in turn (interleaved, so that a drifting clock meets all
points alike); per point the median and the spread (min .. max) over the rounds.  A sample is mj_plan_time_resize(iters=1): one
warm launch, then one between two HIP events — for a reducing plan both launches, the reduce and the resize.

    parent_ms          the single-step launch of ANOTHER build of the library (`--parent-lib path/to/libmijpeg.so`, the parent
                       commit's) loaded into the same process: what users run today
    plain_ms, plain_twin_ms   the same call (no reducing_gap) on this build, twice — the same code on other buffers: how far two
                       plans of one build lie apart is what a difference between builds has to exceed
    gap2_ms, gap3_ms   reducing_gap=2.0 (4 x 2) and 3.0 (2 x 1): reduce + resize
    reduce2_ms, reduce3_ms    the reduce launch alone (mj_plan_time_reduce)
    copy_src_ms        what the library's plain 16-bytes-per-lane copy (mj_device_copy_rate) takes for the bytes the reduce
                       launch reads — the yardstick the README holds the resize launch to; reduce*_over_copy is the ratio
    e2e_ms             decode_device(files, size=, resample=, reducing_gap=) end to end (host assembly, upload, decode, resize),
                       gap None / 2.0 / 3.0, `--e2e-reps` calls each in turn

and whether the reducing plans' first images equal tools/reduce_model.py applied to the plain decode of the same files.

    python tools/reduce_probe.py [--n 1024] [--distinct 64] [--reps 12] [--layouts rowmajor,xmajor] [--parent-lib PATH]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.normalize_probe import other_build, summary  # noqa: E402

W, H, SIZE = 1920, 1080, (224, 224)
LAYOUTS = {"xmajor": 0, "rowmajor": 1}
FILTERS = ("bilinear", "bicubic", "lanczos")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,xmajor")
    ap.add_argument("--filters", default=",".join(FILTERS))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--check-images", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import reduce_model, synth

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
        k = min(args.check_images, nd)
        full = [a if lname == "rowmajor" else a.swapaxes(0, 1) for a in dec.decode(raws[:k])]
        copy_tbs = ctx.copy_rate_gbs(1 << 30, 5) / 1e3
        for f in args.filters.split(","):
            flt = None if f == "bilinear" else f
            plans = {}
            if pctx is not None:
                plans["parent"] = B.Plan(pctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE, filter=flt)
            plans["plain"] = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE, filter=flt)
            plans["plain_twin"] = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE, filter=flt)
            plans["gap2"] = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE, filter=flt, reducing_gap=2.0)
            plans["gap3"] = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE, filter=flt, reducing_gap=3.0)
            try:
                shape = (n,) + dec._shape(SIZE[0], SIZE[1], 3)
                out = {name: torch.empty(shape, dtype=torch.uint8, device=dev) for name in plans}
                ok = True
                for name, plan in plans.items():
                    plan.execute(0, out[name].data_ptr())
                    plan.sync()
                    ok = ok and not plan.read(rgb=False)["status"].any()
                torch.cuda.synchronize()
                equal = {}
                for name, gap in (("plain", None), ("gap2", 2.0), ("gap3", 3.0)):
                    same = True
                    for i in range(k):
                        want = reduce_model.resize(np.ascontiguousarray(full[i]), SIZE, f, gap)
                        got = out[name][i].cpu().numpy()
                        same = same and bool(np.array_equal(got if lname == "rowmajor" else got.swapaxes(0, 1), want))
                    equal[name] = same
                same_parent = bool(torch.equal(out["plain"], out["parent"])) if pctx is not None else None
                samples = {name: [] for name in plans}
                samples["reduce2"], samples["reduce3"] = [], []
                for _ in range(args.reps):
                    for name, plan in plans.items():
                        samples[name].append(plan.time_resize(1, out[name].data_ptr())[0])
                    samples["reduce2"].append(plans["gap2"].time_reduce(1))
                    samples["reduce3"].append(plans["gap3"].time_reduce(1))
                src_bytes = plans["gap2"].time_resize(1, out["gap2"].data_ptr())[1]
                med = {name: statistics.median(xs) for name, xs in samples.items()}
                # (a copy of src_bytes reads and writes them; copy_tbs counts both)
                line = {"layout": lname, "filter": f, "images": n, "distinct": nd, "size": list(SIZE), "source_bytes": int(src_bytes),
                        "copy_tbs": round(copy_tbs, 3), "copy_src_ms": round(2 * int(src_bytes) / (copy_tbs * 1e12) * 1e3, 4)}
                for name in samples:
                    line[name + "_ms"] = summary(samples[name])
                line["reduce2_over_copy"] = round(med["reduce2"] / line["copy_src_ms"], 3)
                line["reduce3_over_copy"] = round(med["reduce3"] / line["copy_src_ms"], 3)
                line["twin_gap_ms"] = round(abs(med["plain"] - med["plain_twin"]), 4)
                if pctx is not None:
                    line["plain_minus_parent_ms"] = round(med["plain"] - med["parent"], 4)
                    line["gap2_minus_parent_ms"] = round(med["gap2"] - med["parent"], 4)
                    line["gap3_minus_parent_ms"] = round(med["gap3"] - med["parent"], 4)
                line["reduce_shape"] = {name: plans[name].reduce_shape(0) for name in ("plain", "gap2", "gap3")}
                line["resize_shape"] = {name: plans[name].resize_shape() for name in ("plain", "gap2", "gap3")}
                line.update(status_ok=ok, equals_model_first_images=equal, parent_equals_this_build=same_parent)
                print(json.dumps(line), flush=True)
            finally:
                for plan in plans.values():
                    plan.close()
            del out
        # end to end through decode_device, the three calls in turn
        e2e = {"none": [], "2.0": [], "3.0": []}
        for rep in range(args.e2e_reps + 1):
            for name, gap in (("none", None), ("2.0", 2.0), ("3.0", 3.0)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dec.decode_device(files, size=SIZE, resample="bicubic", reducing_gap=gap)
                torch.cuda.synchronize()
                if rep:                       # (the first round warms the caches)
                    e2e[name].append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"layout": lname, "e2e_decode_device_bicubic_ms": {name: summary(xs) for name, xs in e2e.items()}}), flush=True)
        del d_blob
        if pctx is not None:
            pctx.close()
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
