"""Derived plans on the GPU box: DINO's multi-crop — 2 x 224 x 224 and 8 x 96 x 96 crops of every file — as ONE call with `also=`
against the TWO calls it replaces, in the same process, on the same build.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan),
bicubic, float16 normalised, per layout (row-major and x-major).  Crops are torchvision's RandomResizedCrop parameters (scale
0.4..1 for the two global crops, 0.05..0.4 for the eight local ones, fixed seed).

    launches     one call: the plan that decodes — mj_plan_time_execute(iters=1), front + main, and mj_plan_time_resize(iters=1) — plus
                 mj_plan_time_resize of the plan derived from it.  Two calls: both of these for each of the two plans.  Every plan is
                 executed once first; then `--reps` rounds, every round one sample of every plan in turn (interleaved, so that a
                 drifting clock meets all alike); medians and spreads (min .. max).
    end to end   decode_device, wall clock around a synchronised call (host assembly, upload, plan creation, every launch): the one
                 call and the pair of calls in turn, `--e2e-reps` rounds after one that warms the caches; medians and spreads.  Once
                 as decode_device cuts a call of this size (four parts in flight: uploads and kernels run under the host's work on
                 the next part) and once with parts=1 (one plan per call, nothing overlapped).

The outputs of the one call are compared with the two calls' (they are equal bit for bit, or the line says so).

    python tools/derive_probe.py [--n 1024] [--distinct 64] [--reps 12] [--e2e-reps 7] [--layouts rowmajor,xmajor]
"""
from __future__ import annotations

import argparse
import json
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.normalize_probe import summary  # noqa: E402
from tools.views_probe import LAYOUTS, MEAN, STD, H, W, random_resized_crop  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--e2e-reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,xmajor")
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
    rng = random.Random(args.seed)
    big = [(k // 2, random_resized_crop(rng, W, H, (0.4, 1.0))) for k in range(2 * n)]
    small = [(k // 8, random_resized_crop(rng, W, H, (0.05, 0.4))) for k in range(8 * n)]
    output = ("float16", MEAN, STD, None)
    common = dict(resample="bicubic", dtype="float16", normalize=(MEAN, STD))

    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx = dec.ctx
        prep = prepare_batch(files, LAYOUTS[lname], 0, parsed)
        d_blob = torch.from_numpy(prep.blob).to(dev)
        torch.cuda.synchronize()
        keep = {"prep": prep, "n_images": n}
        kw = dict(filter="bicubic", output=output)
        plans = {"one_call_224": B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=(224, 224), views=big, **kw)}
        plans["one_call_96_derived"] = plans["one_call_224"].derive(prep, size=(96, 96), views=small, **kw)
        plans["two_calls_224"] = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=(224, 224), views=big, **kw)
        plans["two_calls_96"] = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=(96, 96), views=small, **kw)
        line = {"layout": lname, "files": n, "crops": "2 x 224 x 224 + 8 x 96 x 96", "filter": "bicubic", "dtype": "float16 normalised"}
        try:
            out = {name: torch.empty((len(small if "96" in name else big),) + dec._shape(*((96, 96) if "96" in name else (224, 224)), 3),
                                     dtype=torch.float16, device=dev) for name in plans}
            for name, plan in plans.items():          # (the derived plan right behind its parent, on the context's stream)
                plan.execute(0, out[name].data_ptr())
                plan.sync()
            torch.cuda.synchronize()
            line["status_ok"] = not any(plans[name].read(rgb=False)["status"].any() for name in plans)
            line["one_call_equals_two_calls"] = bool(torch.equal(out["one_call_224"].view(torch.int16), out["two_calls_224"].view(torch.int16)) and
                                                     torch.equal(out["one_call_96_derived"].view(torch.int16), out["two_calls_96"].view(torch.int16)))
            line["fused"] = {name: bool(plans[name].shape()[1]) for name in plans if "derived" not in name}
            dec_ms = {name: [] for name in plans if "derived" not in name}
            rs_ms = {name: [] for name in plans}
            for _ in range(args.reps):
                for name, plan in plans.items():
                    if name in dec_ms:
                        front, main_ms = plan.time_execute(1, out[name].data_ptr())
                        dec_ms[name].append(front + main_ms)
                    rs_ms[name].append(plan.time_resize(1, out[name].data_ptr())[0])
            for name in plans:
                if name in dec_ms:
                    line[name + "_decode_ms"] = summary(dec_ms[name])
                line[name + "_resize_ms"] = summary(rs_ms[name])
            med = statistics.median
            line["one_call_launches_ms"] = round(med(dec_ms["one_call_224"]) + med(rs_ms["one_call_224"]) + med(rs_ms["one_call_96_derived"]), 4)
            line["two_calls_launches_ms"] = round(med(dec_ms["two_calls_224"]) + med(rs_ms["two_calls_224"]) + med(dec_ms["two_calls_96"]) +
                                                  med(rs_ms["two_calls_96"]), 4)
        finally:
            for name in ("one_call_96_derived", "one_call_224", "two_calls_224", "two_calls_96"):
                if name in plans:
                    plans[name].close()
        del out, d_blob
        # (parts: decode_device's own — a call of this size goes as four parts through the batches in flight, uploads and kernels under
        # the host's work on the next part —, and 1: one plan per call, nothing overlapped)
        for label, parts in (("e2e_decode_device_ms", None), ("e2e_decode_device_one_part_ms", 1)):
            t = {"one_call": [], "two_calls": []}
            for r in range(args.e2e_reps + 1):
                for name in t:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if name == "one_call":
                        dec.decode_device(files, size=(224, 224), views=big, also=[dict(size=(96, 96), views=small)], parts=parts, **common)
                    else:
                        dec.decode_device(files, size=(224, 224), views=big, parts=parts, **common)
                        dec.decode_device(files, size=(96, 96), views=small, parts=parts, **common)
                    torch.cuda.synchronize()
                    if r:
                        t[name].append((time.perf_counter() - t0) * 1e3)
            line[label] = {name: summary(xs) for name, xs in t.items()}
        print(json.dumps(line), flush=True)
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
