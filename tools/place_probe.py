"""Aspect-preserving sizing on the GPU box: what the placed resize launch costs beside the launches a user has today, which of
the two decode routes a placed plan of whole images should take, and that the plain launches have not moved.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row), per layout
(row-major and x-major).  One process; every plan executed once first, then `--reps` rounds, every round one sample of every
point in turn (interleaved); per point the median and the spread over the rounds.  A sample is mj_plan_time_resize(iters=1).

    bilinear_ms, bicubic_ms              the plain size=(224, 224) launches, and bilinear_twin_ms: a second plan of this build
    bilinear_parent_ms, bicubic_parent_ms   the same launches from another build (`--parent-lib`, e.g. the parent commit's) in the
                                         same process: the same instances, so the times should agree within the twins' spread
    stretch455_ms                        what a user does today for the evaluation transform: size=(455, 256) bicubic in one
                                         launch (then a torch slice, which the end-to-end figure includes)
    eval_window_ms, eval_whole_ms        resize_to=256 onto 224 x 224, bicubic, the placed launch — over a derived window plan
                                         (MJ_PLACE_WINDOW=1) and over the whole images (MJ_PLACE_WINDOW=0); source_bytes of each
    contain_ms                           "contain" into 224 x 224, bilinear: 56 % of the canvas is image, the rest fill
    e2e_*_ms                             decode_device end to end (host assembly, upload, decode, resize) for today's route and
                                         the two placed routes
    exec_*_ms                            mj_plan_time_execute (front + main) of the two placed plans: the decode alone

    python tools/place_probe.py [--n 1024] [--distinct 64] [--reps 16] [--layouts rowmajor,xmajor] [--parent-lib PATH]
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
LAYOUTS = {"xmajor": 0, "rowmajor": 1, "planar": 2, "planar_rowmajor": 3}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,xmajor")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()

    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import normalize_places, prepare_batch
    from tools import synth

    dev = torch.device("cuda", 0)
    n, nd = args.n, args.distinct
    blob, offs = synth.synth_batch(nd, args.seed, W, H, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nd)]
    files = [raws[i % nd] for i in range(n)]
    parsed = [parse_jpeg(f, headers_only=True) for f in files]
    ev = normalize_places(256, None, SIZE, [(W, H)] * n)
    contain = normalize_places("contain", None, SIZE, [(W, H)] * n)
    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx = dec.ctx
        pctx = other_build(B, args.parent_lib) if args.parent_lib else None
        prep = prepare_batch(files, LAYOUTS[lname], 0, parsed)
        d_blob = torch.from_numpy(prep.blob).to(dev)
        torch.cuda.synchronize()
        keep = {"prep": prep, "n_images": n}

        def make(c, **kw):
            return B.Plan(c, prep.to_c(d_blob.data_ptr()), keep, **kw)
        plans = {"bilinear": make(ctx, size=SIZE), "bicubic": make(ctx, size=SIZE, filter="bicubic"), "bilinear_twin": make(ctx, size=SIZE),
                 "stretch455": make(ctx, size=ev[0][:2], filter="bicubic")}
        B.set_option("MJ_PLACE_WINDOW", 1)
        plans["eval_window"] = make(ctx, size=SIZE, filter="bicubic", places=ev)
        B.set_option("MJ_PLACE_WINDOW", 0)
        plans["eval_whole"] = make(ctx, size=SIZE, filter="bicubic", places=ev)
        B.set_option("MJ_PLACE_WINDOW", None)
        plans["contain"] = make(ctx, size=SIZE, places=contain, fill=(114, 114, 114))
        if pctx is not None:
            plans["bilinear_parent"] = make(pctx, size=SIZE)
            plans["bicubic_parent"] = make(pctx, size=SIZE, filter="bicubic")
        try:
            out = {name: torch.empty(int(plan.info.rgb_bytes), dtype=torch.uint8, device=dev) for name, plan in plans.items()}
            ok = True
            for name, plan in plans.items():
                plan.execute(0, out[name].data_ptr())
                plan.sync()
                ok = ok and not plan.read(rgb=False)["status"].any()
            torch.cuda.synchronize()
            crop = out["stretch455"].view((n,) + dec._shape(ev[0][0], ev[0][1], 3))
            x0, y0 = -ev[0][2], -ev[0][3]
            crop = crop[:, x0:x0 + SIZE[0], y0:y0 + SIZE[1]] if lname == "xmajor" else crop[:, y0:y0 + SIZE[1], x0:x0 + SIZE[0]]
            same = {k: bool(torch.equal(out[k].view(crop.shape), crop)) for k in ("eval_window", "eval_whole")}
            if pctx is not None:
                same["bilinear_parent"] = bool(torch.equal(out["bilinear"], out["bilinear_parent"]))
                same["bicubic_parent"] = bool(torch.equal(out["bicubic"], out["bicubic_parent"]))
            samples = {name: [] for name in plans}
            for _ in range(args.reps):
                for name, plan in plans.items():
                    samples[name].append(plan.time_resize(1, out[name].data_ptr())[0])
            med = {name: statistics.median(xs) for name, xs in samples.items()}
            line = {"layout": lname, "images": n, "distinct": nd, "canvas": list(SIZE), "status_ok": ok, "equal": same}
            for name, plan in plans.items():
                line[name + "_ms"] = summary(samples[name])
            line["source_bytes"] = {k: int(plans[k].time_resize(1, out[k].data_ptr())[1]) for k in ("stretch455", "eval_window", "eval_whole", "contain")}
            line["exec_ms"] = {k: [round(v, 4) for v in plans[k].time_execute(4, out[k].data_ptr())] for k in ("stretch455", "eval_window", "eval_whole")}
            line["shape"] = {k: plans[k].resize_shape() for k in ("bicubic", "stretch455", "eval_window", "eval_whole", "contain")}
            line["eval_window_over_stretch455"] = round(med["eval_window"] / med["stretch455"], 3)
            line["eval_whole_over_stretch455"] = round(med["eval_whole"] / med["stretch455"], 3)
            line["contain_over_bilinear"] = round(med["contain"] / med["bilinear"], 3)
            if pctx is not None:
                line["bilinear_minus_parent_ms"] = round(med["bilinear"] - med["bilinear_parent"], 4)
                line["bicubic_minus_parent_ms"] = round(med["bicubic"] - med["bicubic_parent"], 4)
                line["twin_gap_ms"] = round(abs(med["bilinear"] - med["bilinear_twin"]), 4)
        finally:
            for plan in plans.values():
                plan.close()
        del out, d_blob

        # end to end through decode_device: today's route, and the placed one over each decode route
        def e2e(window, **kw):
            B.set_option("MJ_PLACE_WINDOW", window)
            ts = []
            for _ in range(args.e2e_reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = dec.decode_device(files, resample="bicubic", **kw)
                if "resize_to" not in kw:
                    r = (r[:, x0:x0 + SIZE[0], y0:y0 + SIZE[1]] if lname == "xmajor" else r[:, y0:y0 + SIZE[1], x0:x0 + SIZE[0]]).contiguous()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                del r
            B.set_option("MJ_PLACE_WINDOW", None)
            return summary(ts[1:])
        line["e2e_stretch455_slice_ms"] = e2e(None, size=ev[0][:2])
        line["e2e_eval_window_ms"] = e2e(1, size=SIZE, resize_to=256)
        line["e2e_eval_whole_ms"] = e2e(0, size=SIZE, resize_to=256)
        print(json.dumps(line), flush=True)
        if pctx is not None:
            pctx.close()
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
