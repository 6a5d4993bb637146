"""The perspective transform on the GPU box: what the perspective launch costs beside the SAME build's affine launch, what
`decode_device(files, size=, perspective=)` costs beside the call without it and beside the route users had before, and whether the
launches this change did not mean to touch run as they did.  tools/affine_probe.py's workload and method:

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row), per layout (row-major
and x-major).  One process; the comparison is always against ANOTHER build of the library (`--parent-lib path/to/libmijpeg.so`, the
parent commit's) loaded into the same process.  Every plan is executed once first; then `--reps` rounds, every round one sample of
every plan in turn (interleaved, so that a drifting clock meets all alike); per plan the median and the spread (min .. max).

    launch_<filter>   the perspective launch alone (mj_plan_time_affine, iters = 1) for a keystone of whole images — the corners to
              (0.1 w, 0.15 h), (0.95 w, 0.05 h), (0.85 w, 0.9 h), (0.05 w, 0.8 h): about 35 % fill —, nearest / bilinear / bicubic: ms,
              as a multiple of what the library's own 16-bytes-per-lane copy (mj_device_copy_rate, same process) takes for the bytes
              the launch reads plus writes (both: the decoded images), and beside this build's AFFINE launch of the same filter
              (a 15 degree rotation, tools/affine_probe.py's)
    call      decode_device(size=(224, 224), perspective=..., affine_resample="bilinear", dtype=float16, normalize=...) end to end,
              wall clock around a synchronised call, against the same call without perspective= and against the route the parent
              commit leaves its users: decode at the files' own sizes, then per image torch's grid_sample over a perspective grid
              and interpolate(antialias=True), normalised.  That route does NOT give Pillow's bytes; it is compared for time only.
    untouched the three affine launches, the plain bilinear and bicubic resize launches, the reducing_gap=2.0 reduce launch and the
              ColorJitter colour launches, this build against the parent's, with a second parent plan beside the first: what two
              plans of ONE build differ by

    python tools/perspective_probe.py --parent-lib PATH [--n 1024] [--distinct 64] [--reps 12] [--layouts rowmajor,xmajor]
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

W, H = 1920, 1080
LAYOUTS = {"xmajor": 0, "rowmajor": 1}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILTERS = ("nearest", "bilinear", "bicubic")
JITTER = (("brightness", 1.2), ("contrast", 0.8), ("color", 1.3))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--e2e-reps", type=int, default=4)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,xmajor")
    ap.add_argument("--parent-lib", required=True)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from pyjpegdecoder_amd import BatchDecoder, perspective_coeffs, rotation_matrix
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
    coeffs = perspective_coeffs([(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)], [(0.1 * W, 0.15 * H), (0.95 * W, 0.05 * H), (0.85 * W, 0.9 * H), (0.05 * W, 0.8 * H)])
    matrix = rotation_matrix(15.0, (W, H))

    def emit(**line):
        print(json.dumps(line), flush=True)

    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx, pctx = dec.ctx, other_build(B, args.parent_lib)
        pdec = BatchDecoder(device=0, layout=lname)          # the parent's build behind the same Python
        pdec.ctx.close()
        pdec.ctx = pctx
        once = prepare_batch(files, LAYOUTS[lname], 0, parsed)
        d_once = torch.from_numpy(once.blob).to(dev)
        torch.cuda.synchronize()
        keep = {"prep": once, "n_images": n}
        copy_tbs = ctx.copy_rate_gbs(1 << 30, 5) / 1e3

        # ---- the perspective launch alone, beside this build's affine launch of the same filter
        plans = {}
        for name in FILTERS:
            plans["perspective_" + name] = B.Plan(ctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), output=("float16", MEAN, STD, None),
                                                  perspective=([coeffs] * n, name, (0, 0, 0)))
            plans["affine_" + name] = B.Plan(ctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), output=("float16", MEAN, STD, None),
                                             affine=([matrix] * n, name, (0, 0, 0)))
        try:
            out = torch.empty((n,) + dec._shape(224, 224, 3), dtype=torch.float16, device=dev)
            ok = True
            for plan in plans.values():
                plan.execute(0, out.data_ptr())
                plan.sync()
                ok = ok and not plan.read(rgb=False)["status"].any()
            ms = {name: [] for name in plans}
            for _ in range(args.reps):
                for name, plan in plans.items():
                    ms[name].append(plan.time_affine(1)[0])
            for name in FILTERS:
                plan = plans["perspective_" + name]
                written, source = plan.time_affine(1)[1], plan.time_resize(1, out.data_ptr())[1]
                copy_ms = (int(source) + int(written)) / (copy_tbs * 1e12) * 1e3
                med, amed = statistics.median(ms["perspective_" + name]), statistics.median(ms["affine_" + name])
                emit(layout=lname, point="launch_" + name, status_ok=ok, fused=bool(plan.shape()[1]), perspective_ms=summary(ms["perspective_" + name]),
                     affine_ms=summary(ms["affine_" + name]), perspective_over_affine=round(med / amed, 3), read_bytes=int(source), written_bytes=int(written),
                     copy_tbs=round(copy_tbs, 3), copy_ms=round(copy_ms, 4), perspective_over_copy=round(med / copy_ms, 3),
                     affine_over_copy=round(amed / copy_ms, 3), pixels_per_us=round(n * W * H / (med * 1e3), 1))
        finally:
            for plan in plans.values():
                plan.close()
        del out

        # ---- the whole call
        kw = dict(size=(224, 224), dtype="float16", normalize=(MEAN, STD))
        mean_t, std_t = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1), torch.tensor(STD, device=dev).view(1, 3, 1, 1)
        c = torch.tensor(coeffs, device=dev, dtype=torch.float32)

        def torch_route():
            imgs = pdec.decode_device(files)
            res = []
            grid = None
            for img in imgs:
                x = img.permute(2, 0, 1).unsqueeze(0).float()
                if grid is None:        # (output pixel centres -> source coordinates by the coefficients, normalised for grid_sample)
                    ys, xs = torch.meshgrid(torch.arange(H, device=dev) + 0.5, torch.arange(W, device=dev) + 0.5, indexing="ij")
                    d = c[6] * xs + c[7] * ys + 1
                    gx, gy = (c[0] * xs + c[1] * ys + c[2]) / d, (c[3] * xs + c[4] * ys + c[5]) / d
                    grid = torch.stack((gx / W * 2 - 1, gy / H * 2 - 1), dim=-1).unsqueeze(0)
                x = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
                x = F.interpolate(x, size=(224, 224), mode="bilinear", antialias=True, align_corners=False)
                res.append(((x / 255.0 - mean_t) / std_t).half())
            return torch.cat(res)

        routes = {"perspective": lambda: dec.decode_device(files, perspective=coeffs, affine_resample="bilinear", **kw),
                  "affine": lambda: dec.decode_device(files, affine=matrix, affine_resample="bilinear", **kw),
                  "without": lambda: dec.decode_device(files, **kw),
                  "parent_without": lambda: pdec.decode_device(files, **kw)}
        times = {name: [] for name in routes}
        for r in range(args.e2e_reps + 1):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        times["parent_torch_route"] = []
        for r in range(args.torch_reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch_route()
            torch.cuda.synchronize()
            if r:
                times["parent_torch_route"].append((time.perf_counter() - t0) * 1e3)
        emit(layout=lname, point="call", e2e_decode_device_ms={name: summary(xs) for name, xs in times.items()},
             perspective_cost_ms=round(statistics.median(times["perspective"]) - statistics.median(times["without"]), 3))

        # ---- the launches this change did not mean to touch: this build against the parent's, a second parent plan beside the first
        cases = [("affine_" + name, {"affine": ([matrix] * n, name, (0, 0, 0))}, "affine") for name in FILTERS]
        cases += [("bilinear", {}, "resize"), ("bicubic", {"filter": "bicubic"}, "resize"),
                  ("gap2_bicubic", {"filter": "bicubic", "reducing_gap": 2.0}, "reduce"), ("colour_jitter", {"colour": [JITTER] * n}, "colour")]
        for label, pk, what in cases:
            plans = {"parent": B.Plan(pctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), **pk),
                     "parent_twin": B.Plan(pctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), **pk),
                     "this": B.Plan(ctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), **pk)}
            try:
                out = {name: torch.empty((n,) + dec._shape(224, 224, 3), dtype=torch.uint8, device=dev) for name in plans}
                for name, plan in plans.items():
                    plan.execute(0, out[name].data_ptr())
                    plan.sync()
                torch.cuda.synchronize()
                ts = {name: [] for name in plans}
                for _ in range(2 * args.reps):
                    for name, plan in plans.items():
                        ts[name].append(plan.time_affine(1)[0] if what == "affine" else plan.time_reduce(1) if what == "reduce" else
                                        plan.time_colour(1)[0] if what == "colour" else plan.time_resize(1, out[name].data_ptr())[0])
                line = {"layout": lname, "point": "untouched_" + label, "launch": what, "this_equals_parent": bool(torch.equal(out["this"], out["parent"]))}
                for name in plans:
                    line[name + "_ms"] = summary(ts[name])
                lo, hi = min(ts["parent"] + ts["parent_twin"]), max(ts["parent"] + ts["parent_twin"])
                line["this_median_inside_parents_spread"] = bool(lo <= statistics.median(ts["this"]) <= hi)
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
