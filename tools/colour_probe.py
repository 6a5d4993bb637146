"""Colour operations on the GPU box: what the colour launches cost, what `decode_device(files, size=, color_ops=)` costs beside the
call without it and beside the route users had before, and whether the launches this change did not mean to touch run as they did.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan) to
224 x 224, float16 normalised, per layout (row-major and x-major).  One process; the comparison is always against ANOTHER build of
the library (`--parent-lib path/to/libmijpeg.so`, the parent commit's) loaded into the same process.  Every plan is executed once
first; then `--reps` rounds, every round one sample of every plan in turn (interleaved, so that a drifting clock meets all alike);
per plan the median and the spread (min .. max).

    launches_<chain>  the colour launches alone (mj_plan_time_colour, iters = 1) for a ColorJitter chain (brightness, contrast, color)
              and for (autocontrast, equalize): ms, beside what the library's own 16-bytes-per-lane copy (mj_device_copy_rate, same
              process) takes for the bytes they move — per step the canvas read and written (the last write in float16), and read
              once more where the step takes a histogram —, and beside the resize launch of the same plan (mj_plan_time_resize of
              the plan minus the colour launches, and of the plan without color_ops).  `_padded`: the same on a letterbox — every
              image resized to 112 x 63 in the middle of the canvas, the rest one fill colour —, the histogram launch's worst case:
              most lanes of a workgroup add to the same LDS bin
              `blur` and `simclr`: ("gaussian_blur", r) alone and behind (brightness, contrast, color), r drawn per output from
              U(0.1, 2.0) as the self-supervised recipes do — the plane-resident blur launch (a component plane in LDS, all six
              passes there) —, and `_passes`: the same plans made under option MJ_BLUR=passes, one launch per pass through a third
              canvas (five more reads and writes of the canvas)
    call      decode_device(size=(224, 224), color_ops=jitter, dtype=float16, normalize=...) end to end, wall clock around a
              synchronised call, against the same call without color_ops= (the feature's cost) and against what a user does today:
              the uint8 call, then brightness, contrast and saturation in torch on the GPU, then the normalisation.  That route
              rounds differently — it does NOT give Pillow's bytes; it is compared for time only.
    call_blur the same for color_ops=[("gaussian_blur", r_k)] per output: against the call without it, and against the uint8 call,
              then a separable Gaussian (sigma = r_k, 13 taps, edges reflected) as two grouped convolutions in torch and the
              normalisation — other bytes than Pillow's again, compared for time only
    launches_hue / launches_color / launches_jitter_hue   (`--hue`) the colour launches alone for ("adjust_hue", f_k) with f_k drawn per
              output from U(-0.1, 0.1) as ColorJitter(hue=0.1) does — the hue launch k_colour_hue, four pixels per lane —, for ("color", 1.3)
              alone — the per-pixel three-component op most like it, one k_colour_apply launch —, and for the whole four-op ColorJitter
              chain (jitter + that hue); the three-op chain is launches_jitter as ever
    call_hue  (`--hue`) decode_device end to end with color_ops=[("adjust_hue", f_k)] per output and with the four-op chain, against the
              call without color_ops and against the uint8 call, then the HSV round trip with h + f_k in float32 and the normalisation
              in torch on the GPU (torchvision's tensor branch, restated) — that route does NOT give the PIL branch's bytes, which
              are what a Pillow pipeline trains on; it is compared for time only
    untouched the plain bilinear and bicubic resize launches, the reducing_gap=2.0 reduce launch, the affine launch and the colour
              launches of the ColorJitter chain (and, with `--hue`, of a blur-only chain), this build against the parent's, with a second parent plan beside the first: what two plans of ONE build differ by

    python tools/colour_probe.py --parent-lib PATH [--n 1024] [--distinct 64] [--reps 12] [--layouts rowmajor,xmajor] [--hue]
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
JITTER = (("brightness", 1.2), ("contrast", 0.8), ("color", 1.3))
CHAINS = {"jitter": JITTER, "autocontrast_equalize": (("autocontrast",), ("equalize",))}
# canvases moved: per step one read and one write (the last write is float16: two), one more read per step with a histogram
MOVED = {"jitter": 3 + 2 + 2 + 1, "autocontrast_equalize": 2 + 1 + 2 + 2, "blur": 1 + 2, "simclr": 4 + 3 + 2 + 1,
         "blur_passes": 6 + 5 + 2, "simclr_passes": 3 + 3 + 1 + 6 + 5 + 2, "hue": 1 + 2, "color": 1 + 2, "jitter_hue": 3 + 2 + 2 + 1 + 2}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--e2e-reps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,xmajor")
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--hue", action="store_true", help="the adjust_hue points, in the place of the `_padded` and `_passes` ones (the parent build runs none of them and need not have the op)")
    ap.add_argument("--parent-first", action="store_true", help="call: the parent build's route first in every round (the order's share of a difference)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyjpegdecoder_amd import BatchDecoder, rotation_matrix
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
        output = ("float16", MEAN, STD, None)

        # ---- the colour launches alone
        plans = {name: B.Plan(ctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), output=output, colour=[chain] * n) for name, chain in CHAINS.items()}
        radii = [float(v) for v in np.random.default_rng(args.seed).uniform(0.1, 2.0, n)]
        blurs = {"blur": [(("gaussian_blur", r),) for r in radii], "simclr": [JITTER + (("gaussian_blur", r),) for r in radii]}
        for route in ((None,) if args.hue else (None, "passes")):
            B.set_option("MJ_BLUR", route)          # (read when a plan is created)
            for name, chains in blurs.items():
                plans[name + ("_passes" if route else "")] = B.Plan(ctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), output=output, colour=chains)
        B.set_option("MJ_BLUR", None)
        factors = [float(v) for v in np.random.default_rng(args.seed + 1).uniform(-0.1, 0.1, n)]
        hues = {"hue": [(("adjust_hue", f),) for f in factors], "color": [(("color", 1.3),)] * n, "jitter_hue": [JITTER + (("adjust_hue", f),) for f in factors]}
        if args.hue:
            for name, chains in hues.items():
                plans[name] = B.Plan(ctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), output=output, colour=chains)
        for name, chain in ({} if args.hue else CHAINS).items():
            plans[name + "_padded"] = B.Plan(ctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), output=output, colour=[chain] * n,
                                             places=[(112, 63, 56, 80)] * n, fill=(124, 116, 104))
        plans["without"] = B.Plan(ctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), output=output)
        try:
            out = torch.empty((n,) + dec._shape(224, 224, 3), dtype=torch.float16, device=dev)
            ok = True
            for plan in plans.values():
                plan.execute(0, out.data_ptr())
                plan.sync()
                ok = ok and not plan.read(rgb=False)["status"].any()
            cs, rs = {name: [] for name in plans if name != "without"}, {name: [] for name in plans}
            for _ in range(args.reps):
                for name, plan in plans.items():
                    if name in cs:
                        cs[name].append(plan.time_colour(1)[0])
                    rs[name].append(plan.time_resize(1, out.data_ptr())[0])
            for name in cs:
                canvas = int(plans[name].time_colour(1)[1])
                moved = MOVED[name.replace("_padded", "")] * canvas
                copy_ms = moved / (copy_tbs * 1e12) * 1e3
                med = statistics.median(cs[name])
                emit(layout=lname, point="launches_" + name, status_ok=ok, colour_ms=summary(cs[name]), canvas_bytes=canvas, moved_bytes=moved,
                     copy_tbs=round(copy_tbs, 3), copy_ms=round(copy_ms, 4), colour_over_copy=round(med / copy_ms, 2),
                     resize_and_colour_ms=summary(rs[name]), resize_without_color_ops_ms=summary(rs["without"]))
        finally:
            for plan in plans.values():
                plan.close()
        del out

        # ---- the whole call
        kw = dict(size=(224, 224), dtype="float16", normalize=(MEAN, STD))
        planar = lname.startswith("planar")
        cdim = 1 if planar else 3
        shape = [1, 1, 1, 1]
        shape[cdim] = 3
        mean_t, std_t = torch.tensor(MEAN, device=dev).view(shape), torch.tensor(STD, device=dev).view(shape)
        wts = torch.tensor((0.299, 0.587, 0.114), device=dev).view(shape)

        def torch_route():
            x = pdec.decode_device(files, size=(224, 224)).float()
            x = (x * JITTER[0][1]).clamp_(0, 255)
            grey = (x * wts).sum(dim=cdim, keepdim=True)
            x = (grey.mean(dim=(1, 2, 3), keepdim=True) * (1 - JITTER[1][1]) + x * JITTER[1][1]).clamp_(0, 255)
            grey = (x * wts).sum(dim=cdim, keepdim=True)
            x = (grey * (1 - JITTER[2][1]) + x * JITTER[2][1]).clamp_(0, 255)
            return ((x / 255.0 - mean_t) / std_t).half()

        routes = {"color_ops": lambda: dec.decode_device(files, color_ops=list(JITTER), **kw),
                  "without": lambda: dec.decode_device(files, **kw),
                  "parent_without": lambda: pdec.decode_device(files, **kw),
                  "parent_uint8_then_torch": torch_route}
        if args.parent_first:
            routes = {name: routes[name] for name in ("parent_without", "without", "color_ops", "parent_uint8_then_torch")}
        times = {name: [] for name in routes}
        for r in range(args.e2e_reps + 1):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        emit(layout=lname, point="call", e2e_decode_device_ms={name: summary(xs) for name, xs in times.items()},
             color_ops_cost_ms=round(statistics.median(times["color_ops"]) - statistics.median(times["without"]), 3))

        # ---- the whole call with a blur per output
        taps = torch.arange(-6, 7, device=dev, dtype=torch.float32)
        kern = torch.exp(-0.5 * (taps[None, :] / torch.tensor(radii, device=dev)[:, None]) ** 2)
        kern = (kern / kern.sum(dim=1, keepdim=True)).repeat_interleave(3, dim=0)                  # (one row per output and component)

        def torch_blur_route():             # (interleaved layouts: the two image axes are 1 and 2, whichever is the width)
            x = pdec.decode_device(files, size=(224, 224)).float().movedim(3, 1).reshape(1, n * 3, 224, 224)
            x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (6, 6, 0, 0), mode="reflect"), kern.view(n * 3, 1, 1, 13), groups=n * 3)
            x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (0, 0, 6, 6), mode="reflect"), kern.view(n * 3, 1, 13, 1), groups=n * 3)
            x = x.reshape(n, 3, 224, 224).movedim(1, 3)
            return ((x / 255.0 - mean_t) / std_t).half()

        routes = {"blur": lambda: dec.decode_device(files, color_ops=blurs["blur"], **kw),
                  "without": lambda: dec.decode_device(files, **kw),
                  "parent_uint8_then_torch_blur": torch_blur_route}
        times = {name: [] for name in routes}
        for r in range(args.e2e_reps + 1):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        emit(layout=lname, point="call_blur", e2e_decode_device_ms={name: summary(xs) for name, xs in times.items()},
             blur_cost_ms=round(statistics.median(times["blur"]) - statistics.median(times["without"]), 3))

        # ---- the whole call with a hue shift per output
        if args.hue:
            shifts = torch.tensor(factors, device=dev).view(n, 1, 1)

            def torch_hue_route():              # (torchvision's _rgb2hsv / _hsv2rgb on a float tensor: interleaved layouts, components last)
                x = pdec.decode_device(files, size=(224, 224)).float() / 255.0
                r, g, b = x.unbind(dim=3)
                maxc, minc = x.amax(dim=3), x.amin(dim=3)
                eqc = maxc == minc
                cr = maxc - minc
                ones = torch.ones_like(maxc)
                s = cr / torch.where(eqc, ones, maxc)
                crd = torch.where(eqc, ones, cr)
                rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
                hr = (maxc == r) * (bc - gc)
                hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
                hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
                h = (((hr + hg + hb) / 6.0 + 1.0) % 1.0 + shifts) % 1.0
                i = torch.floor(h * 6.0)
                f = h * 6.0 - i
                i = i.to(torch.int64) % 6
                v = maxc
                p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
                pick = torch.stack((torch.stack((v, q, p, p, t, v)), torch.stack((t, v, v, q, p, p)), torch.stack((p, p, t, v, v, q))))
                x = pick.gather(1, i.expand(3, 1, -1, -1, -1)).squeeze(1).movedim(0, 3)
                return ((x - mean_t) / std_t).half()

            routes = {"hue": lambda: dec.decode_device(files, color_ops=hues["hue"], **kw),
                      "jitter_hue": lambda: dec.decode_device(files, color_ops=hues["jitter_hue"], **kw),
                      "without": lambda: dec.decode_device(files, **kw),
                      "parent_uint8_then_torch_hue": torch_hue_route}
            times = {name: [] for name in routes}
            for r in range(args.e2e_reps + 1):
                for name, fn in routes.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if r:
                        times[name].append((time.perf_counter() - t0) * 1e3)
            emit(layout=lname, point="call_hue", e2e_decode_device_ms={name: summary(xs) for name, xs in times.items()},
                 hue_cost_ms=round(statistics.median(times["hue"]) - statistics.median(times["without"]), 3),
                 jitter_hue_cost_ms=round(statistics.median(times["jitter_hue"]) - statistics.median(times["without"]), 3))

        # ---- the launches this change did not mean to touch: this build against the parent's, a second parent plan beside the first
        matrix = rotation_matrix(15.0, (W, H))
        for label, pk in (("bilinear", {}), ("bicubic", {"filter": "bicubic"}), ("gap2_bicubic", {"filter": "bicubic", "reducing_gap": 2.0}),
                          ("affine_bilinear", {"affine": ([matrix] * n, "bilinear", (0, 0, 0))}), ("colour_jitter", {"colour": [JITTER] * n})) + \
                ((("colour_blur", {"colour": blurs["blur"]}),) if args.hue else ()):
            plans = {"parent": B.Plan(pctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), **pk),
                     "parent_twin": B.Plan(pctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), **pk),
                     "this": B.Plan(ctx, once.to_c(d_once.data_ptr()), keep, size=(224, 224), **pk)}
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
                        if "reducing_gap" in pk:
                            rd[name].append(plan.time_reduce(1))
                        if "affine" in pk:
                            rd[name].append(plan.time_affine(1)[0])
                        if "colour" in pk:
                            rd[name].append(plan.time_colour(1)[0])
                line = {"layout": lname, "point": "untouched_" + label, "this_equals_parent": bool(torch.equal(out["this"], out["parent"]))}
                for name in plans:
                    line[name + "_resize_ms"] = summary(rs[name])
                    if rd[name]:
                        line[name + ("_reduce_ms" if "reducing_gap" in pk else "_affine_ms" if "affine" in pk else "_colour_ms")] = summary(rd[name])
                which = rd if rd["this"] else rs
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
