"""erase= on the GPU box: what RandomErasing costs as one more launch of the plan, beside what a user does today — the call without
it, then a torch loop of one slice assignment per erased output — and whether the launches this change did not touch run as they did.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan) ->
224 x 224, float16 normalised, per layout (row-major and x-major).  Boxes: pyjpegdecoder_amd.random_erasing_rect (torchvision's
RandomErasing.get_params, default scale and ratio, fixed seed) on a quarter of the outputs; once with constants (value 0) and once
with values — a (3, h, w) float16 block of noise per box, drawn on the GPU before anything is timed, the same blocks for both routes.
Medians and spreads (min .. max) of `--reps` / `--e2e-reps` rounds, every round one sample of every variant in turn (interleaved, so
that a drifting clock meets all alike), after one round that warms.

    launch       mj_plan_time_erase(iters=1): the erase launch alone, constants and values, with the bytes it writes (values: reads as
                 many), beside mj_device_copy_rate's k_copy16 on the same number of bytes (read + written: twice that)
    call         decode_device, wall clock around a synchronised call: without erase=, with constants, with values
    torch_loop   the call without erase= followed by the loop `out[k, box] = v` over the erased outputs, synchronised: today's route
    untouched    with --parent-lib: mj_plan_time_resize (bilinear, bicubic), _reduce (reducing_gap 2), _affine (a rotation) and _colour
                 (ColorJitter's brightness, contrast, color, adjust_hue) of this build beside the parent's in the same process

    python tools/erase_probe.py [--n 1024] [--distinct 64] [--reps 12] [--e2e-reps 7] [--layouts rowmajor,xmajor] [--parent-lib PATH]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.normalize_probe import other_build, summary  # noqa: E402
from tools.views_probe import LAYOUTS, MEAN, STD, H, W  # noqa: E402

SIZE = (224, 224)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--e2e-reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,xmajor")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()

    import torch
    from pyjpegdecoder_amd import BatchDecoder, random_erasing_rect
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch, rotation_matrix
    from tools import synth

    dev = torch.device("cuda", 0)
    n, nd = args.n, args.distinct
    blob, offs = synth.synth_batch(nd, args.seed, W, H, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nd)]
    files = [raws[i % nd] for i in range(n)]
    parsed = [parse_jpeg(f, headers_only=True) for f in files]
    g = torch.Generator().manual_seed(args.seed)
    rects = [random_erasing_rect(SIZE, generator=g) if k % 4 == 0 else None for k in range(n)]
    erased = [k for k, r in enumerate(rects) if r is not None]
    elements = sum(3 * rects[k][2] * rects[k][3] for k in erased)
    noise = torch.randn(elements, dtype=torch.float16, device=dev)
    blocks, at = {}, 0
    for k in erased:
        _, _, w, h = rects[k]
        blocks[k] = noise[at:at + 3 * w * h].view(3, h, w)
        at += 3 * w * h
    const = [None if r is None else r + (0.0,) for r in rects]
    values = [None if r is None else r + (blocks[k],) for k, r in enumerate(rects)]
    common = dict(size=SIZE, dtype="float16", normalize=(MEAN, STD))
    output = ("float16", MEAN, STD, None)

    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx = dec.ctx
        line = {"layout": lname, "files": n, "size": "224 x 224", "dtype": "float16 normalised", "erased_outputs": len(erased),
                "bytes_written": 2 * elements, "share_of_tensor": round(elements / (n * 3 * SIZE[0] * SIZE[1]), 4)}
        # ---- the launch alone
        prep = prepare_batch(files, LAYOUTS[lname], 0, parsed)
        d_blob = torch.from_numpy(prep.blob).to(dev)
        keep = {"prep": prep, "n_images": n}
        plans = {name: B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE, output=output) for name in ("const", "values")}
        try:
            out = torch.empty((n,) + dec._shape(*SIZE, 3), dtype=torch.float16, device=dev)
            plans["const"].set_erase([(k,) + rects[k] + (0.0,) for k in erased])
            offsets, at = [], 0
            for k in erased:
                offsets.append(at)
                at += blocks[k].numel()
            plans["values"].set_erase([(k,) + rects[k] + (("values", o),) for k, o in zip(erased, offsets)], noise.data_ptr(), keep=noise)
            for plan in plans.values():
                plan.execute(0, out.data_ptr())
                plan.sync()
            ms = {"const": [], "values": [], "copy16_same_bytes": []}
            copy_bytes = (2 * elements) & ~15
            copy_ms = ctypes.c_float()
            ctx.lib.mj_device_copy_rate.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
            for r in range(args.reps + 1):
                for name in ("const", "values"):
                    t, nbytes = plans[name].time_erase(1)
                    assert nbytes == 2 * elements
                    if r:
                        ms[name].append(t)
                ctx.check(ctx.lib.mj_device_copy_rate(ctx.handle, copy_bytes, 1, ctypes.byref(copy_ms)))
                if r:
                    ms["copy16_same_bytes"].append(copy_ms.value)
            line["launch_ms"] = {name: summary(xs) for name, xs in ms.items()}
            med = {name: line["launch_ms"][name]["median"] for name in ms}
            line["launch_gbs"] = {"const_written": round(2 * elements / med["const"] / 1e6, 1), "values_read_and_written": round(4 * elements / med["values"] / 1e6, 1),
                                  "copy16_read_and_written": round(2 * copy_bytes / med["copy16_same_bytes"] / 1e6, 1)}
        finally:
            for plan in plans.values():
                plan.close()
        del d_blob
        # ---- the whole call, and today's route
        xm = lname == "xmajor"

        def torch_loop(t, with_values):
            for k in erased:
                x, y, w, h = rects[k]
                if xm:
                    t[k, x:x + w, y:y + h, :] = blocks[k].permute(2, 1, 0) if with_values else 0.0
                else:
                    t[k, y:y + h, x:x + w, :] = blocks[k].permute(1, 2, 0) if with_values else 0.0
            return t
        routes = {"call_without_erase": lambda: dec.decode_device(files, **common),
                  "call_with_constants": lambda: dec.decode_device(files, erase=const, **common),
                  "call_with_values": lambda: dec.decode_device(files, erase=values, **common),
                  "torch_loop_constants": lambda: torch_loop(dec.decode_device(files, **common), False),
                  "torch_loop_values": lambda: torch_loop(dec.decode_device(files, **common), True)}
        t, results = {name: [] for name in routes}, {}
        for r in range(args.e2e_reps + 1):
            for name, call in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = call()
                torch.cuda.synchronize()
                if r:
                    t[name].append((time.perf_counter() - t0) * 1e3)
                else:
                    results[name] = res.view(torch.int16).clone()
                del res
        line["e2e_ms"] = {name: summary(xs) for name, xs in t.items()}
        line["library_equals_torch_loop"] = bool(torch.equal(results["call_with_constants"], results["torch_loop_constants"]) and
                                                 torch.equal(results["call_with_values"], results["torch_loop_values"]))
        del results
        # ---- the launches this change did not touch, beside the parent build's
        if args.parent_lib:
            pctx = other_build(B, args.parent_lib)
            prep = prepare_batch(files, LAYOUTS[lname], 0, parsed)
            d_blob = torch.from_numpy(prep.blob).to(dev)
            keep = {"prep": prep, "n_images": n}
            rot = [rotation_matrix(15.0, (W, H))] * n
            jitter = [(("brightness", 1.2), ("contrast", 0.8), ("color", 1.3), ("adjust_hue", 0.05))] * n
            kinds = {"bilinear": (dict(), "time_resize"), "bicubic": (dict(filter="bicubic"), "time_resize"),
                     "reduce": (dict(reducing_gap=2.0), "time_reduce"), "affine": (dict(affine=(rot, "bilinear", (0, 0, 0))), "time_affine"),
                     "colour_jitter": (dict(colour=jitter), "time_colour")}
            un = {}
            for kind, (kw, fn) in kinds.items():
                made = {}
                try:
                    for side, c in (("this", ctx), ("parent", pctx)):
                        made[side] = B.Plan(c, prep.to_c(d_blob.data_ptr()), keep, size=SIZE, output=output, **kw)
                        made[side].execute(0, out.data_ptr())
                        made[side].sync()
                    ms = {"this": [], "parent": []}
                    for r in range(args.reps + 1):
                        for side, plan in made.items():
                            v = getattr(plan, fn)(1)
                            if r:
                                ms[side].append(v[0] if isinstance(v, tuple) else v)
                    un[kind] = {side: summary(xs) for side, xs in ms.items()}
                    un[kind]["this_median_inside_parent_min_max"] = bool(un[kind]["parent"]["min"] <= un[kind]["this"]["median"] <= un[kind]["parent"]["max"])
                finally:
                    for plan in made.values():
                        plan.close()
            line["untouched_launches_ms"] = un
            pctx.close()
            del d_blob
        print(json.dumps(line), flush=True)
        del out
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
