"""Output colour mode on the GPU box: what the launch that converts costs beside the launches it stands in for, and that the
native colour launch has not moved.

1024 x 1920x1080 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan) — 4:2:0
colour and greyscale — to 224 x 224, per layout (row-major and x-major), bilinear.  One process; every plan executed once first
(the resize launch reads what stage 2 left), then `--reps` rounds, every round one sample of every point in turn (interleaved, so
that a drifting clock meets all points alike); per point the median and the spread (min .. max) over the rounds.  A sample is
mj_plan_time_resize(iters=1): one warm launch, then one between two HIP events.

    colour_ms, colour_twin_ms            (a) colour files, mode "RGB" — native: the plan of a call without mode=, twice (two plans of ONE
    colour_parent_ms, ..._parent_twin_ms     build: what a difference between builds has to exceed), and the same launch from another
                                             build (`--parent-lib path/to/libmijpeg.so`, e.g. the parent commit's) in the same process
    grey_ms                              (b) greyscale files, mode "L" — native: a third of the colour launch's bytes on both sides
    grey_to_rgb_ms                       (c) greyscale files, mode "RGB": reads what (b) reads, writes what (a) writes
    colour_to_l_ms                       (d) colour files, mode "L": reads what (a) reads, writes what (b) writes
    own_grey_to_rgb_ms, own_copy_ms      (e) the one extra launch of an own-size plan (mj_plan_request.mode) for the greyscale files
                                             under "RGB", and the library's plain 16-bytes-per-lane copy of the bytes it writes
    shape                                mj_debug_resize_shape of every resized plan

and whether the first images of (c) and (d) equal tools/mode_model.py + resize_model.py applied to the plain decode of the same
files, and the shader clock the board reports.

    python tools/mode_probe.py [--n 1024] [--distinct 64] [--reps 16] [--layouts rowmajor,xmajor] [--parent-lib PATH]
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
LAYOUTS = {"xmajor": 0, "rowmajor": 1}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,xmajor")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--check-images", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import mode_model, resize_model, synth

    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(0)
    clock = {"device": props.name, "shader_clock_max_mhz": round(getattr(props, "clock_rate", 0) / 1e3, 1)}
    try:
        clock["shader_clock_now_mhz"] = int(torch.cuda.clock_rate())
    except Exception as exc:                                  # (no management library on the box: the maximum stands alone)
        clock["shader_clock_now_mhz"] = f"unavailable ({type(exc).__name__})"
    print(json.dumps(clock), flush=True)
    n, nd = args.n, args.distinct
    sets = {}
    for kind, sub in (("colour", "420"), ("grey", "grey")):
        blob, offs = synth.synth_batch(nd, args.seed, W, H, 85, sub, 120)
        raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nd)]
        files = [raws[i % nd] for i in range(n)]
        sets[kind] = (raws, files, [parse_jpeg(f, headers_only=True) for f in files])
    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx = dec.ctx
        pctx = other_build(B, args.parent_lib) if args.parent_lib else None
        preps, blobs, plans, comps = {}, {}, {}, {}
        for kind, (_, files, parsed) in sets.items():
            preps[kind] = prepare_batch(files, LAYOUTS[lname], 0, parsed)
            blobs[kind] = torch.from_numpy(preps[kind].blob).to(dev)
        torch.cuda.synchronize()

        def plan(name, c, kind, co, **kw):
            plans[name] = B.Plan(c, preps[kind].to_c(blobs[kind].data_ptr()), {"prep": preps[kind], "n_images": n}, **kw)
            comps[name] = co
        plan("colour", ctx, "colour", 3, size=SIZE)
        plan("grey", ctx, "grey", 1, size=SIZE)
        plan("grey_to_rgb", ctx, "grey", 3, size=SIZE, mode="RGB")
        plan("colour_to_l", ctx, "colour", 1, size=SIZE, mode="L")
        plan("colour_twin", ctx, "colour", 3, size=SIZE)
        if pctx is not None:
            plan("colour_parent", pctx, "colour", 3, size=SIZE)
            plan("colour_parent_twin", pctx, "colour", 3, size=SIZE)
        plan("own_grey_to_rgb", ctx, "grey", 3, mode="RGB")
        try:
            out, ok = {}, True
            for name, p in plans.items():
                out[name] = torch.empty(int(p.info.rgb_bytes), dtype=torch.uint8, device=dev)
                p.execute(0, out[name].data_ptr())
                p.sync()
                ok = ok and not p.read(rgb=False)["status"].any()
            torch.cuda.synchronize()
            # the first images of the converting plans against the models of the plain decode of the same files
            k = min(args.check_images, nd)
            equal = {}
            for name, kind, mode in (("grey_to_rgb", "grey", "RGB"), ("colour_to_l", "colour", "L")):
                full = dec.decode(sets[kind][0][:k])
                shape = (n,) + dec._shape(SIZE[0], SIZE[1], comps[name])
                got_all = out[name].view(shape)
                same = True
                for i in range(k):
                    a = full[i].swapaxes(0, 1) if lname == "xmajor" else full[i]
                    want = resize_model.resize(np.ascontiguousarray(mode_model.convert(np.ascontiguousarray(a), mode)), SIZE)
                    got = got_all[i].cpu().numpy()
                    same = same and bool(np.array_equal(got.swapaxes(0, 1) if lname == "xmajor" else got, want))
                equal[name] = same
            same_parent = bool(torch.equal(out["colour"], out["colour_parent"])) if pctx is not None else None
            samples = {name: [] for name in plans}
            for _ in range(args.reps):
                for name, p in plans.items():
                    samples[name].append(p.time_resize(1, out[name].data_ptr())[0])
            copy_tbs = ctx.copy_rate_gbs(1 << 30, 5) / 1e3
            med = {name: statistics.median(xs) for name, xs in samples.items()}
            line = {"layout": lname, "images": n, "distinct": nd, "size": list(SIZE), "copy_tbs": round(copy_tbs, 3)}
            for name, p in plans.items():
                src = int(p.time_resize(1, out[name].data_ptr())[1])
                line[name + "_ms"] = dict(summary(samples[name]), source_bytes=src, output_bytes=int(p.info.rgb_bytes))
            # (a copy of N bytes reads N and writes N)
            line["own_copy_ms"] = round(2 * int(plans["own_grey_to_rgb"].info.rgb_bytes) / (copy_tbs * 1e12) * 1e3, 4)
            line["grey_to_rgb_over_grey"] = round(med["grey_to_rgb"] / med["grey"], 3)
            line["grey_to_rgb_over_colour"] = round(med["grey_to_rgb"] / med["colour"], 3)
            line["colour_to_l_over_colour"] = round(med["colour_to_l"] / med["colour"], 3)
            line["shape"] = {name: p.resize_shape() for name, p in plans.items() if not name.startswith("own")}
            line.update(status_ok=ok, equals_models_first_images=equal, parent_colour_equals_this_build=same_parent)
            if pctx is not None:
                line["colour_minus_parent_ms"] = round(med["colour"] - med["colour_parent"], 4)
                line["twin_gap_ms"] = round(max(abs(med["colour"] - med["colour_twin"]), abs(med["colour_parent"] - med["colour_parent_twin"])), 4)
            print(json.dumps(line), flush=True)
        finally:
            for p in plans.values():
                p.close()
        del out, blobs
        if pctx is not None:
            pctx.close()
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
