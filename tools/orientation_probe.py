"""EXIF orientation on the GPU box: what the orient launch (csrc/orient.hip) and the oriented resize launch cost, and that the
existing paths have not moved.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan), one
process, every plan executed once first (the last launch of a plan reads what stage 2 left), then `--reps` rounds, every round one
sample of every point in turn (interleaved, so that a drifting clock meets all points alike); per point the median and the spread
(min .. max).  A sample of a launch is mj_plan_time_resize(iters=1) — one warm launch, then one between two HIP events; for an
oriented plan at the files' own sizes that launch is the orient launch.

    1  orient6_ms, orient3_ms    the orient launch, all files orientation 6 / 3, per layout; copy_ms: the library's plain
                                 16-bytes-per-lane copy of the same bytes (mj_device_copy_rate); the ratios
    2  resize6_ms                the oriented resize launch -> 224 x 224, orientation 6, against resize_ms (the plain launch of the same
                                 layout, same files) and resize_other_layout_ms (the plain launch of the layout whose access pattern it borrows)
    3  resize_ms / resize_twin_ms / resize_parent_ms / resize_parent_twin_ms and default_execute_*_ms
                                 the plain uint8 resize launch and the fused decode of a default call (mj_plan_time_execute), this build
                                 and another build of the library loaded into the same process (`--parent-lib`); the twins — a
                                 second plan of the same build — say how far two plans of ONE build lie apart
    4  e2e_none_ms, e2e_exif_ms  decode_device(orientation=None / "exif") on these files, which have no EXIF: wall clock with a device
                                 synchronize — the host cost of reading the tags

    python tools/orientation_probe.py [--n 1024] [--distinct 64] [--reps 16] [--layouts rowmajor,xmajor] [--parent-lib PATH]
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

W, H, SIZE = 1920, 1080, (224, 224)
LAYOUTS = {"xmajor": 0, "rowmajor": 1, "planar": 2, "planar_rowmajor": 3}
OTHER = {"xmajor": "rowmajor", "rowmajor": "xmajor", "planar": "planar_rowmajor", "planar_rowmajor": "planar"}


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "samples": len(xs)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--e2e-reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,xmajor")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()

    import torch
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools.normalize_probe import other_build

    from tools import synth
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
        other = prepare_batch(files, LAYOUTS[OTHER[lname]], 0, parsed)
        d_blob = torch.from_numpy(prep.blob).to(dev)
        torch.cuda.synchronize()

        def plan(c, p=prep, **kw):
            return B.Plan(c, p.to_c(d_blob.data_ptr()), {"prep": p, "n_images": n}, **kw)
        own_bytes = n * W * H * 3
        # the launches are sampled group by group: every plan owns 6.4 GB of stored-order pixels
        groups = {
            "orient": lambda: {"orient6": plan(ctx, orientation=[6] * n), "orient3": plan(ctx, orientation=[3] * n)},
            "resize": lambda: dict({"resize": plan(ctx, size=SIZE), "resize_twin": plan(ctx, size=SIZE),
                                    "resize6": plan(ctx, size=SIZE, orientation=[6] * n),
                                    "resize_other_layout": plan(ctx, other, size=SIZE)},
                                   **({"resize_parent": plan(pctx, size=SIZE), "resize_parent_twin": plan(pctx, size=SIZE)} if pctx else {})),
        }
        line = {"layout": lname, "images": n, "distinct": nd, "own_size_bytes": own_bytes}
        for gname, make in groups.items():
            plans = make()
            try:
                outs, ok = {}, True
                for name, p in plans.items():
                    outs[name] = torch.empty(p.info.rgb_bytes, dtype=torch.uint8, device=dev)
                    p.execute(0, outs[name].data_ptr())
                    p.sync()
                    ok = ok and not p.read(rgb=False)["status"].any()
                samples = {k: [] for k in plans}
                for _ in range(args.reps):
                    for name, p in plans.items():
                        samples[name].append(p.time_resize(1, outs[name].data_ptr())[0])
                for name in plans:
                    line[name + "_ms"] = summary(samples[name])
                line[gname + "_status_ok"] = bool(ok)
                if "resize_parent" in outs:
                    line["parent_resize_equals_this_build"] = bool(torch.equal(outs["resize"], outs["resize_parent"]))
            finally:
                for p in plans.values():
                    p.close()
            del outs
        copy_ms = 2.0 * own_bytes / (ctx.copy_rate_gbs(1 << 31, 5) * 1e9) * 1e3
        line["copy_ms"] = round(copy_ms, 4)
        line["orient6_over_copy"] = round(line["orient6_ms"]["median"] / copy_ms, 3)
        line["orient3_over_copy"] = round(line["orient3_ms"]["median"] / copy_ms, 3)
        line["resize6_over_resize"] = round(line["resize6_ms"]["median"] / line["resize_ms"]["median"], 3)
        line["resize6_over_other_layout"] = round(line["resize6_ms"]["median"] / line["resize_other_layout_ms"]["median"], 3)
        # the fused decode of a default call, this build and the other
        plans = {"default_execute": plan(ctx), "default_execute_twin": plan(ctx)}
        if pctx:
            plans.update({"default_execute_parent": plan(pctx), "default_execute_parent_twin": plan(pctx)})
        try:
            outs = {k: torch.empty(p.info.rgb_bytes, dtype=torch.uint8, device=dev) for k, p in plans.items()}
            for name, p in plans.items():
                p.execute(0, outs[name].data_ptr())
                p.sync()
            samples = {k: [] for k in plans}
            for _ in range(args.reps):
                for name, p in plans.items():
                    front, main_ms = p.time_execute(1, outs[name].data_ptr())
                    samples[name].append(front + main_ms)
            for name in plans:
                line[name + "_ms"] = summary(samples[name])
            line["default_form"] = plans["default_execute"].stage1_form()
        finally:
            for p in plans.values():
                p.close()
        del outs, d_blob
        print(json.dumps(line), flush=True)
        e2e = {"none": [], "exif": []}
        for r in range(args.e2e_reps + 1):
            for name in e2e:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t = dec.decode_device(files, orientation=None if name == "none" else "exif")
                torch.cuda.synchronize()
                if r:                                      # (round 0 warms both)
                    e2e[name].append((time.perf_counter() - t0) * 1e3)
                del t
        t0 = time.perf_counter()
        for _ in range(10):
            B.exif_orientations(files)
        tags_ms = (time.perf_counter() - t0) * 100.0
        print(json.dumps({"layout": lname, "images": n, "e2e_none_ms": summary(e2e["none"]), "e2e_exif_ms": summary(e2e["exif"]),
                          "read_tags_ms": round(tags_ms, 4)}), flush=True)
        if pctx is not None:
            pctx.close()
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
