"""Model-ready output (mj_plan_request.output: float16, normalised, mixed mirror flags out of the resize launch) against the
plain uint8 resize launch and against what a caller does without it — the uint8 launch followed by the torch chain
`.to(float32).div(255).sub(mean).div(std).to(float16)` and a `torch.where(flags, x.flip(width), x)` — on the GPU box.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan) to
224 x 224, per layout.  One process; every plan executed once first (the resize launch reads what stage 2 left), then `--reps`
rounds, every round one sample of every point in turn (interleaved, so that a drifting clock meets all points alike); per point
the median and the spread (min .. max) over the rounds.  A sample of a resize launch is mj_plan_time_resize(iters=1): one warm
launch, then one between two HIP events.

    u8_ms          the plain resized plan's launch (mj_plan_request.out_width / out_height), this build
    u8_parent_ms   the same from another build of the library (`--parent-lib path/to/libmijpeg.so`, e.g. the parent commit's),
                   loaded into the same process: the same instances, so the two should agree within their spreads
    u8_twin_ms, u8_parent_twin_ms   a second plan of each build — the same code on other buffers: how far two plans of ONE build
                   lie apart is what a difference between the builds has to exceed before it says anything about the code
    fused_ms   (a) ONE launch: float16 + normalize + mixed mirror flags
    chain_ms       the torch chain alone on the uint8 tensor (torch events around all its launches)
    u8_plus_chain_ms (b) u8_ms + chain_ms of the same round: what users do today (the two are timed apart — the resize launch
                   runs on the context's stream — so the gap between them is NOT in (b): it is a lower bound of today's cost)
    copy_extra_ms  what a plain 16-bytes-per-lane copy (mj_device_copy_rate) takes for the bytes (a) writes beyond the uint8 output
    e2e_*          BatchDecoder.decode_device from file bytes in host memory to the tensor, wall clock with a device
                   synchronize, uint8 and model-ready, `--e2e-reps` rounds, interleaved

and whether (a)'s tensor equals the chain's bit for bit (the chain on the CPU, for the first images; and which share of the elements
differs from the chain run on the GPU, whose division by the scalar 255 is a multiplication by the reciprocal).

    python tools/normalize_probe.py [--n 1024] [--distinct 64] [--reps 24] [--layouts planar_rowmajor,xmajor] [--parent-lib PATH]
"""
from __future__ import annotations

import argparse
import ctypes
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
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def other_build(B, path: str, device: int = 0):
    """A Context on another build of the library in this process (its C ABI up to the symbols it has is this binding's)."""
    L, P = B.load_library(), ctypes.CDLL(path)
    for name in B.EXPORTS:
        try:
            f = getattr(P, name)
        except AttributeError:
            continue
        g = getattr(L, name)
        f.argtypes, f.restype = g.argtypes, g.restype
    ctx = B.Context.__new__(B.Context)
    ctx.lib, ctx.device, ctx.handle = P, device, ctypes.c_void_p()
    if P.mj_create(device, ctypes.byref(ctx.handle)) != B.MJ_OK:
        raise RuntimeError(f"mj_create failed in {path}")
    return ctx


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "samples": len(xs)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--e2e-reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="planar_rowmajor,xmajor")
    ap.add_argument("--parent-lib", default=None)
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
    flags = [((i * 2654435761) >> 9) & 1 == 1 for i in range(n)]
    parsed = [parse_jpeg(f, headers_only=True) for f in files]
    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx = dec.ctx
        pctx = other_build(B, args.parent_lib) if args.parent_lib else None
        prep = prepare_batch(files, LAYOUTS[lname], 0, parsed)
        d_blob = torch.from_numpy(prep.blob).to(dev)
        torch.cuda.synchronize()
        keep = {"prep": prep, "n_images": n}
        plans = {"u8": B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE),
                 "fused": B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE, output=("float16", MEAN, STD, flags))}
        if pctx is not None:
            plans["u8_parent"] = B.Plan(pctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE)
        # the control for the comparison of the two builds: a second plan of each, i.e. the same code on other buffers (every
        # plan has its own 6.4 GB of un-resized pixels; where they lie in HBM is not the same from plan to plan)
        plans["u8_twin"] = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE)
        if pctx is not None:
            plans["u8_parent_twin"] = B.Plan(pctx, prep.to_c(d_blob.data_ptr()), keep, size=SIZE)
        try:
            shape = (n,) + dec._shape(SIZE[0], SIZE[1], 3)
            out = {"u8": torch.empty(shape, dtype=torch.uint8, device=dev), "fused": torch.empty(shape, dtype=torch.float16, device=dev)}
            for name in ("u8_parent", "u8_twin", "u8_parent_twin"):
                out[name] = torch.empty(shape, dtype=torch.uint8, device=dev)
            ok = True
            for name, plan in plans.items():
                assert plan.info.rgb_bytes == out[name].numel() * out[name].element_size()
                plan.execute(0, out[name].data_ptr())
                plan.sync()
                ok = ok and not plan.read(rgb=False)["status"].any()
            torch.cuda.synchronize()
            planar = lname.startswith("planar")
            cshape = (1, 3, 1, 1) if planar else (1, 1, 1, 3)
            wdim = {"xmajor": 1, "rowmajor": 2, "planar": 2, "planar_rowmajor": 3}[lname]
            mean = torch.tensor(MEAN, dtype=torch.float32, device=dev).view(cshape)
            std = torch.tensor(STD, dtype=torch.float32, device=dev).view(cshape)
            d_flags = torch.tensor(flags, device=dev).view(n, 1, 1, 1)

            def chain(u8):
                x = u8.to(torch.float32).div(255).sub(mean).div(std).to(torch.float16)
                return torch.where(d_flags, x.flip(wdim), x)
            # (a) against the chain: on the CPU — torch's reference arithmetic, every division correctly rounded — for the first
            # images bit for bit; against the GPU chain the share of elements that differ (torch's GPU kernels divide by the
            # scalar 255 as a multiplication by its reciprocal, which is not the same float32 function)
            k = min(n, 16)
            cpu = out["u8"][:k].cpu().to(torch.float32).div(255).sub(mean.cpu()).div(std.cpu()).to(torch.float16)
            cpu = torch.where(d_flags[:k].cpu(), cpu.flip(wdim), cpu)
            same = bool(torch.equal(cpu, out["fused"][:k].cpu()))
            gpu_chain = chain(out["u8"])
            differ = float((gpu_chain.view(torch.int16) != out["fused"].view(torch.int16)).float().mean())
            del gpu_chain
            same_u8 = bool(torch.equal(out["u8"], out["u8_parent"])) if pctx is not None else None
            for _ in range(3):
                chain(out["u8"])
            torch.cuda.synchronize()
            samples = {k: [] for k in list(plans) + ["chain", "u8_plus_chain"]}
            for _ in range(args.reps):
                for name, plan in plans.items():
                    samples[name].append(plan.time_resize(1, out[name].data_ptr())[0])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                chain(out["u8"])
                e1.record()
                torch.cuda.synchronize()
                samples["chain"].append(e0.elapsed_time(e1))
                samples["u8_plus_chain"].append(samples["u8"][-1] + samples["chain"][-1])
            src_bytes = plans["u8"].time_resize(1, out["u8"].data_ptr())[1]
            extra = int(plans["fused"].info.rgb_bytes - plans["u8"].info.rgb_bytes)
            copy_tbs = ctx.copy_rate_gbs(1 << 30, 5) / 1e3
            line = {"layout": lname, "images": n, "distinct": nd, "size": list(SIZE), "source_bytes": int(src_bytes),
                    "u8_output_bytes": int(plans["u8"].info.rgb_bytes), "fused_output_bytes": int(plans["fused"].info.rgb_bytes),
                    "u8_ms": summary(samples["u8"]), "u8_parent_ms": summary(samples["u8_parent"]) if pctx is not None else None,
                    "u8_twin_ms": summary(samples["u8_twin"]),
                    "u8_parent_twin_ms": summary(samples["u8_parent_twin"]) if pctx is not None else None,
                    "fused_ms": summary(samples["fused"]), "chain_ms": summary(samples["chain"]),
                    "u8_plus_chain_ms": summary(samples["u8_plus_chain"]), "copy_tbs": round(copy_tbs, 3),
                    "copy_extra_ms": round(2 * extra / (copy_tbs * 1e12) * 1e3, 4),
                    "fused_minus_u8_ms": round(statistics.median(samples["fused"]) - statistics.median(samples["u8"]), 4),
                    "fused_le_u8_plus_chain": statistics.median(samples["fused"]) <= statistics.median(samples["u8_plus_chain"]),
                    "status_ok": ok, "fused_equals_cpu_chain_bit_for_bit_first_16": same,
                    "share_of_elements_differing_from_gpu_chain": round(differ, 6), "parent_u8_equals_branch_u8": same_u8}
            print(json.dumps(line), flush=True)
        finally:
            for plan in plans.values():
                plan.close()
        del out, d_blob
        # end to end: file bytes in host memory -> tensor
        e2e = {"u8": [], "model_ready": []}
        for r in range(args.e2e_reps + 1):
            for name in e2e:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "u8":
                    t = dec.decode_device(files, size=SIZE)
                else:
                    t = dec.decode_device(files, size=SIZE, dtype="float16", normalize=(MEAN, STD), mirror=flags)
                torch.cuda.synchronize()
                if r:                                      # (round 0 warms both)
                    e2e[name].append((time.perf_counter() - t0) * 1e3)
                del t
        print(json.dumps({"layout": lname, "images": n, "e2e_u8_ms": summary(e2e["u8"]), "e2e_model_ready_ms": summary(e2e["model_ready"])}),
              flush=True)
        if pctx is not None:
            pctx.close()
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
