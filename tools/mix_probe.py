"""mix= on the GPU box: what MixUp / CutMix cost as the one launch behind the plans, beside a plain copy of the bytes it moves and
beside what a user does today — the call without it, then torch's roll / mul / add (MixUp) or roll and slice assignments (CutMix).

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan) ->
224 x 224, float16 normalised, per layout (row-major and planar row-major).  MixUp: the batch form, partner (k - 1) % N, one lam
(a Beta(0.8, 0.8) draw, fixed seed).  CutMix: the same partners, one pyjpegdecoder_amd.cutmix_box box per output (lam from
Beta(1, 1), fixed seed).  Medians and spreads (min .. max) of `--reps` / `--e2e-reps` rounds, every round one sample of every variant
in turn (interleaved, so that a drifting clock meets all alike), after one round that warms.

    launch       mj_mix_time(iters=1): the mix launch alone on the decoded tensor, MixUp and CutMix, beside mj_device_copy_rate's
                 k_copy16 over the bytes the launch reads plus writes — three tensor passes for MixUp; two, plus the boxes' bytes
                 once more, for CutMix
    torch        torch's own expression on the same tensor on the GPU, torch.cuda events around it: x.roll(1, 0).mul(1 - lam).add_(
                 x.mul(lam)); out = x.clone() and one slice assignment per output from x.roll(1, 0)
    call         decode_device, wall clock around a synchronised call: without mix=, with it, and without it followed by the torch
                 expression
    equal        whether torch's GPU expression gives the library's bits (the model, pinned to torch's CPU ops, is the authority)

    python tools/mix_probe.py [--n 1024] [--distinct 64] [--reps 12] [--e2e-reps 7] [--layouts rowmajor,planar_rowmajor]
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

from tools.normalize_probe import LAYOUTS, MEAN, STD, H, W, summary  # noqa: E402

SIZE = (224, 224)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--e2e-reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,planar_rowmajor")
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyjpegdecoder_amd import BatchDecoder, cutmix_box
    from tools import synth

    dev = torch.device("cuda", 0)
    n, nd = args.n, args.distinct
    blob, offs = synth.synth_batch(nd, args.seed, W, H, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nd)]
    files = [raws[i % nd] for i in range(n)]
    rng = np.random.default_rng(args.seed)
    lam = float(rng.beta(0.8, 0.8))
    g = torch.Generator().manual_seed(args.seed)
    boxes = []
    while len(boxes) < n:
        box, _ = cutmix_box(SIZE, float(rng.beta(1.0, 1.0)), generator=g)
        if box is not None:
            boxes.append(box)
    mixup = [("mixup", (k - 1) % n, lam) for k in range(n)]
    cutmix = [("cutmix", (k - 1) % n, boxes[k]) for k in range(n)]
    box_bytes = sum(3 * b[2] * b[3] for b in boxes) * 2
    common = dict(size=SIZE, dtype="float16", normalize=(MEAN, STD))

    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx = dec.ctx
        x = dec.decode_device(files, **common)
        tensor_bytes = x.numel() * 2
        line = {"layout": lname, "files": n, "size": "224 x 224", "dtype": "float16 normalised", "lam": round(lam, 6), "tensor_bytes": tensor_bytes,
                "cutmix_box_bytes": box_bytes, "box_share_of_tensor": round(box_bytes / tensor_bytes, 4)}
        planar = lname.startswith("planar")

        def torch_mixup(t):
            return t.roll(1, 0).mul(1.0 - lam).add_(t.mul(lam))

        def torch_cutmix(t):
            out, rolled = t.clone(), t.roll(1, 0)
            for k, (bx, by, bw, bh) in enumerate(boxes):
                if planar:
                    out[k, :, by:by + bh, bx:bx + bw] = rolled[k, :, by:by + bh, bx:bx + bw]
                else:
                    out[k, by:by + bh, bx:bx + bw, :] = rolled[k, by:by + bh, bx:bx + bw, :]
            return out
        # ---- the launch alone, the copy, torch's expression
        dst = torch.empty_like(x)
        torch.cuda.synchronize()
        geometry = (LAYOUTS[lname], "float16", 3, SIZE[0], SIZE[1])
        moved = {"mixup": 3 * tensor_bytes, "cutmix": 2 * tensor_bytes + box_bytes}
        ms = {"mixup": [], "cutmix": [], "copy16_mixup_bytes": [], "copy16_cutmix_bytes": [], "torch_mixup": [], "torch_cutmix": []}
        copy_ms = ctypes.c_float()
        ctx.lib.mj_device_copy_rate.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(args.reps + 1):
            for name, entries in (("mixup", mixup), ("cutmix", cutmix)):
                t = ctx.time_mix(x.data_ptr(), dst.data_ptr(), *geometry, entries, iters=1)
                if r:
                    ms[name].append(t)
                # (k_copy16 reads and writes what it is given: half the bytes the launch moves, rounded to 16)
                ctx.check(ctx.lib.mj_device_copy_rate(ctx.handle, (moved[name] // 2) & ~15, 1, ctypes.byref(copy_ms)))
                if r:
                    ms[f"copy16_{name}_bytes"].append(copy_ms.value)
            for name, fn in (("torch_mixup", torch_mixup), ("torch_cutmix", torch_cutmix)):
                torch.cuda.synchronize()
                a.record()
                res = fn(x)
                b.record()
                b.synchronize()
                if r:
                    ms[name].append(a.elapsed_time(b))
                del res
        line["launch_ms"] = {name: summary(xs) for name, xs in ms.items()}
        med = {name: line["launch_ms"][name]["median"] for name in ms}
        line["launch_gbs_read_and_written"] = {name: round(moved[name] / med[name] / 1e6, 1) for name in ("mixup", "cutmix")}
        line["ratio_to_copy16"] = {name: round(med[name] / med[f"copy16_{name}_bytes"], 3) for name in ("mixup", "cutmix")}
        line["torch_over_launch"] = {name: round(med[f"torch_{name}"] / med[name], 3) for name in ("mixup", "cutmix")}
        # ---- whether torch's GPU expression gives the library's bits
        same = {}
        for name, entries, fn in (("mixup", mixup, torch_mixup), ("cutmix", cutmix, torch_cutmix)):
            ctx.mix(x.data_ptr(), dst.data_ptr(), *geometry, entries)
            torch.cuda.synchronize()
            ref = fn(x)
            diff = dst.view(torch.int16) != ref.view(torch.int16)
            same[name] = {"equal": not bool(diff.any().item()), "elements_that_differ": int(diff.sum().item())}
            del ref, diff
        line["torch_gpu_expression_equals_library"] = same
        del dst, x
        # ---- the whole call, and today's route
        routes = {"call_without_mix": lambda: dec.decode_device(files, **common),
                  "call_with_mixup": lambda: dec.decode_device(files, mix=mixup, **common),
                  "call_with_cutmix": lambda: dec.decode_device(files, mix=cutmix, **common),
                  "call_then_torch_mixup": lambda: torch_mixup(dec.decode_device(files, **common)),
                  "call_then_torch_cutmix": lambda: torch_cutmix(dec.decode_device(files, **common))}
        t = {name: [] for name in routes}
        for r in range(args.e2e_reps + 1):
            for name, call in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = call()
                torch.cuda.synchronize()
                if r:
                    t[name].append((time.perf_counter() - t0) * 1e3)
                del res
        line["e2e_ms"] = {name: summary(xs) for name, xs in t.items()}
        print(json.dumps(line), flush=True)
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
