"""Region-of-interest decode (mj_plan_request.rois) against whole-image decode, on the GPU box.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled), once with DRI = one MCU row (120)
and once without restart markers, each through host segmentation and the GPU marker scan.  Per batch, in one process, one
JSON line per configuration:

    plain     whole images, mj_plan_create (the fused launch where the batch takes it)
    full      full-frame windows (mj_plan_request.rois: stage 0 + stage 1 + the window stage 2)
    c224      centred 224 x 224 windows
    c1024     centred 1024 x 1024 windows
    random    a random window per image (seeded)

with execute_ms (HIP events around `--iters` back-to-back executes), front_ms / main_ms (mj_plan_time_execute), stage1_ms /
stage2_ms (mj_plan_time_stages), the restart segments decoded and the MCUs reconstructed.  Every image of every
configuration is compared with the oracle's whole image, sliced (each distinct file decoded by the oracle once).

    python tools/roi_probe.py [--n 1024] [--distinct 64] [--iters 20] [--only c224] [--kinds dri] [--segments gpu] [--no-check]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

W, H = 1920, 1080
MW = MH = 16            # 4:2:0


def windows(config: str, n: int, rng: np.random.Generator):
    if config == "plain":
        return None
    if config == "full":
        return [(0, 0, W, H)] * n
    if config in ("c224", "c1024"):
        s = 224 if config == "c224" else 1024
        return [((W - s) // 2, (H - s) // 2, s, s)] * n
    out = []
    for _ in range(n):
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return out


def segments_and_mcus(wins, n: int, ri: int):
    """(restart segments decoded, MCUs reconstructed) of a batch of n images with these windows (None = whole images)."""
    mch, mcv = -(-W // MW), -(-H // MH)
    segs_per_image = -(-mch * mcv // ri) if ri else 1
    if wins is None:
        return n * segs_per_image, n * mch * mcv
    seg = mcu = 0
    for (x, y, w, h) in wins:
        mx0, mx1, my0, my1 = x // MW, (x + w - 1) // MW, y // MH, (y + h - 1) // MH
        mcu += (mx1 - mx0 + 1) * (my1 - my0 + 1)
        if not ri:
            seg += 1
            continue
        need = set()
        for r in range(my0, my1 + 1):           # a segment is needed when one of its MCUs lies in the rectangle
            need.update(range((r * mch + mx0) // ri, (r * mch + mx1) // ri + 1))
        seg += len(need)
    return seg, mcu


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--only", default="plain,full,c224,c1024,random")
    ap.add_argument("--kinds", default="dri,nodri")
    ap.add_argument("--segments", default="host,gpu")
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()

    import torch
    from oracle import oracle
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import synth

    dev = torch.device("cuda", 0)
    ctx = B.Context(0)
    st = torch.cuda.Stream(device=dev)            # (a stream of its own: the events below time exactly the executes queued on it)
    stream = st.cuda_stream
    n, nd = args.n, args.distinct
    for kind in args.kinds.split(","):
        ri = 120 if kind == "dri" else 0
        blob, offs = synth.synth_batch(nd, args.seed, W, H, 85, "420", ri)
        raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nd)]
        files = [raws[i % nd] for i in range(n)]
        fulls = None
        if not args.no_check:
            with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
                fulls = list(pool.map(lambda r: oracle.decode(r)["rgb"], raws))
        for segment in args.segments.split(","):
            parsed = [parse_jpeg(f, headers_only=True) for f in files] if segment == "gpu" else None
            prep = prepare_batch(files, B.MJ_LAYOUT_XMAJOR, 0, parsed)
            d_blob = torch.from_numpy(prep.blob).to(dev)
            torch.cuda.synchronize()
            for config in args.only.split(","):
                wins = windows(config, n, np.random.default_rng(args.seed + 7))
                plan = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), {"prep": prep, "n_images": n}, rois=wins)
                try:
                    d_rgb = torch.empty(plan.info.rgb_bytes, dtype=torch.uint8, device=dev)
                    plan.execute(stream, d_rgb.data_ptr())
                    plan.sync()
                    status = plan.read(rgb=False)["status"]
                    bad = []
                    if fulls is not None:
                        host = d_rgb.cpu().numpy()
                        off = 0
                        for i in range(n):
                            x, y, w, h = wins[i] if wins is not None else (0, 0, W, H)
                            got = host[off:off + w * h * 3]
                            off += w * h * 3
                            if not np.array_equal(got, np.ascontiguousarray(fulls[i % nd][x:x + w, y:y + h]).reshape(-1)):
                                bad.append(i)
                    for _ in range(3):
                        plan.execute(stream, d_rgb.data_ptr())
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(args.iters):
                        plan.execute(stream, d_rgb.data_ptr())
                    e1.record(st)
                    torch.cuda.synchronize()
                    plan.sync()
                    exec_ms = e0.elapsed_time(e1) / args.iters
                    front, main_ms = plan.time_execute(args.iters, d_rgb.data_ptr())
                    s1, s2 = plan.time_stages(args.iters, d_rgb.data_ptr())
                    segs, mcus = segments_and_mcus(wins, n, ri)
                    line = {"kind": kind, "segment": segment, "config": config, "images": n, "distinct": nd,
                            "fused": bool(plan.stage1_form() & B.MJ_FORM_FUSED), "stage1_form": int(plan.stage1_form()), "execute_ms": round(exec_ms, 3),
                            "front_ms": round(front, 3), "main_ms": round(main_ms, 3), "stage1_ms": round(s1, 3), "stage2_ms": round(s2, 3),
                            "segments_decoded": segs, "mcus_reconstructed": mcus, "entropy_bytes": int(plan.info.entropy_bytes),
                            "rgb_bytes": int(plan.info.rgb_bytes), "status_ok": not status.any(),
                            "parity": "not checked" if fulls is None else ("bit-exact vs oracle, every image" if not bad else f"MISMATCH {bad[:8]}")}
                    print(json.dumps(line), flush=True)
                    del d_rgb
                finally:
                    plan.close()
            del d_blob
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
