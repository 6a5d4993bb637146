"""Decode to a fixed size (mj_plan_request.out_width / out_height) against the decode without it and against resizing afterwards with torch, on
the GPU box.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan).
Per configuration — whole images to 224 x 224, centred 448 x 448 windows to 224 x 224, whole images to 640 x 360 — and layout, in
one process, one JSON line with HIP-event times per step:

    base_ms     (a) the same plan's execute without the resize: mj_plan_create for whole images (the fused launch where the
                    batch takes it), mj_plan_request.rois for windows
    resized_ms  (b) the resized plan's execute: the same launches plus the resize launch
    resize_ms   (c) the resize launch alone; resize_tbs = (un-resized bytes read + output bytes written) / resize_ms, beside
                    copy_tbs, the rate of a plain 16-bytes-per-lane device copy (mj_device_copy_rate) in the same process
    torch_ms    (d) what a caller does without it: the list decode_device returns, image by image through
                    torch.nn.functional.interpolate(mode="bilinear", antialias=True), rounded to uint8 and stacked

and whether the first `--check` distinct images equal tools/resize_model.py applied to the oracle's pixels.

    python tools/resize_probe.py [--n 1024] [--distinct 64] [--iters 20] [--layouts xmajor,planar_rowmajor] [--check 4]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

W, H = 1920, 1080
CONFIGS = {"whole_224": (None, (224, 224)), "c448_224": (((W - 448) // 2, (H - 448) // 2, 448, 448), (224, 224)),
           "whole_640x360": (None, (640, 360))}
LAYOUTS = {"xmajor": 0, "rowmajor": 1, "planar": 2, "planar_rowmajor": 3}


def timed(st, iters, fn):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="xmajor,planar_rowmajor")
    ap.add_argument("--only", default=",".join(CONFIGS))
    ap.add_argument("--check", type=int, default=4)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from oracle import oracle
    from pyjpegdecoder_amd import BatchDecoder
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    from tools import resize_model, synth

    dev = torch.device("cuda", 0)
    n, nd = args.n, args.distinct
    blob, offs = synth.synth_batch(nd, args.seed, W, H, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nd)]
    files = [raws[i % nd] for i in range(n)]
    fulls = [oracle.decode(r)["rgb"] for r in raws[:args.check]]
    parsed = [parse_jpeg(f, headers_only=True) for f in files]
    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx = dec.ctx
        st = torch.cuda.Stream(device=dev)
        stream = st.cuda_stream
        prep = prepare_batch(files, LAYOUTS[lname], 0, parsed)
        d_blob = torch.from_numpy(prep.blob).to(dev)
        torch.cuda.synchronize()
        for config in args.only.split(","):
            win, size = CONFIGS[config]
            wins = [win] * n if win is not None else None
            base = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), {"prep": prep, "n_images": n}, rois=wins)
            rz = B.Plan(ctx, prep.to_c(d_blob.data_ptr()), {"prep": prep, "n_images": n}, rois=wins, size=size)
            try:
                d_base = torch.empty(base.info.rgb_bytes, dtype=torch.uint8, device=dev)
                d_out = torch.empty(rz.info.rgb_bytes, dtype=torch.uint8, device=dev)
                rz.execute(stream, d_out.data_ptr())
                rz.sync()
                ok = not rz.read(rgb=False)["status"].any()
                host = d_out.cpu().numpy().reshape((n,) + dec._shape(size[0], size[1], 3))
                bad = []
                for i, full in enumerate(fulls):
                    x, y, w, h = win or (0, 0, W, H)
                    want = resize_model.resize(np.ascontiguousarray(full[x:x + w, y:y + h].swapaxes(0, 1)), size)
                    if lname in ("xmajor", "planar"):
                        want = want.swapaxes(0, 1)
                    if lname.startswith("planar"):
                        want = np.moveaxis(want, -1, 0)
                    if not np.array_equal(host[i], want):
                        bad.append(i)
                base_ms = timed(st, args.iters, lambda: base.execute(stream, d_base.data_ptr()))
                base.sync()
                resized_ms = timed(st, args.iters, lambda: rz.execute(stream, d_out.data_ptr()))
                rz.sync()
                resize_ms, src_bytes = rz.time_resize(args.iters, d_out.data_ptr())
                moved = src_bytes + int(rz.info.rgb_bytes)
                copy_tbs = ctx.copy_rate_gbs((moved // 2) & ~15, 5) / 1e3
                # (d) the list a caller gets today, resized image by image and stacked (the decode itself is not in this time)
                imgs = dec.decode_device(files, rois=win, parts=1)
                xm = lname in ("xmajor", "planar")

                def torch_way():
                    out = []
                    for t in imgs:
                        chw = t if lname.startswith("planar") else t.permute(2, 0, 1)
                        if xm:
                            chw = chw.transpose(1, 2)                      # (C, H, W)
                        r = F.interpolate(chw.unsqueeze(0).float(), size=(size[1], size[0]), mode="bilinear", antialias=True)
                        out.append(r.round_().clamp_(0, 255).to(torch.uint8))
                    return torch.cat(out)
                with torch.cuda.stream(st):
                    torch_ms = timed(st, max(2, args.iters // 5), torch_way)
                del imgs
                line = {"layout": lname, "config": config, "images": n, "distinct": nd, "size": list(size),
                        "base_fused": bool(base.stage1_form() & B.MJ_FORM_FUSED), "resized_fused": bool(rz.stage1_form() & B.MJ_FORM_FUSED),
                        "base_ms": round(base_ms, 3), "resized_ms": round(resized_ms, 3), "extra_ms": round(resized_ms - base_ms, 3),
                        "resize_ms": round(resize_ms, 3), "source_bytes": int(src_bytes), "output_bytes": int(rz.info.rgb_bytes),
                        "resize_tbs": round(moved / (resize_ms * 1e-3) / 1e12, 3), "copy_tbs": round(copy_tbs, 3),
                        "copy_of_same_bytes_ms": round(moved / (copy_tbs * 1e12) * 1e3, 3), "torch_ms": round(torch_ms, 3),
                        "base_plus_torch_ms": round(base_ms + torch_ms, 3), "status_ok": ok,
                        "parity": f"first {len(fulls)} distinct images equal model(oracle)" if not bad else f"MISMATCH {bad}"}
                print(json.dumps(line), flush=True)
                del d_base, d_out
            finally:
                base.close()
                rz.close()
        del d_blob
        dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
