"""compose= on the GPU box: what a YOLO-style mosaic costs as the one launch behind the plans, beside a plain copy of the bytes it
moves and beside what a user does today — the call without it, then torch.full-style canvases and one slice assignment per tile.

1024 x 1920x1080 4:2:0 files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan) ->
tiles of size=(320, 320), every image resized to its long-side-320 size (320 x 180) and placed top-left, float16 normalised, per
layout (row-major and planar row-major).  256 mosaics of 640 x 640 of four tiles each, pyjpegdecoder_amd.mosaic_tiles with centres
drawn uniformly in 160 .. 480 (Ultralytics' range; fixed seed), fill 114.  Medians and spreads (min .. max) of `--reps` / `--e2e-reps`
rounds, every round one sample of every variant in turn (interleaved, so that a drifting clock meets all alike), after one round
that warms.

    launch       mj_compose_time(iters=1): the compose launch alone on the decoded tile tensor, beside mj_device_copy_rate's k_copy16
                 over the bytes the launch reads (the pasted rectangles) plus writes (the canvases)
    torch        today's route on the same tile tensor on the GPU, torch.cuda events around it: canvases of the fill elements, then
                 one slice assignment per tile, 1024 of them
    call         decode_device, wall clock around a synchronised call: with compose=, without it, and without it followed by the
                 torch route
    equal        whether the torch route gives the library's bits

    python tools/compose_probe.py [--n 1024] [--distinct 64] [--reps 12] [--e2e-reps 7] [--layouts rowmajor,planar_rowmajor]
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

TILE, CANVAS, FILL = (320, 320), (640, 640), (114, 114, 114)


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
    from pyjpegdecoder_amd import BatchDecoder, mosaic_tiles
    from pyjpegdecoder_amd import _binding as B
    from tools import synth

    n, nd = args.n, args.distinct
    blob, offs = synth.synth_batch(nd, args.seed, W, H, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nd)]
    files = [raws[i % nd] for i in range(n)]
    rng = np.random.default_rng(args.seed)
    long_side = max(W, H)
    fitted = (round(W * TILE[0] / long_side), round(H * TILE[0] / long_side))      # the caller's arithmetic: 320 x 180
    outputs = []
    for m in range(n // 4):
        centre = (int(rng.integers(CANVAS[0] // 4, 3 * CANVAS[0] // 4 + 1)), int(rng.integers(CANVAS[1] // 4, 3 * CANVAS[1] // 4 + 1)))
        outputs.append([(4 * m + i, at, win) for i, at, win in mosaic_tiles(CANVAS, centre, [fitted] * 4)])
    n_tiles = sum(len(o) for o in outputs)
    compose = dict(size=CANVAS, fill=FILL, outputs=outputs)
    common = dict(size=TILE, resize_to=[fitted] * n, place=[(0, 0)] * n, dtype="float16", normalize=(MEAN, STD))

    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx = dec.ctx
        x = dec.decode_device(files, **common)
        planar = lname.startswith("planar")
        rects, _ = B.host_compose_resolve(LAYOUTS[lname], 3, TILE, n, CANVAS, outputs)
        read = int(sum(int(r["width"]) * int(r["height"]) for r in rects if r["source"] >= 0)) * 3 * 2
        written = len(outputs) * CANVAS[0] * CANVAS[1] * 3 * 2
        bits = [int(B.normalize_table("float16", MEAN[c], STD[c])[FILL[c]]) for c in range(3)]
        fill_vec = torch.tensor(np.array(bits, dtype=np.uint16).view(np.float16), device=x.device)
        shape = (len(outputs), 3, CANVAS[1], CANVAS[0]) if planar else (len(outputs), CANVAS[1], CANVAS[0], 3)
        line = {"layout": lname, "files": n, "tiles": "320 x 320 canvases, images 320 x 180 top-left", "dtype": "float16 normalised", "mosaics": len(outputs),
                "canvas": "640 x 640", "tiles_pasted": n_tiles, "rectangles": int(len(rects)), "tile_tensor_bytes": x.numel() * 2, "bytes_read": read,
                "bytes_written": written}

        def torch_route(t):
            out = (fill_vec.view(1, 3, 1, 1) if planar else fill_vec.view(1, 1, 1, 3)).expand(shape).contiguous()
            for m, tiles in enumerate(outputs):
                for s, (dx, dy), (sx, sy, w, h) in tiles:       # (mosaic_tiles' tiles lie inside the canvas: no clipping needed)
                    if planar:
                        out[m, :, dy:dy + h, dx:dx + w] = t[s, :, sy:sy + h, sx:sx + w]
                    else:
                        out[m, dy:dy + h, dx:dx + w, :] = t[s, sy:sy + h, sx:sx + w, :]
            return out
        # ---- the launch alone, the copy, today's route
        dst = torch.empty(shape, dtype=x.dtype, device=x.device)
        torch.cuda.synchronize()
        geometry = (LAYOUTS[lname], "float16", 3, TILE, n, CANVAS, bits, outputs)
        ms = {"compose": [], "copy16_same_bytes": [], "torch_route": []}
        copy_ms = ctypes.c_float()
        ctx.lib.mj_device_copy_rate.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(args.reps + 1):
            t = ctx.time_compose(x.data_ptr(), dst.data_ptr(), *geometry, iters=1)
            if r:
                ms["compose"].append(t)
            # (k_copy16 reads and writes what it is given: half the bytes the launch moves, rounded to 16)
            ctx.check(ctx.lib.mj_device_copy_rate(ctx.handle, ((read + written) // 2) & ~15, 1, ctypes.byref(copy_ms)))
            if r:
                ms["copy16_same_bytes"].append(copy_ms.value)
            torch.cuda.synchronize()
            a.record()
            res = torch_route(x)
            b.record()
            b.synchronize()
            if r:
                ms["torch_route"].append(a.elapsed_time(b))
            del res
        line["launch_ms"] = {name: summary(xs) for name, xs in ms.items()}
        med = {name: line["launch_ms"][name]["median"] for name in ms}
        line["launch_gbs_read_and_written"] = round((read + written) / med["compose"] / 1e6, 1)
        line["ratio_to_copy16"] = round(med["compose"] / med["copy16_same_bytes"], 3)
        line["torch_over_launch"] = round(med["torch_route"] / med["compose"], 3)
        # ---- whether today's route gives the library's bits
        ctx.compose(x.data_ptr(), dst.data_ptr(), *geometry)
        torch.cuda.synchronize()
        ref = torch_route(x)
        diff = dst.view(torch.int16) != ref.view(torch.int16)
        line["torch_route_equals_library"] = {"equal": not bool(diff.any().item()), "elements_that_differ": int(diff.sum().item())}
        del ref, diff, dst, x
        # ---- the whole call, and today's route
        routes = {"call_without_compose": lambda: dec.decode_device(files, **common),
                  "call_with_compose": lambda: dec.decode_device(files, compose=compose, **common),
                  "call_then_torch_route": lambda: torch_route(dec.decode_device(files, **common))}
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
