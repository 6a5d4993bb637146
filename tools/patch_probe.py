"""patches= on the GPU box: what packing a batch into a native-resolution encoder's token rows costs as the one launch behind the
plans, beside a plain copy of the bytes it moves and beside what a user does today — the call without it, then per image a slice,
reshape, permute, expand, reshape, and one torch.cat.

`--n` files (tools/synth.synth_batch; `--distinct` distinct seeds tiled, DRI = one MCU row, GPU marker scan), most 1920 x 1080 4:2:0
and every fourth one of 1080 x 1920, 1280 x 960 and 1024 x 1024 in turn.  Every file is resized to
pyjpegdecoder_amd.smart_resize(h, w, max_pixels=256 * 28 * 28) — 588 x 336 for 1080p — and placed top-left on one square canvas,
bfloat16 normalised, bicubic; Qwen2-VL's spec: patch 14, merge 2, repeat 2, packed.  Per layout (row-major and planar row-major).
Medians and spreads (min .. max) of `--reps` / `--e2e-reps` rounds, every round one sample of every variant in turn (interleaved,
so that a drifting clock meets all alike), after one round that warms.

    launch       mj_patchify_time(iters=1): the launch alone on the decoded canvas tensor, beside mj_device_copy_rate's k_copy16 over
                 the bytes the launch reads (the windows) plus writes (the token rows)
    torch        today's route on the same tensor on the GPU, torch.cuda events around it
    call         decode_device, wall clock around a synchronised call: with patches=, without it, and without it followed by the
                 torch route
    equal        whether the torch route gives the library's bits

    python tools/patch_probe.py [--n 1024] [--distinct 64] [--reps 12] [--e2e-reps 7] [--layouts rowmajor,planar_rowmajor]
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

from tools.normalize_probe import LAYOUTS, MEAN, STD, summary  # noqa: E402

P, M, T = 14, 2, 2
OTHERS = ((1080, 1920), (1280, 960), (1024, 1024))             # (width, height) of every fourth file, in turn


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--e2e-reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--layouts", default="rowmajor,planar_rowmajor")
    args = ap.parse_args()

    import torch
    from pyjpegdecoder_amd import BatchDecoder, patch_grids, smart_resize
    from tools import synth

    n, nd = args.n, args.distinct

    def batch_of(count, w, h, seed):
        blob, offs = synth.synth_batch(count, seed, w, h, 85, "420", (w + 15) // 16)
        return [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(count)]
    main_files = batch_of(nd, 1920, 1080, args.seed)
    other_files = [batch_of(max(1, nd // 16), w, h, args.seed + 1 + k) for k, (w, h) in enumerate(OTHERS)]
    files, dims = [], []
    for i in range(n):
        if i % 4 == 3:
            k = (i // 4) % len(OTHERS)
            files.append(other_files[k][(i // 12) % len(other_files[k])])
            dims.append(OTHERS[k])
        else:
            files.append(main_files[i % nd])
            dims.append((1920, 1080))
    hw = [smart_resize(h, w, factor=P * M, max_pixels=256 * 28 * 28) for w, h in dims]
    side = max(max(h, w) for h, w in hw)
    spec = dict(patch=P, merge=M, repeat=T, windows=[(0, 0, w, h) for h, w in hw])
    grids, cu = patch_grids(spec, n, (side, side))
    D = 3 * T * P * P
    common = dict(size=(side, side), resize_to=[(w, h) for h, w in hw], place=[(0, 0)] * n, resample="bicubic", mode="RGB", dtype="bfloat16",
                  normalize=(MEAN, STD))

    for lname in args.layouts.split(","):
        dec = BatchDecoder(device=0, layout=lname)
        ctx = dec.ctx
        x = dec.decode_device(files, **common)
        planar = lname.startswith("planar")
        read = sum(h * w for h, w in hw) * 3 * 2
        written = int(cu[-1]) * D * 2
        line = {"layout": lname, "files": n, "canvas": f"{side} x {side}", "sizes": sorted({f"{w} x {h}" for h, w in hw}), "dtype": "bfloat16 normalised",
                "spec": f"patch {P}, merge {M}, repeat {T}, packed", "tokens": int(cu[-1]), "row_elements": D, "canvas_tensor_bytes": x.numel() * 2, "bytes_read": read,
                "bytes_written": written}

        def torch_route(t):
            rows = []
            for k, (h, w) in enumerate(hw):
                img = t[k, :, :h, :w] if planar else t[k, :h, :w, :].permute(2, 0, 1)
                gh, gw = h // P, w // P
                rows.append(img.reshape(3, gh // M, M, P, gw // M, M, P).permute(1, 4, 2, 5, 0, 3, 6).unsqueeze(5).expand(-1, -1, -1, -1, -1, T, -1, -1)
                            .reshape(gh * gw, D))
            return torch.cat(rows)
        # ---- the launch alone, the copy, today's route
        dst = torch.empty((int(cu[-1]), D), dtype=x.dtype, device=x.device)
        torch.cuda.synchronize()
        geometry = (LAYOUTS[lname], "bfloat16", 3, (side, side), n, spec)
        ms = {"patchify": [], "copy16_same_bytes": [], "torch_route": []}
        copy_ms = ctypes.c_float()
        ctx.lib.mj_device_copy_rate.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(args.reps + 1):
            t = ctx.time_patchify(x.data_ptr(), dst.data_ptr(), *geometry, iters=1)
            if r:
                ms["patchify"].append(t)
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
        line["launch_gbs_read_and_written"] = round((read + written) / med["patchify"] / 1e6, 1)
        line["ratio_to_copy16"] = round(med["patchify"] / med["copy16_same_bytes"], 3)
        line["torch_over_launch"] = round(med["torch_route"] / med["patchify"], 3)
        # ---- whether today's route gives the library's bits
        ctx.patchify(x.data_ptr(), dst.data_ptr(), *geometry)
        torch.cuda.synchronize()
        ref = torch_route(x)
        diff = dst.view(torch.int16) != ref.view(torch.int16)
        line["torch_route_equals_library"] = {"equal": not bool(diff.any().item()), "elements_that_differ": int(diff.sum().item())}
        del ref, diff, dst, x
        # ---- the whole call, and today's route
        routes = {"call_without_patches": lambda: dec.decode_device(files, **common),
                  "call_with_patches": lambda: dec.decode_device(files, patches=spec, **common),
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
