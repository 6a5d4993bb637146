"""One-off stress run on the GPU box for the per-file arguments on every route of the public API: seeded rounds, each a random
list of three-component files of the kinds tests/test_request_routes.py mixes (ordinary ones at random sizes, samplings and
restart intervals; files without restart markers; progressive and odd-layout files the native front end declines; tail files
with a COM segment behind the scan, at random positions), random windows, size, dtype, normalize constants and mirror flags,
a random pixel layout and a random route — decode, decode_device in one call (native or Python front end) or in three parts,
decode_device_iter at depth 1-3, host segmentation.  In half of the rounds the synchronisation form is kept from settling, so
that files go round again under MJ_FLAG_NO_SYNC.  Every output is compared with tests/routes_common.expected (oracle, resize
model, normalize model; floats as bit patterns).  Not part of the test suite:
    python tools/stress_routes.py [n_rounds] [seed]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from tools import synth
from oracle import oracle
from pyjpegdecoder_amd import BatchDecoder, _binding as B
from routes_common import GOLDEN, bits_of, expected, with_com

n_rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 40
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed)
LAYOUTS = ("xmajor", "rowmajor", "planar", "planar_rowmajor")
ROUTES = ("decode", "device_native", "device_python", "device_parts3", "iter1", "iter2", "iter3", "host_decode", "host_device")
UNSETTLED = (("MJ_HUFFMAN", "sync"), ("MJ_SYNC_WARM", "0"), ("MJ_SYNC_CHUNK", "256"), ("MJ_SYNC_ROUNDS", "0"))
odd_npz = np.load(GOLDEN / "odd_layouts.npz")
declined = [f.read_bytes() for f in sorted((GOLDEN / "files").glob("prog_*.jpg")) if "grey" not in f.name]
declined += [odd_npz[k].tobytes() for k in sorted(odd_npz.files) if k.endswith(".jpg")]
declined = [r for r in declined if oracle.decode(r)["rgb"].ndim == 3]


def draw_file():
    kind = rng.choice(["ordinary", "ordinary", "nodri", "tail", "declined"])
    if kind == "declined":
        return declined[int(rng.integers(0, len(declined)))]
    w, h = int(rng.integers(8, 300)), int(rng.integers(8, 300))
    ss = ("420", "444", "422", "440", "411")[int(rng.integers(0, 5))]
    ri = 0 if kind == "nodri" else int(rng.choice([0, 1, 2, 3, 7, 16, 50]))
    raw = synth.synth_jpeg(int(rng.integers(0, 1 << 30)), w, h, int(rng.choice([50, 75, 85, 95])), ss, ri, float(rng.choice([0.0, 5.0, 25.0])))
    return with_com(raw) if kind == "tail" else raw


def draw_window(w, h):
    ww, wh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
    return (int(rng.integers(0, w - ww + 1)), int(rng.integers(0, h - wh + 1)), ww, wh)


total = 0
t0 = time.time()
for rnd in range(n_rounds):
    files = [draw_file() for _ in range(int(rng.integers(3, 15)))]
    fulls = [oracle.decode(r)["rgb"] for r in files]
    route, layout = ROUTES[int(rng.integers(0, len(ROUTES)))], LAYOUTS[int(rng.integers(0, 4))]
    unsettled = bool(rng.integers(0, 2)) and not route.startswith("host")
    wins = [draw_window(f.shape[0], f.shape[1]) if rng.integers(0, 4) else None for f in fulls] if rng.integers(0, 2) else None
    if route.startswith("iter"):
        wins = None
    size = (int(rng.integers(1, 120)), int(rng.integers(1, 120))) if rng.integers(0, 3) else None
    dtype = normalize = flags = None
    if size is not None and rng.integers(0, 3):
        dtype = ("float16", "float32", "bfloat16", "uint8")[int(rng.integers(0, 4))]
        if dtype == "bfloat16" and route in ("decode", "host_decode"):
            dtype = "float16"
        if dtype != "uint8" and rng.integers(0, 2):
            normalize = (tuple(float(v) for v in rng.uniform(-0.5, 1.0, 3)), tuple(float(v) for v in rng.uniform(0.05, 2.0, 3)))
        flags = [bool(rng.integers(0, 2)) for _ in files]
    kw = {k: v for k, v in (("rois", wins), ("size", size), ("dtype", dtype), ("normalize", normalize), ("mirror", flags)) if v is not None}
    for name, value in UNSETTLED:
        B.set_option(name, value if unsettled else None)
    dec = BatchDecoder(0, layout=layout, segment="host" if route.startswith("host") else "gpu", gpu_segment_min_files=1,
                       native_host=route != "device_python")
    try:
        if route in ("decode", "host_decode"):
            got = dec.decode(files, **kw)
        elif route.startswith("iter"):
            cut = sorted(int(c) for c in rng.integers(0, len(files) + 1, 2))
            cut = [0] + cut + [len(files)]
            if flags is not None:
                kw["mirror"] = [flags[cut[k]:cut[k + 1]] for k in range(3)]
            outs = list(dec.decode_device_iter([files[cut[k]:cut[k + 1]] for k in range(3)], depth=int(route[-1]), **kw))
            got = [img for part in outs for img in part]
        else:
            got = dec.decode_device(files, parts=3 if route == "device_parts3" else 1, **kw)
        bad = 0 if len(got) == len(files) else 1
        for i, full in enumerate(fulls):
            want = expected(full, wins[i] if wins else None, size, dtype, normalize, bool(flags[i]) if flags else False, layout)
            have = bits_of(got[i])
            if have.shape != want.shape or have.dtype != want.dtype or not np.array_equal(have, want):
                bad += 1
                if bad < 4:
                    print("   MISMATCH round", rnd, "file", i, have.shape, want.shape)
    finally:
        dec.close()
    torch.cuda.synchronize()
    total += bad
    print("round %3d %-14s %-15s unsettled=%d files=%2d %s: %s" % (rnd, route, layout, unsettled, len(files),
          " ".join(f"{k}={'yes' if k in ('rois', 'mirror', 'normalize') else v}" for k, v in kw.items()), "ok" if not bad else "%d MISMATCHES" % bad))
for name, _ in UNSETTLED:
    B.set_option(name, None)
print("%d rounds in %.1f s" % (n_rounds, time.time() - t0))
print("TOTAL MISMATCHES", total)
sys.exit(1 if total else 0)
