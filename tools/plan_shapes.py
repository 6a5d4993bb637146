"""What plan creation decides for a fixed matrix of small batches, and what it asks of the context's buffer cache: the record
tests/golden/plan_shapes.json holds and tests/test_plan_shapes.py holds mj_plan_create to.  Another form, another table width or
another order of buffer requests decodes the same pixels (the last one into another timing class, api.hip: mj_plan_tune_placement),
so no pixel test notices; this record does.

Every row is one plan on a context of its own: mj_debug_plan_shape's values (Plan.shape, include/mijpeg.h has their order), the
number of requests the plan made to the cache and the running hash of their sizes (mj_debug_cache_stats).  The batches are golden
files, tools/synth.py and tools/craft_jpeg.py files of at most 256 x 256, at most 64 to a batch; the forms a small batch does not
reach by itself are forced through the library's options.  Plan creation needs a context, so this runs on the GPU box:

    python tools/plan_shapes.py [--lib PATH] [--write]     the record of the build in the tree, or of another build (`--lib`, e.g.
                                                           the parent commit's libmijpeg.so); --write: into the golden
    python tools/plan_shapes.py --leaks [--lib PATH]       blocks still handed out behind mj_plan_destroy for four rows
    python tools/plan_shapes.py --time [--lib PATH]        creates and destroys bench.py's batch (1024 x 1080p, 256 distinct) 20
                                                           times on one context: median and spread of the host time, ms
"""
from __future__ import annotations

import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = ROOT / "tests" / "golden"
RECORD = GOLDEN / "plan_shapes.json"
KEEP_PLANES, KEEP_IDCT, GPU_SEGMENT = 2, 4, 32
COLOUR = ("64x64_420_pil", "128x64_420_dri3", "100x36_420_dri7", "48x32_420_flat")
# the kinds of plan the record must hold at least one of each (kinds_of)
KINDS = ("wave", "lanes11", "lanes_resolved", "wg_tables", "sync_classic", "sync_resolved", "by_length", "fused_images",
         "fused_by_length", "generic", "grey", "rowmajor", "planar", "window_host_drops", "window_gpu_gather", "gpu_wave_padded_copy",
         "progressive_banded_fast", "keep_planes_idct")


def matrix():
    """The rows: name -> what the batch is made of (files), layout, flags, options, and how it reaches the library (blob: host |
    device | short = a device blob no longer than MJ_FLAG_GPU_SEGMENT asks for | odd = a device blob at a 2-byte offset, which plan
    creation refuses late; gpu: headers-only parse, the GPU finds the markers; rois: a window plan)."""
    def row(name, files, layout=0, flags=0, opts=(), blob="host", gpu=False, rois=None):
        return {"name": name, "files": list(files), "layout": layout, "flags": flags, "opts": [list(o) for o in opts], "blob": blob,
                "gpu": gpu, "rois": rois}
    gold = [("golden", n) for n in COLOUR]
    uniform = [("synth", 5100 + i % 3, 96, 64, 85, "420", 6, 12.0) for i in range(12)]         # one restart interval per MCU row
    mixed = [("synth", 5200 + i % 4, 96, 64, (50, 95)[i % 2], "444", 12, (0.0, 60.0)[i % 2]) for i in range(16)]
    own_tables = [("craft_wide", 40, 24, 7 + i, 3) for i in range(8)]           # every file its own AC table: ten tables in the batch
    long_segs = [("synth", 5300 + i, 256, 256, 100, "444", 0, 70.0) for i in range(2)]
    prog = [("golden", n) for n in ("prog_64x64_420_pil", "prog_128x64_420_rst_pil", "prog_48x32_420_flat_pil")]
    win = [(8, 8, 24, 16)] * 2
    return [
        row("wave", gold),
        row("lanes11", gold, opts=[("MJ_HUFFMAN", "lanes11")]),
        row("lanes_resolved_by_length", gold, opts=[("MJ_HUFFMAN", "lanes"), ("MJ_SEG_ORDER", "striped")]),
        row("lanes_resolved_binned", gold, opts=[("MJ_HUFFMAN", "lanes"), ("MJ_SEG_ORDER", "binned")]),
        row("lanes_resolved_blob", gold, opts=[("MJ_HUFFMAN", "lanes"), ("MJ_SEG_ORDER", "blob")]),
        row("lanes_as_chosen", gold, opts=[("MJ_HUFFMAN", "lanes")]),
        row("wg_tables_lanes", own_tables, opts=[("MJ_HUFFMAN", "lanes")]),
        row("wg_tables_sync", own_tables, opts=[("MJ_HUFFMAN", "sync")]),
        row("wg_tables_wave", own_tables),
        row("sync_classic", gold, opts=[("MJ_HUFFMAN", "sync"), ("MJ_SYNC_COUNT", "classic")]),
        row("sync_resolved", gold, opts=[("MJ_HUFFMAN", "sync")]),
        row("sync_resolved_chunk256_bits10", gold, opts=[("MJ_HUFFMAN", "sync"), ("MJ_SYNC_CHUNK", "256"), ("MJ_SYNC_BITS", "10")]),
        row("sync_as_chosen_long_segments", long_segs),
        row("sync_gpu_segment_one_each", long_segs, gpu=True, blob="device"),
        row("fused_images", uniform, opts=[("MJ_HUFFMAN", "lanes"), ("MJ_SEG_ORDER", "blob")], blob="device"),
        row("fused_images_consumers3", uniform, opts=[("MJ_HUFFMAN", "lanes"), ("MJ_SEG_ORDER", "blob"), ("MJ_FUSED_CONSUMERS", "3")]),
        row("fused_images_rowmajor", uniform, layout=1, opts=[("MJ_HUFFMAN", "lanes"), ("MJ_SEG_ORDER", "blob")], blob="device"),
        row("fused_images_gpu_segment", uniform, opts=[("MJ_HUFFMAN", "lanes")], gpu=True, blob="device"),
        row("fused_by_length", mixed, opts=[("MJ_HUFFMAN", "lanes"), ("MJ_SEG_ORDER", "striped")], blob="device"),
        row("fused_by_length_luma12", mixed, opts=[("MJ_HUFFMAN", "lanes"), ("MJ_SEG_ORDER", "striped"), ("MJ_FUSED_LUMA13", "0")]),
        row("fused_by_length_rowmajor", mixed, layout=1, opts=[("MJ_HUFFMAN", "lanes"), ("MJ_SEG_ORDER", "striped")]),
        row("fused_off", uniform, opts=[("MJ_HUFFMAN", "lanes"), ("MJ_SEG_ORDER", "blob"), ("MJ_FUSED", "0")]),
        row("generic", [("craft", 40, 24, ((2, 2), (2, 1), (1, 1)), 3, 0), ("craft", 40, 24, ((2, 2), (2, 1), (1, 1)), 4, 2)]),
        row("generic_lanes_asked", [("craft", 40, 24, ((1, 4), (1, 1), (1, 1)), 5, 2)] * 3, opts=[("MJ_HUFFMAN", "lanes")]),
        row("grey", [("golden", "64x64_grey_pil"), ("golden", "50x70_grey_dri4")]),
        row("grey_lanes", [("golden", "64x64_grey_pil"), ("golden", "50x70_grey_dri4")], opts=[("MJ_HUFFMAN", "lanes")]),
        row("rowmajor", gold, layout=1),
        row("rowmajor_lanes", gold, layout=1, opts=[("MJ_HUFFMAN", "lanes")]),
        row("planar", gold, layout=2),
        row("planar_rowmajor_lanes", gold, layout=3, opts=[("MJ_HUFFMAN", "lanes")]),
        row("stage2_chunk3", gold, opts=[("MJ_STAGE2_CHUNK", "3")]),
        row("sampling_422", [("golden", "72x40_422_dri2")] * 2),
        row("window_host_drops", [("golden", "128x64_420_dri3")] * 2, rois=win),
        row("window_host_drops_lanes", [("golden", "128x64_420_dri3")] * 2, rois=win, opts=[("MJ_HUFFMAN", "lanes")]),
        row("window_whole_images", [("golden", "128x64_420_dri3")] * 2, rois=[(0, 0, 128, 64)] * 2),
        row("window_gpu_gather", [("golden", "128x64_420_dri3")] * 2, rois=win, gpu=True, blob="device"),
        row("window_gpu_gather_lanes", [("golden", "128x64_420_dri3")] * 2, rois=win, gpu=True, blob="device", opts=[("MJ_HUFFMAN", "lanes")]),
        row("gpu_wave_padded_copy", gold, gpu=True, blob="short"),
        row("gpu_lanes_no_copy", gold, gpu=True, blob="short", opts=[("MJ_HUFFMAN", "lanes")]),
        row("device_blob_wave", gold, blob="device"),
        row("progressive_banded_fast", prog),
        row("progressive_levels", prog, opts=[("MJ_PROG_BANDS", "0")]),
        row("progressive_slow_walks", prog, opts=[("MJ_PROG_FAST", "0")]),
        row("progressive_split_all", prog, opts=[("MJ_PROG_SPLIT", "2")]),
        row("progressive_rowmajor", prog, layout=1),
        row("keep_planes_idct", gold, flags=KEEP_PLANES | KEEP_IDCT),
        row("keep_planes_idct_lanes", gold, flags=KEEP_PLANES | KEEP_IDCT, opts=[("MJ_HUFFMAN", "lanes")]),
        row("no_entropy", gold, blob="none"),
        row("refused_late_odd_blob", gold, blob="odd"),
    ]


def make_file(spec) -> bytes:
    kind = spec[0]
    if kind == "golden":
        return (GOLDEN / "files" / (spec[1] + ".jpg")).read_bytes()
    if kind == "synth":
        from tools import synth
        _, seed, w, h, q, ss, ri, sigma = spec
        return synth.synth_jpeg(seed, w, h, q, ss, ri, sigma)
    from tools import craft_jpeg
    if kind == "craft":
        _, w, h, factors, seed, ri = spec
        return craft_jpeg.craft_baseline(w, h, factors, seed=seed, restart_interval=ri)
    _, w, h, seed, ri = spec                # craft_wide: 4:4:4, every component on the file's own wide AC table
    return craft_jpeg.craft_baseline(w, h, ((1, 1),) * 3, seed=seed, restart_interval=ri, tables=[(0, 2), (1, 2), (1, 2)],
                                     ac_tables=[craft_jpeg.wide_ac_table(seed)], max_size=12)


def prepare(row):
    """(prepared batch, every restart segment the files hold) of a row."""
    from pyjpegdecoder_amd import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    files = [make_file(tuple(tuple(x) if isinstance(x, list) else x for x in s)) for s in row["files"]]
    parsed = [parse_jpeg(f, headers_only=True) for f in files] if row["gpu"] else None
    prep = prepare_batch(files, row["layout"], row["flags"], parsed)
    all_segs = 0
    for d in prep.descs:
        mcus = d.mcu_count_h * d.mcu_count_v
        all_segs += -(-mcus // d.restart_interval) if d.restart_interval > 0 else 1
    return prep, all_segs


def batch_c(row, prep, torch):
    """(mj_batch, what it points to) as the row hands the blob over."""
    how = row["blob"]
    if how == "host":
        return prep.to_c(), None
    if how == "none":
        b = prep.to_c()
        b.blob, b.blob_mem = None, 0
        return b, None
    d_blob = torch.from_numpy(np.concatenate([prep.blob, np.zeros(64, np.uint8)])).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    b = prep.to_c(d_blob.data_ptr() + (2 if how == "odd" else 0))
    if how == "short":          # MJ_FLAG_GPU_SEGMENT promises 16 readable bytes behind blob_len, not the 512 the wave form reads
        b.blob_len = (int(prep.seg_end.max()) + 16 + 15) & ~15
    return b, d_blob


def shape_of(ctx, row, prepared=None):
    """One row's plan on the library of `ctx`, which is only asked for its device: the plan is made on a fresh context.  Returns
    {"shape": mj_debug_plan_shape's values or None (creation refused), "rc": mj_plan_create_with's answer, "requests", "size_hash": the
    cache's counters behind the creation, "all_segs": the files' restart segments, "leak": blocks handed out behind
    mj_plan_destroy minus before the creation}."""
    from pyjpegdecoder_amd import _binding as B
    import torch
    lib = ctx.lib
    prep, all_segs = prepared or prepare(row)
    own = B.Context.__new__(B.Context)
    own.lib, own.device, own.handle = lib, ctx.device, ctypes.c_void_p()
    if lib.mj_create(ctx.device, ctypes.byref(own.handle)) != B.MJ_OK:
        raise RuntimeError("mj_create failed")
    for k, v in row["opts"]:
        assert lib.mj_set_option(k.encode(), str(v).encode()) == B.MJ_OK, (k, v)
    try:
        b, keep = batch_c(row, prep, torch)
        before = own.cache_stats()
        h = ctypes.c_void_p()
        request, _arrays = B.plan_request(b.n_images, rois=row["rois"])
        rc = lib.mj_plan_create_with(own.handle, ctypes.byref(b), ctypes.byref(request), ctypes.byref(h))
        after = own.cache_stats()
        shape = None
        if rc == B.MJ_OK:
            out = (ctypes.c_int32 * B.PLAN_SHAPE_WORDS)()
            assert lib.mj_debug_plan_shape(h, out, B.PLAN_SHAPE_WORDS) == B.MJ_OK
            shape = [int(v) for v in out]
            lib.mj_plan_destroy(h)
        del keep
        return {"shape": shape, "rc": int(rc), "requests": after[2] - before[2], "size_hash": f"{after[3]:016x}", "all_segs": all_segs,
                "leak": own.cache_stats()[0] - before[0]}
    finally:
        for k, _ in row["opts"]:
            lib.mj_set_option(k.encode(), None)
        own.close()


def tuned_leak(ctx, row, candidates: int = 2):
    """Blocks the context has handed out behind create, mj_plan_tune_placement(candidates) and destroy, minus before: (leak, the
    plan was a fused one).  The tuning executes the plan into its own output buffer, which it takes on first use."""
    from pyjpegdecoder_amd import _binding as B
    import torch
    lib = ctx.lib
    prep, _ = prepare(row)
    own = B.Context.__new__(B.Context)
    own.lib, own.device, own.handle = lib, ctx.device, ctypes.c_void_p()
    if lib.mj_create(ctx.device, ctypes.byref(own.handle)) != B.MJ_OK:
        raise RuntimeError("mj_create failed")
    for k, v in row["opts"]:
        assert lib.mj_set_option(k.encode(), str(v).encode()) == B.MJ_OK, (k, v)
    try:
        b, keep = batch_c(row, prep, torch)
        before = own.cache_stats()[0]
        h = ctypes.c_void_p()
        own.check(lib.mj_plan_create(own.handle, ctypes.byref(b), ctypes.byref(h)))
        fused = bool(lib.mj_plan_stage1_form(h) & B.MJ_FORM_FUSED)
        ms = (ctypes.c_float * candidates)()
        chosen, best = ctypes.c_int32(), ctypes.c_float()
        lib.mj_plan_tune_placement.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                               ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)]
        own.check(lib.mj_plan_tune_placement(h, None, None, candidates, ms, ctypes.byref(chosen), ctypes.byref(best)))
        own.check(lib.mj_plan_sync(h))
        held = own.cache_stats()[0]
        lib.mj_plan_destroy(h)
        del keep
        return own.cache_stats()[0] - before, fused, held - before
    finally:
        for k, _ in row["opts"]:
            lib.mj_set_option(k.encode(), None)
        own.close()


def kinds_of(row, rec):
    """Which of KINDS a row's record is."""
    from pyjpegdecoder_amd import _binding as B
    s = rec["shape"]
    if s is None:
        return set()
    form, base, out = s[0], s[0] & 15, set()
    prog = base == B.MJ_FORM_SCANS
    if base == B.MJ_FORM_WAVE:
        out.add("wave")
    if base == B.MJ_FORM_LANES:
        out.add("lanes_resolved" if form & B.MJ_FORM_RESOLVED else "lanes11")
    if form & B.MJ_FORM_WG_TABLES and s[10]:
        out.add("wg_tables")
    if base == B.MJ_FORM_SYNC:
        out.add("sync_resolved" if form & B.MJ_FORM_COUNT_RESOLVED and s[8] else "sync_classic")
    if s[12]:
        out.add("by_length")
    if s[1]:
        out.add("fused_by_length" if s[25] else "fused_images")
    if any(f[0] == "craft" and tuple(map(tuple, f[3])) not in (((1, 1),) * 3, ((2, 1), (1, 1), (1, 1)), ((2, 2), (1, 1), (1, 1)))
           for f in row["files"]):
        out.add("generic")
    if all("grey" in str(f[1]) for f in row["files"]):
        out.add("grey")
    if row["layout"] == 1 and "generic" not in out and not prog:
        out.add("rowmajor")
    if row["layout"] >= 2:
        out.add("planar")
    if row["rois"] is not None and s[3] < rec["all_segs"]:
        out.add("window_gpu_gather" if s[4] else "window_host_drops")
    if s[32] and base == B.MJ_FORM_WAVE and s[4]:
        out.add("gpu_wave_padded_copy")
    if prog and s[33] and s[34]:
        out.add("progressive_banded_fast")
    if row["flags"] & (KEEP_PLANES | KEEP_IDCT) == (KEEP_PLANES | KEEP_IDCT):
        out.add("keep_planes_idct")
    return out


def missing_kinds(rows, recs):
    have = set()
    for row, rec in zip(rows, recs):
        have |= kinds_of(row, rec)
    return [k for k in KINDS if k not in have]


def bench_batch():
    """bench.py's default batch: 1024 x 1920x1080 4:2:0, quality 85, one restart interval per MCU row, 256 distinct files."""
    from tools import synth
    from pyjpegdecoder_amd.batch import prepare_batch
    blob, offs = synth.synth_batch(256, 0, 1920, 1080, 85, "420", 120)
    raws = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(256)]
    return prepare_batch([raws[i % 256] for i in range(1024)], 0, 0)


def time_creation(ctx, reps: int = 20):
    import torch
    from pyjpegdecoder_amd import _binding as B
    prep = bench_batch()
    d_blob = torch.from_numpy(prep.blob).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    b = prep.to_c(d_blob.data_ptr())
    ms = []
    for i in range(reps + 1):       # (the first one makes the context's buffers: hipMalloc, not plan creation)
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        rc = ctx.lib.mj_plan_create(ctx.handle, ctypes.byref(b), ctypes.byref(h))
        t1 = time.perf_counter()
        assert rc == B.MJ_OK, rc
        ctx.lib.mj_plan_destroy(h)
        if i:
            ms.append((t1 - t0) * 1e3)
    return {"plan": "1024 x 1920x1080 4:2:0, 256 distinct, device blob", "creations": reps, "median_ms": round(statistics.median(ms), 3),
            "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "ms": [round(x, 3) for x in ms]}


def main() -> int:
    from pyjpegdecoder_amd import _binding as B
    from tools.normalize_probe import other_build
    argv = sys.argv[1:]
    ctx = other_build(B, argv[argv.index("--lib") + 1]) if "--lib" in argv else B.Context(0)
    try:
        if "--time" in argv:
            print(json.dumps(time_creation(ctx)))
            return 0
        if "--leaks" in argv:       # what tests/test_plan_shapes.py asks of the build in the tree, of another build
            by_name = {r["name"]: r for r in matrix()}
            for name in ("fused_images", "sync_resolved", "progressive_banded_fast", "refused_late_odd_blob"):
                rec = shape_of(ctx, by_name[name])
                print(f"{name}: rc {rec['rc']}, blocks left handed out {rec['leak']}")
            print("fused_images tuned: blocks left handed out %d (fused %s, held meanwhile %d)" % tuned_leak(ctx, by_name["fused_images"]))
            return 0
        rows = matrix()
        recs = [shape_of(ctx, r) for r in rows]
    finally:
        ctx.close()
    for row, rec in zip(rows, recs):
        print(f"# {row['name']}: rc {rec['rc']} leak {rec['leak']} {sorted(kinds_of(row, rec))}", file=sys.stderr)
    miss = missing_kinds(rows, recs)
    text = "[\n" + ",\n".join(json.dumps({"name": r["name"], **{k: c[k] for k in ("shape", "rc", "requests", "size_hash", "all_segs")}})
                              for r, c in zip(rows, recs)) + "\n]\n"
    if "--write" in argv:
        if miss:
            print(f"not written: no plan of kind {', '.join(miss)} in the matrix", file=sys.stderr)
            return 1
        RECORD.write_text(text)
    else:
        sys.stdout.write(text)
        if miss:
            print(f"missing kinds: {', '.join(miss)}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
