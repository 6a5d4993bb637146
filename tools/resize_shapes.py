"""The tile shapes of a fixed matrix of small resized plans: what tests/golden/resize_shapes.json records and
tests/test_resize_shapes.py holds plan creation's tile search to.  A different tile gives the same pixels, so no pixel test notices
a change of the search; this record does.

Every row is one plan of one golden file: source (64 x 64 colour and grey, 100 x 36, 1920 x 1080), output (224 x 224, 17 x 5,
1 x 1), filter, source order, uint8 or normalised float32, and plain / mode-converting / placed.  The values are
mj_debug_resize_shape's eight (Plan.resize_shape).  Plan creation needs a context, so this runs on the GPU box:

    python tools/resize_shapes.py [--lib PATH] [--write]

prints the record of the build in the tree, or of another build of the library (`--lib`, e.g. the parent commit's libmijpeg.so);
`--write` puts it into tests/golden/resize_shapes.json instead.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = ROOT / "tests" / "golden"
RECORD = GOLDEN / "resize_shapes.json"
FILES = {"64x64": "64x64_420_pil.jpg", "64x64_grey": "64x64_grey_pil.jpg", "100x36": "100x36_420_dri7.jpg",
         "1920x1080": "c3_1920x1080_420_dri120.jpg"}
LAYOUTS = {"xmajor": 0, "rowmajor": 1}
OUTPUTS = ((224, 224), (17, 5), (1, 1))
FILTERS = ("bilinear", "box", "hamming", "bicubic", "lanczos")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def matrix():
    """The rows' parameters: (source, output, filter, layout, dtype, kind) — kind "plain", "mode" (colour to L, grey to RGB) or
    "placed" (the image resized to 2/3 of the canvas, rounded up, and placed across its upper left edge: fill on one side, a crop
    on the other), "placed_mode" both."""
    rows = []
    for src in ("64x64", "100x36", "1920x1080"):
        for out in OUTPUTS:
            for layout in LAYOUTS:
                rows.append((src, out, "bicubic", layout, "uint8", "plain"))
    for filter in FILTERS:
        for layout in LAYOUTS:
            rows.append(("1920x1080", (224, 224), filter, layout, "float32", "plain"))
    for layout in LAYOUTS:
        for src in ("64x64", "100x36", "1920x1080"):
            rows.append((src, (224, 224), "lanczos", layout, "uint8", "mode"))
        rows.append(("64x64_grey", (17, 5), "hamming", layout, "float32", "mode"))
    for layout in LAYOUTS:
        for src in ("64x64", "100x36", "1920x1080"):
            rows.append((src, (224, 224), "bilinear", layout, "uint8", "placed"))
        rows.append(("1920x1080", (224, 224), "bicubic", layout, "float32", "placed_mode"))
    return rows


def shape_of(ctx, row):
    """The eight values of one row's plan, in mj_debug_resize_shape's order; None where plan creation refuses the plan because no
    tile fits a workgroup's LDS (1920 x 1080 to 1 x 1), which is part of what the tile search answers."""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd.errors import UnsupportedJpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    src, out, filter, layout, dtype, kind = row
    raw = (GOLDEN / "files" / FILES[src]).read_bytes()
    prep = prepare_batch([raw], LAYOUTS[layout], 0)
    kw = {}
    if "mode" in kind:
        kw["mode"] = "RGB" if src.endswith("grey") else "L"
    nc = 1 if kw.get("mode", "L" if src.endswith("grey") else "RGB") == "L" else 3
    if dtype != "uint8":
        kw["output"] = (dtype, MEAN[:nc], STD[:nc], None)
    if "placed" in kind:
        w, h = (2 * out[0] + 2) // 3, (2 * out[1] + 2) // 3
        kw["places"] = [(w, h, -(w // 4), out[1] - h + h // 4)]
        kw["fill"] = (114, 7, 200)[:nc]
    try:
        plan = B.Plan(ctx, prep.to_c(), {"prep": prep, "n_images": 1}, size=tuple(out), filter=filter, **kw)
    except UnsupportedJpeg as e:
        assert "LDS" in str(e), e
        return None
    try:
        return [int(v) for v in plan.resize_shape().values()]
    finally:
        plan.close()


def main() -> int:
    from pyjpegdecoder_amd import _binding as B
    from tools.normalize_probe import other_build
    argv = sys.argv[1:]
    ctx = other_build(B, argv[argv.index("--lib") + 1]) if "--lib" in argv else B.Context(0)
    try:
        rows = [{"source": r[0], "output": list(r[1]), "filter": r[2], "layout": r[3], "dtype": r[4], "kind": r[5],
                 "shape": shape_of(ctx, r)} for r in matrix()]
    finally:
        ctx.close()
    text = "[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n"
    if "--write" in argv:
        RECORD.write_text(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
