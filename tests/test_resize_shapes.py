"""The tile search of resized-plan creation on the MI355X, pinned: tests/golden/resize_shapes.json holds mj_debug_resize_shape's
eight values for a fixed matrix of small plans (tools/resize_shapes.py: sources 64 x 64, 100 x 36 and 1920 x 1080, outputs 224 x 224,
17 x 5 and 1 x 1, every filter, both source orders, uint8 and float32, plain / converting / placed), recorded from the build before
plan creation was split into steps (null: the plan is refused because no tile fits a workgroup's LDS, 1920 x 1080 to 1 x 1 row-major).
A different tile gives the same pixels, so no pixel test notices a change of the search."""
import json

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def test_tile_search_gives_the_recorded_shapes():
    from tools import resize_shapes
    from pyjpegdecoder_amd import _binding as B
    rows = json.loads((GOLDEN / "resize_shapes.json").read_text())
    assert [(r["source"], tuple(r["output"]), r["filter"], r["layout"], r["dtype"], r["kind"]) for r in rows] == resize_shapes.matrix()
    assert len(rows) >= 40 and sum(r["shape"] is not None for r in rows) >= 40
    ctx = B.Context(0)
    try:
        for r, row in zip(rows, resize_shapes.matrix()):
            assert resize_shapes.shape_of(ctx, row) == r["shape"], row
    finally:
        ctx.close()
