"""What mj_plan_create decides, and what it asks of the context's buffer cache, pinned on the MI355X: tests/golden/plan_shapes.json
holds, for a fixed matrix of small batches (tools/plan_shapes.py: golden, synthetic and crafted files of at most 256 x 256, at most
64 to a batch, the forms such a batch does not reach by itself forced through the library's options), mj_debug_plan_shape's values,
the number of buffer requests the plan made and the running hash of their sizes in order (mj_debug_cache_stats).  It was recorded from
the build before plan creation was cut into named steps, with nothing but the two accessors added; it is never recorded from the
code under test.  Another form or table width decodes the same pixels, and another ORDER of requests gives a plan other cached
blocks — for a fused plan possibly the slower of two timing classes — so no pixel test notices either; this record does.

Not in the matrix: the chunked first scans of progressive batches (MJ_FORM_SCANS | MJ_FORM_COUNT_RESOLVED), which plan creation
chooses from 2 048 files on.

The leak checks below (blocks handed out before a creation = blocks handed out behind mj_plan_destroy) also pass on the build the
record was taken from (tools/plan_shapes.py --leaks --lib): the hand-written list it freed from forgot nothing.

The plans run no kernel, apart from the one plan that mj_plan_tune_placement executes."""
import json

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyjpegdecoder_amd import _binding as B
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def recorded():
    return json.loads((GOLDEN / "plan_shapes.json").read_text())


def test_the_record_holds_every_kind_of_plan(recorded):
    from tools import plan_shapes
    rows = plan_shapes.matrix()
    assert [r["name"] for r in recorded] == [r["name"] for r in rows]
    assert plan_shapes.missing_kinds(rows, recorded) == []
    assert all(len(r["shape"]) == 38 for r in recorded if r["shape"] is not None)
    assert sum(r["shape"] is not None for r in recorded) >= 40


def test_plan_creation_gives_the_recorded_shapes_and_buffer_requests(ctx, recorded):
    from tools import plan_shapes
    for row, want in zip(plan_shapes.matrix(), recorded):
        got = plan_shapes.shape_of(ctx, row)
        assert got["rc"] == want["rc"], row["name"]
        assert got["shape"] == want["shape"], row["name"]
        assert (got["requests"], got["size_hash"]) == (want["requests"], want["size_hash"]), row["name"]
        assert got["all_segs"] == want["all_segs"], row["name"]
        assert got["leak"] == 0, row["name"]


@pytest.mark.parametrize("name", ["fused_images", "sync_resolved", "progressive_banded_fast"])
def test_a_destroyed_plan_has_returned_every_buffer(ctx, name):
    from tools import plan_shapes
    row = next(r for r in plan_shapes.matrix() if r["name"] == name)
    got = plan_shapes.shape_of(ctx, row)
    assert got["rc"] == 0 and got["requests"] > 8
    assert got["leak"] == 0


def test_a_creation_refused_late_has_returned_every_buffer(ctx):
    """A device blob at a 2-byte offset is refused ("device blob must be 4-byte aligned") behind the tables and the stage-1 buffers."""
    from pyjpegdecoder_amd import _binding as B
    from tools import plan_shapes
    row = next(r for r in plan_shapes.matrix() if r["name"] == "refused_late_odd_blob")
    got = plan_shapes.shape_of(ctx, row)
    assert got["rc"] == B.MJ_ERR_INVALID and got["shape"] is None
    assert got["requests"] > 4, "refused before any buffer was taken: not the late refusal this test is about"
    assert got["leak"] == 0


def test_a_plan_tuned_for_placement_and_destroyed_has_returned_every_buffer(ctx):
    from tools import plan_shapes
    row = next(r for r in plan_shapes.matrix() if r["name"] == "fused_images")
    leak, fused, held = plan_shapes.tuned_leak(ctx, row, candidates=2)
    assert fused and held > 8
    assert leak == 0
