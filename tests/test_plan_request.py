"""mj_plan_create_with on the MI355X: a request that names every default is the plan of the request without it — the same
decisions (mj_debug_plan_shape), the same cut of the resize launch (mj_debug_resize_shape), the same bytes — because the library
turns a field that names its default into its absence before anything is made.  One colour and one greyscale file, x-major and
row-major; and a field that needs a size, given without one, is refused with nothing left handed out."""
import ctypes

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FILES = ("128x64_420_dri3", "50x70_grey_dri4")
SIZE = (17, 5)


@pytest.fixture(scope="module")
def ctx():
    from pyjpegdecoder_amd import _binding as B
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(params=[(f, layout) for f in FILES for layout in (0, 1)], ids=lambda p: f"{p[0]}-{('xmajor', 'rowmajor')[p[1]]}")
def batch(request):
    """(prepared one-image batch, its component count)"""
    from pyjpegdecoder_amd.batch import prepare_batch
    name, layout = request.param
    prep = prepare_batch([(GOLDEN / "files" / f"{name}.jpg").read_bytes()], layout, 0)
    return prep, 1 if "grey" in name else 3


class made:
    """A plan of `fields` through mj_plan_create_with (fields None: through mj_plan_create), as a _binding.Plan; destroyed on exit."""

    def __init__(self, ctx, prep, fields):
        from pyjpegdecoder_amd import _binding as B
        from routes_common import create_with
        self.bc = prep.to_c()
        p = self.plan = B.Plan.__new__(B.Plan)
        p.ctx, p._keep, p.handle, p.info = ctx, {"prep": prep, "n_images": 1}, ctypes.c_void_p(), B.PlanInfoC()
        if fields is None:
            ctx.check(ctx.lib.mj_plan_create(ctx.handle, ctypes.byref(self.bc), ctypes.byref(p.handle)))
        else:
            ctx.check(create_with(ctx.lib, ctx.handle, self.bc, p.handle, **fields))
        ctx.check(ctx.lib.mj_plan_get_info(p.handle, ctypes.byref(p.info)))

    def __enter__(self):
        return self.plan

    def __exit__(self, *exc):
        self.plan.close()


def output_bytes(plan):
    plan.execute()
    plan.sync()
    got = plan.read()
    assert int(got["status"][0]) == 0
    return got["rgb"]


def test_a_resized_request_naming_every_default_is_the_request_with_the_size_alone(ctx, batch):
    from pyjpegdecoder_amd import _binding as B
    prep, ncomp = batch
    size = dict(out_width=SIZE[0], out_height=SIZE[1])
    plain_output = B.OutputDescC()                  # {MJ_DTYPE_U8, 0, .., NULL}
    plain_output.dtype, plain_output.normalize, plain_output.mirror = B.MJ_DTYPE_U8, 0, None
    defaults = dict(orientations=np.ones(1, dtype=np.uint8), mode=ncomp, filter=B.MJ_FILTER_BILINEAR,
                    places=(B.PlaceC * 1)(B.PlaceC(SIZE[0], SIZE[1], 0, 0)), output=plain_output, fill=None)
    with made(ctx, prep, size) as a, made(ctx, prep, {**size, **defaults}) as b:
        assert a.shape() == b.shape()
        assert a.resize_shape() == b.resize_shape()
        assert a.info.rgb_bytes == b.info.rgb_bytes == SIZE[0] * SIZE[1] * ncomp
        want, got = output_bytes(a), output_bytes(b)
        assert len(np.unique(want)) > 4, "a flat output would prove nothing"
        assert np.array_equal(want, got)


def test_an_own_size_request_naming_every_default_is_mj_plan_create(ctx, batch):
    prep, ncomp = batch
    defaults = dict(orientations=np.ones(1, dtype=np.uint8), mode=ncomp)
    with made(ctx, prep, None) as plain, made(ctx, prep, {}) as zeroed, made(ctx, prep, defaults) as named:
        assert plain.shape() == zeroed.shape() == named.shape()            # (word 1: the fused launch, where the plain plan takes it)
        assert plain.stage1_form() == zeroed.stage1_form() == named.stage1_form()
        assert plain.info.rgb_bytes == zeroed.info.rgb_bytes == named.info.rgb_bytes == prep.parsed[0].image_width * prep.parsed[0].image_height * ncomp
        want = output_bytes(plain)
        assert len(np.unique(want)) > 4, "a flat output would prove nothing"
        assert np.array_equal(want, output_bytes(zeroed)) and np.array_equal(want, output_bytes(named))


def test_slots_without_a_size_are_refused_and_nothing_stays_handed_out(ctx, batch):
    from pyjpegdecoder_amd import _binding as B
    from routes_common import create_with
    prep, _ = batch
    bc, h = prep.to_c(), ctypes.c_void_p()
    before = ctx.cache_stats()
    assert create_with(ctx.lib, ctx.handle, bc, h, slots=np.zeros(1, dtype=np.int32), n_slots=1) == B.MJ_ERR_INVALID
    assert not h.value and b"slots needs a size" in ctx.lib.mj_last_error(ctx.handle)
    assert ctx.cache_stats()[0] == before[0] and ctx.cache_stats()[2] == before[2], "a buffer was asked for, or is still handed out"
