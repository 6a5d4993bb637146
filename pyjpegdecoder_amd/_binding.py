"""ctypes binding of libmijpeg.so (include/mijpeg.h).  Fails loudly when the HIP library is missing or
no GPU is present — there is no CPU fallback in the product path."""
from __future__ import annotations

import ctypes
from pathlib import Path
from typing import Optional

import numpy as np

from .errors import BackendError

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libmijpeg.so"
MJ_VERSION = 2      # include/mijpeg.h's: the layout of the structures below; load_library refuses a library of another version

MJ_OK, MJ_ERR_INVALID, MJ_ERR_HIP, MJ_ERR_UNSUPPORTED = 0, -1, -2, -3
MJ_ST_OK, MJ_ST_BAD_CODE, MJ_ST_OVERRUN, MJ_ST_DESYNC, MJ_ST_TAIL, MJ_ST_UNCONVERGED, MJ_ST_INTERNAL = 0, 1, 2, 3, 4, 5, 6
MJ_MEM_NONE, MJ_MEM_HOST, MJ_MEM_DEVICE = 0, 1, 2
MJ_LAYOUT_XMAJOR, MJ_LAYOUT_ROWMAJOR, MJ_LAYOUT_PLANAR_XMAJOR, MJ_LAYOUT_PLANAR_ROWMAJOR = 0, 1, 2, 3
MJ_FLAG_KEEP_COEF, MJ_FLAG_KEEP_PLANES, MJ_FLAG_KEEP_IDCT, MJ_FLAG_EXACT_ONLY, MJ_FLAG_SPEC_REFINE = 1, 2, 4, 8, 16
MJ_FLAG_GPU_SEGMENT = 32
MJ_FLAG_NO_SYNC = 64
MJ_DTYPE_U8, MJ_DTYPE_F16, MJ_DTYPE_BF16, MJ_DTYPE_F32 = 0, 1, 2, 3
# the element types of a model-ready output (mj_output_desc.dtype) by the name NumPy and torch share
DTYPES = {"uint8": MJ_DTYPE_U8, "float16": MJ_DTYPE_F16, "bfloat16": MJ_DTYPE_BF16, "float32": MJ_DTYPE_F32}
DTYPE_BYTES = {"uint8": 1, "float16": 2, "bfloat16": 2, "float32": 4}
MJ_FILTER_BILINEAR, MJ_FILTER_BOX, MJ_FILTER_HAMMING, MJ_FILTER_BICUBIC, MJ_FILTER_LANCZOS = 0, 1, 2, 3, 4
# the resample filters of a decode to a fixed size by name (tools/resize_model.py: FILTERS)
MJ_AFFINE_NEAREST, MJ_AFFINE_BILINEAR, MJ_AFFINE_BICUBIC = 1, 2, 3
AFFINE_FILTERS = {"nearest": MJ_AFFINE_NEAREST, "bilinear": MJ_AFFINE_BILINEAR, "bicubic": MJ_AFFINE_BICUBIC}
FILTERS = {"bilinear": MJ_FILTER_BILINEAR, "box": MJ_FILTER_BOX, "hamming": MJ_FILTER_HAMMING, "bicubic": MJ_FILTER_BICUBIC,
           "lanczos": MJ_FILTER_LANCZOS}

MJ_MODE_NATIVE, MJ_MODE_L, MJ_MODE_RGB = 0, 1, 3
# colour operations (mj_plan_request.colour): the ops by name (tools/colour_model.py: OPS), MJ_COLOUR_*
MJ_COLOUR_MAX_OPS = 4
COLOUR_OPS = {"brightness": 1, "color": 2, "contrast": 3, "sharpness": 4, "posterize": 5, "solarize": 6, "autocontrast": 7,
              "equalize": 8, "invert": 9, "gaussian_blur": 10, "box_blur": 11, "adjust_hue": 13}          # (12 is no kind)
COLOUR_VALUED = ("brightness", "color", "contrast", "sharpness", "posterize", "solarize", "gaussian_blur", "box_blur", "adjust_hue")        # the ops that take a value
COLOUR_BLURS = ("gaussian_blur", "box_blur")           # ... whose value is a radius, 0 .. MJ_COLOUR_MAX_RADIUS
MJ_COLOUR_MAX_RADIUS = 1024
# the output colour modes by Pillow's name: MJ_MODE_*, which is the component count of the output
MODES = {"L": MJ_MODE_L, "RGB": MJ_MODE_RGB}

# every symbol include/mijpeg.h declares (tests check the library exports all of them)
EXPORTS = (
    "mj_create", "mj_destroy", "mj_last_error", "mj_version", "mj_context_wait_event",
    "mj_plan_create", "mj_plan_create_with", "mj_plan_destroy", "mj_plan_get_info", "mj_plan_image_offsets",
    "mj_plan_execute", "mj_plan_execute_stage1", "mj_plan_execute_stage2", "mj_plan_sync",
    "mj_plan_device_buffers", "mj_plan_read", "mj_plan_write_coef", "mj_plan_fill_coef",
    "mj_decode_baseline_batch", "mj_idct_batch", "mj_plan_time_stages", "mj_plan_time_execute", "mj_plan_idct_levels", "mj_host_idct_table", "mj_host_assemble", "mj_plan_stage1_form", "mj_set_option", "mj_get_option", "mj_debug_stage1_form", "mj_debug_fused_shape", "mj_debug_count_tables",
    "mj_device_copy_rate", "mj_context_launch_clock", "mj_debug_prog_split", "mj_debug_fused_applies", "mj_plan_tune_placement",
    "mj_plan_fill_source", "mj_plan_time_resize", "mj_host_resize_table", "mj_host_normalize_table", "mj_host_exif_orientations",
    "mj_host_resize_table_filtered", "mj_debug_resize_shape", "mj_host_convert_mode",
    "mj_host_resize_table_boxed", "mj_host_reduce_factors", "mj_host_reduce", "mj_debug_reduce_shape", "mj_debug_normalise_request",
    "mj_plan_time_reduce", "mj_host_affine", "mj_host_perspective", "mj_plan_time_affine", "mj_debug_reduce_launch", "mj_host_colour_ops", "mj_plan_time_colour",
    "mj_debug_plan_shape", "mj_debug_cache_stats", "mj_debug_resolved_tables", "mj_plan_derive",
    "mj_plan_set_erase", "mj_plan_time_erase", "mj_host_erase",
    "mj_mix", "mj_mix_time", "mj_host_mix",
    "mj_compose", "mj_compose_time", "mj_host_compose", "mj_host_compose_resolve",
    "mj_patchify", "mj_patchify_time", "mj_host_patchify", "mj_host_patchify_count",
)
MJ_FORM_WAVE, MJ_FORM_LANES, MJ_FORM_SYNC, MJ_FORM_SCANS, MJ_FORM_WG_TABLES, MJ_FORM_RESOLVED, MJ_FORM_FUSED, MJ_FORM_COUNT_RESOLVED = 0, 1, 2, 3, 16, 32, 64, 128
MJ_HOST_DECLINED = 1
PLAN_SHAPE_WORDS = 38       # MJ_DEBUG_PLAN_SHAPE_WORDS


class HuffSpecC(ctypes.Structure):
    _fields_ = [("bits", ctypes.c_uint8 * 16), ("vals", ctypes.c_uint8 * 256)]


class ImageDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32),
                ("hs", ctypes.c_int32 * 3), ("vs", ctypes.c_int32 * 3), ("qt_sel", ctypes.c_int32 * 3),
                ("dc_sel", ctypes.c_int32 * 3), ("ac_sel", ctypes.c_int32 * 3),
                ("restart_interval", ctypes.c_int32),
                ("mcu_count_h", ctypes.c_int32), ("mcu_count_v", ctypes.c_int32),
                ("n_segments", ctypes.c_int32), ("first_segment", ctypes.c_int64)]


class ScanDescC(ctypes.Structure):
    _fields_ = [("image", ctypes.c_int32), ("n_comp", ctypes.c_int32), ("comp", ctypes.c_int32 * 3),
                ("dc_sel", ctypes.c_int32 * 3), ("ac_sel", ctypes.c_int32 * 3),
                ("ss", ctypes.c_int32), ("se", ctypes.c_int32), ("ah", ctypes.c_int32), ("al", ctypes.c_int32),
                ("restart_interval", ctypes.c_int32), ("mcu_count_h", ctypes.c_int32), ("mcu_count_v", ctypes.c_int32),
                ("n_segments", ctypes.c_int32), ("first_segment", ctypes.c_int64)]


class BatchC(ctypes.Structure):
    _fields_ = [("n_images", ctypes.c_int32), ("images", ctypes.POINTER(ImageDescC)),
                ("blob", ctypes.c_void_p), ("blob_len", ctypes.c_int64), ("blob_mem", ctypes.c_int32),
                ("n_segments", ctypes.c_int64), ("seg_begin", ctypes.c_void_p), ("seg_end", ctypes.c_void_p),
                ("n_huff", ctypes.c_int32), ("huff", ctypes.POINTER(HuffSpecC)),
                ("n_qt", ctypes.c_int32), ("qt", ctypes.c_void_p),
                ("layout", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("n_scans", ctypes.c_int32), ("scans", ctypes.POINTER(ScanDescC))]


class HostJobC(ctypes.Structure):
    _fields_ = [("n_files", ctypes.c_int32), ("files", ctypes.POINTER(ctypes.c_char_p)), ("sizes", ctypes.c_void_p),
                ("file_off", ctypes.c_void_p), ("blob", ctypes.c_void_p), ("blob_len", ctypes.c_int64),
                ("images", ctypes.POINTER(ImageDescC)), ("seg_begin", ctypes.c_void_p), ("seg_end", ctypes.c_void_p),
                ("huff", ctypes.POINTER(HuffSpecC)), ("huff_cap", ctypes.c_int32),
                ("qt", ctypes.c_void_p), ("qt_cap", ctypes.c_int32), ("n_threads", ctypes.c_int32),
                ("n_huff", ctypes.c_int32), ("n_qt", ctypes.c_int32), ("declined_file", ctypes.c_int32),
                ("skip", ctypes.c_void_p), ("n_accepted", ctypes.c_int32)]


class RoiC(ctypes.Structure):
    """mj_roi: one image's window (x along image_width, y along image_height)."""
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32)]


class PlaceC(ctypes.Structure):
    """mj_place: the size one image is resized to and where its top-left lies on the canvas."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("x", ctypes.c_int32), ("y", ctypes.c_int32)]


class OutputDescC(ctypes.Structure):
    """mj_output_desc: element type, normalisation and mirror flags of a model-ready output."""
    _fields_ = [("dtype", ctypes.c_int32), ("normalize", ctypes.c_int32), ("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3),
                ("mirror", ctypes.c_void_p)]


class ViewC(ctypes.Structure):
    """mj_view: one output of a plan with views — the image it shows and the window of it (all zero: the whole oriented image)."""
    _fields_ = [("image", ctypes.c_int32), ("window", RoiC)]


class AffineC(ctypes.Structure):
    """mj_affine: one output's matrix, output to source (all zero: no transform)."""
    _fields_ = [("a", ctypes.c_double * 6)]


class PerspectiveC(ctypes.Structure):
    """mj_perspective: one output's eight coefficients, output to source (all zero: no transform)."""
    _fields_ = [("a", ctypes.c_double * 8)]


class ColourOpC(ctypes.Structure):
    """mj_colour_op: one colour operation — MJ_COLOUR_* and its factor, bits or threshold."""
    _fields_ = [("kind", ctypes.c_int32), ("value", ctypes.c_float)]


class ColourChainC(ctypes.Structure):
    """mj_colour_chain: one output's ops, applied in order (n == 0: none)."""
    _fields_ = [("n", ctypes.c_int32), ("op", ColourOpC * MJ_COLOUR_MAX_OPS)]


MJ_ERASE_CONST, MJ_ERASE_VALUES = 0, 1


class EraseRectC(ctypes.Structure):
    """mj_erase_rect: one box of mj_plan_set_erase / mj_host_erase."""
    _fields_ = [("output", ctypes.c_int32), ("x", ctypes.c_int32), ("y", ctypes.c_int32), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("kind", ctypes.c_int32), ("value", ctypes.c_float * 3), ("offset", ctypes.c_int64)]


def erase_rects(rects):
    """an array of mj_erase_rect from (output, x, y, width, height, value) records — value: up to three numbers (MJ_ERASE_CONST, one
    per output component) or an int element offset wrapped as ``("values", offset)`` (MJ_ERASE_VALUES) —, from ready EraseRectC's, or
    from a NumPy array of ERASE_RECT_DTYPE records (made in bulk: batch.py's).  Returns (what the C call takes, what keeps it alive)."""
    if isinstance(rects, np.ndarray) and rects.dtype == ERASE_RECT_DTYPE:
        rects = np.ascontiguousarray(rects)
        return ctypes.cast(rects.ctypes.data, ctypes.POINTER(EraseRectC)), rects
    arr = (EraseRectC * max(1, len(rects)))()
    _fill_erase_rects(arr, rects)
    return arr, arr


# mj_erase_rect as a NumPy record: a list of tuples (output, x, y, width, height, kind, value[3], offset) becomes the array in one call
ERASE_RECT_DTYPE = np.dtype([("output", "<i4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"), ("kind", "<i4"),
                             ("value", "<f4", (3,)), ("offset", "<i8")], align=True)
assert ERASE_RECT_DTYPE.itemsize == ctypes.sizeof(EraseRectC)


def _fill_erase_rects(arr, rects):
    for k, r in enumerate(rects):
        if isinstance(r, EraseRectC):
            arr[k] = r
            continue
        out, x, y, w, h, value = r
        arr[k].output, arr[k].x, arr[k].y, arr[k].width, arr[k].height = int(out), int(x), int(y), int(w), int(h)
        if isinstance(value, tuple) and len(value) == 2 and value[0] == "values":
            arr[k].kind, arr[k].offset = MJ_ERASE_VALUES, int(value[1])
        else:
            vals = [float(v) for v in (value if isinstance(value, (list, tuple)) else [value] * 3)]
            arr[k].kind = MJ_ERASE_CONST
            for c, v in enumerate(vals[:3]):
                arr[k].value[c] = v
    return arr


MJ_MIX_NONE, MJ_MIX_MIXUP, MJ_MIX_CUTMIX = 0, 1, 2


class MixOpC(ctypes.Structure):
    """mj_mix_op: what mj_mix / mj_host_mix do to one output."""
    _fields_ = [("kind", ctypes.c_int32), ("partner", ctypes.c_int32), ("x", ctypes.c_int32), ("y", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("lam", ctypes.c_double)]


# mj_mix_op as a NumPy record: a list of tuples (kind, partner, x, y, width, height, lam) becomes the array in one call
MIX_OP_DTYPE = np.dtype([("kind", "<i4"), ("partner", "<i4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"), ("lam", "<f8")], align=True)
assert MIX_OP_DTYPE.itemsize == ctypes.sizeof(MixOpC)


def mix_ops(entries):
    """what the C calls take as ``ops`` from one entry per output: None, ``("mixup", partner, lam)``, ``("cutmix", partner, (x, y,
    width, height))`` — or ready MixOpC's, which the tests of the library's refusals pass.  Returns (pointer, what keeps it alive)."""
    if any(isinstance(e, MixOpC) for e in entries):
        arr = (MixOpC * max(1, len(entries)))()
        rest = mix_ops([None if isinstance(e, MixOpC) else e for e in entries])[1]
        for k, e in enumerate(entries):
            if isinstance(e, MixOpC):
                arr[k] = e
            else:
                ctypes.memmove(ctypes.byref(arr[k]), rest.ctypes.data + k * MIX_OP_DTYPE.itemsize, MIX_OP_DTYPE.itemsize)
        return arr, arr
    arr = np.zeros(max(1, len(entries)), dtype=MIX_OP_DTYPE)
    # (column by column from plain arrays: a structured array made from a list of tuples costs several times as much)
    blends = [(k, e[1], e[2]) for k, e in enumerate(entries) if e is not None and e[0] == "mixup"]
    if blends:
        cols = np.array(blends, dtype=np.float64)       # (indices are exact in float64)
        at = cols[:, 0].astype(np.intp)
        arr["kind"][at], arr["partner"][at], arr["lam"][at] = MJ_MIX_MIXUP, cols[:, 1].astype(np.int32), cols[:, 2]
    cuts = [(k, e[1]) + tuple(e[2]) for k, e in enumerate(entries) if e is not None and e[0] != "mixup"]
    if cuts:
        cols = np.array(cuts, dtype=np.int64)
        at = cols[:, 0]
        arr["kind"][at], arr["partner"][at] = MJ_MIX_CUTMIX, cols[:, 1]
        arr["x"][at], arr["y"][at], arr["width"][at], arr["height"][at] = cols[:, 2], cols[:, 3], cols[:, 4], cols[:, 5]
    return ctypes.cast(arr.ctypes.data, ctypes.POINTER(MixOpC)), arr


class ComposeTileC(ctypes.Structure):
    """mj_compose_tile: one window of one source slot pasted onto one output canvas."""
    _fields_ = [("output", ctypes.c_int32), ("source", ctypes.c_int32), ("sx", ctypes.c_int32), ("sy", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("dx", ctypes.c_int32), ("dy", ctypes.c_int32)]


# mj_compose_tile / mj_compose_rect as NumPy records: eight int32 each
COMPOSE_TILE_DTYPE = np.dtype([(n, "<i4") for n in ("output", "source", "sx", "sy", "width", "height", "dx", "dy")])
COMPOSE_RECT_DTYPE = np.dtype([(n, "<i4") for n in ("output", "x", "y", "width", "height", "source", "sx", "sy")])
assert COMPOSE_TILE_DTYPE.itemsize == ctypes.sizeof(ComposeTileC) == COMPOSE_RECT_DTYPE.itemsize


def compose_tiles(outputs):
    """what the C calls take as ``tiles`` from one list per output of tiles ``(source, (dx, dy), (sx, sy, width, height))``, in paste
    order — or a ready array of COMPOSE_TILE_DTYPE records, which the tests of the library's refusals pass.  Returns (pointer or
    None, number of tiles, what keeps them alive)."""
    if isinstance(outputs, np.ndarray):
        arr = np.ascontiguousarray(outputs, dtype=COMPOSE_TILE_DTYPE)
    else:
        rows = [(m, s, w[0], w[1], w[2], w[3], d[0], d[1]) for m, tiles in enumerate(outputs) for s, d, w in tiles]
        arr = np.zeros(len(rows), dtype=COMPOSE_TILE_DTYPE)
        if rows:
            arr.view(np.int32).reshape(-1, 8)[:] = np.array(rows, dtype=np.int64)
    return (ctypes.cast(arr.ctypes.data, ctypes.POINTER(ComposeTileC)) if len(arr) else None), len(arr), arr


class PatchWindowC(ctypes.Structure):
    """mj_patch_window: the window of one source that is cut into patches."""
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32)]


PATCH_ORDERS = {"chw": 0, "hwc": 1}          # MJ_PATCH_*


def patch_windows(windows, n_sources: int):
    """what the C calls take as ``windows``: None (every source's whole canvas), or one ``(x, y, width, height)`` per source — an
    entry None being the whole ``canvas`` = (width, height), which the caller has put in its place.  Returns (pointer or None,
    what keeps it alive)."""
    if windows is None:
        return None, None
    arr = np.ascontiguousarray(np.array([tuple(int(v) for v in w) for w in windows], dtype=np.int32).reshape(-1, 4))
    if len(arr) != n_sources:
        raise ValueError(f"patches: {len(arr)} windows for {n_sources} sources")
    return ctypes.cast(arr.ctypes.data, ctypes.POINTER(PatchWindowC)), arr


def _patch_args(spec):
    """(patch, merge, repeat, order, length) of a patch spec as the C calls take them (length None: 0, the packed form)"""
    return (int(spec["patch"]), int(spec.get("merge", 1)), int(spec.get("repeat", 1)), PATCH_ORDERS[spec.get("order", "chw")], int(spec.get("length") or 0))


def _fill_bits(fill_bits):
    return (ctypes.c_uint32 * 3)(*([int(v) for v in fill_bits] + [0, 0, 0])[:3])


class PlanRequestC(ctypes.Structure):
    """mj_plan_request: what a plan's output is to be; zeroed, the plain plan.  Every field of the header's struct, in its order."""
    _fields_ = [("rois", ctypes.POINTER(RoiC)), ("orientations", ctypes.c_void_p), ("mode", ctypes.c_int32),
                ("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32),
                ("transform_filter", ctypes.c_int32), ("affine", ctypes.POINTER(AffineC)), ("perspective", ctypes.POINTER(PerspectiveC)),
                ("slots", ctypes.c_void_p), ("n_slots", ctypes.c_int32), ("n_views", ctypes.c_int32), ("views", ctypes.POINTER(ViewC)),
                ("output", ctypes.POINTER(OutputDescC)), ("filter", ctypes.c_int32), ("reducing_gap", ctypes.c_float),
                ("places", ctypes.POINTER(PlaceC)), ("fill", ctypes.c_void_p), ("colour", ctypes.POINTER(ColourChainC)),
                ("transform_fill", ctypes.c_uint8 * 3)]


def colour_chain(chain) -> ColourChainC:
    """mj_colour_chain from None or a sequence of at most MJ_COLOUR_MAX_OPS ops ``(name,)`` / ``(name, value)`` (an MJ_COLOUR_* number
    passes for the name).  A blur that comes without its radius gets NaN, which the library refuses: no radius is not radius 0."""
    c = ColourChainC()
    ops = list(chain) if chain is not None else []
    if len(ops) > MJ_COLOUR_MAX_OPS:
        raise ValueError(f"a chain has at most {MJ_COLOUR_MAX_OPS} ops, not {len(ops)}")
    c.n = len(ops)
    for s, op in enumerate(ops):
        c.op[s].kind = COLOUR_OPS[op[0]] if isinstance(op[0], str) else int(op[0])
        blur = c.op[s].kind in (COLOUR_OPS["gaussian_blur"], COLOUR_OPS["box_blur"])
        c.op[s].value = float(op[1]) if len(op) > 1 else float("nan") if blur else 0.0
    return c


class PlanInfoC(ctypes.Structure):
    _fields_ = [("total_blocks", ctypes.c_int64), ("total_mcus", ctypes.c_int64), ("total_pixels", ctypes.c_int64),
                ("rgb_bytes", ctypes.c_int64), ("entropy_bytes", ctypes.c_int64)]


_lib = None


def load_library():
    """dlopen libmijpeg.so and declare the prototypes.  Raises BackendError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise BackendError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C pyjpegdecoder_amd/csrc`). There is no CPU fallback.")
    # PyTorch's ROCm wheels bundle their own HIP / HSA runtime under the same soname as /opt/rocm's.  Whichever is loaded first
    # serves the whole process: torch's first, and this library binds to it; /opt/rocm's first (through this library), and a
    # later `import torch` finds "No HIP GPUs are available".  So torch — which the device-tensor API needs anyway — goes first.
    try:
        import torch  # noqa: F401
    except Exception:      # no PyTorch: the host-array API works on /opt/rocm's runtime alone
        pass
    try:
        L = ctypes.CDLL(str(LIB_PATH))
    except OSError as exc:
        raise BackendError(f"cannot load {LIB_PATH}: {exc}") from exc
    if L.mj_version() != MJ_VERSION:      # (a library of another version lays mj_plan_request out differently)
        raise BackendError(f"{LIB_PATH} is version {L.mj_version()} of the C ABI and this binding version {MJ_VERSION}: rebuild the "
                           f"library (`make -C pyjpegdecoder_amd/csrc`)")
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.mj_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.mj_destroy.argtypes = [vp]
    L.mj_destroy.restype = None
    L.mj_last_error.argtypes = [vp]
    L.mj_last_error.restype = ctypes.c_char_p
    L.mj_context_wait_event.argtypes = [vp, vp]
    L.mj_plan_create.argtypes = [vp, ctypes.POINTER(BatchC), ctypes.POINTER(vp)]
    L.mj_plan_create_with.argtypes = [vp, ctypes.POINTER(BatchC), ctypes.POINTER(PlanRequestC), ctypes.POINTER(vp)]
    L.mj_plan_derive.argtypes = [vp, ctypes.POINTER(BatchC), ctypes.POINTER(PlanRequestC), ctypes.POINTER(vp)]
    L.mj_host_convert_mode.argtypes = [i32, vp, i32, i64, vp]
    L.mj_host_resize_table_filtered.argtypes = [i32, i32, i32, vp, vp, vp, i32, ctypes.POINTER(i32)]
    L.mj_debug_resize_shape.argtypes = [vp, ctypes.POINTER(i32)]
    L.mj_host_resize_table_boxed.argtypes = [i32, i32, ctypes.c_double, ctypes.c_double, i32, vp, vp, vp, i32, ctypes.POINTER(i32)]
    L.mj_host_reduce_factors.argtypes = [i32, i32, i32, i32, ctypes.c_double, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.mj_host_reduce.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.mj_debug_reduce_shape.argtypes = [vp, i32, ctypes.POINTER(i32)]
    L.mj_debug_reduce_launch.argtypes = [vp, ctypes.POINTER(i32)]
    L.mj_debug_normalise_request.argtypes = [ctypes.POINTER(BatchC), ctypes.POINTER(PlanRequestC), ctypes.POINTER(PlanRequestC)]
    L.mj_debug_plan_shape.argtypes = [vp, ctypes.POINTER(i32), i32]
    L.mj_debug_cache_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.mj_host_exif_orientations.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.mj_host_normalize_table.argtypes = [i32, ctypes.c_float, ctypes.c_float, vp]
    L.mj_plan_fill_source.argtypes = [vp, ctypes.c_int]
    L.mj_plan_time_resize.argtypes = [vp, ctypes.c_int, vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(i64)]
    L.mj_plan_time_reduce.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    L.mj_host_affine.argtypes = [vp, i32, i32, i32, ctypes.POINTER(ctypes.c_double), i32, vp, i32, i32, i32, i32, vp]
    L.mj_plan_time_colour.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)]
    L.mj_host_colour_ops.argtypes = [vp, i32, i32, i32, ctypes.POINTER(ColourChainC), vp]
    L.mj_host_perspective.argtypes = [vp, i32, i32, i32, ctypes.POINTER(ctypes.c_double), i32, vp, i32, i32, i32, i32, vp]
    L.mj_plan_time_affine.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)]
    L.mj_plan_set_erase.argtypes = [vp, i32, ctypes.POINTER(EraseRectC), vp]
    L.mj_plan_time_erase.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)]
    L.mj_host_erase.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, ctypes.POINTER(EraseRectC), vp]
    L.mj_mix.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, ctypes.POINTER(MixOpC)]
    L.mj_mix_time.argtypes = [vp, ctypes.c_int, vp, vp, i32, i32, i32, i32, i32, i32, ctypes.POINTER(MixOpC), ctypes.POINTER(ctypes.c_float)]
    L.mj_host_mix.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, ctypes.POINTER(MixOpC)]
    u32p, tiles = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ComposeTileC)
    L.mj_compose.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, u32p, i32, tiles]
    L.mj_compose_time.argtypes = [vp, ctypes.c_int, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, u32p, i32, tiles, ctypes.POINTER(ctypes.c_float)]
    L.mj_host_compose.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, u32p, i32, tiles]
    pw = ctypes.POINTER(PatchWindowC)
    L.mj_patchify.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, pw]
    L.mj_patchify_time.argtypes = [vp, ctypes.c_int, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, pw, ctypes.POINTER(ctypes.c_float)]
    L.mj_host_patchify.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, pw]
    L.mj_host_patchify_count.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, pw, ctypes.POINTER(ctypes.c_int64)]
    L.mj_host_compose_resolve.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, i32, tiles, vp, i32, ctypes.POINTER(i32)]
    L.mj_host_resize_table.argtypes = [i32, i32, vp, vp, vp, i32, ctypes.POINTER(i32)]
    L.mj_plan_destroy.argtypes = [vp]
    L.mj_plan_destroy.restype = None
    L.mj_plan_get_info.argtypes = [vp, ctypes.POINTER(PlanInfoC)]
    L.mj_plan_image_offsets.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.mj_plan_execute.argtypes = [vp, vp, vp]
    L.mj_plan_execute_stage1.argtypes = [vp, vp]
    L.mj_plan_execute_stage2.argtypes = [vp, vp, vp]
    L.mj_plan_sync.argtypes = [vp]
    L.mj_plan_device_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.mj_plan_read.argtypes = [vp, vp, vp, vp, vp, vp]
    L.mj_plan_write_coef.argtypes = [vp, vp, i32]
    L.mj_decode_baseline_batch.argtypes = [vp, ctypes.POINTER(BatchC), vp, vp, vp]
    L.mj_idct_batch.argtypes = [vp, ctypes.POINTER(BatchC), vp, vp]
    L.mj_plan_time_stages.argtypes = [vp, ctypes.c_int, vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.mj_plan_fill_coef.argtypes = [vp, ctypes.c_int]
    L.mj_plan_time_execute.argtypes = [vp, ctypes.c_int, vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.mj_host_idct_table.argtypes = [vp]
    L.mj_host_idct_table.restype = None
    L.mj_host_assemble.argtypes = [ctypes.POINTER(HostJobC)]
    L.mj_plan_stage1_form.argtypes = [vp]
    L.mj_plan_idct_levels.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.mj_set_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.mj_get_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32]
    L.mj_debug_stage1_form.argtypes = [vp, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int32,
                                       ctypes.POINTER(ctypes.c_int32)]
    _lib = L
    return L


def stage1_form_rule(seg_len, blob_len=None, n_huff=4, traits=0, force=None, forced_chunk=0):
    """mj_debug_stage1_form (host only): (MJ_FORM_*, chunk bytes, chunks, dealt out by length) for a batch whose restart
    segments have these byte lengths — the rule mj_plan_create applies (csrc/form_select.h)."""
    a = np.ascontiguousarray(seg_len, dtype=np.int32)
    out = (ctypes.c_int32 * 4)()
    rc = load_library().mj_debug_stage1_form(_ptr(a), a.size, int(a.sum()) + 4096 if blob_len is None else blob_len, n_huff, traits,
                                             force.encode() if force else None, forced_chunk, out)
    if rc != MJ_OK:
        raise ValueError("mj_debug_stage1_form: bad arguments")
    return int(out[0]), int(out[1]), int(out[2]), bool(out[3])


def count_tables(huff_specs, roles, wbits=12):
    """mj_debug_count_tables (host only): (words, tab_bytes) — the synchronisation form's counting tables for these tables
    (list of (bits[16], vals) pairs; roles: 1 = DC, 2 = AC) — or None where such a batch takes the classic rounds."""
    L = load_library()
    n = len(huff_specs)
    arr = (HuffSpecC * n)()
    for i, (bits, vals) in enumerate(huff_specs):
        for j in range(16):
            arr[i].bits[j] = int(bits[j])
        for j, v in enumerate(vals):
            arr[i].vals[j] = int(v)
    r = (ctypes.c_int32 * n)(*[int(x) for x in roles])
    tb = ctypes.c_int32(0)
    L.mj_debug_count_tables.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.POINTER(ctypes.c_int32)]
    rc = L.mj_debug_count_tables(ctypes.byref(arr), n, ctypes.byref(r), wbits, None, 0, ctypes.byref(tb))
    if rc == MJ_ERR_UNSUPPORTED:
        return None
    if rc != MJ_OK:
        raise ValueError("mj_debug_count_tables: bad arguments")
    out = np.zeros(n * tb.value // 4, dtype=np.uint32)
    rc = L.mj_debug_count_tables(ctypes.byref(arr), n, ctypes.byref(r), wbits, _ptr(out), out.size, ctypes.byref(tb))
    if rc != MJ_OK:
        raise ValueError("mj_debug_count_tables: bad arguments")
    return out, tb.value


def resolved_tables(huff_specs, roles, slots, index_bits, fixed_slot_bytes=0):
    """mj_debug_resolved_tables (host only): (words, slot offsets in bytes) — the lane walk's resolved AC tables for these tables
    (list of (bits[16], vals) pairs; roles: 2 = AC; slots[t] = the slot of AC table t; index_bits per slot, 10..13), `fixed_slot_bytes`
    apart or (0) packed back to back — or None where they do not fit."""
    L = load_library()
    n = len(huff_specs)
    arr = (HuffSpecC * n)()
    for i, (bits, vals) in enumerate(huff_specs):
        for j in range(16):
            arr[i].bits[j] = int(bits[j])
        for j, v in enumerate(vals):
            arr[i].vals[j] = int(v)
    n_ac = max(s for s, r in zip(slots, roles) if r == 2) + 1
    r = (ctypes.c_int32 * n)(*[int(x) for x in roles])
    sl = (ctypes.c_int32 * n)(*[int(x) for x in slots])
    ab = (ctypes.c_int32 * 4)(*(list(index_bits) + [13] * 4)[:4])
    off = (ctypes.c_int32 * 4)()
    total = ctypes.c_int32(0)
    L.mj_debug_resolved_tables.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                           ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
    rc = L.mj_debug_resolved_tables(ctypes.byref(arr), n, ctypes.byref(r), ctypes.byref(sl), n_ac, ctypes.byref(ab), fixed_slot_bytes, None, 0,
                                    ctypes.byref(off), ctypes.byref(total))
    if rc == MJ_ERR_UNSUPPORTED:
        return None
    if rc != MJ_OK:
        raise ValueError("mj_debug_resolved_tables: bad arguments")
    out = np.zeros(total.value // 4, dtype=np.uint32)
    rc = L.mj_debug_resolved_tables(ctypes.byref(arr), n, ctypes.byref(r), ctypes.byref(sl), n_ac, ctypes.byref(ab), fixed_slot_bytes, _ptr(out),
                                    out.size, ctypes.byref(off), ctypes.byref(total))
    if rc != MJ_OK:
        raise ValueError("mj_debug_resolved_tables: bad arguments")
    return out, [int(off[s]) for s in range(n_ac)]


def fused_shape_rule(n_images, segments_per_image, hmax=2, vmax=2, transposed=False, cus=256, n_ac=2, n_dc=2, ac_slot_bytes=17024,
                     want_consumers=8):
    """mj_debug_fused_shape (host only): dict(ok, images_per_wg [and pass], producers, lanes, consumers, producer_lds, passes,
    workgroups) of a fused launch."""
    out = (ctypes.c_int32 * 8)()
    L = load_library()
    L.mj_debug_fused_shape.argtypes = [ctypes.c_int32] * 10 + [ctypes.POINTER(ctypes.c_int32)]
    if L.mj_debug_fused_shape(cus, n_ac, n_dc, ac_slot_bytes, hmax, vmax, int(transposed), n_images, segments_per_image, want_consumers, out) != MJ_OK:
        raise ValueError("mj_debug_fused_shape: bad arguments")
    return dict(zip(("ok", "images_per_wg", "producers", "lanes", "consumers", "producer_lds", "passes", "workgroups"),
                    (bool(out[0]),) + tuple(int(x) for x in out[1:])))


def fused_applies_rule(layout, hmax, vmax, mcus_per_row, mcu_rows, restart_interval, n_images=1024, ncomp=3, traits=0, flags=0):
    """mj_debug_fused_applies (host only): 0 the two launches, 1 one fused launch, 2 fused with the hand-off across workgroups."""
    L = load_library()
    out = ctypes.c_int32(-1)
    L.mj_debug_fused_applies.argtypes = [ctypes.c_int32] * 8 + [ctypes.c_uint32] * 2 + [ctypes.POINTER(ctypes.c_int32)]
    if L.mj_debug_fused_applies(layout, ncomp, hmax, vmax, mcus_per_row, mcu_rows, restart_interval, n_images, traits, flags, ctypes.byref(out)) != MJ_OK:
        raise ValueError("mj_debug_fused_applies: bad arguments")
    return out.value


def prog_split_rule(n_images, scans, mode=1, n_bands=68, wave_slots=0, parts=0):
    """mj_debug_prog_split (host only): (split flags per scan, parts per band) for a progressive batch whose scans are
    (image, restart segments, entropy-coded bytes or -1 where the scan is no refining AC scan of one component)."""
    n = len(scans)
    img = np.asarray([s[0] for s in scans], dtype=np.int32)
    seg = np.asarray([s[1] for s in scans], dtype=np.int32)
    byt = np.asarray([s[2] for s in scans], dtype=np.int64)
    out = np.zeros(max(n, 1), dtype=np.uint8)
    po = ctypes.c_int32()
    L = load_library()
    L.mj_debug_prog_split.argtypes = [ctypes.c_int32] * 6 + [ctypes.c_void_p] * 4 + [ctypes.POINTER(ctypes.c_int32)]
    if L.mj_debug_prog_split(mode, n_images, n_bands, wave_slots, parts, n, _ptr(img), _ptr(seg), _ptr(byt), _ptr(out), ctypes.byref(po)) != MJ_OK:
        raise ValueError("mj_debug_prog_split: bad arguments")
    return out[:n].astype(bool).tolist(), int(po.value)


def filter_id(filter) -> int:
    """MJ_FILTER_* from that number or the filter's name (ValueError otherwise); None is bilinear."""
    if filter is None:
        return MJ_FILTER_BILINEAR
    if isinstance(filter, str) and filter in FILTERS:
        return FILTERS[filter]
    if isinstance(filter, (int, np.integer)) and not isinstance(filter, bool) and int(filter) in FILTERS.values():
        return int(filter)
    raise ValueError(f"filter must be one of {', '.join(FILTERS)} (or its MJ_FILTER_* number), not {filter!r}")


def resize_table(in_size: int, out_size: int, filter=None):
    """mj_host_resize_table (host only): (xmin[out_size], count[out_size], taps[out_size, ksize]) int32 — one axis of the
    resize of ``decode(..., size=...)`` as the library builds it (tools/resize_model.py: axis_table).  ``filter``: a name of
    FILTERS or an MJ_FILTER_* — mj_host_resize_table_filtered's table for that filter (None: the bilinear one, through the
    function that was there before the filters)."""
    L = load_library()
    ks = ctypes.c_int32()
    if filter is None:
        fn, call = "mj_host_resize_table", L.mj_host_resize_table
    else:
        fid = filter_id(filter)
        fn, call = "mj_host_resize_table_filtered", lambda *a: L.mj_host_resize_table_filtered(fid, *a)
    if call(in_size, out_size, None, None, None, 0, ctypes.byref(ks)) != MJ_OK:
        raise ValueError(f"{fn}: sizes must be 1..65535")
    xmin, count = np.zeros(out_size, dtype=np.int32), np.zeros(out_size, dtype=np.int32)
    taps = np.zeros((out_size, ks.value), dtype=np.int32)
    if call(in_size, out_size, _ptr(xmin), _ptr(count), _ptr(taps), ks.value, ctypes.byref(ks)) != MJ_OK:
        raise ValueError(f"{fn}: bad arguments")
    return xmin, count, taps


def resize_table_boxed(in_size: int, out_size: int, box, filter=None):
    """mj_host_resize_table_boxed (host only): :func:`resize_table` over the part ``box`` = (in0, in1) of the axis, which the
    function rounds to 32-bit floats — the resample behind a reduce (tools/reduce_model.py: axis_table)."""
    L = load_library()
    ks = ctypes.c_int32()
    fid = filter_id(filter)
    if L.mj_host_resize_table_boxed(fid, in_size, float(box[0]), float(box[1]), out_size, None, None, None, 0, ctypes.byref(ks)) != MJ_OK:
        raise ValueError("mj_host_resize_table_boxed: sizes must be 1..65535 and the box inside the axis")
    xmin, count = np.zeros(out_size, dtype=np.int32), np.zeros(out_size, dtype=np.int32)
    taps = np.zeros((out_size, ks.value), dtype=np.int32)
    if L.mj_host_resize_table_boxed(fid, in_size, float(box[0]), float(box[1]), out_size, _ptr(xmin), _ptr(count), _ptr(taps), ks.value,
                                    ctypes.byref(ks)) != MJ_OK:
        raise ValueError("mj_host_resize_table_boxed: bad arguments")
    return xmin, count, taps


def reduce_factors(src_w: int, src_h: int, dst_w: int, dst_h: int, gap: float):
    """mj_host_reduce_factors (host only): (fx, fy) of a two-step resize (tools/reduce_model.py: reduce_factors)."""
    fx, fy = ctypes.c_int32(), ctypes.c_int32()
    if load_library().mj_host_reduce_factors(src_w, src_h, dst_w, dst_h, float(gap), ctypes.byref(fx), ctypes.byref(fy)) != MJ_OK:
        raise ValueError("mj_host_reduce_factors: sizes must be 1..65535 and the gap a finite number >= 1.0")
    return fx.value, fy.value


def reduce(a: np.ndarray, fx: int, fy: int, phase_x: int = 0, phase_y: int = 0) -> np.ndarray:
    """mj_host_reduce (host only): the reduce kernel's arithmetic on a row-major uint8 (H, W) or (H, W, 3) array
    (tools/reduce_model.py: reduce)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    h, w = a.shape[:2]
    nc = a.shape[2] if a.ndim == 3 else 1
    out = np.empty((-(-h // fy), -(-w // fx)) + a.shape[2:], dtype=np.uint8)
    if load_library().mj_host_reduce(_ptr(a), w, h, nc, fx, fy, phase_x, phase_y, _ptr(out)) != MJ_OK:
        raise ValueError("mj_host_reduce: bad arguments")
    return out


def affine(a: np.ndarray, matrix, filter="nearest", fill=0, window=None) -> np.ndarray:
    """mj_host_affine (host only): the affine launch's arithmetic on a row-major uint8 (H, W) or (H, W, 3) array — the window
    (x, y, width, height) (None: all) of Image.transform(size, AFFINE, matrix, filter, fillcolor=fill) (tools/affine_model.py)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    h, w = a.shape[:2]
    nc = a.shape[2] if a.ndim == 3 else 1
    x0, y0, ww, wh = window if window is not None else (0, 0, w, h)
    fb = np.zeros(3, dtype=np.uint8)
    fb[:] = fill
    out = np.empty((max(wh, 0), max(ww, 0)) + a.shape[2:], dtype=np.uint8)
    m = (ctypes.c_double * 6)(*[float(v) for v in matrix])
    fid = AFFINE_FILTERS.get(filter, filter) if isinstance(filter, str) else filter
    if not isinstance(fid, int) or load_library().mj_host_affine(_ptr(a), w, h, nc, m, fid, _ptr(fb), x0, y0, ww, wh, _ptr(out)) != MJ_OK:
        raise ValueError("mj_host_affine: bad arguments")
    return out


def perspective(a: np.ndarray, coeffs, filter="nearest", fill=0, window=None) -> np.ndarray:
    """mj_host_perspective (host only): the perspective launch's arithmetic on a row-major uint8 (H, W) or (H, W, 3) array — the
    window (x, y, width, height) (None: all) of Image.transform(size, PERSPECTIVE, coeffs, filter, fillcolor=fill)
    (tools/perspective_model.py)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    h, w = a.shape[:2]
    nc = a.shape[2] if a.ndim == 3 else 1
    x0, y0, ww, wh = window if window is not None else (0, 0, w, h)
    fb = np.zeros(3, dtype=np.uint8)
    fb[:] = fill
    out = np.empty((max(wh, 0), max(ww, 0)) + a.shape[2:], dtype=np.uint8)
    c = (ctypes.c_double * 8)(*[float(v) for v in coeffs])
    fid = AFFINE_FILTERS.get(filter, filter) if isinstance(filter, str) else filter
    if not isinstance(fid, int) or load_library().mj_host_perspective(_ptr(a), w, h, nc, c, fid, _ptr(fb), x0, y0, ww, wh, _ptr(out)) != MJ_OK:
        raise ValueError("mj_host_perspective: bad arguments")
    return out


def colour_ops(a: np.ndarray, chain) -> np.ndarray:
    """mj_host_colour_ops (host only): the colour launches' arithmetic on a row-major uint8 (H, W) or (H, W, 3) array — ``chain``
    applied to it as to a Pillow "L" / "RGB" image (tools/colour_model.py: apply_chain)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    h, w = a.shape[:2]
    nc = a.shape[2] if a.ndim == 3 else 1
    out = np.empty_like(a)
    c = colour_chain(chain)
    if load_library().mj_host_colour_ops(_ptr(a), w, h, nc, ctypes.byref(c), _ptr(out)) != MJ_OK:
        raise ValueError("mj_host_colour_ops: bad arguments")
    return out


def host_erase(a: np.ndarray, layout: int, dtype: str, ncomp: int, width: int, height: int, n_slots: int, rects, values=None,
               offset: int = 0) -> None:
    """mj_host_erase (host only): the erase launch's records over the host array ``a``, IN PLACE — ``a`` holds, from element
    ``offset`` on, ``n_slots`` slots of width x height pixels of ``ncomp`` components of ``dtype`` (bfloat16: uint16 bit patterns)
    in MJ_LAYOUT_* ``layout``; ``rects``: :func:`erase_rects`' records with the slot as output; ``values``: the array MJ_ERASE_VALUES
    offsets point into, elements of ``dtype``.  ValueError with the library's message for what it refuses."""
    if not a.flags["C_CONTIGUOUS"] or a.itemsize != DTYPE_BYTES[dtype]:
        raise ValueError("mj_host_erase: a contiguous array of the dtype's element size")
    L = load_library()
    arr, _keep = erase_rects(rects)
    base = ctypes.c_void_p(a.ctypes.data + int(offset) * a.itemsize)
    if L.mj_host_erase(base, int(layout), DTYPES[dtype], int(ncomp), int(width), int(height), int(n_slots), len(rects), arr,
                       _ptr(values)) != MJ_OK:
        raise ValueError(L.mj_last_error(None).decode())


def host_mix(src: np.ndarray, layout: int, dtype: str, ncomp: int, width: int, height: int, entries) -> np.ndarray:
    """mj_host_mix (host only): the mix launch's records over the host array ``src`` — one slot of width x height pixels of
    ``ncomp`` components of ``dtype`` (bfloat16: uint16 bit patterns) in MJ_LAYOUT_* ``layout`` per entry of ``entries``
    (:func:`mix_ops`') — into a new array of the same shape.  ValueError with the library's message for what it refuses."""
    if not src.flags["C_CONTIGUOUS"] or src.itemsize != DTYPE_BYTES[dtype]:
        raise ValueError("mj_host_mix: a contiguous array of the dtype's element size")
    L = load_library()
    dst = np.empty_like(src)
    ops, _keep = mix_ops(entries)
    if L.mj_host_mix(_ptr(src), _ptr(dst), int(layout), DTYPES[dtype], int(ncomp), int(width), int(height), len(entries), ops) != MJ_OK:
        raise ValueError(L.mj_last_error(None).decode())
    return dst


def host_compose(src: np.ndarray, layout: int, dtype: str, ncomp: int, src_size, dst_size, fill_bits, outputs, n_outputs: Optional[int] = None) -> np.ndarray:
    """mj_host_compose (host only): the compose launch's records over the host array ``src`` — ``len(src)`` slots of ``src_size`` =
    (width, height) pixels of ``ncomp`` components of ``dtype`` (bfloat16: uint16 bit patterns) in MJ_LAYOUT_* ``layout`` — into a
    new array of ``len(outputs)`` (or ``n_outputs``) slots of ``dst_size``; ``outputs``: :func:`compose_tiles`'; ``fill_bits``: one
    element bit pattern per component.  ValueError with the library's message for what it refuses."""
    if not src.flags["C_CONTIGUOUS"] or src.itemsize != DTYPE_BYTES[dtype]:
        raise ValueError("mj_host_compose: a contiguous array of the dtype's element size")
    L = load_library()
    (sw, sh), (dw, dh) = src_size, dst_size
    tiles, n_tiles, _keep = compose_tiles(outputs)
    m = int(n_outputs) if n_outputs is not None else len(outputs)
    dst = np.empty((max(m, 0), max(int(dw) * int(dh) * int(ncomp), 0)), dtype=src.dtype)
    if L.mj_host_compose(_ptr(src), _ptr(dst), int(layout), DTYPES[dtype], int(ncomp), int(sw), int(sh), len(src), int(dw), int(dh), m,
                         _fill_bits(fill_bits), n_tiles, tiles) != MJ_OK:
        raise ValueError(L.mj_last_error(None).decode())
    return dst


def host_compose_resolve(layout: int, ncomp: int, src_size, n_sources: int, dst_size, outputs, n_outputs: Optional[int] = None):
    """mj_host_compose_resolve (host only): (the rectangles the launch resolves ``outputs`` into, as an array of COMPOSE_RECT_DTYPE
    records; the capacity the library reports as always sufficient).  ValueError with the library's message for what it refuses."""
    L = load_library()
    (sw, sh), (dw, dh) = src_size, dst_size
    tiles, n_tiles, _keep = compose_tiles(outputs)
    m = int(n_outputs) if n_outputs is not None else len(outputs)
    args = (int(layout), int(ncomp), int(sw), int(sh), int(n_sources), int(dw), int(dh), m, n_tiles, tiles)
    cap = ctypes.c_int32()
    if L.mj_host_compose_resolve(*args, None, 0, ctypes.byref(cap)) != MJ_OK:
        raise ValueError(L.mj_last_error(None).decode())
    rects = np.zeros(cap.value, dtype=COMPOSE_RECT_DTYPE)
    n = ctypes.c_int32()
    if L.mj_host_compose_resolve(*args, _ptr(rects), cap.value, ctypes.byref(n)) != MJ_OK:
        raise ValueError(L.mj_last_error(None).decode())
    return rects[:n.value].copy(), cap.value


def host_patchify_count(layout: int, dtype: str, ncomp: int, src_size, n_sources: int, spec) -> int:
    """mj_host_patchify_count (host only): the token rows the patchify launch writes for ``spec`` — a dict ``patch``, ``merge``,
    ``repeat``, ``order``, ``length``, ``windows`` (every entry four integers, or ``windows`` None) — over ``n_sources`` slots of
    ``src_size`` = (width, height).  ValueError with the library's message, which names the source, for what it refuses."""
    L = load_library()
    win, _keep = patch_windows(spec.get("windows"), n_sources)
    rows = ctypes.c_int64()
    if L.mj_host_patchify_count(int(layout), DTYPES[dtype], int(ncomp), int(src_size[0]), int(src_size[1]), int(n_sources), *_patch_args(spec), win,
                                ctypes.byref(rows)) != MJ_OK:
        raise ValueError(L.mj_last_error(None).decode())
    return rows.value


def host_patchify(src: np.ndarray, layout: int, dtype: str, ncomp: int, src_size, spec, dst: Optional[np.ndarray] = None) -> np.ndarray:
    """mj_host_patchify (host only): the patchify launch's jobs over the host array ``src`` — ``len(src)`` slots of ``src_size`` =
    (width, height) pixels of ``ncomp`` components of ``dtype`` (bfloat16: uint16 bit patterns) in MJ_LAYOUT_* ``layout`` — into a
    new (rows, D) array, or into ``dst``, which holds exactly that.  ValueError with the library's message for what it refuses."""
    if not src.flags["C_CONTIGUOUS"] or src.itemsize != DTYPE_BYTES[dtype]:
        raise ValueError("mj_host_patchify: a contiguous array of the dtype's element size")
    L = load_library()
    patch, merge, repeat, order, length = _patch_args(spec)
    if dst is None:
        rows = host_patchify_count(layout, dtype, ncomp, src_size, len(src), spec)
        dst = np.empty((rows, int(ncomp) * repeat * patch * patch), dtype=src.dtype)
    win, _keep = patch_windows(spec.get("windows"), len(src))
    if L.mj_host_patchify(_ptr(src), _ptr(dst), int(layout), DTYPES[dtype], int(ncomp), int(src_size[0]), int(src_size[1]), len(src), patch, merge, repeat,
                          order, length, win) != MJ_OK:
        raise ValueError(L.mj_last_error(None).decode())
    return dst


class DeviceBytes:
    """A block of device memory of the HIP runtime's own (hipMalloc), filled from a host array: what the NumPy route keeps the values
    of ``erase=`` and the arrays of ``mix=`` in — no torch there.  ``ptr`` is the device address; close() frees it."""

    def __init__(self, host: np.ndarray, nbytes: Optional[int] = None):
        """``host`` None: ``nbytes`` uninitialised bytes"""
        load_library()                          # (the runtime libmijpeg.so bound to is the process's)
        self._hip = ctypes.CDLL("libamdhip64.so")
        self._hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self._hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self._hip.hipFree.argtypes = [ctypes.c_void_p]
        host = np.ascontiguousarray(host) if host is not None else np.empty(0, np.uint8)
        p = ctypes.c_void_p()
        if self._hip.hipMalloc(ctypes.byref(p), max(16, host.nbytes, nbytes or 0)) != 0:
            raise BackendError("hipMalloc failed for a block of device memory (DeviceBytes)")
        self.ptr = p.value
        if host.nbytes and self._hip.hipMemcpy(p, _ptr(host), host.nbytes, 1) != 0:       # hipMemcpyHostToDevice
            self.close()
            raise BackendError("hipMemcpy to the device failed (DeviceBytes)")

    def download(self, out: np.ndarray) -> np.ndarray:
        """the block's first ``out.nbytes`` bytes into the contiguous host array ``out`` (a blocking copy, behind everything queued)"""
        if self._hip.hipDeviceSynchronize() != 0 or self._hip.hipMemcpy(_ptr(out), ctypes.c_void_p(self.ptr), out.nbytes, 2) != 0:    # hipMemcpyDeviceToHost
            raise BackendError("hipMemcpy to the host failed")
        return out

    def close(self):
        if getattr(self, "ptr", None):
            self._hip.hipFree(ctypes.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def normalize_table(dtype: str, mean: float = 0.0, std: float = 1.0) -> np.ndarray:
    """mj_host_normalize_table (host only): the 256 bit patterns (uint16 for "float16" / "bfloat16", uint32 for "float32") one
    component's resized bytes 0..255 are stored as with this mean and std (tools/normalize_model.py: table_bits)."""
    if dtype not in DTYPES or dtype == "uint8":
        raise ValueError(f"mj_host_normalize_table: no float dtype {dtype!r}")
    out = np.zeros(256, dtype=np.uint32 if dtype == "float32" else np.uint16)
    if load_library().mj_host_normalize_table(DTYPES[dtype], float(mean), float(std), _ptr(out)) != MJ_OK:
        raise ValueError("mj_host_normalize_table: mean must be finite, std finite and > 0")
    return out


def mode_id(mode) -> int:
    """MJ_MODE_* from that number or the mode's name (ValueError otherwise); None is MJ_MODE_NATIVE."""
    if mode is None:
        return MJ_MODE_NATIVE
    if isinstance(mode, str) and mode in MODES:
        return MODES[mode]
    if isinstance(mode, (int, np.integer)) and not isinstance(mode, bool) and int(mode) in (MJ_MODE_NATIVE, MJ_MODE_L, MJ_MODE_RGB):
        return int(mode)
    raise ValueError(f"mode must be one of {', '.join(MODES)} (or its MJ_MODE_* number), not {mode!r}")


def convert_mode(a: np.ndarray, mode) -> np.ndarray:
    """mj_host_convert_mode (host only): uint8 pixels ``a`` — (..., 3) colour, or any other shape greyscale — in ``mode`` ("L",
    "RGB", None or an MJ_MODE_*): the host twin of the kernels' conversion (tools/mode_model.py: convert)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    mid = mode_id(mode)
    nc = 3 if a.ndim >= 2 and a.shape[-1] == 3 else 1
    pix = a.shape[:-1] if nc == 3 else a.shape
    co = mid or nc
    out = np.empty(tuple(pix) + ((3,) if co == 3 else ()), dtype=np.uint8)
    if load_library().mj_host_convert_mode(mid, _ptr(a), nc, int(np.prod(pix, dtype=np.int64)), _ptr(out)) != MJ_OK:
        raise ValueError("mj_host_convert_mode: bad arguments")
    return out


def exif_orientations(files, n_threads: int = 0) -> np.ndarray:
    """mj_host_exif_orientations (host only): the EXIF Orientation tag (1..8) of every file of a list of ``bytes``, uint8 — what
    ``_parse.exif_orientation`` answers for each, read on host threads."""
    n = len(files)
    out = np.ones(n, dtype=np.uint8)
    if n == 0:
        return out
    if not all(type(f) is bytes for f in files):
        from ._parse import exif_orientation
        out[:] = [exif_orientation(bytes(f)) for f in files]
        return out
    sizes = np.fromiter(map(len, files), dtype=np.int64, count=n)
    ptrs = (ctypes.c_char_p * n)(*files)
    if n_threads <= 0:
        import os
        n_threads = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
    if load_library().mj_host_exif_orientations(ctypes.cast(ptrs, ctypes.c_void_p), None, None, _ptr(sizes), n, n_threads, _ptr(out)) != MJ_OK:
        raise BackendError("mj_host_exif_orientations failed")
    return out


def output_desc(output):
    """(mj_output_desc, what it points to) from (dtype name, mean or None, std or None, mirror flags or None) — mean and std
    one float per component."""
    dtype, mean, std, mirror = output
    d = OutputDescC()
    d.dtype = DTYPES[dtype]
    d.normalize = 0 if mean is None else 1
    for c in range(3):
        d.mean[c] = float(mean[min(c, len(mean) - 1)]) if mean is not None else 0.0
        d.std[c] = float(std[min(c, len(std) - 1)]) if std is not None else 1.0
    flags = None
    if mirror is not None:
        flags = np.ascontiguousarray(mirror, dtype=np.uint8)
        d.mirror = flags.ctypes.data if flags.size else None
    return d, flags


def plan_request(n_images, rois=None, size=None, slots=None, output=None, orientation=None, filter=None, mode=None, places=None,
                 fill=None, reducing_gap=None, views=None, affine=None, colour=None, perspective=None):
    """(mj_plan_request, the arrays it points to) for a batch of ``n_images`` from Plan's keywords: every keyword is one field of
    the request (include/mijpeg.h), None its default.  Pure: no library, no context.  ValueError for what only a sized or placed
    plan has and for a per-image list that has not one entry for each image (with ``views``: places and the mirror flags have one
    for each view)."""
    if size is None and views is not None:
        raise ValueError("views needs size: only a resized plan has several outputs per image")
    if size is None and affine is not None:
        raise ValueError("affine needs size: only a resized plan reads the transformed images")
    if size is None and perspective is not None:
        raise ValueError("perspective needs size: only a resized plan reads the transformed images")
    if affine is not None and perspective is not None:
        raise ValueError("affine and perspective do not go together: the request's one field names one of them")
    if size is None and colour is not None:
        raise ValueError("colour needs size: only a resized plan has a canvas the operations work on")
    if size is None and (places is not None or filter is not None or output is not None):
        raise ValueError("places, filter and output need size: only a resized plan has a canvas, resamples and has a dense output")
    if size is None and reducing_gap is not None:
        raise ValueError("reducing_gap needs size: only a resized plan resamples, in one step or two")
    if fill is not None and places is None:
        raise ValueError("fill needs places: only a placed plan has canvas elements no image covers")
    keep = {}
    r = PlanRequestC()
    if rois is not None:
        keep["rois"] = r.rois = (RoiC * max(1, len(rois)))(*[RoiC(*(int(v) for v in w)) for w in rois])
    if orientation is not None:
        keep["orientations"] = turns = np.ascontiguousarray(orientation, dtype=np.uint8)
        r.orientations = turns.ctypes.data
    r.mode, r.filter = mode_id(mode), filter_id(filter)
    if reducing_gap is not None:
        r.reducing_gap = float(reducing_gap)
    if size is not None:
        r.out_width, r.out_height = int(size[0]), int(size[1])
    if slots is not None:
        keep["slots"] = sl = np.ascontiguousarray(slots[0], dtype=np.int32)
        r.slots, r.n_slots = sl.ctypes.data, int(slots[1])
    if output is not None:
        keep["output"], keep["mirror"] = output_desc(output)
        r.output = ctypes.pointer(keep["output"])
    if places is not None:
        keep["places"] = r.places = (PlaceC * max(1, len(places)))(*[PlaceC(*(int(v) for v in pl)) for pl in places])
    if fill is not None:
        keep["fill"] = fb = np.zeros(3, dtype=np.uint8)
        fb[:len(fill)] = fill
        r.fill = fb.ctypes.data
    if views is not None:
        keep["views"] = r.views = (ViewC * max(1, len(views)))(*[ViewC(int(i), RoiC(*(int(v) for v in (w if w is not None else (0, 0, 0, 0)))))
                                                                 for i, w in views])
        r.n_views = len(views)
    # affine: (matrices: one 6-tuple or None per output, a name of AFFINE_FILTERS or its MJ_AFFINE_*, the fill bytes);
    # perspective: (coefficients: one 8-tuple or None per output, the filter and the fill bytes as affine's)
    for name, given, entry, width in (("affine", affine, AffineC, 6), ("perspective", perspective, PerspectiveC, 8)):
        if given is not None:
            entries, filter_name, fb = given
            keep[name] = (entry * max(1, len(entries)))(*[entry((ctypes.c_double * width)(*(e if e is not None else (0.0,) * width))) for e in entries])
            setattr(r, name, keep[name])
            r.transform_filter = AFFINE_FILTERS[filter_name] if isinstance(filter_name, str) else int(filter_name)
            r.transform_fill[:] = (tuple(int(v) for v in fb) + (0, 0, 0))[:3]
    if colour is not None:      # (one chain — None or a sequence of ops — per output)
        keep["colour"] = r.colour = (ColourChainC * max(1, len(colour)))(*[colour_chain(c) for c in colour])
    for name, given in (("affine", affine[0] if affine is not None else None),
                        ("perspective", perspective[0] if perspective is not None else None), ("colour", colour),
                        ("places", places), ("orientation", orientation), ("mirror", keep.get("mirror"))):
        per_view = views is not None and name != "orientation"
        if given is not None and len(given) != (len(views) if per_view else n_images):
            raise ValueError(f"{name}: {len(given)} entries, not one for each of the {len(views) if per_view else n_images} {'views' if per_view else 'images'}")
    return r, keep


class UnknownOption(ValueError):
    """mj_set_option / mj_get_option: no such option in this library."""


def get_option(name: str) -> str:
    """mj_get_option: the value an option holds, "" = the default."""
    buf = ctypes.create_string_buffer(64)
    if load_library().mj_get_option(name.encode(), buf, 64) != MJ_OK:
        raise UnknownOption(f"libmijpeg has no option {name!r}")
    return buf.value.decode()


def set_option(name: str, value=None):
    """mj_set_option: a test / tuning switch of the library, process-wide (the library does not read the environment for
    these).  value None = back to the default.  UnknownOption for a name the library does not have, ValueError for a value
    outside the option's range (the option keeps what it had)."""
    get_option(name)
    rc = load_library().mj_set_option(name.encode(), None if value is None else str(value).encode())
    if rc != MJ_OK:
        raise ValueError(f"libmijpeg: {value!r} is outside what option {name} takes (include/mijpeg.h)")


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Context:
    """mj_context: one per GPU per thread."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.mj_create(device, ctypes.byref(h))
        if rc != MJ_OK:
            raise BackendError(self.lib.mj_last_error(None).decode() or f"mj_create failed ({rc})")
        self.handle = h
        self.device = device

    def check(self, rc: int):
        if rc != MJ_OK:
            msg = self.lib.mj_last_error(self.handle).decode()
            if rc == MJ_ERR_UNSUPPORTED:
                from .errors import UnsupportedJpeg
                raise UnsupportedJpeg(msg)
            raise BackendError(f"libmijpeg error {rc}: {msg}")

    def wait_event(self, hip_event: int):
        """Everything queued on the context's stream from now on runs after `hip_event` (a hipEvent_t handle, e.g.
        ``torch.cuda.Event.cuda_event``) has happened."""
        self.check(self.lib.mj_context_wait_event(self.handle, hip_event))

    def mix(self, src: int, dst: int, layout: int, dtype: str, ncomp: int, width: int, height: int, entries, stream: int = 0):
        """mj_mix: one launch on ``stream`` (0: the context's) that writes the ``len(entries)`` slots at device address ``dst`` from
        those at ``src`` — entry k (:func:`mix_ops`') says what output k becomes: a copy, a MixUp with its partner, a CutMix box
        from it.  BackendError with the library's message, which names the output, for what it refuses."""
        ops, _keep = mix_ops(entries)
        self.check(self.lib.mj_mix(self.handle, stream or None, src, dst, int(layout), DTYPES[dtype], int(ncomp), int(width), int(height),
                                   len(entries), ops))

    def time_mix(self, src: int, dst: int, layout: int, dtype: str, ncomp: int, width: int, height: int, entries, iters: int = 10) -> float:
        """ms per mix launch alone, on the context's stream (mj_mix_time)."""
        ms = ctypes.c_float()
        ops, _keep = mix_ops(entries)
        self.check(self.lib.mj_mix_time(self.handle, iters, src, dst, int(layout), DTYPES[dtype], int(ncomp), int(width), int(height),
                                        len(entries), ops, ctypes.byref(ms)))
        return ms.value

    def compose(self, src: int, dst: int, layout: int, dtype: str, ncomp: int, src_size, n_sources: int, dst_size, fill_bits, outputs,
                stream: int = 0, n_outputs: Optional[int] = None):
        """mj_compose: one launch on ``stream`` (0: the context's) that writes the ``len(outputs)`` (or ``n_outputs``) canvases of
        ``dst_size`` = (width, height) at device address ``dst`` from the ``n_sources`` slots of ``src_size`` at ``src`` — ``outputs``:
        :func:`compose_tiles`', ``fill_bits``: one element bit pattern per component.  BackendError with the library's message, which
        names the tile, for what it refuses."""
        tiles, n_tiles, _keep = compose_tiles(outputs)
        m = int(n_outputs) if n_outputs is not None else len(outputs)
        self.check(self.lib.mj_compose(self.handle, stream or None, src, dst, int(layout), DTYPES[dtype], int(ncomp), int(src_size[0]), int(src_size[1]),
                                       int(n_sources), int(dst_size[0]), int(dst_size[1]), m, _fill_bits(fill_bits), n_tiles, tiles))

    def time_compose(self, src: int, dst: int, layout: int, dtype: str, ncomp: int, src_size, n_sources: int, dst_size, fill_bits, outputs,
                     iters: int = 10) -> float:
        """ms per compose launch alone, on the context's stream (mj_compose_time)."""
        ms = ctypes.c_float()
        tiles, n_tiles, _keep = compose_tiles(outputs)
        self.check(self.lib.mj_compose_time(self.handle, iters, src, dst, int(layout), DTYPES[dtype], int(ncomp), int(src_size[0]), int(src_size[1]),
                                            int(n_sources), int(dst_size[0]), int(dst_size[1]), len(outputs), _fill_bits(fill_bits), n_tiles, tiles,
                                            ctypes.byref(ms)))
        return ms.value

    def patchify(self, src: int, dst: int, layout: int, dtype: str, ncomp: int, src_size, n_sources: int, spec, stream: int = 0):
        """mj_patchify: one launch on ``stream`` (0: the context's) that writes the token rows of ``spec`` (as
        :func:`host_patchify_count` takes it) at device address ``dst`` — exactly rows x D elements — from the ``n_sources`` slots of
        ``src_size`` = (width, height) at ``src``.  BackendError with the library's message, which names the source, for what it
        refuses."""
        win, _keep = patch_windows(spec.get("windows"), n_sources)
        self.check(self.lib.mj_patchify(self.handle, stream or None, src, dst, int(layout), DTYPES[dtype], int(ncomp), int(src_size[0]), int(src_size[1]),
                                        int(n_sources), *_patch_args(spec), win))

    def time_patchify(self, src: int, dst: int, layout: int, dtype: str, ncomp: int, src_size, n_sources: int, spec, iters: int = 10) -> float:
        """ms per patchify launch alone, on the context's stream (mj_patchify_time)."""
        ms = ctypes.c_float()
        win, _keep = patch_windows(spec.get("windows"), n_sources)
        self.check(self.lib.mj_patchify_time(self.handle, iters, src, dst, int(layout), DTYPES[dtype], int(ncomp), int(src_size[0]), int(src_size[1]),
                                             int(n_sources), *_patch_args(spec), win, ctypes.byref(ms)))
        return ms.value

    def cache_stats(self):
        """mj_debug_cache_stats: (blocks handed out now, their bytes, requests so far, running hash of the requested sizes)."""
        out = (ctypes.c_uint64 * 4)()
        self.check(self.lib.mj_debug_cache_stats(self.handle, out))
        return tuple(int(v) for v in out)

    def copy_rate_gbs(self, nbytes: int = 1 << 31, iters: int = 5) -> float:
        """mj_device_copy_rate: GB/s (read + written) of a plain 16-bytes-per-lane device copy of `nbytes`."""
        ms = ctypes.c_float()
        self.lib.mj_device_copy_rate.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        self.check(self.lib.mj_device_copy_rate(self.handle, int(nbytes), int(iters), ctypes.byref(ms)))
        return 2.0 * (int(nbytes) & ~15) / (ms.value * 1e-3) / 1e9

    def launch_clock(self):
        """mj_context_launch_clock: (shader MHz held during the latest fused launch, that launch's ms as workgroup 0 saw it)."""
        mhz, ms = ctypes.c_float(), ctypes.c_float()
        self.lib.mj_context_launch_clock.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        self.check(self.lib.mj_context_launch_clock(self.handle, ctypes.byref(mhz), ctypes.byref(ms)))
        return mhz.value, ms.value

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mj_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan:
    """mj_plan over a prepared batch (see batch.PreparedBatch).  The keywords are the fields of mj_plan_request (include/mijpeg.h
    specifies each there), None the field's default.  rois: one (x, y, width, height) per image — a window plan whose output for
    every image is that window.  size: (width, height) — a resized plan whose output is one dense array of every image (or
    window) at that size; slots: with size, (slot of every image, slots of the array) when the plan fills part of a larger array.
    output: with size, (dtype name, mean or None, std or None, mirror flag per image or None) — a model-ready output: elements of
    that type, normalised, flagged images mirrored; info.rgb_bytes is then in bytes of that type.  orientation: one EXIF
    orientation 1..8 per image — outputs as the orientation shows the images, rois in oriented coordinates.  filter: with size, a
    name of FILTERS / its MJ_FILTER_*: the resize with that resample filter.  mode: a name of MODES / its MJ_MODE_* — the
    components of the output; info.rgb_bytes, slots and image_offsets then count those.  places: with size — then the canvas —,
    one (width, height, x, y) per image: the size it is resized to and where it lies on the canvas; fill: with places, up to three
    bytes, one per output component.  reducing_gap: with size, a number >= 1.0 — the two-step resize, Pillow's argument of that name.
    views: with size, one (image, (x, y, width, height) or None) per OUTPUT — several windows of one decoded image; slots, the mirror
    flags and places then have one entry per view.  affine: with size, (matrices, filter, fill) — one 6-tuple or None per output, a
    name of AFFINE_FILTERS, up to three fill bytes: the affine transform in front of the windows and the resize.  perspective: the
    same with 8-tuples of coefficients, in affine's stead.  colour: with size,
    one chain (None or a sequence of ops, :func:`colour_chain`) per output: the colour operations on the finished canvas."""

    def __init__(self, ctx: Context, batch_c: BatchC, keepalive, rois=None, size=None, slots=None, output=None, orientation=None,
                 filter=None, mode=None, places=None, fill=None, reducing_gap=None, views=None, affine=None, colour=None, perspective=None):
        request, _ = plan_request(getattr(batch_c, "n_images", 0), rois, size, slots, output, orientation, filter, mode, places, fill,
                                  reducing_gap, views, affine, colour, perspective)
        self.ctx = ctx
        self._keep = keepalive
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.mj_plan_create_with(ctx.handle, ctypes.byref(batch_c), ctypes.byref(request), ctypes.byref(h)))
        self.handle = h
        info = PlanInfoC()
        ctx.check(ctx.lib.mj_plan_get_info(h, ctypes.byref(info)))
        self.info = info

    def derive(self, prep, **kwargs) -> "Plan":
        """mj_plan_derive: a plan of only the launches behind the decode — with a size, views, mode, filter, ... of its own, the
        keywords of :func:`plan_request`, ``size`` required and no ``rois`` — that reads THIS plan's decoded images.  ``prep``: the
        prepared batch this plan was made from (or its mj_batch).  Execute it behind an execute of this plan, on the same stream,
        and in front of this plan's next one; it holds this plan, so the two may be closed in either order."""
        batch_c = prep.to_c() if hasattr(prep, "to_c") else prep
        request, _ = plan_request(getattr(batch_c, "n_images", 0), **kwargs)
        child = Plan.__new__(Plan)
        child.ctx, child._keep, child.handle = self.ctx, dict(self._keep, prep=prep), None
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.mj_plan_derive(self.handle, ctypes.byref(batch_c), ctypes.byref(request), ctypes.byref(h)))
        child.handle = h
        child.info = PlanInfoC()
        self.ctx.check(self.ctx.lib.mj_plan_get_info(h, ctypes.byref(child.info)))
        return child

    def execute(self, stream: int = 0, rgb_device: int = 0):
        self.ctx.check(self.ctx.lib.mj_plan_execute(self.handle, stream or None, rgb_device or None))

    def execute_stage1(self, stream: int = 0):
        self.ctx.check(self.ctx.lib.mj_plan_execute_stage1(self.handle, stream or None))

    def execute_stage2(self, stream: int = 0, rgb_device: int = 0):
        self.ctx.check(self.ctx.lib.mj_plan_execute_stage2(self.handle, stream or None, rgb_device or None))

    def sync(self):
        self.ctx.check(self.ctx.lib.mj_plan_sync(self.handle))

    def stage1_form(self) -> int:
        """MJ_FORM_* (| MJ_FORM_WG_TABLES): which stage-1 form the library chose for this batch."""
        return int(self.ctx.lib.mj_plan_stage1_form(self.handle))

    def write_coef(self, coef: np.ndarray):
        coef = np.ascontiguousarray(coef, dtype=np.int16)
        assert coef.size == self.info.total_blocks * 64
        self.ctx.check(self.ctx.lib.mj_plan_write_coef(self.handle, _ptr(coef), MJ_MEM_HOST))

    def fill_coef(self, byte_value: int):
        """Test hook (mj_plan_fill_coef): poison the coefficient store."""
        self.ctx.check(self.ctx.lib.mj_plan_fill_coef(self.handle, int(byte_value)))

    def fill_source(self, byte_value: int):
        """Test hook (mj_plan_fill_source): poison a resized plan's intermediate buffer."""
        self.ctx.check(self.ctx.lib.mj_plan_fill_source(self.handle, int(byte_value)))

    def resize_shape(self) -> dict:
        """mj_debug_resize_shape: how a resized plan's launch is cut (tile_rows, tile_cols, tiles_x, tiles_y per image, lds_bytes),
        its filter (MJ_FILTER_*), whether it runs the signed instances, and the most taps a pixel has along an axis."""
        out = (ctypes.c_int32 * 8)()
        self.ctx.check(self.ctx.lib.mj_debug_resize_shape(self.handle, out))
        d = dict(zip(("tile_rows", "tile_cols", "tiles_x", "tiles_y", "lds_bytes", "filter", "signed", "max_ksize"), (int(v) for v in out)))
        d["signed"] = bool(d["signed"])
        return d

    def reduce_shape(self, image: int = 0) -> dict:
        """mj_debug_reduce_shape: the first step of a resized plan for one image, in the stored image's axes — the factors, the
        phases (size mod f along an axis the orientation reverses), the reduced size, and whether the plan reduces at all."""
        out = (ctypes.c_int32 * 7)()
        self.ctx.check(self.ctx.lib.mj_debug_reduce_shape(self.handle, int(image), out))
        d = dict(zip(("fx", "fy", "phase_x", "phase_y", "width", "height", "reduces"), (int(v) for v in out)))
        d["reduces"] = bool(d["reduces"])
        return d

    def reduce_launch(self) -> dict:
        """mj_debug_reduce_launch: how a reducing plan's reduce launch is cut — reduced rows and reduced pixels of a row per tile,
        tiles per image along the rows and along the contiguous axis, and the source pixels of a row a wavefront stages at a time."""
        out = (ctypes.c_int32 * 5)()
        self.ctx.check(self.ctx.lib.mj_debug_reduce_launch(self.handle, out))
        return dict(zip(("tile_slow", "tile_fast", "tiles_slow", "tiles_fast", "piece"), (int(v) for v in out)))

    def shape(self) -> list:
        """mj_debug_plan_shape: what plan creation decided, in the order include/mijpeg.h documents."""
        out = (ctypes.c_int32 * PLAN_SHAPE_WORDS)()
        self.ctx.check(self.ctx.lib.mj_debug_plan_shape(self.handle, out, PLAN_SHAPE_WORDS))
        return [int(v) for v in out]

    def time_resize(self, iters: int = 10, rgb_device: int = 0):
        """(ms per resize launch, bytes of un-resized pixels it reads) of a resized plan that has been executed."""
        ms, nb = ctypes.c_float(), ctypes.c_int64()
        self.ctx.check(self.ctx.lib.mj_plan_time_resize(self.handle, iters, rgb_device or None, ctypes.byref(ms), ctypes.byref(nb)))
        return ms.value, nb.value

    def time_affine(self, iters: int = 10):
        """(ms per affine — or perspective — launch, bytes it writes) of a plan with such a transform that has been executed
        (mj_plan_time_affine)."""
        ms, nb = ctypes.c_float(), ctypes.c_int64()
        self.ctx.check(self.ctx.lib.mj_plan_time_affine(self.handle, iters, ctypes.byref(ms), ctypes.byref(nb)))
        return ms.value, nb.value

    def time_colour(self, iters: int = 10):
        """(ms per run of the colour launches, bytes of one set of canvases) of a plan with colour operations that has been executed
        (mj_plan_time_colour)."""
        ms, nb = ctypes.c_float(), ctypes.c_int64()
        self.ctx.check(self.ctx.lib.mj_plan_time_colour(self.handle, iters, ctypes.byref(ms), ctypes.byref(nb)))
        return ms.value, nb.value

    def set_erase(self, rects, values_device: int = 0, keep=None):
        """mj_plan_set_erase: ``rects`` (:func:`erase_rects`' records; ``[]`` takes the erase off again) are what every execute from
        now on overwrites last; ``values_device``: the device address MJ_ERASE_VALUES offsets point into, elements of the plan's
        dtype — borrowed: ``keep`` (whatever owns that memory) is held by this plan until the next set_erase or close()."""
        arr, _keep = erase_rects(rects)
        self.ctx.check(self.ctx.lib.mj_plan_set_erase(self.handle, len(rects), arr, values_device or None))
        self._erase_keep = keep

    def time_erase(self, iters: int = 10):
        """(ms per run of the erase launches, bytes one run writes) of a plan with boxes set that has been executed (mj_plan_time_erase)."""
        ms, nb = ctypes.c_float(), ctypes.c_int64()
        self.ctx.check(self.ctx.lib.mj_plan_time_erase(self.handle, iters, ctypes.byref(ms), ctypes.byref(nb)))
        return ms.value, nb.value

    def time_reduce(self, iters: int = 10) -> float:
        """ms per reduce launch of a reducing plan that has been executed (mj_plan_time_reduce)."""
        ms = ctypes.c_float()
        self.ctx.check(self.ctx.lib.mj_plan_time_reduce(self.handle, iters, ctypes.byref(ms)))
        return ms.value

    def read(self, rgb=True, coef=False, planes=False, idct=False):
        out = {}
        a_rgb = np.empty(self.info.rgb_bytes, dtype=np.uint8) if rgb else None
        a_coef = np.empty((self.info.total_blocks, 64), dtype=np.int16) if coef else None
        a_pl = np.empty(self.info.rgb_bytes, dtype=np.int16) if planes else None
        a_id = np.empty((self.info.total_blocks, 64), dtype=np.int16) if idct else None
        n_images = self._keep["n_images"]
        st = np.zeros(n_images, dtype=np.int32)
        self.ctx.check(self.ctx.lib.mj_plan_read(self.handle, _ptr(a_rgb), _ptr(a_coef), _ptr(a_pl), _ptr(a_id), _ptr(st)))
        out.update(rgb=a_rgb, coef=a_coef, planes=a_pl, idct=a_id, status=st)
        return out

    def image_offsets(self, i: int):
        b, r = ctypes.c_int64(), ctypes.c_int64()
        self.ctx.check(self.ctx.lib.mj_plan_image_offsets(self.handle, i, ctypes.byref(b), ctypes.byref(r)))
        return b.value, r.value

    def device_buffers(self):
        c, r, p, d = (ctypes.c_void_p() for _ in range(4))
        self.ctx.check(self.ctx.lib.mj_plan_device_buffers(self.handle, ctypes.byref(c), ctypes.byref(r), ctypes.byref(p), ctypes.byref(d)))
        return {"coef": c.value, "rgb": r.value, "planes": p.value, "idct": d.value}

    def idct_levels(self):
        """(blocks, sent on by the fp32 level, sent on by the fp64 level) of the latest stage-2 execute with seam outputs."""
        c = (ctypes.c_uint64 * 3)()
        self.ctx.check(self.ctx.lib.mj_plan_idct_levels(self.handle, c))
        return int(c[0]), int(c[1]), int(c[2])

    def time_stages(self, iters: int = 10, rgb_device: int = 0):
        s1, s2 = ctypes.c_float(), ctypes.c_float()
        self.ctx.check(self.ctx.lib.mj_plan_time_stages(self.handle, iters, rgb_device or None, ctypes.byref(s1), ctypes.byref(s2)))
        return s1.value, s2.value

    def time_execute(self, iters: int = 10, rgb_device: int = 0):
        """(front_ms, main_ms) of the launches execute() makes: a fused plan's stage 0 and fused launch, else the two stages."""
        f, m = ctypes.c_float(), ctypes.c_float()
        self.ctx.check(self.ctx.lib.mj_plan_time_execute(self.handle, iters, rgb_device or None, ctypes.byref(f), ctypes.byref(m)))
        return f.value, m.value

    def tune_placement(self, stream: int = 0, rgb_device: int = 0, candidates: int = 4):
        """mj_plan_tune_placement: tries `candidates` coefficient stores for a fused plan that will be executed many times into
        `rgb_device` (then as many stage-0 stream buffers), keeps the fastest.  Returns (ms per execute of every store tried, index
        of the one that stayed); `best_ms` afterwards = ms per execute with what the plan ended up with."""
        ms = (ctypes.c_float * candidates)()
        chosen, best = ctypes.c_int32(), ctypes.c_float()
        self.ctx.lib.mj_plan_tune_placement.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                                        ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)]
        self.ctx.check(self.ctx.lib.mj_plan_tune_placement(self.handle, stream or None, rgb_device or None, candidates, ms, ctypes.byref(chosen),
                                                           ctypes.byref(best)))
        self.best_ms = float(best.value)
        return [float(x) for x in ms], int(chosen.value)

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.mj_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
