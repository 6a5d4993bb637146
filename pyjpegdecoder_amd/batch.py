"""Batched decode: many JPEG files -> one plan on one MI355X.

Python host code (header parsing + restart segmentation, `_parse.py`) prepares the arrays the C ABI
takes (`include/mijpeg.h`); all pixel work happens in libmijpeg.so's HIP kernels.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _binding as B
from ._parse import ParsedJpeg, ScanInfo, exif_orientation, parse_jpeg
from .errors import CorruptedJpeg, JpegError, UnsupportedJpeg

_STATUS_TEXT = {
    B.MJ_ST_BAD_CODE: "Failed to decode image (no Huffman code within 16 bits).",
    B.MJ_ST_OVERRUN: "Failed to decode image (a restart segment ends before its MCUs do).",
    B.MJ_ST_DESYNC: "Failed to decode image (restart markers are not where the restart interval puts them).",
}


def check_supported(p: ParsedJpeg) -> ScanInfo:
    """What the MI355X path accepts: one interleaved baseline scan covering all frame components, or a
    progressive file whose DC scans are interleaved (libjpeg's scripts) and whose AC scans are single-component."""
    if not p.scans:
        raise CorruptedJpeg("No scan found in the file.")
    if p.scan_mode == "progressive_dct":
        comps = list(p.color_components.values())
        if len(comps) > 1:
            hmax = max(c.horizontal_sampling for c in comps)
            vmax = max(c.vertical_sampling for c in comps)
            for c in comps:
                h, v = c.horizontal_sampling, c.vertical_sampling
                if (h, v) != (1, 1) and (h, v) != (hmax, vmax):
                    # the reference's final pass resizes every 8x8 block to the full MCU shape and stores it into a
                    # ratio x ratio region (jpeg_decoder.py:1345-1358): a shape mismatch for such a component (ValueError)
                    raise UnsupportedJpeg(f"Progressive files need every component at 1x1 or at the full resolution "
                                          f"(a {h}x{v} component under {hmax}x{vmax} is not supported).")
        for sc in p.scans:
            # the reference's own checks (jpeg_decoder.py:917-934, :966-967)
            if sc.spectral_start == 0 and sc.spectral_end != 0 or sc.spectral_start > sc.spectral_end:
                raise CorruptedJpeg("Progressive JPEG images cannot contain both DC and AC values in the same scan.")
            if sc.bit_high != 0 and sc.bit_high - sc.bit_low != 1:
                raise CorruptedJpeg("Progressive JPEG images cannot contain more than 1 bit for each value on a refining scan.")
            if sc.spectral_start > 0 and len(sc.component_ids) > 1:
                raise CorruptedJpeg("An AC progressive scan can only have a single color component.")
            if sc.spectral_start == 0 and len(sc.component_ids) == 1 and len(p.color_components) > 1:
                c = p.color_components[sc.component_ids[0]]
                if c.horizontal_sampling > 1 or c.vertical_sampling > 1:
                    raise UnsupportedJpeg("Single-component DC scan of a component with sampling > 1 "
                                          "(the reference steps such a scan's blocks by the component's MCU size, "
                                          "jpeg_decoder.py:993-994, and runs off its array: IndexError) is not supported.")
        return p.scans[0]
    if p.scan_mode != "baseline_dct":
        raise UnsupportedJpeg("Encoding mode not supported. Only 'Baseline DCT' and 'Progressive DCT' are supported.")
    if len(p.scans) == 1 and len(p.scans[0].component_ids) == len(p.color_components):
        return p.scans[0]
    # Non-interleaved baseline: one scan per component.  The reference only gets these right when no component is
    # subsampled (it assigns the resized MCU into an 8x8 slot otherwise, jpeg_decoder.py:882-891), so that is the scope.
    comps = p.color_components
    single = all(len(sc.component_ids) == 1 for sc in p.scans)
    once = sorted(sc.component_ids[0] for sc in p.scans) == sorted(comps) if single else False
    flat = all(c.horizontal_sampling == 1 and c.vertical_sampling == 1 for c in comps.values())
    if not (single and once and flat):
        raise UnsupportedJpeg("Baseline files with several scans are supported when every scan holds one component, "
                              "every component has one scan and no component is subsampled.")
    return p.scans[0]


def is_scan_list(p: ParsedJpeg) -> bool:
    """Files decoded scan by scan into the coefficient store (mj_batch.scans): progressive ones and baseline files
    with one scan per component."""
    return p.scan_mode == "progressive_dct" or len(p.scans) > 1


def _segments_of(scan: ScanInfo, off: int):
    """(begin[], end[]) blob offsets of a scan's restart segments; checks the marker count (:898 is count driven)."""
    so = scan.segment_offsets
    if so is None:          # headers-only parse: one byte range, the GPU segments it (MJ_FLAG_GPU_SEGMENT)
        return (np.array([scan.entropy_start + off], dtype=np.int64), np.array([scan.entropy_end + off], dtype=np.int64))
    if scan.restart_interval > 0:
        want = -(-scan.mcu_count // scan.restart_interval)
        if so.size - 1 != want:
            raise CorruptedJpeg(f"Failed to decode image ({so.size - 2} restart markers found, {want - 1} expected).")
        b = so[:-1].copy()
        e = np.concatenate([so[1:-1] - 2, so[-1:]])
    else:
        b = np.array([scan.entropy_start], dtype=np.int64)
        e = np.array([scan.entropy_end], dtype=np.int64)
    return b + off, e + off


@dataclass
class PreparedBatch:
    """Host-side arrays of one mj_batch (kept alive for the life of the plan)."""
    parsed: List[ParsedJpeg]
    blob: np.ndarray
    file_offsets: np.ndarray
    descs: ctypes.Array
    seg_begin: np.ndarray
    seg_end: np.ndarray
    huff: ctypes.Array
    n_huff: int
    qt: np.ndarray
    layout: int
    flags: int
    shapes: List[Tuple[int, int, int]] = field(default_factory=list)   # (W, H, ncomp)
    scans: Optional[ctypes.Array] = None                               # progressive batches: mj_scan_desc[]
    n_scans: int = 0

    def to_c(self, blob_device_ptr: int = 0) -> B.BatchC:
        b = B.BatchC()
        b.n_images = len(self.parsed)
        b.images = ctypes.cast(self.descs, ctypes.POINTER(B.ImageDescC))
        if blob_device_ptr:
            b.blob, b.blob_mem = blob_device_ptr, B.MJ_MEM_DEVICE
        else:
            b.blob, b.blob_mem = self.blob.ctypes.data, B.MJ_MEM_HOST
        b.blob_len = int(self.blob.size)
        b.n_segments = int(self.seg_begin.size)
        b.seg_begin, b.seg_end = self.seg_begin.ctypes.data, self.seg_end.ctypes.data
        b.n_huff = self.n_huff
        b.huff = ctypes.cast(self.huff, ctypes.POINTER(B.HuffSpecC))
        b.n_qt = self.qt.shape[0]
        b.qt = self.qt.ctypes.data
        b.layout, b.flags = self.layout, self.flags
        b.n_scans = self.n_scans
        b.scans = ctypes.cast(self.scans, ctypes.POINTER(B.ScanDescC)) if self.n_scans else None
        return b


def prepare_batch(files: Sequence[bytes], layout: int = B.MJ_LAYOUT_XMAJOR, flags: int = 0,
                  parsed: Optional[List[ParsedJpeg]] = None) -> PreparedBatch:
    """Parse every file and build the descriptor / table / segment arrays of include/mijpeg.h."""
    if parsed is None:
        parsed = [parse_jpeg(f) for f in files]
    n = len(parsed)
    sizes = np.array([len(p.raw) for p in parsed], dtype=np.int64)
    # keep every file 4-byte aligned inside the blob (stage 1 fetches aligned dwords)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum((sizes + 3) & ~3)
    # stage 1 reads up to 512 bytes ahead of a segment (mijpeg.h, mj_batch.blob_mem): keep 1 KiB of readable slack behind the last file
    blob = np.zeros(int(offs[-1]) + 1024, dtype=np.uint8)
    if parsed and any(p.headers_only for p in parsed):
        if not all(p.headers_only for p in parsed):
            raise UnsupportedJpeg("A batch is segmented either on the GPU (headers-only parse) or on the host; split it.")
        flags |= B.MJ_FLAG_GPU_SEGMENT
    descs = (B.ImageDescC * n)()
    huff_ids: Dict[bytes, int] = {}
    huff_list: List[Tuple[np.ndarray, np.ndarray]] = []
    qt_ids: Dict[bytes, int] = {}
    qt_list: List[np.ndarray] = []
    seg_b: List[np.ndarray] = []
    seg_e: List[np.ndarray] = []
    n_seg_total = 0
    shapes = []

    def huff_id(spec) -> int:
        key = spec.bits.tobytes() + spec.vals.tobytes()
        if key not in huff_ids:
            huff_ids[key] = len(huff_list)
            huff_list.append((spec.bits, spec.vals))
        return huff_ids[key]

    def qt_id(zz: np.ndarray) -> int:
        key = zz.tobytes()
        if key not in qt_ids:
            qt_ids[key] = len(qt_list)
            qt_list.append(zz.astype(np.uint16))
        return qt_ids[key]

    progressive = is_scan_list(parsed[0]) if parsed else False       # "progressive" = scan-list batch from here on
    scan_list: List[B.ScanDescC] = []
    for i, p in enumerate(parsed):
        scan = check_supported(p)
        if is_scan_list(p) != progressive:
            raise UnsupportedJpeg("A batch holds either single-scan baseline files or scan-by-scan (progressive / "
                                  "non-interleaved) files; split it.")
        blob[offs[i]:offs[i] + sizes[i]] = np.frombuffer(p.raw, dtype=np.uint8)
        d = descs[i]
        if progressive:
            comp_ids = list(p.color_components)
            d.width, d.height, d.ncomp = p.image_width, p.image_height, len(comp_ids)
            for c, cid in enumerate(comp_ids):
                comp = p.color_components[cid]
                d.hs[c], d.vs[c] = comp.horizontal_sampling, comp.vertical_sampling
                # baseline files decoded scan by scan dequantise each component with the table in force at ITS scan
                # (:869); progressive files with the tables in force at the final pass (:1348)
                qsrc = p.quantization_zz
                if p.scan_mode == "baseline_dct":
                    qsrc = next((sc.quantization_zz for sc in p.scans if cid in sc.component_ids and sc.quantization_zz), qsrc)
                if comp.quantization_table_id not in qsrc:
                    raise CorruptedJpeg("Scan uses a quantization table that the file does not define.")
                d.qt_sel[c] = qt_id(qsrc[comp.quantization_table_id])
            if d.ncomp == 1:
                d.hs[0] = d.vs[0] = 1
                mw = mh = 8
            else:
                mw, mh = 8 * max(d.hs[c] for c in range(3)), 8 * max(d.vs[c] for c in range(3))
            d.mcu_count_h, d.mcu_count_v = -(-p.image_width // mw), -(-p.image_height // mh)
            d.restart_interval, d.n_segments, d.first_segment = 0, 0, 0
            for sc in p.scans:
                sd = B.ScanDescC()
                sd.image, sd.n_comp = i, len(sc.component_ids)
                for k, cid in enumerate(sc.component_ids):
                    sd.comp[k] = comp_ids.index(cid)
                    tabs = sc.huffman_tables_id[cid]
                    need_dc, need_ac = sc.spectral_start == 0 and sc.bit_high == 0, sc.spectral_end > 0
                    if (need_dc and tabs.dc not in sc.huffman) or (need_ac and tabs.ac not in sc.huffman):
                        raise CorruptedJpeg("Scan uses a Huffman table that the file does not define.")
                    sd.dc_sel[k] = huff_id(sc.huffman[tabs.dc]) if need_dc else 0
                    sd.ac_sel[k] = huff_id(sc.huffman[tabs.ac]) if need_ac else 0
                sd.ss, sd.se, sd.ah, sd.al = sc.spectral_start, sc.spectral_end, sc.bit_high, sc.bit_low
                sd.restart_interval = sc.restart_interval
                sd.mcu_count_h, sd.mcu_count_v = sc.mcu_count_h, sc.mcu_count_v
                b_, e_ = _segments_of(sc, int(offs[i]))
                sd.n_segments, sd.first_segment = int(b_.size), n_seg_total
                n_seg_total += int(b_.size)
                seg_b.append(b_)
                seg_e.append(e_)
                scan_list.append(sd)
            shapes.append((p.image_width, p.image_height, d.ncomp))
            continue
        d.width, d.height, d.ncomp = p.image_width, p.image_height, len(scan.component_ids)
        if list(scan.component_ids) != list(p.color_components)[:len(scan.component_ids)]:
            # descriptors are filled by scan position and stage 2 takes position 0 for Y, 1 and 2 for Cb and Cr
            raise UnsupportedJpeg("The scan lists the color components in another order than the frame.")
        for c, cid in enumerate(scan.component_ids):
            comp = p.color_components[cid]
            d.hs[c], d.vs[c] = comp.horizontal_sampling, comp.vertical_sampling
            if comp.quantization_table_id not in p.quantization_zz:
                raise CorruptedJpeg("Scan uses a quantization table that the file does not define.")
            d.qt_sel[c] = qt_id(p.quantization_zz[comp.quantization_table_id])
            tabs = scan.huffman_tables_id[cid]
            if tabs.dc not in scan.huffman or tabs.ac not in scan.huffman:
                raise CorruptedJpeg("Scan uses a Huffman table that the file does not define.")
            d.dc_sel[c] = huff_id(scan.huffman[tabs.dc])
            d.ac_sel[c] = huff_id(scan.huffman[tabs.ac])
        if d.ncomp == 1:
            d.hs[0] = d.vs[0] = 1     # a single-component scan is always 8x8 MCUs (jpeg_decoder.py:595-598)
        d.restart_interval = scan.restart_interval
        d.mcu_count_h, d.mcu_count_v = scan.mcu_count_h, scan.mcu_count_v
        b, e = _segments_of(scan, int(offs[i]))
        d.n_segments = int(b.size)
        d.first_segment = n_seg_total
        n_seg_total += int(b.size)
        seg_b.append(b)
        seg_e.append(e)
        shapes.append((p.image_width, p.image_height, d.ncomp))

    huff = (B.HuffSpecC * max(1, len(huff_list)))()
    for k, (bits, vals) in enumerate(huff_list):
        huff[k].bits[:] = bits.tolist()
        v = np.zeros(256, dtype=np.uint8)
        v[:min(256, vals.size)] = vals[:256]
        huff[k].vals[:] = v.tolist()
    qt = np.ascontiguousarray(np.stack(qt_list), dtype=np.uint16)
    scans_c = (B.ScanDescC * len(scan_list))(*scan_list) if scan_list else None
    return PreparedBatch(scans=scans_c, n_scans=len(scan_list), parsed=parsed, blob=blob, file_offsets=offs, descs=descs,
                         seg_begin=np.ascontiguousarray(np.concatenate(seg_b), dtype=np.int64),
                         seg_end=np.ascontiguousarray(np.concatenate(seg_e), dtype=np.int64),
                         huff=huff, n_huff=len(huff_list), qt=qt, layout=layout, flags=flags, shapes=shapes)


# numpy view of mj_image_desc (include/mijpeg.h), to read what the native front end filled in without a Python loop
_DESC_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hs", "<i4", 3), ("vs", "<i4", 3),
                        ("qt_sel", "<i4", 3), ("dc_sel", "<i4", 3), ("ac_sel", "<i4", 3), ("restart_interval", "<i4"),
                        ("mcu_count_h", "<i4"), ("mcu_count_v", "<i4"), ("n_segments", "<i4"), ("first_segment", "<i8")])
assert _DESC_DTYPE.itemsize == ctypes.sizeof(B.ImageDescC)


def prepare_batch_native(files: Sequence[bytes], layout: int = B.MJ_LAYOUT_XMAJOR, flags: int = 0, n_threads: int = 0,
                         staging: Optional[np.ndarray] = None, split: bool = False):
    """`prepare_batch` for a GPU-segmented batch of everyday baseline files through libmijpeg.so's host front end
    (``mj_host_assemble``: header parse and assembly on host threads).  Returns None when the front end declines a file —
    the caller then takes the Python path, which also raises the reference's exceptions — and, when the files are fine but
    do not belong in one plan (several sampling layouts; files with and without restart markers), the groups they fall
    into as lists of indices.  ``split=True``: files the front end does not take do not sink the batch; the result is then
    ``(groups, declined)`` — index lists for the front end, grouped as above, and the indices left for the Python path.
    ``staging``: a uint8 buffer to build the blob in (reused between batches by BatchDecoder)."""
    n = len(files)
    if n == 0 or not all(type(f) is bytes for f in files):
        return None
    lib = B.load_library()
    sizes = np.fromiter(map(len, files), dtype=np.int64, count=n)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum((sizes + 3) & ~3, out=offs[1:])
    blob_len = int(offs[-1]) + 1024
    blob = staging[:blob_len] if staging is not None and staging.size >= blob_len else np.empty(blob_len, dtype=np.uint8)
    descs = (B.ImageDescC * n)()
    seg_b, seg_e = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    huff = (B.HuffSpecC * (6 * n))()
    qt = np.empty((3 * n, 64), dtype=np.uint16)
    job = B.HostJobC()
    job.n_files = n
    ptrs = (ctypes.c_char_p * n)(*files)
    job.files = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_char_p))
    job.sizes, job.file_off = sizes.ctypes.data, offs.ctypes.data
    job.blob, job.blob_len = blob.ctypes.data, blob_len
    job.images = ctypes.cast(descs, ctypes.POINTER(B.ImageDescC))
    job.seg_begin, job.seg_end = seg_b.ctypes.data, seg_e.ctypes.data
    job.huff, job.huff_cap = ctypes.cast(huff, ctypes.POINTER(B.HuffSpecC)), 6 * n
    job.qt, job.qt_cap = qt.ctypes.data, 3 * n
    if n_threads <= 0:
        import os
        n_threads = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
    job.n_threads = n_threads
    skip = np.zeros(n, dtype=np.uint8)
    if split:
        job.skip = skip.ctypes.data
    rc = lib.mj_host_assemble(ctypes.byref(job))
    if rc == B.MJ_HOST_DECLINED:
        return ([], list(range(n))) if split else None
    if rc != B.MJ_OK:
        raise B.BackendError(f"mj_host_assemble failed ({rc})")
    m = int(job.n_accepted)
    accepted = np.flatnonzero(skip == 0)
    d = np.frombuffer(descs, dtype=_DESC_DTYPE)[:m]
    lay = np.concatenate([d["ncomp"][:, None], d["hs"], d["vs"], (d["restart_interval"] > 0)[:, None]], axis=1)
    mixed = bool((lay != lay[0]).any())
    if mixed or m < n:
        # several sampling layouts, or files with and without restart markers (only a batch without any can be cut into
        # chunks when the GPU finds the markers): one plan each — the caller gets the groups (lists of file indices)
        _, inverse = np.unique(lay, axis=0, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        groups = [accepted[np.flatnonzero(inverse == g)].tolist() for g in range(int(inverse.max()) + 1)]
        return (groups, np.flatnonzero(skip).tolist()) if split else groups
    shapes = list(zip(d["width"].tolist(), d["height"].tolist(), d["ncomp"].tolist()))
    if split:
        return ([list(range(n))], [])         # (the caller assembles group by group; this pass only sorted the files)
    return PreparedBatch(parsed=[None] * n, blob=blob, file_offsets=offs, descs=descs, seg_begin=seg_b, seg_end=seg_e,
                         huff=huff, n_huff=int(job.n_huff), qt=np.ascontiguousarray(qt[:max(1, int(job.n_qt))]),
                         layout=layout, flags=flags | B.MJ_FLAG_GPU_SEGMENT, shapes=shapes)


def _image_info(raw: bytes) -> Tuple[int, int, int]:
    """(width, height, components) from a file's frame header (SOF0-SOF15 but DHT / JPG / DAC), walking the marker segments
    in front of it; anything unusual goes through the parser, which raises the reference's exceptions."""
    pos, n = 2, len(raw)
    if raw[:2] == b"\xFF\xD8":
        while pos + 10 <= n and raw[pos] == 0xFF:
            m = raw[pos + 1]
            if m == 0xFF:
                pos += 1
                continue
            seg = (raw[pos + 2] << 8) | raw[pos + 3]
            if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
                return (raw[pos + 7] << 8) | raw[pos + 8], (raw[pos + 5] << 8) | raw[pos + 6], raw[pos + 9]
            if m == 0xDA or seg < 2:
                break
            pos += 2 + seg
    p = parse_jpeg(raw, headers_only=True)
    return p.image_width, p.image_height, len(p.color_components)


def _image_dims(raw: bytes) -> Tuple[int, int]:
    """(width, height) of :func:`_image_info`."""
    return _image_info(raw)[:2]


def normalize_size(size) -> Optional[Tuple[int, int]]:
    """The (width, height) of a decode to a fixed size: None, or two positive integers (ValueError otherwise)."""
    if size is None:
        return None
    ok = isinstance(size, (tuple, list, np.ndarray)) and len(size) == 2 and all(
        isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in size)
    if not ok or int(size[0]) < 1 or int(size[1]) < 1 or int(size[0]) > 65535 or int(size[1]) > 65535:
        raise ValueError(f"size must be (width, height), two positive integers up to 65535, not {size!r}")
    return int(size[0]), int(size[1])


def normalize_reducing_gap(reducing_gap, size) -> Optional[float]:
    """``reducing_gap`` of a decode to a fixed size, checked: None (no first step), or a float >= 1.0 — Pillow's
    ``Image.resize(..., reducing_gap=)``.  It needs ``size``.  ValueError otherwise (below 1.0: Pillow's message) — also for a gap
    that a 32-bit float does not hold exactly: the plan request carries a float, and a rounded gap could give other factors than
    Pillow computes from the double (1.0, 1.5, 2.0, 3.0 and the like are exact)."""
    if reducing_gap is None:
        return None
    if size is None:
        raise ValueError("reducing_gap needs size=(width, height): without it nothing is resized")
    if isinstance(reducing_gap, (bool, np.bool_)) or not isinstance(reducing_gap, (int, float, np.integer, np.floating)):
        raise ValueError(f"reducing_gap must be None or a number 1.0 or greater, not {reducing_gap!r}")
    gap = float(reducing_gap)
    if not (gap >= 1.0 and math.isfinite(gap)):
        raise ValueError("reducing_gap must be 1.0 or greater")
    if float(np.float32(gap)) != gap:
        raise ValueError(f"reducing_gap {reducing_gap!r} is not exact as a 32-bit float, which is what the plan request carries; "
                         f"the nearest values that are: {float(np.float32(gap))!r}")
    return gap


# Pillow's Image.Resampling numbering of the convolution filters (0 is NEAREST)
_PILLOW_FILTERS = {1: "lanczos", 2: "bilinear", 3: "bicubic", 4: "box", 5: "hamming"}


def normalize_resample(resample, size) -> Optional[str]:
    """The resample filter of a decode to a fixed size, checked: None for the default — ``None``, "bilinear" or Pillow's
    ``Image.Resampling.BILINEAR`` / 2, which all are a call without the argument — else "box", "hamming", "bicubic" or "lanczos".
    ``resample``: such a name (in any case), the ``Image.Resampling`` member, or its integer value.  It needs ``size``.
    ValueError otherwise."""
    if resample is None:
        return None
    if size is None:
        raise ValueError("resample needs size=(width, height): without it nothing is resized")
    name = None
    if isinstance(resample, str):
        name = resample.lower()
    elif isinstance(resample, (int, np.integer)) and not isinstance(resample, (bool, np.bool_)):      # (Image.Resampling is an IntEnum)
        name = "nearest" if int(resample) == 0 else _PILLOW_FILTERS.get(int(resample))
    if name == "nearest":
        raise ValueError("resample: Pillow's NEAREST is not a convolution (it walks an affine transform) and is not offered; "
                         "the filters are bilinear, box, hamming, bicubic and lanczos")
    if name not in B.FILTERS:
        raise ValueError(f"resample must be one of {', '.join(B.FILTERS)} (a name, Pillow's Image.Resampling member or its integer "
                         f"value), not {resample!r}")
    return None if name == "bilinear" else name


def normalize_mode(mode) -> Optional[str]:
    """The output colour mode of a call, checked: None (every file in its own components: a call without the argument), "RGB"
    (three components: a greyscale file's value in all of them, Pillow's ``convert("RGB")``) or "L" (one: a colour file's
    ``convert("L")``, tools/mode_model.py).  ``mode``: None or one of these two names of Pillow's.  ValueError otherwise."""
    if mode is None:
        return None
    if not isinstance(mode, str) or mode not in B.MODES:
        raise ValueError(f"mode must be None or one of {', '.join(repr(m) for m in B.MODES)} (Pillow's mode names), not {mode!r}")
    return mode


def one_component_count(ncomps: Sequence[int]) -> int:
    """The component count the files of a decode to a fixed size share (they fill one array); ValueError naming the first file
    that differs from file 0.  No files at all: 3 — the empty result then has a colour batch's shape, (0, ..., 3)."""
    if not ncomps:
        return 3
    for i, nc in enumerate(ncomps):
        if nc != ncomps[0]:
            raise ValueError(f"file {i}: {nc} colour component(s) where file 0 has {ncomps[0]}: greyscale and colour files do "
                             f"not share one array; decode them in separate calls")
    return int(ncomps[0])


def dtype_name(dtype) -> str:
    """"uint8", "float16", "bfloat16" or "float32" from such a name or the torch.dtype / numpy.dtype object of that name
    (ValueError for anything else)."""
    name = dtype if isinstance(dtype, str) else None
    if name is None:
        text = str(dtype)
        if text.startswith("torch."):
            name = text[len("torch."):]
        else:
            try:
                name = np.dtype(dtype).name
            except TypeError:
                name = text
    if name not in B.DTYPES:
        raise ValueError(f"dtype must be one of {', '.join(B.DTYPES)} (a name, a torch.dtype or a numpy.dtype), not {dtype!r}")
    return name


@dataclass
class OutputSpec:
    """What a decode to a fixed size stores instead of the resized bytes (:func:`normalize_output`): elements of ``dtype``;
    ``mean`` / ``std`` one float per component, or both None (value / 255 for a float dtype); ``mirror`` one bool per file of
    the call, or None."""
    dtype: str
    mean: Optional[Tuple[float, ...]] = None
    std: Optional[Tuple[float, ...]] = None
    mirror: Optional[List[bool]] = None

    def for_files(self, idxs: Sequence[int]) -> "OutputSpec":
        """the same output for some files of the call: their flags go with them"""
        return OutputSpec(self.dtype, self.mean, self.std, [self.mirror[i] for i in idxs] if self.mirror is not None else None)

    def plan_output(self, idxs: Optional[Sequence[int]] = None):
        """``output`` of :class:`_binding.Plan` for a plan of these files (None: all, in order)"""
        return (self.dtype, self.mean, self.std, self.mirror if idxs is None else self.for_files(idxs).mirror)

    @property
    def numpy_dtype(self) -> np.dtype:
        return np.dtype(self.dtype)

    @property
    def torch_dtype(self):
        import torch
        return getattr(torch, self.dtype)


def normalize_output(dtype, normalize, mirror, size, n_files: Optional[int] = None, ncomp: Optional[int] = None,
                     host: bool = False) -> Optional[OutputSpec]:
    """The model-ready output of a decode to a fixed size, checked: None when the call asks for none (the resized bytes, as
    without these arguments), else an :class:`OutputSpec`.

    ``dtype``: None, "uint8", "float16", "bfloat16", "float32" or the torch / numpy dtype of that name (``host``: the NumPy
    route, which has no bfloat16).  ``normalize``: None or (mean, std), each one float or one per component (``ncomp``; a
    scalar stands for all), in units of value / 255; it needs a float dtype and makes a missing one "float32"; std > 0 and
    both finite as float32.  ``mirror``: None, one bool, or one bool per file (``n_files``).  All of them need ``size``.
    ``n_files`` / ``ncomp`` None: not known yet — everything but the lengths is checked.  ValueError otherwise."""
    if dtype is None and normalize is None and mirror is None:
        return None
    if size is None:
        raise ValueError("dtype, normalize and mirror need size=(width, height): without it the outputs are ragged and stay uint8 "
                         "(files that share one size: pass that size, which the resize leaves as it is)")
    name = dtype_name(dtype) if dtype is not None else ("float32" if normalize is not None else "uint8")
    if host and name == "bfloat16":
        raise ValueError("dtype bfloat16: NumPy has no such type; decode_device returns torch.bfloat16")
    mean = std = None
    if normalize is not None:
        if name == "uint8":
            raise ValueError("normalize needs a float dtype (float32, float16 or bfloat16), not uint8")
        if not isinstance(normalize, (tuple, list)) or len(normalize) != 2:
            raise ValueError(f"normalize must be (mean, std), not {normalize!r}")

        def per_component(what, v):
            if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool):
                vals = [float(v)] * (ncomp or 1)
            else:
                try:
                    vals = [float(x) for x in v]
                except (TypeError, ValueError):
                    raise ValueError(f"normalize: {what} must be one float or one per component, not {v!r}") from None
                if ncomp is not None and len(vals) != ncomp or not vals or len(vals) > 3:
                    raise ValueError(f"normalize: {what} has {len(vals)} entries for files of {ncomp if ncomp is not None else '1 or 3'} "
                                     f"component(s)")
            return vals
        mean, std = per_component("mean", normalize[0]), per_component("std", normalize[1])
        with np.errstate(over="ignore"):
            m32, s32 = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
        if not np.isfinite(m32).all():
            raise ValueError(f"normalize: mean must be finite, not {normalize[0]!r}")
        if not (np.isfinite(s32).all() and (s32 > 0).all()):
            raise ValueError(f"normalize: std must be finite and > 0 (as float32), not {normalize[1]!r}")
        mean, std = tuple(mean), tuple(std)
    flags = None
    if mirror is not None:
        def flag(v) -> bool:
            if isinstance(v, (bool, np.bool_)) or (isinstance(v, (int, np.integer)) and int(v) in (0, 1)):
                return bool(v)
            raise ValueError(f"mirror must be None, one bool or one bool per file, not {mirror!r}")
        if isinstance(mirror, (bool, np.bool_)):
            flags = [bool(mirror)] * (n_files if n_files is not None else 1)
        else:
            try:
                flags = [flag(v) for v in (mirror.tolist() if hasattr(mirror, "tolist") else mirror)]
            except TypeError:
                raise ValueError(f"mirror must be None, one bool or one bool per file, not {mirror!r}") from None
            if n_files is not None and len(flags) != n_files:
                raise ValueError(f"mirror has {len(flags)} entries for {n_files} files")
    if name == "uint8" and flags is None:
        return None
    return OutputSpec(name, mean, std, flags)


def normalize_rois(rois, dims: Sequence[Tuple[int, int]]) -> Optional[List[Tuple[int, int, int, int]]]:
    """The windows of a region-of-interest decode, one (x, y, width, height) per file, checked against the files' (width,
    height) — x along the width, y along the height.  ``rois``: None (whole images: returns None), one (x, y, width, height)
    for every file, or a sequence of ``len(dims)`` entries, each such a 4-tuple or None (that file's whole image).  Raises
    ValueError naming the file for a malformed, empty or out-of-image window."""
    if rois is None:
        return None
    n = len(dims)

    def is_window(r) -> bool:
        return isinstance(r, (tuple, list, np.ndarray)) and len(r) == 4 and all(isinstance(v, (int, np.integer)) for v in r)

    if is_window(rois):
        entries = [rois] * n
    else:
        try:
            entries = list(rois)
        except TypeError:
            raise ValueError("rois must be None, one (x, y, width, height) or one entry per file") from None
        if len(entries) != n:
            raise ValueError(f"rois has {len(entries)} entries for {n} files")
    out = []
    for i, (r, (w, h)) in enumerate(zip(entries, dims)):
        if r is None:
            out.append((0, 0, int(w), int(h)))
            continue
        if not is_window(r):
            raise ValueError(f"file {i}: window {r!r} is not an (x, y, width, height) tuple of integers")
        x, y, ww, wh = (int(v) for v in r)
        if ww <= 0 or wh <= 0 or x < 0 or y < 0 or x + ww > w or y + wh > h:
            raise ValueError(f"file {i}: window (x={x}, y={y}, width={ww}, height={wh}) is empty or not inside the {w}x{h} image")
        out.append((x, y, ww, wh))
    return out


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def normalize_views(views, dims, size, rois=None, return_seams: bool = False, index: Optional[Sequence[int]] = None):
    """The views of a call, checked: None for a call without them, else one (file, (x, y, width, height)) per OUTPUT — output k is
    that window of that file's image (as its orientation shows it, after the mode), resized to ``size``; a file is decoded once
    however many views name it, and a file no view names is not looked at.  ``views``: None, or a list whose entries are
    ``(file_index, (x, y, width, height))``, ``(file_index, None)`` — the whole image — or a bare ``file_index`` (the same).
    ``dims``: one (width, height) per file of the call, or None for a file whose header has not been read (its views' windows are
    then left as given: a first pass, which finds the files to read).  Views need ``size`` and go neither with ``rois`` nor with
    ``return_seams``.  ValueError naming the view and its file (``index``: the file's position in the caller's list) otherwise."""
    if views is None:
        return None
    if size is None:
        raise ValueError("views needs size=(width, height): every view is resized to it (crops at their own sizes would be ragged)")
    if rois is not None:
        raise ValueError("views and rois do not go together: a view names its own window")
    if return_seams:
        raise ValueError("views and return_seams do not go together: the seam outputs are whole images, one per file")
    if not isinstance(views, (list, tuple)):
        raise ValueError(f"views must be None or a list with one entry per output — (file_index, (x, y, width, height)), (file_index, None) "
                         f"or file_index —, not {views!r}")
    n = len(dims)

    def is_window(r) -> bool:
        return isinstance(r, (tuple, list, np.ndarray)) and len(r) == 4 and all(_is_int(v) for v in r)

    out = []
    for k, v in enumerate(views):
        if _is_int(v):
            i, r = int(v), None
        elif isinstance(v, (tuple, list)) and len(v) == 2 and _is_int(v[0]) and (v[1] is None or is_window(v[1])):
            i, r = int(v[0]), v[1]
        else:
            raise ValueError(f"view {k}: {v!r} is none of (file_index, (x, y, width, height)), (file_index, None) and file_index")
        if i < 0 or i >= n:
            raise ValueError(f"view {k}: file {i} is not one of the {n} files of the call")
        name = i if index is None else index[i]
        if dims[i] is None:
            out.append((i, tuple(int(t) for t in r) if r is not None else None))
            continue
        w, h = (int(t) for t in dims[i])
        if r is None:
            out.append((i, (0, 0, w, h)))
            continue
        x, y, ww, wh = (int(t) for t in r)
        if ww <= 0 or wh <= 0 or x < 0 or y < 0 or x + ww > w or y + wh > h:
            raise ValueError(f"view {k} (file {name}): window (x={x}, y={y}, width={ww}, height={wh}) is empty or not inside the {w}x{h} image")
        out.append((i, (x, y, ww, wh)))
    return out


def select_view_files(files: Sequence[bytes], views, size, rois=None, return_seams: bool = False):
    """Which files a call with ``views`` reads at all: None for a call without views, else (kept, views) — the positions, ascending,
    of the files some view names, and :func:`normalize_views`' first pass with every view's file numbered among THOSE.  The files
    left out are neither parsed nor decoded."""
    entries = normalize_views(views, [None] * len(files), size, rois, return_seams)
    if entries is None:
        return None
    kept = sorted({i for i, _ in entries})
    pos = {i: k for k, i in enumerate(kept)}
    return kept, [(pos[i], r) for i, r in entries]


def select_union_files(files: Sequence[bytes], groups: Sequence[dict]):
    """:func:`select_view_files` for a call with ``also``: ``groups`` holds the call's own arguments and every extra group's
    (:func:`normalize_also`), each with ``views`` and ``size``.  Returns the positions, ascending, of the files that SOME group names
    — a group without views names every file —; the rest are neither parsed nor decoded."""
    kept, every = set(), False
    for k, g in enumerate(groups):
        try:
            sel = select_view_files(files, g.get("views"), g.get("size"))
        except ValueError as e:                 # (the call's own group first, then also[0], also[1], ...)
            if k == 0:
                raise
            raise ValueError(f"also[{k - 1}]: {e}") from None
        if sel is None:
            every = True
        else:
            kept.update(sel[0])
    return list(range(len(files))) if every else sorted(kept)


# the keys of an entry of ``also``: what is per output and never inherited, and what is the call's unless the entry says otherwise
ALSO_PER_OUTPUT = ("views", "mirror", "resize_to", "place", "affine", "perspective", "color_ops", "erase", "mix", "compose", "patches")
ALSO_CALL_WIDE = ("dtype", "normalize", "resample", "mode", "reducing_gap", "fill", "affine_resample", "affine_fill")


def normalize_also(also, call: dict, size, rois=None, return_seams: bool = False, host: bool = False) -> Optional[List[dict]]:
    """``also`` of a call, checked as far as no file is needed: None for a call without extra groups (``None`` or ``[]``), else one dict
    per extra group with ``size`` and every key of ALSO_PER_OUTPUT and ALSO_CALL_WIDE — the keywords of the call that group alone
    would be.  An entry of ``also`` is a dict: ``size`` is required; ``views``, ``mirror``, ``resize_to``, ``place``, ``affine``,
    ``perspective`` and ``color_ops`` are the group's own (None when absent, never the call's); ``dtype``, ``normalize``, ``resample``,
    ``mode``, ``reducing_gap``, ``fill``, ``affine_resample`` and ``affine_fill`` are the call's (``call``) unless the entry names them.
    ``orientation`` is per file and the call's, ``rois`` are views, and there are no seam outputs: an entry with one of these, or any
    other key, is refused, as is ``also`` on a call without ``size``, with ``rois`` or with ``return_seams``.  ValueError naming the
    entry (``also[1]: ...``) otherwise."""
    if also is None:
        return None
    if not isinstance(also, (list, tuple)):
        raise ValueError(f"also must be None or a list with one dict per extra group of outputs, not {also!r}")
    if len(also) == 0:
        return None
    if size is None:
        raise ValueError("also needs size=(width, height): every group of outputs is one array at its own size")
    if rois is not None:
        raise ValueError("also and rois do not go together: windows are views, which every group has for itself")
    if return_seams:
        raise ValueError("also and return_seams do not go together: the seam outputs are whole images, one per file")
    refused = {"rois": "windows are views, which every group has for itself", "orientation": "it is per file and the call's",
               "return_seams": "the seam outputs are whole images, one per file", "also": "groups do not nest"}
    groups = []
    for k, entry in enumerate(also):
        if not isinstance(entry, dict):
            raise ValueError(f"also[{k}]: an entry is a dict of keywords (size=, views=, ...), not {entry!r}")
        for key in entry:
            if key in refused:
                raise ValueError(f"also[{k}]: {key} is not a key of an entry: {refused[key]}")
            if key != "size" and key not in ALSO_PER_OUTPUT and key not in ALSO_CALL_WIDE:
                raise ValueError(f"also[{k}]: unknown key {key!r} (size, {', '.join(ALSO_PER_OUTPUT + ALSO_CALL_WIDE)})")
        if entry.get("size") is None:
            raise ValueError(f"also[{k}]: size is required: every group of outputs is one array at its own size")
        g = {key: entry.get(key) for key in ALSO_PER_OUTPUT}
        g.update({key: entry[key] if key in entry else call.get(key) for key in ALSO_CALL_WIDE})
        # (what the call says about placing and transforming is inherited by the groups that place and transform)
        if g["resize_to"] is None and "fill" not in entry:
            g["fill"] = None
        if g["affine"] is None and g["perspective"] is None:
            g.update({key: None for key in ("affine_resample", "affine_fill") if key not in entry})
        try:                                  # (what needs no file, as the call's own arguments are checked before any is read)
            g["size"] = normalize_size(entry["size"])
            normalize_output(g["dtype"], g["normalize"], g["mirror"], g["size"], host=host)
            normalize_resample(g["resample"], g["size"])
            gap = normalize_reducing_gap(g["reducing_gap"], g["size"])
            normalize_mode(g["mode"])
            normalize_places(g["resize_to"], g["place"], g["size"])
            normalize_fill(g["fill"], g["resize_to"])
            normalize_transform(g["affine"], g["perspective"], g["affine_resample"], g["affine_fill"], g["size"], None, gap)
            normalize_color_ops(g["color_ops"], g["size"])
            normalize_erase(g["erase"], g["size"], device=None if host else -1)
            composed = normalize_compose(g["compose"], g["size"], mix=normalize_mix(g["mix"], g["size"]))
            normalize_patches(g["patches"], g["size"], compose=composed)
            if g["views"] is not None and not isinstance(g["views"], (list, tuple)):
                normalize_views(g["views"], [], g["size"])
        except ValueError as e:
            raise ValueError(f"also[{k}]: {e}") from None
        groups.append(g)
    return groups


def _per_file_of(value, n_files: int, kept: Sequence[int], what: str):
    """a per-file argument of a call with views — one entry per file of the caller's list — for the files that are read; anything
    that is not such a list (None, one value for all files) as it is"""
    if value is None or isinstance(value, (str, int, np.integer, bytes)):
        return value
    try:
        entries = value.tolist() if hasattr(value, "tolist") else list(value)
    except TypeError:
        return value
    if len(entries) != n_files:
        raise ValueError(f"{what} has {len(entries)} entries for {n_files} files")
    return [entries[i] for i in kept]


def _named(index: Optional[Sequence[int]], i: int, fn, *args, **kwargs):
    """fn(...) for file i of a call with views: what the parser raises about the file names its position in the caller's list"""
    if index is None:
        return fn(*args, **kwargs)
    try:
        return fn(*args, **kwargs)
    except JpegError as e:
        raise type(e)(f"file {index[i]}: {e}") from None


# Pillow's Image.Resampling numbering of the filters Image.transform takes
_PILLOW_AFFINE_FILTERS = {0: "nearest", 2: "bilinear", 3: "bicubic"}


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _is_matrix(m) -> bool:
    return isinstance(m, (tuple, list, np.ndarray)) and len(m) == 6 and all(_is_number(v) for v in m)


def affine_fault(a: Sequence[float], resample: str, w: int, h: int) -> Optional[str]:
    """What is refused of one matrix for a ``w`` x ``h`` image (None: nothing) — csrc/affine.hip's affine_fault, restated: an entry
    that is not finite, a side of 32768 or more, a corner pixel whose source coordinate has a magnitude of 32768 or more (Pillow
    leaves its defined arithmetic there) and, under "nearest", the same for the corners Pillow's check_fixed tests and entries that
    do not fit 16.16 fixed point."""
    if not all(math.isfinite(v) for v in a):
        return "a matrix entry is not finite"
    if w >= 32768 or h >= 32768:
        return "an image with a side of 32768 or more"
    corners = [(x, y) for y in (0.5, h - 0.5) for x in (0.5, w - 0.5)]
    if resample == "nearest":
        corners += [(float(x), float(y)) for y in (0, h) for x in (0, w)]
    for x, y in corners:
        if not (abs(a[0] * x + a[1] * y + a[2]) < 32768.0 and abs(a[3] * x + a[4] * y + a[5]) < 32768.0):
            return "a corner of the output has a source coordinate of magnitude 32768 or more"
    if resample == "nearest" and not (a[1] == 0 and a[3] == 0):
        fixed = (a[0], a[1], a[2] + a[0] * 0.5 + a[1] * 0.5, a[3], a[4], a[5] + a[3] * 0.5 + a[4] * 0.5)
        if not all(abs(v) < 32767.0 for v in fixed):
            return "a matrix entry of magnitude 32767 or more does not fit NEAREST's 16.16 fixed point"
    return None


@dataclass
class AffineSpec:
    """The affine transform of a call (:func:`normalize_affine`): ``matrices`` one 6-tuple of floats or None per OUTPUT, ``resample``
    "nearest", "bilinear" or "bicubic", ``fill`` one byte per output component (or the one byte given for all of them, until the
    component count is known).  ``perspective``: the transform is a perspective one (:func:`normalize_perspective`) and ``matrices``
    holds 8-tuples of coefficients."""
    matrices: List[Optional[Tuple[float, ...]]]
    resample: str
    fill: Tuple[int, ...]
    perspective: bool = False


def normalize_affine(affine, affine_resample, affine_fill, size, n_outputs: Optional[int] = None, reducing_gap=None, return_seams: bool = False,
                     ncomp: Optional[int] = None) -> Optional[AffineSpec]:
    """``affine``, ``affine_resample`` and ``affine_fill`` of a call, checked: None for a call without a transform — ``affine`` None or
    a list of Nones, which both make the request of a call without the argument — else an :class:`AffineSpec`.  ``affine``: None, one
    matrix ``(a0, .., a5)`` of numbers for every output, or a list with one matrix or None per output (per file; per view with
    ``views``); the matrix maps OUTPUT pixel centres to source coordinates, as the ``data`` of Pillow's ``Image.transform(size,
    Image.AFFINE, data)`` and torchvision's inverse matrix do.  ``affine_resample``: None or "nearest" (the default, as Pillow's and
    torchvision's is), "bilinear" or "bicubic" — a name in any case, the ``Image.Resampling`` member or its integer.
    ``affine_fill``: None (0), one byte, or one per output component (``ncomp``, where known).  The transform needs ``size`` and goes
    neither with ``return_seams`` nor — yet — with ``reducing_gap``.  ``n_outputs`` None: what needs no file.  ValueError otherwise."""
    name, fill = _transform_resample_fill(affine_resample, affine_fill, ncomp)
    if affine is None:
        if affine_resample is not None or affine_fill is not None:
            raise ValueError("affine_resample and affine_fill need affine or perspective: without one nothing is transformed")
        return None
    if size is None:
        raise ValueError("affine needs size=(width, height): the transformed images are resized to it")
    if return_seams:
        raise ValueError("affine and return_seams do not go together: the seam outputs are the decoded images")
    if reducing_gap is not None:
        raise ValueError("affine and reducing_gap do not go together yet: the reduce step would have to read the transformed images "
                         "(a later step)")
    if _is_matrix(affine):
        matrices = None if n_outputs is None else [tuple(float(v) for v in affine)] * n_outputs
    elif isinstance(affine, (list, tuple)) and all(m is None or _is_matrix(m) for m in affine):
        if n_outputs is not None and len(affine) != n_outputs:
            raise ValueError(f"affine has {len(affine)} entries for {n_outputs} outputs")
        matrices = [tuple(float(v) for v in m) if m is not None else None for m in affine]
    else:
        raise ValueError(f"affine must be None, one matrix (a0, a1, a2, a3, a4, a5) of numbers, or a list with one matrix or None per output, "
                         f"not {affine!r}")
    for k, m in enumerate(matrices or []):
        if m is not None and not all(math.isfinite(v) for v in m):
            raise ValueError(f"affine: output {k}: a matrix entry is not finite")
        if m is not None and not any(m):
            raise ValueError(f"affine: output {k}: a matrix that is all zero maps every pixel to the source's corner (None: no transform)")
    if matrices is not None and all(m is None for m in matrices):
        return None
    return AffineSpec(matrices if matrices is not None else [], name, fill)


def _transform_resample_fill(affine_resample, affine_fill, ncomp: Optional[int] = None):
    """(name, fill) of ``affine_resample`` and ``affine_fill``, which serve ``affine`` and ``perspective`` alike"""
    name = "nearest"
    if affine_resample is not None:
        name = None
        if isinstance(affine_resample, str):
            name = affine_resample.lower()
        elif isinstance(affine_resample, (int, np.integer)) and not isinstance(affine_resample, (bool, np.bool_)):
            name = _PILLOW_AFFINE_FILTERS.get(int(affine_resample))
        if name not in B.AFFINE_FILTERS:
            raise ValueError(f"affine_resample must be one of {', '.join(B.AFFINE_FILTERS)} (a name, Pillow's Image.Resampling member or its "
                             f"integer value), not {affine_resample!r}")
    fill = (0,)
    if affine_fill is not None:
        entries = (affine_fill,) if _is_int(affine_fill) else tuple(affine_fill) if isinstance(affine_fill, (tuple, list, np.ndarray)) else None
        if entries is None or len(entries) not in (1, 3) or not all(_is_int(v) and 0 <= int(v) <= 255 for v in entries):
            raise ValueError(f"affine_fill must be one byte 0..255 or one per output component, not {affine_fill!r}")
        fill = tuple(int(v) for v in entries)
    if ncomp is not None:
        if len(fill) == 1:
            fill = fill * ncomp
        if len(fill) != ncomp:
            raise ValueError(f"affine_fill has {len(fill)} bytes for outputs of {ncomp} component{'s' if ncomp > 1 else ''}")
    return name, fill


def _is_coeffs(c) -> bool:
    return isinstance(c, (tuple, list, np.ndarray)) and len(c) == 8 and all(_is_number(v) for v in c)


def perspective_fault(c: Sequence[float], w: int, h: int) -> Optional[str]:
    """What is refused of one set of coefficients for a ``w`` x ``h`` image (None: nothing) — csrc/affine.hip's perspective_fault,
    restated.  No magnitude is: a source coordinate of any size, NaN included, is tested before it is used."""
    if not all(math.isfinite(v) for v in c):
        return "a coefficient is not finite"
    if w >= 32768 or h >= 32768:
        return "an image with a side of 32768 or more"
    return None


def normalize_perspective(perspective, affine_resample, affine_fill, size, n_outputs: Optional[int] = None, reducing_gap=None,
                          return_seams: bool = False, ncomp: Optional[int] = None) -> Optional[AffineSpec]:
    """``perspective`` of a call, with the ``affine_resample`` and ``affine_fill`` it shares with ``affine``, checked as
    :func:`normalize_affine` checks a matrix: None for a call without a transform, else an :class:`AffineSpec` with ``perspective``
    set.  ``perspective``: None, one sequence ``(c0, .., c7)`` of eight numbers for every output, or a list with one such sequence
    or None per output (per file; per view with ``views``).  The coefficients map OUTPUT pixel centres to source coordinates —
    ``x_in = (c0 x + c1 y + c2) / (c6 x + c7 y + 1)``, ``y_in = (c3 x + c4 y + c5) / (c6 x + c7 y + 1)`` — as the ``data`` of Pillow's
    ``Image.transform(size, Image.PERSPECTIVE, data)`` and torchvision's ``_get_perspective_coeffs`` do
    (:func:`perspective_coeffs` solves for them).  ValueError otherwise; what depends on the output's file — a coefficient that is
    not finite is reported with it — is :func:`check_affine`'s."""
    name, fill = _transform_resample_fill(affine_resample, affine_fill, ncomp)
    if perspective is None:
        if affine_resample is not None or affine_fill is not None:
            raise ValueError("affine_resample and affine_fill need affine or perspective: without one nothing is transformed")
        return None
    if size is None:
        raise ValueError("perspective needs size=(width, height): the transformed images are resized to it")
    if return_seams:
        raise ValueError("perspective and return_seams do not go together: the seam outputs are the decoded images")
    if reducing_gap is not None:
        raise ValueError("perspective and reducing_gap do not go together yet: the reduce step would have to read the transformed images "
                         "(a later step)")
    if _is_coeffs(perspective):
        coeffs = None if n_outputs is None else [tuple(float(v) for v in perspective)] * n_outputs
    elif isinstance(perspective, (list, tuple)) and all(c is None or _is_coeffs(c) for c in perspective):
        if n_outputs is not None and len(perspective) != n_outputs:
            raise ValueError(f"perspective has {len(perspective)} entries for {n_outputs} outputs")
        coeffs = [tuple(float(v) for v in c) if c is not None else None for c in perspective]
    else:
        raise ValueError(f"perspective must be None, one sequence (c0, .., c7) of eight numbers, or a list with one such sequence or None per "
                         f"output, not {perspective!r}")
    for k, c in enumerate(coeffs or []):            # (a coefficient that is not finite: check_affine's, which can name the file)
        if c is not None and not any(c):
            raise ValueError(f"perspective: output {k}: coefficients that are all zero map every pixel to the source's corner (None: no transform)")
    if coeffs is not None and all(c is None for c in coeffs):
        return None
    return AffineSpec(coeffs if coeffs is not None else [], name, fill, True)


def normalize_transform(affine, perspective, affine_resample, affine_fill, size, n_outputs: Optional[int] = None, reducing_gap=None,
                        return_seams: bool = False, ncomp: Optional[int] = None) -> Optional[AffineSpec]:
    """the one geometric transform of a call: :func:`normalize_affine` or :func:`normalize_perspective` — not both"""
    if affine is not None and perspective is not None:
        raise ValueError("affine and perspective do not go together: a call has one transform in front of the window "
                         "(a perspective transform with c6 = c7 = 0 is an affine one)")
    if perspective is not None:
        return normalize_perspective(perspective, affine_resample, affine_fill, size, n_outputs, reducing_gap, return_seams, ncomp)
    return normalize_affine(affine, affine_resample, affine_fill, size, n_outputs, reducing_gap, return_seams, ncomp)


def _spec_for_outputs(spec: AffineSpec, size, n_outputs: int, ncomp: int) -> Optional[AffineSpec]:
    """a checked spec again, now that the outputs' count and components are known (the fill then has one byte per component)"""
    return (normalize_perspective if spec.perspective else normalize_affine)(spec.matrices, spec.resample, spec.fill, size, n_outputs, ncomp=ncomp)


def perspective_coeffs(startpoints, endpoints) -> Tuple[float, ...]:
    """The eight coefficients of the perspective transform that takes the four corners ``startpoints`` of the source to
    ``endpoints`` in the output — each four ``(x, y)`` pairs, torchvision's order: top-left, top-right, bottom-right, bottom-left —,
    as ``perspective=`` takes them: the solution torchvision's ``_get_perspective_coeffs(startpoints, endpoints)`` solves for, i.e.
    what ``F.perspective(img, startpoints, endpoints)`` hands Pillow.  The 8 x 8 system in float64 — per pair the rows
    ``[ex, ey, 1, 0, 0, 0, -sx ex, -sx ey]`` and ``[0, 0, 0, ex, ey, 1, -sy ex, -sy ey]``, right-hand side the start points —
    solved with NumPy.  NOT pinned to torchvision's bits: torchvision solves the same system with ``torch.linalg.lstsq`` in
    float64 and rounds to float32 on the way, so its coefficients agree with these to rounding, not bit for bit; the pixels are
    Pillow's for whichever coefficients are given.  ValueError for anything but four pairs of finite numbers each, or corners
    that determine no transform (three on a line)."""
    def pairs(pts, what):
        ok = isinstance(pts, (list, tuple, np.ndarray)) and len(pts) == 4 and all(
            isinstance(q, (list, tuple, np.ndarray)) and len(q) == 2 and all(_is_number(v) and math.isfinite(v) for v in q) for q in pts)
        if not ok:
            raise ValueError(f"{what} must be four (x, y) pairs of finite numbers, not {pts!r}")
        return [(float(q[0]), float(q[1])) for q in pts]
    start, end = pairs(startpoints, "startpoints"), pairs(endpoints, "endpoints")
    a = np.zeros((8, 8), dtype=np.float64)
    b = np.zeros(8, dtype=np.float64)
    for i, ((sx, sy), (ex, ey)) in enumerate(zip(start, end)):
        a[2 * i] = [ex, ey, 1, 0, 0, 0, -sx * ex, -sx * ey]
        a[2 * i + 1] = [0, 0, 0, ex, ey, 1, -sy * ex, -sy * ey]
        b[2 * i], b[2 * i + 1] = sx, sy
    try:
        c = np.linalg.solve(a, b)
    except np.linalg.LinAlgError:
        raise ValueError(f"startpoints {startpoints!r} and endpoints {endpoints!r} determine no perspective transform") from None
    if not np.all(np.isfinite(c)):
        raise ValueError(f"startpoints {startpoints!r} and endpoints {endpoints!r} determine no perspective transform")
    return tuple(float(v) for v in c)


def rois_as_views(rois, n_files: int):
    """The windows of a call with an affine transform as views, one per file: such a call decodes whole images — a rotated window
    needs source pixels outside itself — and cuts the window out of the transformed image.  ``rois`` as :func:`normalize_rois`
    takes it; the windows are checked as views are (:func:`normalize_views`)."""
    def is_window(r) -> bool:
        return isinstance(r, (tuple, list, np.ndarray)) and len(r) == 4 and all(_is_int(v) for v in r)
    if rois is None:
        return [(i, None) for i in range(n_files)]
    if is_window(rois):
        return [(i, tuple(int(v) for v in rois)) for i in range(n_files)]
    if not isinstance(rois, (list, tuple)) or len(rois) != n_files or not all(r is None or is_window(r) for r in rois):
        raise ValueError(f"rois must be None, one (x, y, width, height) or a list with one such window or None per file ({n_files}), not {rois!r}")
    return [(i, tuple(int(v) for v in r) if r is not None else None) for i, r in enumerate(rois)]


def check_affine(spec: Optional[AffineSpec], views, odims, index=None) -> None:
    """every matrix of ``spec`` against the oriented image of its output's file (:func:`affine_fault`): ValueError naming the output"""
    if spec is None:
        return
    for k, ((f, _), m) in enumerate(zip(views, spec.matrices)):
        why = None if m is None else perspective_fault(m, *odims[f]) if spec.perspective else affine_fault(m, spec.resample, *odims[f])
        if why:
            raise ValueError(f"{'perspective' if spec.perspective else 'affine'}: output {k} (file {f if index is None else index[f]}): {why}")


def _is_colour_op(op) -> bool:
    """an op is always a tuple whose first element is a string: that tells one chain from a list of chains"""
    return isinstance(op, tuple) and len(op) >= 1 and isinstance(op[0], str)


def _is_chain(c) -> bool:
    return isinstance(c, (list, tuple)) and all(_is_colour_op(op) for op in c)


def _colour_chain(chain, where: str) -> Optional[Tuple[tuple, ...]]:
    """one chain, checked: a tuple of ``(name,)`` / ``(name, value)`` with the value the C ABI takes, or None for an empty one"""
    if len(chain) > B.MJ_COLOUR_MAX_OPS:
        raise ValueError(f"color_ops: {where}{len(chain)} ops in one chain; at most {B.MJ_COLOUR_MAX_OPS} are offered yet")
    ops = []
    for op in chain:
        name = op[0]
        if name not in B.COLOUR_OPS:
            raise ValueError(f"color_ops: {where}unknown op {name!r} (one of {', '.join(B.COLOUR_OPS)}; hue is ('adjust_hue', f))")
        if name not in B.COLOUR_VALUED:
            if len(op) != 1:
                raise ValueError(f"color_ops: {where}{name!r} takes no value (cutoffs and masks are not offered yet), not {op!r}")
            ops.append((name,))
            continue
        if len(op) != 2 or not _is_number(op[1]):
            raise ValueError(f"color_ops: {where}{name!r} takes one number, not {op!r}")
        v = float(op[1])
        if not math.isfinite(v):
            raise ValueError(f"color_ops: {where}{name!r}: {op[1]!r} is not finite")
        if name == "posterize":
            if v != int(v) or not 1 <= int(v) <= 8:
                raise ValueError(f"color_ops: {where}posterize takes 1..8 bits, not {op[1]!r}")
        elif name == "solarize":            # (v stays where v < t: for a byte, where v < ceil(t))
            v = float(min(max(math.ceil(v), 0), 256))
        elif name in B.COLOUR_BLURS and not 0 <= v <= B.MJ_COLOUR_MAX_RADIUS:
            raise ValueError(f"color_ops: {where}{name} takes a radius of 0..{B.MJ_COLOUR_MAX_RADIUS}, not {op[1]!r}")
        elif name == "adjust_hue" and not -0.5 <= v <= 0.5:          # (torchvision raises there too)
            raise ValueError(f"color_ops: {where}adjust_hue takes a factor of -0.5..0.5, not {op[1]!r}")
        ops.append((name, v))
    return tuple(ops) or None


def normalize_color_ops(color_ops, size, n_outputs: Optional[int] = None, return_seams: bool = False):
    """``color_ops`` of a call, checked: None for a call without colour operations — ``color_ops`` None, or chains that are all None or
    empty, which make the request of a call without the argument — else a list with one chain (a tuple of ops) or None per OUTPUT.
    ``color_ops``: None, one chain for every output, or a list with one chain or None per output (per file; per view with
    ``views``).  A chain is a sequence of at most four ops, applied in order to the finished canvas as to a Pillow image of the
    output's mode, each op the one Pillow call that defines its bytes (tools/colour_model.py): ``("brightness", f)``, ``("color", f)``,
    ``("contrast", f)``, ``("sharpness", f)`` — ``ImageEnhance.<Name>(im).enhance(f)`` —, ``("posterize", bits)`` with 1..8 bits,
    ``("solarize", t)``, ``("autocontrast",)``, ``("equalize",)``, ``("invert",)`` — ``ImageOps.<name>(im[, value])`` —,
    ``("gaussian_blur", radius)``, ``("box_blur", radius)`` with one radius of 0..1024 — ``im.filter(ImageFilter.GaussianBlur(radius))``
    / ``BoxBlur(radius)`` —, ``("adjust_hue", f)`` with -0.5 <= f <= 0.5 — torchvision's ``F.adjust_hue(im, f)`` on a PIL image: Pillow's
    HSV round trip with ``int(f * 255) & 255`` added to H, the identity on an "L" output and NOT the identity for f = 0.  An op is always
    a tuple whose first element is a string; that is how one chain is told from a list of chains.  The operations need ``size`` and
    do not go with ``return_seams``.  ``n_outputs`` None: what needs no file.  ValueError otherwise."""
    if color_ops is None:
        return None
    if size is None:
        raise ValueError("color_ops needs size=(width, height): the operations work on the finished canvas")
    if return_seams:
        raise ValueError("color_ops and return_seams do not go together: the seam outputs are the decoded images")
    if _is_chain(color_ops):
        one = _colour_chain(color_ops, "")
        chains = None if n_outputs is None else [one] * n_outputs
    elif isinstance(color_ops, (list, tuple)) and all(c is None or _is_chain(c) for c in color_ops):
        if n_outputs is not None and len(color_ops) != n_outputs:
            raise ValueError(f"color_ops has {len(color_ops)} entries for {n_outputs} outputs")
        chains = [_colour_chain(c, f"output {k}: ") if c is not None else None for k, c in enumerate(color_ops)]
    else:
        raise ValueError(f"color_ops must be None, one chain — a sequence of ops such as ('brightness', 1.2) or ('equalize',), each a tuple "
                         f"that starts with the op's name — or a list with one chain or None per output, not {color_ops!r}")
    if chains is None or all(c is None for c in chains):
        return None
    return chains


def _is_tensor(v) -> bool:
    """a torch tensor, told without importing torch (the NumPy route does not need it)"""
    return type(v).__module__.split(".")[0] == "torch" and hasattr(v, "data_ptr")


def _is_erase_box(b) -> bool:
    """a box is a tuple whose first element is not itself a sequence: that tells one box from a list of boxes"""
    return isinstance(b, tuple) and len(b) > 0 and not isinstance(b[0], (list, tuple))


def normalize_erase(erase, size, n_outputs: Optional[int] = None, ncomp: Optional[int] = None, dtype: Optional[str] = None,
                    return_seams: bool = False, device: Optional[int] = None):
    """``erase`` of a call, checked: None for a call without it — ``erase`` None, or entries that are all None or empty, which make
    the request of a call without the argument — else a list with, per OUTPUT, None or a tuple of boxes ``(x, y, width, height, value)``.

    ``erase``: None, or a list with one entry per output (per file; per view with ``views``); there is no one-for-all form.  An entry
    is None, one box, or a list of boxes applied in order — a later box wins where two overlap (timm's ``count > 1``).  A box is a
    tuple ``(x, y, width, height)`` or ``(x, y, width, height, value)``, integers, ``x`` along the width as in ``rois`` (not
    torchvision's ``(i, j, h, w)``), wholly inside the ``size`` canvas: torchvision's ``F.erase``, ``img[..., y:y+height, x:x+width] =
    value``, on the finished output — after the mirror, in the output's ``dtype`` (tools/erase_model.py).  ``value``: absent or a
    number — every component gets it (0 when absent), as float32 first (``torch.tensor(value)``), then the output's type; a sequence
    of ``ncomp`` numbers — one per output component; an array or tensor of shape ``(ncomp, height, width)`` — one value per element,
    always in that order whatever the decoder's layout, converted from its own type with one rounding (``v.to(dtype)``): the noise of
    torchvision's ``value="random"`` / timm's ``mode="pixel"``, which the caller draws.  NumPy arrays everywhere; torch tensors, CPU
    or on the decoder's GPU (``device``: its index; None: the NumPy route), on the ``decode_device`` calls.  For a uint8 output
    numbers are integers 0..255 and arrays uint8.  The returned value is a tuple of ``ncomp`` floats (float32 values) or the array —
    with ``ncomp`` None a lone number stays one float, which :func:`erase_for_components` completes once the count is known.

    ``erase`` needs ``size`` and does not go with ``return_seams``.  ``n_outputs`` / ``ncomp`` / ``dtype`` None: not known yet — what
    needs them is not checked.  ValueError, naming output and box, otherwise."""
    if erase is None:
        return None
    if size is None:
        raise ValueError("erase needs size=(width, height): boxes are in the coordinates of the finished canvas")
    if return_seams:
        raise ValueError("erase and return_seams do not go together: the seam outputs are the decoded images")
    if not isinstance(erase, (list, tuple)) or (isinstance(erase, tuple) and len(erase) in (4, 5) and _is_int(erase[0])):
        raise ValueError(f"erase must be None or a list with, per output, None, one box (x, y, width, height[, value]) or a list of boxes "
                         f"(there is no one-for-all form), not {erase!r}")
    if n_outputs is not None and len(erase) != n_outputs:
        raise ValueError(f"erase has {len(erase)} entries for {n_outputs} outputs")
    W, H = size
    u8 = dtype == "uint8"

    def number(v, where) -> float:
        if type(v) is not float and type(v) is not int and not _is_number(v):
            raise ValueError(f"erase: {where()}: a value is a number, {ncomp or 'one per component'} numbers or an array of shape (C, height, width), "
                             f"not {v!r}")
        f = ctypes.c_float(v).value             # (the nearest float32, as torch.tensor(v) holds it; too large: infinity)
        if f - f != 0.0:
            raise ValueError(f"erase: {where()}: value {v!r} is not finite (as float32)")
        if u8 and (f != int(f) or not 0 <= f <= 255):
            raise ValueError(f"erase: {where()}: a uint8 output takes integers 0..255, not {v!r}")
        return f

    def box(b, k, j):
        def where():
            return f"output {k}, box {j}"
        if type(b) is not tuple or not 4 <= len(b) <= 5:
            raise ValueError(f"erase: {where()}: a box is (x, y, width, height) or (x, y, width, height, value), not {b!r}")
        x, y, w, h = b[0], b[1], b[2], b[3]
        if not (type(x) is int and type(y) is int and type(w) is int and type(h) is int):
            if not all(_is_int(t) for t in b[:4]):
                raise ValueError(f"erase: {where()}: x, y, width and height must be integers, not {b[:4]!r}")
            x, y, w, h = int(x), int(y), int(w), int(h)
        if w < 1 or h < 1:
            raise ValueError(f"erase: {where()}: width and height must be at least 1, not {w} x {h}")
        if x < 0 or y < 0 or x + w > W or y + h > H:
            raise ValueError(f"erase: {where()}: box ({x}, {y}, {w}, {h}) is not inside the {W} x {H} canvas")
        v = b[4] if len(b) == 5 and b[4] is not None else 0
        if type(v) is float or type(v) is int:
            f = number(v, where)
            return (x, y, w, h, (f,) * ncomp if ncomp else f)
        if isinstance(v, np.ndarray) and v.ndim == 0:
            v = v.item()
        if isinstance(v, np.ndarray) or _is_tensor(v):
            if _is_tensor(v):
                if device is None:
                    raise ValueError(f"erase: {where()}: a torch tensor is accepted on the decode_device calls; decode takes NumPy arrays")
                if v.device.type != "cpu" and device >= 0 and v.device.index != device:       # (device < 0: some GPU, not known yet)
                    raise ValueError(f"erase: {where()}: values on {v.device}, not on the CPU or the decoder's GPU cuda:{device}")
            shape = tuple(v.shape)
            if len(shape) == 1 and shape[0] <= 3 and not _is_tensor(v):
                v = v.tolist()                # (a short vector: numbers per component)
            else:
                if len(shape) != 3 or shape[1] != h or shape[2] != w or (ncomp is not None and shape[0] != ncomp) or shape[0] not in (1, 3):
                    raise ValueError(f"erase: {where()}: values of shape {tuple(int(t) for t in shape)} for a box of ({ncomp if ncomp is not None else 'C'}, {h}, {w})")
                name = str(v.dtype).split(".")[-1]
                if u8 and name != "uint8":
                    raise ValueError(f"erase: {where()}: a uint8 output takes uint8 arrays, not {v.dtype}")
                if not u8 and name not in ("uint8", "float16", "bfloat16", "float32", "float64"):
                    raise ValueError(f"erase: {where()}: values of type {v.dtype}; uint8, float16, bfloat16, float32 or float64 are taken")
                return (x, y, w, h, v)
        if isinstance(v, (list, tuple)):
            if (ncomp is not None and len(v) != ncomp) or len(v) not in (1, 3):
                raise ValueError(f"erase: {where()}: {len(v)} values for {ncomp if ncomp is not None else '1 or 3'} component(s)")
            return (x, y, w, h, tuple(number(t, where) for t in v))
        f = number(v, where)
        return (x, y, w, h, (f,) * ncomp if ncomp else f)

    out, some = [], False
    for k, entry in enumerate(erase):
        if entry is None:
            out.append(None)
            continue
        if _is_erase_box(entry):
            boxes = (box(entry, k, 0),)
        elif isinstance(entry, (list, tuple)):
            boxes = tuple(box(b, k, j) for j, b in enumerate(entry))
        else:
            raise ValueError(f"erase: output {k}: an entry is None, one box or a list of boxes, not {entry!r}")
        out.append(boxes or None)
        some = some or bool(boxes)
    return out if some else None


def erase_for_components(erase, ncomp: int):
    """:func:`normalize_erase`'s boxes, checked before the files' component count was known, for outputs of ``ncomp`` components: a
    number stands for all of them, and per-component values and arrays must have that many.  ValueError, naming output and box."""
    if erase is None:
        return None
    out = []
    for k, boxes in enumerate(erase):
        if boxes is None:
            out.append(None)
            continue
        done = []
        for j, b in enumerate(boxes):
            v = b[4]
            if type(v) is float:                # (one number: every component gets it)
                done.append(b[:4] + ((v,) * ncomp,))
                continue
            n = len(v) if type(v) is tuple else int(v.shape[0])
            if n != ncomp:
                if type(v) is tuple:
                    raise ValueError(f"erase: output {k}, box {j}: {n} values for {ncomp} component(s)")
                else:
                    raise ValueError(f"erase: output {k}, box {j}: values of shape {tuple(int(t) for t in v.shape)} for a box of ({ncomp}, {b[3]}, {b[2]})")
            done.append(b)
        out.append(tuple(done))
    return out


def random_erasing_rect(size, scale=(0.02, 0.33), ratio=(0.3, 3.3), generator=None) -> Optional[Tuple[int, int, int, int]]:
    """A box for ``erase=`` drawn as torchvision's ``RandomErasing.get_params`` draws it for a ``size = (width, height)`` canvas:
    ``(x, y, w, h)``, or None when ten tries find none.  Restated: up to ten tries, each drawing the area — ``H * W`` times a uniform
    ``torch.empty(1).uniform_(scale[0], scale[1])`` — and then the aspect ratio, log-uniform between ``ratio[0]`` and ``ratio[1]``;
    ``h = int(round(sqrt(area * aspect)))``, ``w = int(round(sqrt(area / aspect)))``; the box is taken if ``h < H and w < W``, its
    corner from two ``torch.randint`` draws (the row first).  torchvision is not a dependency here and this function is NOT pinned
    to its draws: the same seed need not give torchvision's box (it passes no generator, for one).  Whether to erase at all
    (``p``) and the value are the caller's."""
    import torch
    W, H = (int(t) for t in size)
    area = H * W
    log_ratio = torch.log(torch.tensor([float(ratio[0]), float(ratio[1])]))
    for _ in range(10):
        erase_area = area * torch.empty(1).uniform_(float(scale[0]), float(scale[1]), generator=generator).item()
        aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0].item(), log_ratio[1].item(), generator=generator)).item()
        h = int(round(math.sqrt(erase_area * aspect)))
        w = int(round(math.sqrt(erase_area / aspect)))
        if not (h < H and w < W) or h < 1 or w < 1:     # (a side that rounds to 0 erases nothing in torchvision; here it is a failed try)
            continue
        i = int(torch.randint(0, H - h + 1, size=(1,), generator=generator).item())
        j = int(torch.randint(0, W - w + 1, size=(1,), generator=generator).item())
        return (j, i, w, h)
    return None


def normalize_mix(mix, size, n_outputs: Optional[int] = None, dtype: Optional[str] = None, return_seams: bool = False):
    """``mix`` of a call, checked: None for a call without it — ``mix`` None, or entries that are all None, which make the plans,
    launches and tensor of a call without the argument — else a list with, per OUTPUT, None, ``("mixup", partner, lam)`` or
    ``("cutmix", partner, (x, y, width, height))``.

    ``mix``: None, or a list with one entry per output (per file; per view with ``views``); there is no one-for-all form.
    ``partner``: the index of an output of the same group — any mapping: torchvision's ``roll(1, 0)`` is ``(k - 1) % N``, timm's
    ``flip(0)`` is ``N - 1 - k``, and an output may be its own partner.  ``("mixup", partner, lam)``, float outputs only: ``out[k] =
    lam * pre[k] + (1 - lam) * pre[partner]`` as ``pre.roll(1, 0).mul(1.0 - lam).add_(pre.mul(lam))`` computes it with torch's CPU
    ops, bit for bit (tools/mix_model.py); ``lam`` a finite number in 0..1.  ``("cutmix", partner, box)``, any ``dtype``: ``out[k] =
    pre[k]`` with ``[..., y:y+height, x:x+width]`` taken from ``pre[partner]``; the box as in ``erase``: integers, ``x`` along the
    width, wholly inside the ``size`` canvas, sides of at least 1 (:func:`cutmix_box` draws one).  ``pre`` is the call's result
    without the argument — behind the mirror, the element type and ``erase`` —, and every output reads ``pre``: the mixing is
    simultaneous.  Per-output ``lam`` and boxes are timm's ``elem`` / ``pair`` modes; labels are the caller's business.

    ``mix`` needs ``size`` and does not go with ``return_seams``.  ``n_outputs`` / ``dtype`` None: not known yet — what needs them
    is not checked.  ValueError, naming the output, otherwise."""
    if mix is None:
        return None
    if size is None:
        raise ValueError("mix needs size=(width, height): the outputs of one array are mixed with each other")
    if return_seams:
        raise ValueError("mix and return_seams do not go together: the seam outputs are the decoded images")
    if not isinstance(mix, (list, tuple)) or (isinstance(mix, tuple) and len(mix) == 3 and isinstance(mix[0], str)):
        raise ValueError(f"mix must be None or a list with, per output, None, (\"mixup\", partner, lam) or (\"cutmix\", partner, (x, y, width, height)) "
                         f"(there is no one-for-all form), not {mix!r}")
    if n_outputs is not None and len(mix) != n_outputs:
        raise ValueError(f"mix has {len(mix)} entries for {n_outputs} outputs")
    W, H = size
    n = len(mix)
    u8 = dtype == "uint8"
    out, some = [], False
    for k, e in enumerate(mix):
        if e is None:
            out.append(None)
            continue
        some = True
        if type(e) is tuple and len(e) == 3:    # (the everyday entries, told by exact types: a batch has a thousand of them)
            op, partner, arg = e
            if type(partner) is int and 0 <= partner < n:
                if op == "mixup" and type(arg) is float and 0.0 <= arg <= 1.0 and not u8:
                    out.append(e)
                    continue
                if op == "cutmix" and type(arg) is tuple and len(arg) == 4:
                    x, y, w, h = arg
                    if (type(x) is int and type(y) is int and type(w) is int and type(h) is int and w >= 1 and h >= 1 and x >= 0 and y >= 0
                            and x + w <= W and y + h <= H):
                        out.append(e)
                        continue
        if not isinstance(e, (tuple, list)) or len(e) != 3 or not isinstance(e[0], str):
            raise ValueError(f"mix: output {k}: an entry is None, (\"mixup\", partner, lam) or (\"cutmix\", partner, (x, y, width, height)), not {e!r}")
        op, partner, arg = e
        if op not in ("mixup", "cutmix"):
            raise ValueError(f"mix: output {k}: unknown op {op!r} (\"mixup\", \"cutmix\")")
        if not _is_int(partner) or not 0 <= int(partner) < n:
            raise ValueError(f"mix: output {k}: partner {partner!r} is not the index of an output, an integer 0..{n - 1}")
        partner = int(partner)
        if op == "mixup":
            if u8:
                raise ValueError(f"mix: output {k}: \"mixup\" needs a float output (dtype= or normalize=), not uint8; \"cutmix\" takes any")
            if not _is_number(arg) or not math.isfinite(float(arg)) or not 0.0 <= float(arg) <= 1.0:
                raise ValueError(f"mix: output {k}: lam {arg!r} is not a finite number in 0..1")
            out.append(("mixup", partner, float(arg)))
        else:
            if not isinstance(arg, (tuple, list, np.ndarray)) or len(arg) != 4 or not all(_is_int(t) for t in arg):
                raise ValueError(f"mix: output {k}: a box is four integers (x, y, width, height), not {arg!r}")
            x, y, w, h = (int(t) for t in arg)
            if w < 1 or h < 1:
                raise ValueError(f"mix: output {k}: width and height must be at least 1, not {w} x {h}")
            if x < 0 or y < 0 or x + w > W or y + h > H:
                raise ValueError(f"mix: output {k}: box ({x}, {y}, {w}, {h}) is not inside the {W} x {H} canvas")
            out.append(("cutmix", partner, (x, y, w, h)))
    return out if some else None


def cutmix_box(size, lam: float, generator=None):
    """A box for ``("cutmix", partner, box)`` drawn as torchvision v2's ``CutMix`` draws it for a ``size = (width, height)`` canvas and
    a ``lam`` (the caller's Beta draw): ``((x, y, w, h), lam_adjusted)``, or ``(None, 1.0)`` for an empty box.  Restated: ``r = 0.5 *
    sqrt(1 - lam)``, half sides ``int(r * W)`` and ``int(r * H)``, the centre from two ``torch.randint`` draws (x in 0..W-1 first,
    then y in 0..H-1), the box ``centre +- half side`` clamped to the canvas; ``lam_adjusted = 1 - w * h / (W * H)`` is the weight
    of the output's own label.  torchvision is not a dependency here and this function is NOT pinned to its draws."""
    import torch
    W, H = (int(t) for t in size)
    lam = float(lam)
    if not math.isfinite(lam) or not 0.0 <= lam <= 1.0:
        raise ValueError(f"lam {lam!r} is not a finite number in 0..1")
    r = 0.5 * math.sqrt(1.0 - lam)
    rw, rh = int(r * W), int(r * H)
    cx = int(torch.randint(0, W, size=(1,), generator=generator).item())
    cy = int(torch.randint(0, H, size=(1,), generator=generator).item())
    x1, y1 = max(cx - rw, 0), max(cy - rh, 0)
    x2, y2 = min(cx + rw, W), min(cy + rh, H)
    w, h = x2 - x1, y2 - y1
    if w < 1 or h < 1:
        return None, 1.0
    return (x1, y1, w, h), 1.0 - (w * h) / float(W * H)


COMPOSE_MAX_TILES = 64          # tiles of one composed output (csrc/compose_addr.h: kComposeMaxTiles)
COMPOSE_MAX_OFFSET = 1 << 20    # |dx|, |dy| stay below it


def normalize_compose(compose, size, n_outputs: Optional[int] = None, ncomp: Optional[int] = None, return_seams: bool = False, mix=None):
    """``compose`` of a call, checked: None for a call without it, else ``{"size": (W, H), "fill": None or a tuple of bytes,
    "outputs": [[(source, (dx, dy), (sx, sy, w, h)), ...], ...]}`` with every tile in its full form.

    ``compose``: None, or a dict with ``size`` — (W, H) of the composed canvases, 1..65535 each, independent of the call's ``size``,
    which stays the size of the tiles —, optionally ``fill`` — None (the call's ``fill``, 0 where that is absent), one byte 0..255
    or one per output component; it goes through ``dtype`` / ``normalize`` like a pixel — and ``outputs``: a list with one entry
    per composed output, each a list of at most 64 tiles applied in order (``[]``: a canvas of fill).  A tile is ``(source, (dx,
    dy))`` or ``(source, (dx, dy), (sx, sy, w, h))``: the window (default: the whole canvas; x along the width, after the mirror)
    of output ``source`` of the same group lands with its top-left corner at the integers ``(dx, dy)``, which may be negative or
    beyond the canvas; the paste is clipped as ``Image.paste`` clips it and a later tile wins (tools/compose_model.py).  The call
    then returns the ``len(outputs)`` composed canvases in place of the tiles.

    ``compose`` needs ``size`` and goes neither with ``return_seams`` nor, for now, with ``mix`` (:func:`normalize_mix`'s result
    for the same group).  ``n_outputs`` / ``ncomp`` None: not known yet — what needs them is not checked.  ValueError, naming the
    output and the tile, otherwise."""
    if compose is None:
        return None
    if size is None:
        raise ValueError("compose needs size=(width, height): the tiles are the outputs of one array")
    if return_seams:
        raise ValueError("compose and return_seams do not go together: the seam outputs are the decoded images")
    if mix is not None:
        raise ValueError("compose and mix do not go together in one group (for now): mix's entries would have to mean composed outputs")
    if not isinstance(compose, dict):
        raise ValueError(f"compose must be None or a dict (size=, fill=, outputs=), not {compose!r}")
    for key in compose:
        if key not in ("size", "fill", "outputs"):
            raise ValueError(f"compose: unknown key {key!r} (size, fill, outputs)")
    cs = compose.get("size")
    if not isinstance(cs, (tuple, list)) or len(cs) != 2 or not all(_is_int(v) and 1 <= int(v) <= 65535 for v in cs):
        raise ValueError(f"compose: size is required: (width, height) of the composed canvases, 1..65535 each, not {cs!r}")
    fill = compose.get("fill")
    if fill is not None:
        if _is_int(fill):
            fill = (int(fill),) * (ncomp or 1)
        elif isinstance(fill, (tuple, list, np.ndarray)) and 1 <= len(fill) <= 3 and all(_is_int(v) for v in fill) and (ncomp is None or len(fill) == ncomp):
            fill = tuple(int(v) for v in fill)
        else:
            raise ValueError(f"compose: fill must be None, one byte or one per output component ({ncomp if ncomp is not None else '1 or 3'}), not {fill!r}")
        if any(v < 0 or v > 255 for v in fill):
            raise ValueError(f"compose: fill must be 0..255, not {fill!r}")
    outputs = compose.get("outputs")
    if not isinstance(outputs, list) or len(outputs) == 0:
        raise ValueError(f"compose: outputs must be a list with one list of tiles per composed output, at least one, not {outputs!r}")
    W, H = size
    whole = (0, 0, W, H)
    limit = n_outputs if n_outputs is not None else 1 << 31
    out = []
    for m, tiles in enumerate(outputs):
        if not isinstance(tiles, (list, tuple)):
            raise ValueError(f"compose: output {m}: an entry is a list of tiles, not {tiles!r}")
        if len(tiles) > COMPOSE_MAX_TILES:
            raise ValueError(f"compose: output {m}: {len(tiles)} tiles, more than {COMPOSE_MAX_TILES}")
        entry = []
        for t, tile in enumerate(tiles):
            if type(tile) is tuple and len(tile) == 3:      # (the everyday tile, told by exact types: a batch has a thousand of them)
                s, at, win = tile
                if type(s) is int and type(at) is tuple and type(win) is tuple and len(at) == 2 and len(win) == 4 and 0 <= s < limit:
                    (dx, dy), (sx, sy, w, h) = at, win
                    if (type(dx) is int and type(dy) is int and type(sx) is int and type(sy) is int and type(w) is int and type(h) is int
                            and -COMPOSE_MAX_OFFSET < dx < COMPOSE_MAX_OFFSET and -COMPOSE_MAX_OFFSET < dy < COMPOSE_MAX_OFFSET
                            and w >= 1 and h >= 1 and sx >= 0 and sy >= 0 and sx + w <= W and sy + h <= H):
                        entry.append(tile)
                        continue
            where = f"compose: output {m}, tile {t}"
            if not isinstance(tile, (tuple, list)) or len(tile) not in (2, 3):
                raise ValueError(f"{where}: a tile is (source, (dx, dy)) or (source, (dx, dy), (sx, sy, w, h)), not {tile!r}")
            s, at = tile[0], tile[1]
            win = tile[2] if len(tile) == 3 else whole
            if not _is_int(s) or int(s) < 0 or (n_outputs is not None and int(s) >= n_outputs):
                raise ValueError(f"{where}: source {s!r} is not the index of an output, an integer 0..{n_outputs - 1 if n_outputs is not None else 'N-1'}")
            if not isinstance(at, (tuple, list, np.ndarray)) or len(at) != 2 or not all(_is_int(v) for v in at):
                raise ValueError(f"{where}: the offset is two integers (dx, dy), not {at!r}")
            if not isinstance(win, (tuple, list, np.ndarray)) or len(win) != 4 or not all(_is_int(v) for v in win):
                raise ValueError(f"{where}: the window is four integers (sx, sy, w, h), not {win!r}")
            dx, dy = (int(v) for v in at)
            if abs(dx) >= COMPOSE_MAX_OFFSET or abs(dy) >= COMPOSE_MAX_OFFSET:
                raise ValueError(f"{where}: offset ({dx}, {dy}) is 2**20 or more from the origin")
            sx, sy, w, h = (int(v) for v in win)
            if w < 1 or h < 1:
                raise ValueError(f"{where}: the window's width and height must be at least 1, not {w} x {h}")
            if sx < 0 or sy < 0 or sx + w > W or sy + h > H:
                raise ValueError(f"{where}: window ({sx}, {sy}, {w}, {h}) is not inside the {W} x {H} tile canvas")
            entry.append((int(s), (dx, dy), (sx, sy, w, h)))
        out.append(entry)
    return {"size": (int(cs[0]), int(cs[1])), "fill": fill, "outputs": out}


def compose_for_components(composed, compose, size, ncomp: int):
    """:func:`normalize_compose`'s result (``composed``, of ``compose``) once the files' component count is known: its fill checked
    against it (the tiles are as they were)"""
    if composed is None:
        return None
    fill = normalize_compose({"size": composed["size"], "fill": compose.get("fill"), "outputs": [[]]}, size, None, ncomp)["fill"]
    return dict(composed, fill=fill)


def mosaic_tiles(size, centre, tile_sizes):
    """The tiles of one four-image mosaic as Ultralytics' ``Mosaic._mosaic4`` places them, for ``compose``'s ``outputs``: ``size`` =
    (W, H) of the composed canvas, ``centre`` = (xc, yc) on it, ``tile_sizes`` = four (w_i, h_i), the extents of the resized images,
    each at the top left of its tile canvas (``place=(0, 0)``).  Image 0 goes top-left of the centre, 1 top-right, 2 bottom-left,
    3 bottom-right, each with its inner corner at the centre, and of each the part next to that corner that the canvas holds is
    taken.  Returns up to four ``(i, (dx, dy), (sx, sy, w, h))``; an image the canvas does not reach is left out.  The centre is
    the caller's draw, and this function is NOT pinned to Ultralytics' draws; boxes and labels stay with the caller."""
    W, H = (int(v) for v in size)
    xc, yc = (int(v) for v in centre)
    if len(tile_sizes) != 4:
        raise ValueError(f"mosaic_tiles takes four (width, height), not {len(tile_sizes)}")
    out = []
    for i, (w, h) in enumerate(tile_sizes):
        w, h = int(w), int(h)
        if i == 0:
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b = w - (x2a - x1a), h - (y2a - y1a)
        elif i == 1:
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, W), yc
            x1b, y1b = 0, h - (y2a - y1a)
        elif i == 2:
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(H, yc + h)
            x1b, y1b = w - (x2a - x1a), 0
        else:
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, W), min(H, yc + h)
            x1b, y1b = 0, 0
        if x2a - x1a >= 1 and y2a - y1a >= 1:
            out.append((i, (x1a, y1a), (x1b, y1b, x2a - x1a, y2a - y1a)))
    return out


PATCH_MAX_PATCH, PATCH_MAX_MERGE, PATCH_MAX_REPEAT = 64, 8, 4      # (csrc/patch_addr.h)
PATCH_BLOCK_BYTES = 65536       # a merge block's most: the least a job of the launch holds
PATCH_KEYS = ("patch", "merge", "repeat", "order", "windows", "length")


def normalize_patches(patches, size, n_outputs: Optional[int] = None, ncomp: Optional[int] = None, dtype: Optional[str] = None,
                      return_seams: bool = False, compose=None):
    """``patches`` of a call, checked: None for a call without it, else ``{"patch": P, "merge": m, "repeat": t, "order": "chw" or
    "hwc", "windows": None or one (x, y, width, height) per source, "length": None or L}``.

    ``patches``: None, or a dict with ``patch`` — P, 1..64, patches are square —, ``merge`` — m, 1..8, default 1: tokens are ordered
    in m x m blocks of patches, Qwen's ``merge_size`` —, ``repeat`` — t, 1..4, default 1: every component's patch is written t times
    in a row, Qwen's ``temporal_patch_size`` for a still image —, ``order`` — "chw" (default): a token is (C, t, P, P) as in
    Qwen2-VL; "hwc": (P, P, C) as in SigLIP 2 NaFlex and timm's NaFlexVit, with ``repeat`` 1; the order of a token's elements is
    this, whatever the decoder's layout —, ``windows`` — None, or one entry per source, None (the whole canvas) or ``(x, y, width,
    height)`` in the coordinates of what the caller would receive, inside the canvas, ``width`` and ``height`` multiples of P * m —
    and ``length`` — None: the packed form, ONE (T, D) array with D = C * t * P * P whose rows ``cu[k] .. cu[k + 1]`` are source
    k's tokens (:func:`patch_grids`); an integer L >= 1: the padded form (N, L, D), the rows behind a source's tokens zero bits.
    A source is an output of the group, or a composed canvas under ``compose`` (``compose``: :func:`normalize_compose`'s result).
    The rule: tools/patch_model.py.  ``n_outputs``, ``ncomp`` and ``dtype`` (a name) are checked against where they are known.

    ``patches`` needs ``size`` and does not go with ``return_seams``.  ValueError naming the source otherwise."""
    if patches is None:
        return None
    if size is None:
        raise ValueError("patches needs size=(width, height): the sources are the outputs of one array")
    if return_seams:
        raise ValueError("patches and return_seams do not go together: the seam outputs are the decoded images")
    if not isinstance(patches, dict):
        raise ValueError(f"patches must be None or a dict (patch=, merge=, repeat=, order=, windows=, length=), not {patches!r}")
    for key in patches:
        if key not in PATCH_KEYS:
            raise ValueError(f"patches: unknown key {key!r} ({', '.join(PATCH_KEYS)})")
    out = {}
    for key, most, default in (("patch", PATCH_MAX_PATCH, None), ("merge", PATCH_MAX_MERGE, 1), ("repeat", PATCH_MAX_REPEAT, 1)):
        v = patches.get(key, default)
        if not _is_int(v) or not 1 <= int(v) <= most:
            raise ValueError(f"patches: {key} must be an integer 1..{most}, not {v!r}")
        out[key] = int(v)
    P, m, t = out["patch"], out["merge"], out["repeat"]
    order = patches.get("order", "chw")
    if order not in ("chw", "hwc"):
        raise ValueError(f"patches: order must be 'chw' or 'hwc', not {order!r}")
    if order == "hwc" and t != 1:
        raise ValueError(f"patches: order 'hwc' needs repeat 1, not {t}")
    out["order"] = order
    length = patches.get("length")
    if length is not None and (not _is_int(length) or int(length) < 1 or int(length) >= 1 << 31):
        raise ValueError(f"patches: length must be None or an integer of at least 1, not {length!r}")
    out["length"] = None if length is None else int(length)
    esize = B.DTYPE_BYTES[dtype] if dtype is not None else 1
    block = m * m * (ncomp or 1) * t * P * P * esize
    if block > PATCH_BLOCK_BYTES:
        raise ValueError(f"patches: a merge block of {block} bytes (merge {m}, patch {P}, repeat {t}, {ncomp or 1} components of {esize} bytes), "
                         f"more than {PATCH_BLOCK_BYTES}")
    if compose is not None:                     # (the sources are the composed canvases)
        size, n_outputs = compose["size"], len(compose["outputs"])
    W, H = size
    u = P * m
    windows = patches.get("windows")
    if windows is not None:
        if not isinstance(windows, (list, tuple)):
            raise ValueError(f"patches: windows must be None or a list with one entry per source, not {windows!r}")
        if n_outputs is not None and len(windows) != n_outputs:
            raise ValueError(f"patches: windows has {len(windows)} entries for {n_outputs} sources")
    full = []
    for k in range(len(windows) if windows is not None else 1 if n_outputs is None else n_outputs):
        win = windows[k] if windows is not None else None
        if win is None:
            if W % u or H % u:
                raise ValueError(f"patches: source {k}: the whole {W} x {H} canvas is not a multiple of patch * merge = {u} per side")
            x, y, w, h = 0, 0, W, H
        else:
            if not isinstance(win, (tuple, list, np.ndarray)) or len(win) != 4 or not all(_is_int(v) for v in win):
                raise ValueError(f"patches: source {k}: a window is None or four integers (x, y, width, height), not {win!r}")
            x, y, w, h = (int(v) for v in win)
            if w < 1 or h < 1 or x < 0 or y < 0 or x + w > W or y + h > H:
                raise ValueError(f"patches: source {k}: window ({x}, {y}, {w}, {h}) is not inside the {W} x {H} canvas")
            if w % u or h % u:
                raise ValueError(f"patches: source {k}: window ({x}, {y}, {w}, {h}) is not a multiple of patch * merge = {u} per side")
        if out["length"] is not None and (w // P) * (h // P) > out["length"]:
            raise ValueError(f"patches: source {k}: {(w // P) * (h // P)} tokens, more than length {out['length']}")
        full.append((x, y, w, h))
    out["windows"] = full if windows is not None else None
    return out


def patches_for_components(patched, patches, size, n_outputs: int, ncomp: int, dtype: str, compose=None):
    """:func:`normalize_patches`' result (``patched``, of ``patches``) once the files' component count and so the bytes of a merge
    block are known"""
    if patched is None:
        return None
    return normalize_patches(patches, size, n_outputs, ncomp, dtype, compose=compose)


def patch_grids(patches, n_sources: int, size):
    """``(grids, cu)`` of a ``patches`` value for ``n_sources`` sources on canvases of ``size`` = (width, height) — the composed
    canvases' size under ``compose`` —: ``grids``, an int64 array (N, 2) of (gh, gw), the patches down and across of every source
    (Qwen's ``image_grid_thw`` without the 1, NaFlex's spatial shapes), and ``cu``, an int64 array (N + 1,) of row offsets — source
    k's tokens are rows ``cu[k] .. cu[k + 1]`` of the packed form: the ``cu_seqlens`` of a variable-length attention call.  In the
    padded form source k's tokens are rows ``0 .. cu[k + 1] - cu[k]`` of ``out[k]``.  A convenience that restates the rule; NOT
    pinned to any processor's own arrays."""
    spec = normalize_patches(patches, normalize_size(size), int(n_sources))
    if spec is None:
        raise ValueError("patch_grids takes a patches dict, not None")
    W, H = normalize_size(size)
    P = spec["patch"]
    wins = spec["windows"] if spec["windows"] is not None else [(0, 0, W, H)] * int(n_sources)
    grids = np.array([(h // P, w // P) for _, _, w, h in wins], dtype=np.int64).reshape(-1, 2)
    cu = np.zeros(len(grids) + 1, dtype=np.int64)
    np.cumsum(grids[:, 0] * grids[:, 1], out=cu[1:])
    return grids, cu


def smart_resize(height: int, width: int, factor: int = 28, min_pixels: int = 56 * 56, max_pixels: int = 14 * 14 * 4 * 1280):
    """Qwen2-VL's size rule in plain Python, for ``resize_to``: ``(height, width)``, both multiples of ``factor``, their product
    within ``min_pixels .. max_pixels``, the aspect ratio kept as closely as that allows.  Each side is rounded to the nearest
    multiple of ``factor``; beyond ``max_pixels`` both are scaled down by sqrt(height * width / max_pixels) and rounded DOWN to
    multiples, below ``min_pixels`` scaled up and rounded UP.  An aspect ratio beyond 200 is refused, as there.  A restatement; NOT pinned to any release of the processor."""
    import math
    height, width, factor = int(height), int(width), int(factor)
    if height < 1 or width < 1 or factor < 1:
        raise ValueError(f"smart_resize: height {height}, width {width}, factor {factor}")
    if max(height, width) / min(height, width) > 200:
        raise ValueError(f"smart_resize: an aspect ratio beyond 200: {max(height, width) / min(height, width)}")
    h_bar = max(factor, round(height / factor) * factor)
    w_bar = max(factor, round(width / factor) * factor)
    if h_bar * w_bar > max_pixels:
        beta = math.sqrt((height * width) / max_pixels)
        h_bar = max(factor, math.floor(height / beta / factor) * factor)
        w_bar = max(factor, math.floor(width / beta / factor) * factor)
    elif h_bar * w_bar < min_pixels:
        beta = math.sqrt(min_pixels / (height * width))
        h_bar = math.ceil(height * beta / factor) * factor
        w_bar = math.ceil(width * beta / factor) * factor
    return h_bar, w_bar


def rotation_matrix(angle: float, size: Tuple[int, int], center=None, translate=None) -> Tuple[float, ...]:
    """The matrix ``Image.rotate(angle, center=center, translate=translate)`` builds for ``expand=False`` on an image of ``size`` =
    (width, height) — counter-clockwise by ``angle`` degrees around ``center`` (None: the image's centre), then moved by
    ``translate`` — its ``round(.., 15)`` of the sine and cosine included: ``decode(.., affine=rotation_matrix(a, img.size))`` is
    ``img.rotate(a, resample, fillcolor=fill)``.  At angles that are multiples of 90 Pillow does not transform in some cases (0: a
    copy; 180, and 90 / 270 of a square image or with expand, without center and translate: a transpose), so its result there is
    not this matrix's for every filter."""
    w, h = size
    angle = angle % 360.0
    tx, ty = translate if translate is not None else (0, 0)
    cx, cy = center if center is not None else (w / 2.0, h / 2.0)
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def transform(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2], m[5] = transform(-cx - tx, -cy - ty)
    m[2] += cx
    m[5] += cy
    return tuple(m)


def _is_resize_kind(k) -> bool:
    """one file's ``resize_to``: an int (the shorter side), (width, height) or "contain" """
    if isinstance(k, str):
        return k == "contain"
    if _is_int(k):
        return 1 <= int(k) <= 65535
    return isinstance(k, tuple) and len(k) == 2 and all(_is_int(v) and 1 <= int(v) <= 65535 for v in k)


def resized_size(kind, w: int, h: int, canvas: Tuple[int, int]) -> Tuple[int, int]:
    """The (width, height) a w x h image is resized to under one file's ``resize_to`` (tools/place_model.py: resized_size).  An
    int ``s``: torchvision's ``Resize(s)`` — the shorter side becomes s, the longer ``int(s * long / short)``.  (width, height):
    that.  "contain": Pillow's ``ImageOps.contain`` into the canvas — ``round(h / w * W)`` or ``round(w / h * H)``, half to even."""
    if isinstance(kind, str):
        cw, ch = canvas
        im_ratio, dest_ratio = w / h, cw / ch
        if im_ratio == dest_ratio:
            return cw, ch
        return (cw, round(h / w * cw)) if im_ratio > dest_ratio else (round(w / h * ch), ch)
    if isinstance(kind, tuple):
        return int(kind[0]), int(kind[1])
    short, long = sorted((w, h))
    new_long = int(int(kind) * long / short)
    return (int(kind), new_long) if w <= h else (new_long, int(kind))


def centred(kind, resized: Tuple[int, int], canvas: Tuple[int, int]) -> Tuple[int, int]:
    """Where the resized image's top-left lies on the canvas by the rule of its ``resize_to`` kind (tools/place_model.py:
    centred): torchvision's ``center_crop`` — crop at ``int(round((r - c) / 2.0))``, pad ``(c - r) // 2`` in front — or, for
    "contain", ``ImageOps.pad``'s ``round((c - r) * 0.5)``."""
    if isinstance(kind, str):
        return tuple(round((c - r) * 0.5) for r, c in zip(resized, canvas))
    return tuple(-int(round((r - c) / 2.0)) if r >= c else (c - r) // 2 for r, c in zip(resized, canvas))


def normalize_fill(fill, resize_to, ncomp: Optional[int] = None) -> Optional[Tuple[int, ...]]:
    """The fill of a placed decode, checked: None, or one byte 0..255 per output component (``ncomp``; None: not known yet) —
    from one int for all of them or a sequence of that length.  It needs ``resize_to``.  ValueError otherwise."""
    if fill is None:
        return None
    if resize_to is None:
        raise ValueError("fill needs resize_to: without it every image covers the whole of size")
    if _is_int(fill):
        vals = [int(fill)] * (ncomp or 1)
    else:
        ok = isinstance(fill, (tuple, list, np.ndarray)) and 1 <= len(fill) <= 3 and all(_is_int(v) for v in fill)
        if not ok or (ncomp is not None and len(fill) != ncomp):
            raise ValueError(f"fill must be one int or one per output component ({ncomp if ncomp is not None else '1 or 3'}), 0..255 each, not {fill!r}")
        vals = [int(v) for v in fill]
    if any(v < 0 or v > 255 for v in vals):
        raise ValueError(f"fill must be one int or one per output component, 0..255 each, not {fill!r}")
    return tuple(vals)


def normalize_places(resize_to, place, size, dims: Optional[Sequence[Tuple[int, int]]] = None, index: Optional[Sequence[int]] = None):
    """The placement of a decode onto a canvas, checked: None for a call without it, else one (width, height, x, y) per file — the
    size the file's image (as its orientation shows it; its window, with ``rois``) is resized to, and where its top-left lies on
    the canvas ``size``; or None where every file is stretched over the whole canvas, which is a call without the arguments.

    ``resize_to``: None, an int (the shorter side: torchvision's ``Resize``), a tuple (width, height), "contain" (Pillow's
    ``ImageOps.contain``), or a list with one of these per file.  ``place``: None (centred by the rule of the file's kind:
    :func:`centred`), one (x, y), or a list with (x, y) or None per file.  Both need ``size``; ``place`` needs ``resize_to``.
    ``dims``: the files' (width, height); None: not known yet — everything but the lengths and the geometry is checked.
    ValueError naming the file (``index``: its position in the caller's list) otherwise."""
    if resize_to is None:
        if place is not None:
            raise ValueError("place needs resize_to: without it every image covers the whole of size")
        return None
    if size is None:
        raise ValueError("resize_to needs size=(width, height): the canvas the resized images are placed on")
    per_file = isinstance(resize_to, list)       # ((width, height) is a tuple; a list is one entry per file)
    for k in (resize_to if per_file else [resize_to]):
        if not _is_resize_kind(k):
            raise ValueError(f"resize_to must be None, an int 1..65535 (the shorter side), a tuple (width, height), 'contain' or a list with one of "
                             f"these per file, not {resize_to!r}")

    def is_xy(v) -> bool:
        return isinstance(v, (tuple, list, np.ndarray)) and len(v) == 2 and all(_is_int(t) and abs(int(t)) <= 65535 for t in v)
    one_xy = place is None or is_xy(place)
    if not one_xy:
        if not isinstance(place, (list, tuple)) or not all(v is None or is_xy(v) for v in place):
            raise ValueError(f"place must be None, one (x, y) of integers within +-65535 or a list with (x, y) or None per file, not {place!r}")
    if dims is None:
        return None
    n = len(dims)
    if per_file and len(resize_to) != n:
        raise ValueError(f"resize_to has {len(resize_to)} entries for {n} files")
    if not one_xy and len(place) != n:
        raise ValueError(f"place has {len(place)} entries for {n} files")
    out, plain = [], True
    for i, (w, h) in enumerate(dims):
        kind = resize_to[i] if per_file else resize_to
        xy = place if one_xy else place[i]
        name = i if index is None else index[i]
        rw, rh = resized_size(kind, int(w), int(h), size)
        if rw < 1 or rh < 1 or rw > 65535 or rh > 65535:
            raise ValueError(f"file {name}: resize_to={kind!r} makes the {w}x{h} image {rw}x{rh}; both sides must be 1..65535")
        x, y = (int(v) for v in xy) if xy is not None else centred(kind, (rw, rh), size)
        if x >= size[0] or y >= size[1] or x + rw <= 0 or y + rh <= 0:
            raise ValueError(f"file {name}: the {rw}x{rh} image at ({x}, {y}) does not meet the {size[0]}x{size[1]} canvas")
        plain = plain and (rw, rh, x, y) == (size[0], size[1], 0, 0)
        out.append((rw, rh, x, y))
    return None if plain else out


_TRANSPOSING = (5, 6, 7, 8)          # EXIF orientations that exchange width and height (tools/orient_model.py)


def normalize_orientation(orientation, files: Sequence[bytes]) -> Optional[List[int]]:
    """The EXIF orientation every file of a call is decoded with, 1..8 each — or None where all of them are 1, which is a call
    without the argument.  ``orientation``: None; "exif" (every file's own tag, :func:`exif_orientation`; 1 without one); one
    int 1..8 for every file; or a sequence with one int, "exif" or None per file.  ValueError for anything else."""
    n = len(files)

    def is_value(v) -> bool:
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and 1 <= int(v) <= 8

    if orientation is None:
        return None
    if isinstance(orientation, str):
        if orientation != "exif":
            raise ValueError(f"orientation must be None, 'exif', an int 1..8 or one of these per file, not {orientation!r}")
        turns = B.exif_orientations(files).tolist()
    elif is_value(orientation):
        turns = [int(orientation)] * n
    else:
        if isinstance(orientation, (int, float, bool, np.number, np.bool_, bytes)):
            raise ValueError(f"orientation must be None, 'exif', an int 1..8 or one of these per file, not {orientation!r}")
        try:
            entries = orientation.tolist() if hasattr(orientation, "tolist") else list(orientation)
        except TypeError:
            raise ValueError(f"orientation must be None, 'exif', an int 1..8 or one of these per file, not {orientation!r}") from None
        if len(entries) != n:
            raise ValueError(f"orientation has {len(entries)} entries for {n} files")
        turns = []
        for i, v in enumerate(entries):
            if v is None:
                turns.append(1)
            elif isinstance(v, str) and v == "exif":
                turns.append(exif_orientation(bytes(files[i])))
            elif is_value(v):
                turns.append(int(v))
            else:
                raise ValueError(f"file {i}: orientation {v!r} is none of None, 'exif' and an int 1..8")
    return turns if any(t != 1 for t in turns) else None


def _oriented_dims(dims, orient: Optional[List[int]]):
    """(width, height) of every file as its orientation shows it."""
    if orient is None:
        return list(dims)
    return [(h, w) if o in _TRANSPOSING else (w, h) for (w, h), o in zip(dims, orient)]


def _orient_class(o: int, sized: bool) -> int:
    """What keeps files of different orientations out of one plan: upright files form the plans they form without the argument
    (0); with ``size`` the orientations that exchange width and height read their source the other way and are a launch of
    their own (2), the other turned ones (1)."""
    return 0 if o == 1 else (2 if sized and o in _TRANSPOSING else 1)


def raise_for_status(status: np.ndarray, index: Optional[Sequence[int]] = None):
    """Raise for the first image of a plan whose status is not 0.  ``index``: where every image of the plan sits in the
    caller's list of files (None: the plan is that list) — the message names that position, not the one inside the plan."""
    bad = np.flatnonzero(status)
    if bad.size:
        k = int(bad[0])
        i = k if index is None else int(index[k])
        if int(status[k]) == B.MJ_ST_INTERNAL:          # not the file's fault (include/mijpeg.h)
            raise B.BackendError(f"image {i}: a fused launch gave up waiting for its decoder wavefronts (internal error)")
        raise CorruptedJpeg(f"image {i}: {_STATUS_TEXT.get(int(status[k]), 'decode failed')}")


@dataclass
class _Request:
    """What one call asks of a set of files: the windows (:func:`normalize_rois`' list, or None), ``size``
    (:func:`normalize_size`'s, or None), the model-ready output (or None) and, with ``size``, the array or tensor the plans
    write the images into and every file's slot in it (both None: every plan fills a dense array of its own).  ``index``:
    where every file sits in the list the caller passed, for the messages of errors (None: this is that list).  ``orient``:
    :func:`normalize_orientation`'s list (None: every file as stored); the windows are then windows of the oriented images.
    ``resample``: :func:`normalize_resample`'s filter of the resize (None: bilinear, the request of a call without the argument).
    ``mode``: :func:`normalize_mode`'s output colour mode (None: every file's own components).
    ``places``: :func:`normalize_places`' list (None: every image stretched over ``size``, the request of a call without
    ``resize_to``) and ``fill``: :func:`normalize_fill`'s bytes for the canvas elements no image covers (None: zeros).
    ``reducing_gap``: :func:`normalize_reducing_gap`'s gap of the two-step resize (None: one step).
    ``views``: :func:`normalize_views`' list (None: one output per file) — the OUTPUTS of the request, each a window of one of
    ``files``; ``slots``, the mirror flags and ``places`` then have one entry per view, ``wins`` is None, and every file is named
    by a view."""
    files: Sequence[bytes]
    wins: Optional[List[Tuple[int, int, int, int]]] = None
    size: Optional[Tuple[int, int]] = None
    output: Optional[OutputSpec] = None
    dest: object = None
    slots: Optional[List[int]] = None
    index: Optional[List[int]] = None
    orient: Optional[List[int]] = None
    resample: Optional[str] = None
    mode: Optional[str] = None
    places: Optional[List[Tuple[int, int, int, int]]] = None
    fill: Optional[Tuple[int, ...]] = None
    reducing_gap: Optional[float] = None
    views: Optional[List[Tuple[int, Tuple[int, int, int, int]]]] = None
    affine: Optional[AffineSpec] = None         # :func:`normalize_transform`'s, affine or perspective (None: no transform); always with ``views``
    colour: Optional[List[Optional[tuple]]] = None      # :func:`normalize_color_ops`' chains, one or None per OUTPUT (None: no operations)
    erase: Optional[List[Optional[tuple]]] = None       # :func:`normalize_erase`'s boxes, a tuple or None per OUTPUT (None: no box anywhere)
    # :func:`normalize_mix`'s entries, one or None per OUTPUT of the whole group (None: no mixing).  The CALL's, not a plan's: the
    # requests of its parts, kinds and rounds (:meth:`narrow`) do not carry it, and it is applied once they have all been collected
    mix: Optional[List[Optional[tuple]]] = None
    # :func:`normalize_compose`'s dict (None: the outputs as they are).  The CALL's as ``mix`` is: the group's tensor is composed into a
    # new one of ``compose["size"]`` once every plan has been collected
    compose: Optional[dict] = None
    # :func:`normalize_patches`' dict (None: the outputs as they are).  The CALL's too, and its last step: the group's tensor — mixed or
    # composed where it is — is packed into a new one of token rows
    patches: Optional[dict] = None
    # the extra groups of a call with ``also``: requests over the SAME files, index and orientations, each with its own size, views, output,
    # tensor and slots (None: a call without).  A group with views need not name every file here; what it has none of it is left out of.
    also: Optional[List["_Request"]] = None

    @property
    def n_outputs(self) -> int:
        return len(self.views) if self.views is not None else len(self.files)

    @property
    def groups(self) -> List["_Request"]:
        """the request's groups of outputs: itself, then the extra ones"""
        return [self] + list(self.also or [])

    @property
    def ncomp(self) -> Optional[int]:
        """the components of every output under the request's mode (None: the files' own)"""
        return B.MODES[self.mode] if self.mode is not None else None

    def narrow(self, idxs) -> "_Request":
        """the same request for some of its files: their windows, slots, mirror flags, orientations and positions in the call go
        with them (files that are all upright: no orientations, the request a call without the argument makes)"""
        idxs = [int(i) for i in idxs]
        index = self.index if self.index is not None else range(len(self.files))

        def pick(per_file):
            return [per_file[i] for i in idxs] if per_file is not None else None
        orient = pick(self.orient)
        if orient is not None and all(o == 1 for o in orient):
            orient = None

        def chains(picked):                 # (outputs without operations / boxes: the request of a call without color_ops / erase)
            return picked if picked is not None and any(c is not None for c in picked) else None
        also = [g.narrow(idxs) for g in self.also] if self.also is not None else None      # (every group follows the files)
        if self.views is not None:
            # a file takes its views with it: they keep their order, and what is per view goes with the view
            pos = {i: k for k, i in enumerate(idxs)}
            vk = [k for k, (f, _) in enumerate(self.views) if f in pos]

            def pick_view(per_view):
                return [per_view[k] for k in vk] if per_view is not None else None
            affine = (AffineSpec(pick_view(self.affine.matrices), self.affine.resample, self.affine.fill, self.affine.perspective)
                      if self.affine is not None else None)
            if affine is not None and all(m is None for m in affine.matrices):
                affine = None
            return _Request(pick(self.files), None, self.size, self.output.for_files(vk) if self.output else None, self.dest, pick_view(self.slots),
                            pick(index), orient, self.resample, self.mode, pick_view(self.places), self.fill, self.reducing_gap,
                            [(pos[self.views[k][0]], self.views[k][1]) for k in vk], affine, chains(pick_view(self.colour)), chains(pick_view(self.erase)), also=also)
        return _Request(pick(self.files), pick(self.wins), self.size, self.output.for_files(idxs) if self.output else None,
                        self.dest, pick(self.slots), pick(index), orient, self.resample, self.mode, pick(self.places), self.fill, self.reducing_gap,
                        colour=chains(pick(self.colour)), erase=chains(pick(self.erase)), also=also)

    def orient_classes(self) -> List[List[int]]:
        """its files (indices) sorted by :func:`_orient_class`: what cannot share a plan because of its orientation — and, in a
        request with extra groups, by the groups that name them: a plan's groups then each name every file of it"""
        if self.orient is None and self.also is None:
            return [list(range(len(self.files)))]
        classes: Dict[tuple, List[int]] = {}
        for i, key in enumerate(self.plan_keys()):
            classes.setdefault(key, []).append(i)
        return list(classes.values())

    def plan_keys(self) -> Optional[List[tuple]]:
        """per file, what keeps it apart from files of its kind: its :func:`_orient_class` and, in a request with extra groups, which
        of the groups have an output of it (None: nothing does, for any file)"""
        if self.orient is None and self.also is None:
            return None
        named = [None if g.views is None else {f for f, _ in g.views} for g in self.groups] if self.also is not None else []
        return [(_orient_class(self.orient[i], self.size is not None) if self.orient is not None else 0,) + tuple(s is None or i in s for s in named)
                for i in range(len(self.files))]

    def plan_kwargs(self, native: Optional[int] = None) -> dict:
        """``rois``, ``size``, ``slots``, ``output``, ``orientation``, ``filter`` and ``mode`` of :class:`_binding.Plan` for one plan of all
        its files, in order (``native``: the component count these files have, which decides whether the plan converts)"""
        kw = {"rois": self.wins, "size": self.size,
              "slots": (self.slots, self.dest.shape[0]) if self.slots is not None and self.dest is not None else None,
              "output": self.output.plan_output() if self.output else None}
        if self.views is not None:          # (one output per file: the arguments of a call without views)
            kw["views"] = self.views
        if self.orient is not None:         # (files as stored: the arguments of a call without orientation)
            kw["orientation"] = self.orient
        if self.resample is not None:       # (bilinear: the arguments of a call without resample)
            kw["filter"] = self.resample
        if self.mode is not None and native != self.ncomp:      # (files of the mode's own count: the arguments of a call without mode)
            kw["mode"] = self.mode
        if self.places is not None:         # (every image over the whole of size: the arguments of a call without resize_to)
            kw["places"], kw["fill"] = self.places, self.fill
            kw.setdefault("mode", self.mode)
        if self.reducing_gap is not None:   # (one step: the arguments of a call without reducing_gap)
            kw["reducing_gap"] = self.reducing_gap
        if self.affine is not None:         # (no output transformed: the arguments of a call without affine)
            kw["perspective" if self.affine.perspective else "affine"] = (self.affine.matrices, self.affine.resample, self.affine.fill)
        if self.colour is not None:         # (no output with operations: the arguments of a call without color_ops)
            kw["colour"] = self.colour
        return kw


@dataclass
class _Work:
    """One plan still to be made: the files (indices into the call's request), how their batch is assembled — ``prep`` (done
    already), by the native front end, or else by the Python path from the call's parsed headers — and that plan's extra
    MJ_FLAG_* bits."""
    idxs: List[int]
    prep: Optional[PreparedBatch] = None
    native: bool = False
    flags: int = 0


@dataclass
class _Flight:
    """A submitted plan: the request it serves (``idxs``: where its files sit in the call's request, when it serves a part of
    one), and the tensors its kernels touch, which stay alive here until the plan has been collected."""
    req: _Request
    idxs: Optional[List[int]]
    prep: PreparedBatch
    plan: B.Plan
    d_rgb: object = None
    d_blob: object = None
    # a request with extra groups: the plans derived from ``plan`` — (the group's request for these files, its plan) —, executed
    # right behind it on its stream, each into its group's tensor; synced and closed with it
    extra: list = field(default_factory=list)

    def sync(self):
        for p in [self.plan] + [p for _, p in self.extra]:
            p.sync()

    def close(self):
        for p in [p for _, p in self.extra] + [self.plan]:
            p.close()


def _group_by_kind(files: Sequence[bytes], idxs, parsed: Dict[int, ParsedJpeg], headers_only: bool, turn=None, index=None) -> List[List[int]]:
    """Files ``idxs`` sorted into one index list per kind — what can share a plan (``turn``: index -> :func:`_orient_class`,
    part of the kind; None: no file is turned).  Those that ``parsed`` (index -> ParsedJpeg)
    does not hold yet are parsed into it (``headers_only`` as asked); every one goes through :func:`check_supported`.
    ``index`` (a call with views): every file's position in the caller's list, which an error about the file then names."""
    groups: Dict[tuple, List[int]] = {}
    for i in idxs:
        p = parsed.get(i)
        if p is None:
            p = parsed[i] = _named(index, i, parse_jpeg, files[i], headers_only=headers_only)
        _named(index, i, check_supported, p)
        comps = list(p.color_components.values())
        key = (p.scan_mode, len(comps), p.headers_only, is_scan_list(p), p.headers_only and p.restart_interval > 0, turn[i] if turn is not None else 0) + (tuple((c.horizontal_sampling, c.vertical_sampling) for c in comps) if len(comps) > 1 else ())
        groups.setdefault(key, []).append(i)
    return list(groups.values())


def _triage(status: np.ndarray, idxs, files: Optional[Sequence[bytes]] = None, parsed: Optional[Dict[int, ParsedJpeg]] = None,
            index: Optional[Sequence[int]] = None):
    """Sort a plan's per-image status (``idxs``: every image's index in the request the plan is a part of; ``index``: its
    position in the caller's list, which an error names — None: the same).  Returns (tail, unconverged): the files the
    GPU scan handed back (MJ_ST_TAIL: something other than EOI follows the scan — the host finds their segments) and those whose
    synchronisation rounds had not settled (MJ_ST_UNCONVERGED: the serial walk, MJ_FLAG_NO_SYNC).  Both go round again, so
    their entries are zeroed before :func:`raise_for_status` sees the rest.  With ``parsed`` (index -> ParsedJpeg of
    ``files``) the host parse those files' next round needs is stored there first: what the parser raises comes before what
    the status says."""
    idxs = np.asarray(idxs)
    tail = idxs[status == B.MJ_ST_TAIL].tolist()
    unconverged = idxs[status == B.MJ_ST_UNCONVERGED].tolist()
    if parsed is not None:
        for i in tail + [i for i in unconverged if i not in parsed]:
            parsed[i] = parse_jpeg(files[i])
            check_supported(parsed[i])
    status[(status == B.MJ_ST_TAIL) | (status == B.MJ_ST_UNCONVERGED)] = 0
    raise_for_status(status, idxs if index is None else index)
    return tail, unconverged


class BatchDecoder:
    """Decode lists of baseline JPEG files on one GPU.

    >>> dec = BatchDecoder(device=0)
    >>> images = dec.decode([open(p, 'rb').read() for p in paths])      # list of uint8 (W,H,3) arrays
    """

    def __init__(self, device: int = 0, layout: str = "xmajor", exact_only: bool = False, spec_refine: bool = False,
                 segment: str = "gpu", native_host: bool = True, gpu_segment_min_files: int = 8):
        self.ctx = B.Context(device)
        # "planar" / "planar_rowmajor": the components apart, (3, W, H) / (3, H, W) per colour image
        self.layout = {"xmajor": B.MJ_LAYOUT_XMAJOR, "rowmajor": B.MJ_LAYOUT_ROWMAJOR, "planar": B.MJ_LAYOUT_PLANAR_XMAJOR,
                       "planar_rowmajor": B.MJ_LAYOUT_PLANAR_ROWMAJOR}[layout]
        # exact_only: stage 2 uses the reference's summation order for every block (slow; for A/B checks)
        # spec_refine: progressive AC refinement as ITU-T T.81 defines it instead of the reference's behaviour
        self.base_flags = (B.MJ_FLAG_EXACT_ONLY if exact_only else 0) | (B.MJ_FLAG_SPEC_REFINE if spec_refine else 0)
        # segment="gpu" (the default since round 5): the host parses headers only; restart markers and the end of each
        # baseline scan are found on the GPU — the host's NumPy marker search was 76x the GPU step for a
        # batch of 1024 files.  Files the GPU scan hands back (MJ_ST_TAIL: something other than EOI follows the scan) and
        # progressive files take the host path, as do calls with fewer than `gpu_segment_min_files` files (below).
        # segment="host": the marker loop's restart segmentation in Python for every file (jpeg_decoder.py:667-669, :898).
        if segment not in ("host", "gpu"):
            raise ValueError("segment must be 'host' or 'gpu'")
        self.gpu_segment = segment == "gpu"
        # native_host: with segment="gpu", decode_device reads headers and assembles batches in libmijpeg.so's
        # multi-threaded host front end instead of _parse.py (identical arrays; anything unusual is handed back to Python)
        self.native_host = native_host
        # segment="gpu" applies from this many files per call on (or from 4 MiB of files on): a handful of ordinary files is
        # segmented on the host, which costs ~1 ms per MB and lets files with restart markers take the chunked stage-1 form
        # (it needs the segment lengths at plan time; one 1080p file: 2.3 ms instead of 6.6)
        self.gpu_segment_min_files = gpu_segment_min_files
        self._staging: Optional[np.ndarray] = None

    def _gpu_segment_for(self, files: Sequence[bytes]) -> bool:
        """segment="gpu" applies from `gpu_segment_min_files` files per call on, or from 4 MiB of files on (see __init__)."""
        return self.gpu_segment and (len(files) >= self.gpu_segment_min_files or sum(map(len, files)) > (4 << 20))

    def plan(self, files: Sequence[bytes], flags: int = 0, blob_device_ptr: int = 0):
        """(prepared batch, plan) for files of ONE kind.  Like decode(), a handful of files is segmented on the host (the plan
        then knows the segment lengths and can take the chunked stage-1 form); from `gpu_segment_min_files` files on the GPU
        finds the markers, and a caller that executes such a plan itself handles MJ_ST_TAIL (a file the scan handed back)."""
        parsed = [parse_jpeg(f, headers_only=True) for f in files] if self._gpu_segment_for(files) else None
        if parsed is not None and not all(p.headers_only for p in parsed):
            parsed = None                       # progressive / multi-scan files: host segmentation for the whole batch
        prep = prepare_batch(files, self.layout, flags | self.base_flags, parsed)
        plan = B.Plan(self.ctx, prep.to_c(blob_device_ptr), {"prep": prep, "n_images": len(prep.parsed)})
        return prep, plan

    def _shape(self, w: int, h: int, nc: int) -> tuple:
        """Array shape of one decoded image in this decoder's layout."""
        wh = (w, h) if (self.layout & 1) == B.MJ_LAYOUT_XMAJOR else (h, w)
        if nc != 3:
            return wh
        return (3,) + wh if self.layout >= B.MJ_LAYOUT_PLANAR_XMAJOR else wh + (3,)

    @staticmethod
    def _out_shapes(prep: PreparedBatch, wins=None, orient=None, ncomp: Optional[int] = None) -> List[Tuple[int, int, int]]:
        """(width, height, ncomp) of every image's output: the image — as its orientation shows it —, or its window; in ``ncomp``
        components (an output colour mode's), or the files' own."""
        shapes = prep.shapes if ncomp is None else [(w, h, ncomp) for (w, h, _) in prep.shapes]
        if wins is None:
            if orient is not None:
                return [(h, w, nc) if o in _TRANSPOSING else (w, h, nc) for (w, h, nc), o in zip(shapes, orient)]
            return list(shapes)
        return [(w[2], w[3], nc) for w, (_, _, nc) in zip(wins, shapes)]

    def _views(self, flat, shapes: Sequence[Tuple[int, int, int]], per_pixel: int = 1) -> list:
        """Per-image views of a flat buffer (NumPy array or torch tensor) that holds images of ``shapes`` back to back."""
        out, off = [], 0
        for (w, h, nc) in shapes:
            n = w * h * nc * per_pixel
            out.append(flat[off:off + n].reshape(self._shape(w, h, nc)))
            off += n
        return out

    def split_outputs(self, prep: PreparedBatch, flat: np.ndarray, per_pixel: int = 1, wins=None, orient=None, ncomp=None) -> List[np.ndarray]:
        return self._views(flat, self._out_shapes(prep, wins, orient, ncomp), per_pixel)

    def _plan(self, req: _Request, prep: PreparedBatch, blob_device_ptr: int = 0) -> B.Plan:
        """The plan of a request whose files are ``prep``'s, in order."""
        native = prep.shapes[0][2] if prep.shapes else None
        return B.Plan(self.ctx, prep.to_c(blob_device_ptr), {"prep": prep, "n_images": len(req.files)}, **req.plan_kwargs(native))

    def _set_erase(self, g: _Request, plan: B.Plan, native: Optional[int], host: bool) -> None:
        """Group ``g``'s boxes (:func:`normalize_erase`) onto its plan (mj_plan_set_erase): output k of the plan is output k of ``g``.
        All blocks of values go into ONE array of the output's type — host arrays converted and concatenated on the host and uploaded
        once, device tensors converted where they are, one ``torch.cat`` on torch's current stream, which the stream the plan
        executes on is made to wait for before the execute — that the plan holds until it is closed.  ``host``: the NumPy route,
        whose array lives in a block of the HIP runtime's own."""
        dtype = g.output.dtype if g.output else "uint8"
        # mj_erase_rect records as tuples (output, x, y, width, height, kind, value[3], offset), made into the array in one call
        rects, blocks = [], []                  # blocks: (record, values), host ones first below
        for k, boxes in enumerate(g.erase):
            for (x, y, w, h, v) in boxes or ():
                if type(v) is tuple:
                    rects.append((k, x, y, w, h, B.MJ_ERASE_CONST, v + (0.0,) * (3 - len(v)), 0))
                else:
                    blocks.append((len(rects), v))
                    rects.append((k, x, y, w, h, B.MJ_ERASE_VALUES, (0.0, 0.0, 0.0), 0))
        if not blocks:
            plan.set_erase(np.array(rects, dtype=B.ERASE_RECT_DTYPE))
            return
        on_host = [(r, v) for r, v in blocks if not _is_tensor(v) or v.device.type == "cpu"]
        on_device = [(r, v) for r, v in blocks if _is_tensor(v) and v.device.type != "cpu"]
        off = 0
        for r, v in on_host + on_device:
            rects[r] = rects[r][:7] + (off,)
            off += int(v.shape[0]) * int(v.shape[1]) * int(v.shape[2])
        rects = np.array(rects, dtype=B.ERASE_RECT_DTYPE)
        if host:
            flat = np.concatenate([np.ascontiguousarray(v).astype(np.dtype(dtype)).reshape(-1) for _, v in on_host])
            values = B.DeviceBytes(flat)
            plan.set_erase(rects, values.ptr, keep=values)
            return
        import torch
        tdt, dev = getattr(torch, dtype), torch.device("cuda", self.ctx.device)
        parts = []
        if on_host:
            cpu = [(v if _is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(tdt).reshape(-1) for _, v in on_host]
            parts.append((torch.cat(cpu) if len(cpu) > 1 else cpu[0]).to(dev))
        parts += [v.to(tdt).reshape(-1) for _, v in on_device]
        values = torch.cat(parts)               # (a copy even of one block: the caller's tensor is free when the call returns)
        plan.set_erase(rects, values.data_ptr(), keep=values)

    def _group_plans(self, req: _Request, prep: PreparedBatch, blob_device_ptr: int = 0, host: bool = False) -> list:
        """The plans of a request whose files are ``prep``'s, in order, as (group's request, plan): the first group that has outputs
        among these files makes the plan that decodes, every later one that has some derives from it (mj_plan_derive) and reads its
        decoded images; a group with none is left out.  A request without extra groups: its one plan.  A group with boxes
        (``erase``) has them put on its plan here (:meth:`_set_erase`); ``host``: for the NumPy route."""
        native = prep.shapes[0][2] if prep.shapes else None
        plans = []
        try:
            for g in req.groups:
                if g.n_outputs == 0 and req.also is not None:
                    continue
                if not plans:
                    plans.append((g, self._plan(g, prep, blob_device_ptr)))
                    continue
                kw = g.plan_kwargs(native)
                kw.pop("rois")                  # (None: an extra group's windows are views)
                plans.append((g, plans[0][1].derive(prep, **kw)))
            for g, plan in plans:               # (every plan erases the outputs it writes: second rounds and derived plans too)
                if g.erase is not None:
                    self._set_erase(g, plan, native, host)
        except BaseException:
            for _, p in reversed(plans):
                p.close()
            raise
        return plans

    @staticmethod
    def _merged_request(files: Sequence[bytes], orientation, groups: List[dict], build) -> _Request:
        """The request of a call with ``also``: ``groups`` are the keywords of the call's own group and of every extra one
        (:func:`normalize_also`), ``build(files, orientation=, **group)`` the checked request of one group alone.  Every group is
        built as the call it would be alone; the groups are then put over ONE list of files — those that some group names, each
        parsed, uploaded and decoded once — with the call's orientations, and the extra groups hang on the first."""
        kept = select_union_files(files, groups)
        o = _per_file_of(orientation, len(files), kept, "orientation")
        ufiles = [files[i] for i in kept]
        turns = normalize_orientation(o, ufiles)
        full = None
        if turns is not None:                   # (one int per file of the caller's list, which every group picks its files' from)
            full = [1] * len(files)
            for i, t in zip(kept, turns):
                full[i] = t
        pos = {i: k for k, i in enumerate(kept)}
        merged = []
        for k, g in enumerate(groups):
            try:
                merged.append(build(files, orientation=full, **g))
            except ValueError as e:
                if k == 0:
                    raise
                raise ValueError(f"also[{k - 1}]: {e}") from None
        any_views = any(r.views is not None for r in merged)
        for r in merged:
            own = r.index if r.index is not None else range(len(r.files))
            if r.views is not None:
                r.views = [(pos[own[f]], w) for f, w in r.views]
            r.files, r.index, r.orient = ufiles, (kept if any_views else None), turns
        merged[0].also = merged[1:]
        return merged[0]

    def decode(self, files: Sequence[bytes], rois=None, return_seams: bool = False, size=None, dtype=None, normalize=None, mirror=None,
               orientation=None, resample=None, mode=None, resize_to=None, place=None, fill=None, reducing_gap=None, views=None,
               affine=None, affine_resample=None, affine_fill=None, color_ops=None, perspective=None, also=None, erase=None, mix=None, compose=None, patches=None):
        """Decode files that may mix sampling layouts (one plan per layout).  ``rois``: decode only a window of each image —
        None, one (x, y, width, height) for every file, or one such tuple or None (whole image) per file; every array then has
        the window's shape (see :func:`normalize_rois`).  ``size=(width, height)``: every image (or window) resized to that size
        on the GPU — Pillow's ``resize(size, Image.BILINEAR)`` of it, byte for byte — and ONE array of shape ``(len(files),) +
        shape of one image`` instead of a list.  With ``size``, ``dtype`` / ``normalize=(mean, std)`` / ``mirror`` make that array
        model-ready in the same launch (:func:`normalize_output`): float32 or float16 elements, torchvision's
        ``Normalize(mean, std)(to_tensor(img))`` of the resized bytes bit for bit, flagged files flipped along the width.
        ``orientation``: None (the pixels as stored), "exif" (every file turned as its EXIF Orientation tag says: Pillow's
        ``ImageOps.exif_transpose``), an int 1..8 for every file, or one of these per file (:func:`normalize_orientation`).
        Shapes, ``rois`` and ``size`` then all refer to the turned image; ``mirror`` comes after it.
        ``resample``, with ``size``: the filter of the resize — None or "bilinear" (the default), "box", "hamming", "bicubic" or
        "lanczos", Pillow's ``Image.Resampling`` member or its integer value (:func:`normalize_resample`); one filter for the whole
        call.  Every image is then Pillow's ``resize(size, <that filter>)`` byte for byte, and everything else composes as ever.
        ``mode``: None (every file in its own components), "RGB" or "L" — Pillow's mode names (:func:`normalize_mode`): every output
        has three components, a greyscale file's value in all of them, or one, a colour file's ``convert("L")``.  The conversion
        comes first: the result is ``exif_transpose(img.convert(mode)).resize(size, filter)``, then the output table, then the
        mirror.  With ``size`` a list may then mix greyscale and colour files, and ``normalize`` is checked against the mode's
        count; files that already have it decode exactly as without the argument.
        ``resize_to``, with ``size``: aspect-preserving sizing — ``size`` becomes a canvas, every image (oriented; its window) is
        resized to a size of its own and placed on it, in the same one resize launch (:func:`normalize_places`).  An int ``s``:
        torchvision's ``Resize(s)`` (the shorter side) then ``CenterCrop(size)``; a tuple (width, height): that size; "contain":
        Pillow's ``ImageOps.pad(img, size, filter, color=fill)``; or a list with one of these per file.  ``place``: None (centred by
        the rule of the file's kind), one (x, y) or one per file — the resized image's top-left on the canvas, negative where it is
        cropped.  ``fill``: the byte (or one per output component) of canvas elements no image covers, 0 by default; it goes
        through ``dtype`` / ``normalize`` like a pixel, and ``mirror`` flips the finished canvas.  Only the canvas is computed.
        ``reducing_gap``, with ``size``: None, or a number >= 1.0 — the two-step resize of Pillow's ``Image.resize(size, filter,
        reducing_gap=g)`` (``Image.thumbnail`` uses 2.0): every image is first shrunk by the integer factors ``int(w / width / g)``
        and ``int(h / height / g)`` with ``Image.reduce`` (one more launch, a box average) and the small image is then resampled
        over the fractional box.  Not the single-step bytes — Pillow calls the difference invisible from 3.0 on — but far fewer
        taps for a strong shrink.  What lands on the canvas is ``exif_transpose(img.convert(mode)).crop(window).resize(target,
        filter, reducing_gap=g)`` bit for bit, ``target`` being ``size`` or the place's size under ``resize_to``.
        ``views``, with ``size``: several outputs per file from one decode (:func:`normalize_views`) — a list with one entry per
        OUTPUT, ``(file_index, (x, y, width, height))``, ``(file_index, None)`` or a bare ``file_index``: output k is that window of
        that file's image (oriented, after the mode) resized to ``size``, exactly output 0 of the call on that one file with
        ``rois=[window]`` and the k-th entry of ``mirror`` and of the list forms of ``resize_to`` and ``place``, which then have one
        entry per view (``orientation`` stays per file).  The result is one array of ``len(views)`` images in the views' order.  A
        file is uploaded, entropy-decoded and reconstructed once however many views name it; a file no view names is not looked
        at.  Not with ``rois`` or ``return_seams``.
        ``affine``, with ``size``: rotate, shear, translate, scale — Pillow's ``Image.transform(img.size, Image.AFFINE, matrix,
        affine_resample, fillcolor=affine_fill)`` of the whole oriented image, in front of the window and the resize
        (:func:`normalize_affine`): None, one matrix ``(a0, .., a5)`` for every output, or a list with one matrix or None per output —
        per file, per view with ``views``.  The matrix maps output to input, as Pillow's and torchvision's inverse matrix do
        (:func:`rotation_matrix` builds ``Image.rotate``'s).  ``affine_resample``: "nearest" (the default), "bilinear" or "bicubic", one
        for the call; ``affine_fill``: the byte, or one per output component, of pixels whose source lies outside the image (0).  The
        transformed image has the oriented image's size (``expand=False``); ``rois``, ``views``, ``resize_to`` and ``size`` refer to
        it.  What lands on the canvas is ``exif_transpose(img.convert(mode)).transform(img.size, AFFINE, a, affine_resample,
        fillcolor=affine_fill).crop(window).resize(target, filter)`` bit for bit, then the mirror and the output's element type; an
        output whose matrix is None is the output of the call without the argument.  Files are decoded whole (a rotated window
        needs pixels outside itself); one more launch per plan writes every output's window of its transformed image.  Not with
        ``return_seams``, and not yet with ``reducing_gap``.
        ``perspective``, with ``size``: torchvision's ``RandomPerspective`` / ``F.perspective`` on PIL images — Pillow's
        ``Image.transform(img.size, Image.PERSPECTIVE, coeffs, affine_resample, fillcolor=affine_fill)`` in ``affine``'s place and in
        its stead (:func:`normalize_perspective`): None, one sequence ``(c0, .., c7)`` for every output, or a list with one or None
        per output.  The coefficients map output to input, as Pillow's do; :func:`perspective_coeffs` solves for them from four
        corners.  ``affine_resample`` and ``affine_fill`` serve it as they serve ``affine``, and all that is said of ``affine`` above
        holds, bit for bit in the same way.  The coordinates are two double divisions per pixel; where the denominator is zero or
        the coordinates lie outside the image — beyond a pole line that crosses the frame, say — the pixel is ``affine_fill``, as
        Pillow's is.  No coefficient magnitude is refused.  Not together with ``affine``.
        ``color_ops``, with ``size``: the colour half of ColorJitter, RandAugment, AutoAugment and TrivialAugment, on the finished
        canvas (:func:`normalize_color_ops`): None, one chain for every output, or a list with one chain or None per output — per
        file, per view with ``views``.  A chain is a sequence of at most four ops — ``("brightness", f)``, ``("color", f)``,
        ``("contrast", f)``, ``("sharpness", f)``, ``("posterize", bits)``, ``("solarize", t)``, ``("autocontrast",)``,
        ``("equalize",)``, ``("invert",)`` —, each what the one call of Pillow's ``ImageEnhance`` / ``ImageOps`` of that name does,
        ``("gaussian_blur", radius)`` or ``("box_blur", radius)`` with one radius of 0..1024 — ``im.filter(ImageFilter.GaussianBlur(radius))``
        / ``BoxBlur(radius)``, the random blur of the SimCLR / MoCo / BYOL / DINO recipes —, or ``("adjust_hue", f)`` with
        -0.5 <= f <= 0.5: torchvision's ``F.adjust_hue`` on a PIL image, the fourth knob of ``ColorJitter`` (Pillow's HSV round trip
        with ``int(f * 255) & 255`` added to H; f = 0 is that round trip, not the identity; the identity on an "L" output).
        The order is decode, mode, orientation, affine, window, resize / place / fill, colour ops, mirror, element type
        (torchvision's: crop, flip, jitter, ToTensor, Normalize — every op commutes with the flip): output k is its chain applied to
        the uint8 canvas the call gives without the argument, without ``mirror`` and with ``dtype="uint8"`` — fill pixels
        included —, as a Pillow image of the output's mode, bit for bit; then the mirror and the element type.  An output whose
        chain is None or empty is the output of the call without the argument.  Not with ``return_seams``; autocontrast's
        cutoffs and masks, and more than four ops are not offered yet.
        ``erase``, with ``size``: RandomErasing on the finished outputs (:func:`normalize_erase`, tools/erase_model.py) — None, or a list
        with one entry per output (per file; per view with ``views``): None, one box ``(x, y, width, height[, value])`` or a list of
        boxes applied in order.  It comes LAST — decode, mode, orientation, affine, window, resize / place / fill, colour ops, mirror,
        element type, erase — and is torchvision's ``F.erase``, ``img[..., y:y+height, x:x+width] = value``, on output k in its ``dtype``,
        boxes in the coordinates of what the call returns: bit for bit the call without the argument with those elements overwritten.
        ``value``: absent (0) or a number, one number per component, or a ``(C, height, width)`` NumPy array (noise, which the caller
        draws).  One more launch per plan (csrc/erase.hip), on every plan of the call, second rounds included.  Not with
        ``return_seams``; an ``also`` entry takes a key ``erase`` of its own.
        ``mix``, with ``size``: MixUp and CutMix over the finished outputs (:func:`normalize_mix`, tools/mix_model.py) — None, or a list
        with one entry per output: None, ``("mixup", partner, lam)`` or ``("cutmix", partner, (x, y, width, height))``, ``partner`` the
        index of an output of the same array.  It comes behind ``erase`` — torchvision's order: RandomErasing is a per-sample transform,
        the mixing is in the collate function — and every output reads the array as it stands before any mixing.  Not a step of any
        plan: ONE launch (csrc/mix.hip) over the whole array once every plan of the call has been collected, from that array into a
        second one, which is what the call returns — here the array is uploaded, mixed by the library and downloaded.  Entries that are
        all None: the call without the argument.  An ``also`` entry takes a key ``mix`` of its own, over its own outputs.
        ``compose``, with ``size``: several outputs pasted onto one canvas (:func:`normalize_compose`, tools/compose_model.py) — None, or
        a dict ``size`` (of the composed canvases; the call's ``size`` stays the tiles'), ``fill`` and ``outputs``, one list of tiles
        ``(source, (dx, dy)[, (sx, sy, w, h)])`` per composed output: Mosaic (:func:`mosaic_tiles`), image grids, a crop of one
        sample in another.  The last step, behind ``erase``, and like ``mix`` not a step of any plan: ONE launch (csrc/compose.hip)
        over the tile array once every plan of the call has been collected, into an array of ``len(outputs)`` canvases, which is what
        the call returns in place of the tiles.  Not together with ``mix`` in one group.  An ``also`` entry takes a key ``compose`` of
        its own, over its own outputs.
        ``patches``, with ``size``: the outputs packed into the token rows of a native-resolution vision encoder (:func:`normalize_patches`,
        tools/patch_model.py) — None, or a dict ``patch``, ``merge``, ``repeat``, ``order``, ``windows`` and ``length``.  The LAST step,
        behind ``erase``, ``mix`` and ``compose``, and like them not a step of any plan: ONE launch (csrc/patch.hip) once every plan
        has been collected, from the group's array as it then stands (the composed canvases under ``compose``) into a new one —
        ``(T, D)`` packed, ``(N, length, D)`` padded —, which the call returns in place of the outputs (:func:`patch_grids` gives the row
        offsets).  An ``also`` entry takes a key ``patches`` of its own.
        ``also``, with ``size``: several groups of outputs from ONE decode (:func:`normalize_also`) — None or ``[]`` (the call as it
        is), else a list with one dict per extra group: ``size`` (required) and that group's own ``views``, ``mirror``, ``resize_to``,
        ``place``, ``affine``, ``perspective`` and ``color_ops`` (None when absent, never the call's); ``dtype``, ``normalize``,
        ``resample``, ``mode``, ``reducing_gap``, ``fill``, ``affine_resample`` and ``affine_fill`` are the call's unless the entry names
        them.  The result is then a tuple ``(primary, extra_0, extra_1, ...)``: element g is, bit for bit, what the call returns with
        group g's arguments alone and the call's ``orientation`` — DINO's 2 x 224 and 8 x 96 crops, or one batch at 224 and at
        384, from one upload and one decode.  Every file some group names is parsed, uploaded and decoded once; a file no group names
        is not looked at.  Not with ``rois`` (windows are views) or ``return_seams``; an entry takes no ``rois``, ``orientation`` or
        ``return_seams``."""
        main = dict(size=size, dtype=dtype, normalize=normalize, mirror=mirror, resample=resample, mode=mode, resize_to=resize_to, place=place, fill=fill,
                    reducing_gap=reducing_gap, views=views, affine=affine, affine_resample=affine_resample, affine_fill=affine_fill, color_ops=color_ops,
                    perspective=perspective, erase=erase, mix=mix, compose=compose, patches=patches)
        mode = normalize_mode(mode)
        if mode is not None and return_seams:
            raise ValueError("mode and return_seams do not go together: the seam outputs are in the files' own components")
        if orientation is not None and return_seams:
            raise ValueError("orientation and return_seams do not go together: the seam outputs are in stored order")
        if rois is not None and return_seams:
            raise ValueError("rois and return_seams do not go together: the seam outputs are whole-image")
        size = normalize_size(size)
        if size is not None and return_seams:
            raise ValueError("size and return_seams do not go together: the seam outputs are at the files' own sizes")
        normalize_output(dtype, normalize, mirror, size, host=True)       # (what needs no file: before any is parsed)
        resample = normalize_resample(resample, size)
        reducing_gap = normalize_reducing_gap(reducing_gap, size)
        normalize_places(resize_to, place, size)
        normalize_fill(fill, resize_to)
        extra = normalize_also(also, main, size, rois, return_seams, host=True)
        cache: Dict[int, ParsedJpeg] = {}       # the parsed files, by their position in the caller's list
        if extra is None:
            req, dense = self._host_request(files, cache, None, rois, return_seams, orientation=orientation, **main)
            denses = [dense]
        else:
            denses = []
            gpu_segment = self._gpu_segment_for([files[i] for i in select_union_files(files, [main] + extra)])

            def build(fs, **kw):
                r, d = self._host_request(fs, cache, gpu_segment, **kw)
                denses.append(d)
                return r
            req = self._merged_request(files, orientation, [main] + extra, build)
        files, index, size, orient = req.files, req.index, req.size, req.orient
        gpu_segment = self._gpu_segment_for(files)
        parsed = {i: cache[index[i] if index is not None else i] for i in range(len(files))}
        turn = req.plan_keys()
        results: List[Optional[np.ndarray]] = [None] * len(files)
        seams: List[Optional[dict]] = [None] * len(files)
        flags = ((B.MJ_FLAG_KEEP_PLANES | B.MJ_FLAG_KEEP_IDCT) if return_seams else 0) | self.base_flags
        work = [_Work(idxs) for idxs in _group_by_kind(files, range(len(files)), parsed, gpu_segment, turn, index)]
        while work:
            item = work.pop(0)
            idxs, sub = item.idxs, req.narrow(item.idxs)
            prep = prepare_batch(sub.files, self.layout, flags | item.flags, [parsed[i] for i in idxs])
            plans = self._group_plans(sub, prep, host=True)
            plan = plans[0][1]
            try:
                for _, p in plans:              # (the derived plans right behind the plan that decodes, on the context's stream)
                    p.execute()
                for _, p in plans:
                    p.sync()
                out = plan.read(rgb=True, coef=return_seams, planes=return_seams, idct=return_seams)
                tail, unconverged = _triage(out["status"], idxs, files, parsed, sub.index)
                if tail:
                    work.append(_Work(tail, flags=item.flags))
                if unconverged:
                    work.append(_Work(unconverged, flags=item.flags | B.MJ_FLAG_NO_SYNC))
                again = set(tail) | set(unconverged)
                which = {id(g): j for j, g in enumerate(sub.groups)}
                for g, p in plans:
                    dense = denses[which[id(g)]]
                    rgb = out["rgb"] if p is plan else p.read(rgb=True)["rgb"]
                    if dense is not None:
                        imgs = rgb.view(dense.dtype).reshape((g.n_outputs,) + dense.shape[1:])
                    else:
                        imgs = self.split_outputs(prep, rgb, wins=g.wins, orient=g.orient, ncomp=g.ncomp)
                    if g.views is not None:     # (the plan's outputs are its views, each to its place in the array)
                        for k, (f, _) in enumerate(g.views):
                            if idxs[f] not in again:
                                dense[g.slots[k]] = imgs[k]
                        continue
                    for k, i in enumerate(idxs):
                        if i in again:
                            continue
                        if dense is not None:
                            dense[i] = imgs[k]
                            continue
                        results[i] = imgs[k]
                        if return_seams:
                            b0, _ = plan.image_offsets(k)
                            b1 = plan.image_offsets(k + 1)[0] if k + 1 < len(idxs) else plan.info.total_blocks
                            w, h, nc = prep.shapes[k]
                            po = sum(s[0] * s[1] * s[2] for s in prep.shapes[:k])
                            seams[i] = {"coef": out["coef"][b0:b1], "idct": out["idct"][b0:b1].reshape(-1, 8, 8),
                                        "planes": out["planes"][po:po + w * h * nc].reshape(w, h, nc)}
            finally:
                for _, p in reversed(plans):
                    p.close()
        for j, g in enumerate(req.groups):      # (behind every plan of the call: the groups' arrays mixed, each within itself)
            if g.mix is not None:
                denses[j] = self._mix_host(g, denses[j])
            if g.compose is not None:
                denses[j] = self._compose_host(g, denses[j])
            if g.patches is not None:
                denses[j] = self._patchify_host(g, denses[j])
        if extra is not None:
            return tuple(denses)
        if denses[0] is not None:
            return denses[0]
        return (results, seams) if return_seams else results

    def _host_request(self, files: Sequence[bytes], cache: Dict[int, ParsedJpeg], gpu_segment: Optional[bool], rois=None, return_seams: bool = False,
                      size=None, dtype=None, normalize=None, mirror=None, orientation=None, resample=None, mode=None, resize_to=None, place=None,
                      fill=None, reducing_gap=None, views=None, affine=None, affine_resample=None, affine_fill=None, color_ops=None, perspective=None, erase=None,
                      mix=None, compose=None, patches=None):
        """The checked request of a :meth:`decode` call, or of one group of it, and the array it fills (None without ``size``).  ``cache``:
        the parsed files by their position in ``files``, filled with those this request names; ``gpu_segment``: whether they are parsed
        headers only (None: decided by the files this request names)."""
        size = normalize_size(size)
        mode = normalize_mode(mode)
        resample = normalize_resample(resample, size)
        reducing_gap = normalize_reducing_gap(reducing_gap, size)
        spec = normalize_transform(affine, perspective, affine_resample, affine_fill, size,
                                   len(views) if isinstance(views, (list, tuple)) else len(files), reducing_gap, return_seams)
        colour = normalize_color_ops(color_ops, size, len(views) if isinstance(views, (list, tuple)) else len(files), return_seams)
        # (before any file is read: everything but what the files' component count decides)
        boxes = normalize_erase(erase, size, len(views) if isinstance(views, (list, tuple)) else len(files), B.MODES[mode] if mode else None,
                                dtype_name(dtype) if dtype is not None else "float32" if normalize is not None else "uint8", return_seams)
        mixes = normalize_mix(mix, size, len(views) if isinstance(views, (list, tuple)) else len(files),
                              dtype_name(dtype) if dtype is not None else "float32" if normalize is not None else "uint8", return_seams)
        composed = normalize_compose(compose, size, len(views) if isinstance(views, (list, tuple)) else len(files), B.MODES[mode] if mode else None, return_seams, mixes)
        patched = normalize_patches(patches, size, len(views) if isinstance(views, (list, tuple)) else len(files), B.MODES[mode] if mode else None,
                                    dtype_name(dtype) if dtype is not None else "float32" if normalize is not None else "uint8", return_seams, composed)
        if spec is not None and views is None:  # (windows of the TRANSFORMED images: whole files are decoded)
            views, rois = rois_as_views(rois, len(files)), None
        index = None                            # views: where the files that are read sit in the caller's list
        selected = select_view_files(files, views, size, rois, return_seams)
        if selected is not None:
            index, views = selected
            orientation = _per_file_of(orientation, len(files), index, "orientation")
            files = [files[i] for i in index]
        if gpu_segment is None:
            gpu_segment = self._gpu_segment_for(files)
        parsed = {}
        for i, f in enumerate(files):
            at = index[i] if index is not None else i
            if at not in cache:
                cache[at] = _named(index, i, parse_jpeg, f, headers_only=gpu_segment)
            parsed[i] = cache[at]
        orient = normalize_orientation(orientation, files)
        odims = _oriented_dims([(p.image_width, p.image_height) for p in parsed.values()], orient)
        req = _Request(files, normalize_rois(rois, odims), size, orient=orient, resample=resample, mode=mode, reducing_gap=reducing_gap, index=index,
                       views=normalize_views(views, odims, size, index=index) if selected is not None else None, colour=colour)
        if req.views is not None:               # (what is per output is per view; an error names the view's file)
            req.places = normalize_places(resize_to, place, size, [r[2:] for _, r in req.views], [index[f] for f, _ in req.views])
            req.slots = list(range(len(req.views)))
            check_affine(spec, req.views, odims, index)
        else:
            req.places = normalize_places(resize_to, place, size, [w[2:] for w in req.wins] if req.wins is not None else odims)
        dense = None                            # size=: the one array (every plan's own dense output is copied into it)
        if size is not None:
            nc = req.ncomp or one_component_count([len(p.color_components) for p in parsed.values()])
            req.output = normalize_output(dtype, normalize, mirror, size, req.n_outputs, nc, host=True)
            req.fill = normalize_fill(fill, resize_to, nc)
            if spec is not None:
                req.affine = _spec_for_outputs(spec, size, req.n_outputs, nc)
            req.erase = erase_for_components(boxes, nc)
            req.mix = mixes
            req.compose = compose_for_components(composed, compose, size, nc)
            req.patches = patches_for_components(patched, patches, size, req.n_outputs, nc, req.output.dtype if req.output else "uint8", req.compose)
            dense = np.empty((req.n_outputs,) + self._shape(size[0], size[1], nc), dtype=req.output.numpy_dtype if req.output else np.uint8)
        return req, dense

    def _staging_for(self, files: Sequence[bytes]) -> np.ndarray:
        """Host buffer the native front end builds the blob in, kept between calls (first touch of a fresh 300 MB
        allocation costs as much as the parse)."""
        need = sum(map(len, files)) + 3 * len(files) + 1024
        if self._staging is None or self._staging.size < need:
            self._staging = np.empty(need + need // 4, dtype=np.uint8)
        return self._staging

    def _device_request(self, files: Sequence[bytes], rois, size, dtype, normalize, mirror, orientation=None, resample=None, mode=None,
                        resize_to=None, place=None, fill=None, reducing_gap=None, views=None, affine=None, affine_resample=None,
                        affine_fill=None, color_ops=None, perspective=None, erase=None, mix=None, compose=None, patches=None) -> _Request:
        """The checked request of a :meth:`decode_device` call (``size``: :func:`normalize_size`'s): the windows against the
        files' headers and, with ``size``, the output against their component count and the one tensor they fill on this
        decoder's GPU, one slot per file in order — with ``views``, one slot per view, and only the files some view names."""
        spec = normalize_transform(affine, perspective, affine_resample, affine_fill, size,
                                   len(views) if isinstance(views, (list, tuple)) else len(files), reducing_gap)
        colour = normalize_color_ops(color_ops, size, len(views) if isinstance(views, (list, tuple)) else len(files))
        # (before any file is read: everything but what the files' component count decides)
        boxes = None
        if erase is not None:
            boxes = normalize_erase(erase, size, len(views) if isinstance(views, (list, tuple)) else len(files), B.MODES.get(mode) if isinstance(mode, str) else None,
                                    dtype_name(dtype) if dtype is not None else "float32" if normalize is not None else "uint8", device=self.ctx.device)
        mixes = normalize_mix(mix, size, len(views) if isinstance(views, (list, tuple)) else len(files),
                              dtype_name(dtype) if dtype is not None else "float32" if normalize is not None else "uint8")
        composed = normalize_compose(compose, size, len(views) if isinstance(views, (list, tuple)) else len(files), B.MODES.get(mode) if isinstance(mode, str) else None, mix=mixes)
        patched = normalize_patches(patches, size, len(views) if isinstance(views, (list, tuple)) else len(files), B.MODES.get(mode) if isinstance(mode, str) else None,
                                    dtype_name(dtype) if dtype is not None else "float32" if normalize is not None else "uint8", compose=composed)
        if spec is not None and views is None:  # (windows of the TRANSFORMED images: whole files are decoded)
            views, rois = rois_as_views(rois, len(files)), None
        index = None
        selected = select_view_files(files, views, size, rois)
        if selected is not None:
            index, views = selected
            orientation = _per_file_of(orientation, len(files), index, "orientation")
            files = [files[i] for i in index]
        req = _Request(files, None, size, orient=normalize_orientation(orientation, files), resample=normalize_resample(resample, size),
                       mode=normalize_mode(mode), reducing_gap=normalize_reducing_gap(reducing_gap, size), index=index, colour=colour)
        if size is not None:
            import torch
            info = [_named(index, i, _image_info, f) for i, f in enumerate(files)]
            nc = req.ncomp or one_component_count([t[2] for t in info])
            odims = _oriented_dims([t[:2] for t in info], req.orient)
            if selected is not None:            # (what is per output is per view; an error names the view's file)
                req.views = normalize_views(views, odims, size, index=index)
                req.places = normalize_places(resize_to, place, size, [r[2:] for _, r in req.views], [index[f] for f, _ in req.views])
                check_affine(spec, req.views, odims, index)
                if spec is not None:
                    req.affine = _spec_for_outputs(spec, size, len(req.views), nc)
            else:
                req.wins = normalize_rois(rois, odims)
                req.places = normalize_places(resize_to, place, size, [w[2:] for w in req.wins] if req.wins is not None else odims)
            req.output = normalize_output(dtype, normalize, mirror, size, req.n_outputs, nc)
            req.fill = normalize_fill(fill, resize_to, nc)
            req.erase = erase_for_components(boxes, nc)
            req.mix = mixes
            req.compose = compose_for_components(composed, compose, size, nc)
            req.patches = patches_for_components(patched, patches, size, req.n_outputs, nc, req.output.dtype if req.output else "uint8", req.compose)
            req.dest = torch.empty((req.n_outputs,) + self._shape(size[0], size[1], nc), dtype=req.output.torch_dtype if req.output else torch.uint8,
                                   device=torch.device("cuda", self.ctx.device))
            req.slots = list(range(req.n_outputs))
        elif rois is not None:
            req.wins = normalize_rois(rois, _oriented_dims([_image_dims(f) for f in files], req.orient))
        return req

    def _wait_for_current_stream(self, cur):
        """An output buffer comes from torch's caching allocator on torch's CURRENT stream (``cur``): a block a consumer has
        just dropped may still be read by kernels queued there, so the stream that is about to overwrite it — here the
        context's — waits for the current stream first (the allocator only orders reuse within one stream)."""
        import torch
        ev = torch.cuda.Event()
        ev.record(cur)
        self.ctx.wait_event(ev.cuda_event)

    def decode_device(self, files: Sequence[bytes], rois=None, parts: Optional[int] = None, size=None, dtype=None, normalize=None,
                      mirror=None, orientation=None, resample=None, mode=None, resize_to=None, place=None, fill=None, reducing_gap=None, views=None,
                      affine=None, affine_resample=None, affine_fill=None, color_ops=None, perspective=None, also=None, erase=None, mix=None, compose=None, patches=None):
        """Like :meth:`decode`, but the pixels stay in HBM: a list of ``torch.uint8`` tensors on this decoder's GPU,
        views into one packed buffer per plan (zero-copy for any DLPack consumer via ``tensor.__dlpack__()``).
        torch is only the allocator here; import it before this package.

        With ``segment="gpu"`` a batch of everyday baseline files never meets the Python parser: libmijpeg.so's host
        front end (``mj_host_assemble``) reads the headers and assembles the batch on host threads; whatever it declines
        takes the Python path, which raises the reference's exceptions.  A large batch on that route goes as ``parts``
        plans of 256 files or more (up to four) through :meth:`decode_device_iter`, so that one part's upload runs under the
        assembly of the next and under the kernels of the one before — inside one call the three would otherwise add up.
        ``rois`` as in :meth:`decode`: the windows are checked against the files' headers before any GPU work.
        ``size=(width, height)``: ONE ``torch.uint8`` tensor of shape ``(len(files),) + shape of one image`` — every image (or
        window) resized as in :meth:`decode`; files of several kinds are still one plan per kind, and every plan writes its
        images straight into their slots of that tensor.
        ``dtype`` ("uint8", "float32", "float16", "bfloat16" or the torch / numpy dtype), ``normalize=(mean, std)`` and
        ``mirror`` (one bool, or one per file), all with ``size``: the tensor a model takes, out of the same resize launch — its
        elements are torchvision's ``Normalize(mean, std)(to_tensor(img))`` of the resized bytes (mean 0, std 1 without
        ``normalize``), computed in float32 and converted with ``.to(dtype)``, bit for bit; a flagged file's image is the
        un-flagged result flipped along its width axis (:func:`normalize_output`).
        ``orientation`` as in :meth:`decode`: None, "exif", an int 1..8, or one of these per file.  The tags are read on host
        threads; turned files are plans of their own (upright ones decode exactly as without the argument), written turned by
        one more launch per plan — or, with ``size``, by the resize launch itself, whose result is Pillow's resize of the
        turned image.
        ``resample`` as in :meth:`decode`: the filter of the resize, one for the whole call — every plan of it (second rounds,
        files of several kinds, parts) resamples with it.
        ``mode`` as in :meth:`decode`: None, "RGB" or "L".  Greyscale and colour files are plans of their own as ever; the plans of
        the files that do not have the mode's components convert inside the launch they end in anyway — the resize launch, or the
        one extra launch of an own-size plan — and with ``size`` all of them fill their slots of the one tensor.
        ``resize_to``, ``place`` and ``fill`` as in :meth:`decode`: ``size`` is a canvas, every image is resized to a size of its
        own and placed on it by the one resize launch of its plan; files of several kinds and orientation classes are still one
        plan per kind, each writing its slots of the one tensor.
        ``reducing_gap`` as in :meth:`decode`: the two-step resize; every plan of the call (second rounds, files of several kinds,
        parts) carries it.
        ``views`` as in :meth:`decode`: one tensor of ``len(views)`` images in the views' order, every file decoded once.  Files of
        several kinds are still one plan per kind, each writing its views' slots of the one tensor, and a large call is split into
        parts by FILE, every file's views in its part.
        ``affine``, ``affine_resample`` and ``affine_fill`` as in :meth:`decode`: every plan of the call (files of several kinds and
        orientation classes, second rounds, parts) runs its own affine launch between its decode and its resize launch.
        ``perspective`` as in :meth:`decode`, in ``affine``'s place: every such plan runs the perspective launch there instead.
        ``color_ops`` as in :meth:`decode`: every plan of the call whose outputs have operations writes its canvases into a buffer of
        its own and runs the colour launches behind its resize launch — histograms, tables and the operations themselves, all on the
        GPU —, which store into the one tensor; plans whose outputs have none are the plans of a call without the argument.
        ``also`` as in :meth:`decode`: a tuple of tensors, one per group.  Every plan of the call (files of several kinds and
        orientation classes, second rounds, parts) is made by the first group that has outputs among its files; every later group
        that has some derives a plan from it, executed right behind it on the same stream into that group's tensor.
        ``erase`` as in :meth:`decode`; a box's ``(C, height, width)`` values may also be a torch tensor, on the CPU or on this decoder's
        GPU.  Every plan of the call erases the outputs it writes as its last launch; its blocks of values go into one tensor of the
        output's type (host arrays uploaded once, one ``torch.cat``) that the plan holds until it is collected.
        ``mix`` as in :meth:`decode`: once every plan of the call — kinds of files, orientation classes, parts, second rounds — has been
        collected, each group's tensor is the source of ONE launch on torch's current stream into a new tensor of the same shape, which
        the caller gets; the source goes back to torch's allocator.
        ``compose`` as in :meth:`decode`: likewise once every plan of the call has been collected, one launch on torch's current stream
        from the group's tile tensor into a new tensor of ``len(outputs)`` composed canvases, which the caller gets.
        ``patches`` as in :meth:`decode`: the last step, one launch on torch's current stream from the group's tensor — mixed or composed
        where it is — into a new tensor of token rows, which the caller gets."""
        size = normalize_size(size)
        normalize_output(dtype, normalize, mirror, size)                 # (what needs no file: before any is read)
        normalize_resample(resample, size)
        normalize_reducing_gap(reducing_gap, size)
        normalize_mode(mode)
        normalize_places(resize_to, place, size)
        normalize_fill(fill, resize_to)
        main = dict(size=size, dtype=dtype, normalize=normalize, mirror=mirror, resample=resample, mode=mode, resize_to=resize_to, place=place, fill=fill,
                    reducing_gap=reducing_gap, views=views, affine=affine, affine_resample=affine_resample, affine_fill=affine_fill, color_ops=color_ops,
                    perspective=perspective, erase=erase, mix=mix, compose=compose, patches=patches)
        extra = normalize_also(also, main, size, rois)
        if extra is None:
            req = self._device_request(files, rois, orientation=orientation, **main)
        else:
            req = self._merged_request(files, orientation, [main] + extra, lambda fs, **kw: self._device_request(fs, None, **kw))
        files = req.files                       # (with views: the files some view names)
        if parts is None:
            parts = min(4, len(files) // 256) if (self.native_host and self._gpu_segment_for(files)) else 1
        if parts <= 1:
            return self._mixed(req, self._decode_request(req))
        cut = [len(files) * i // parts for i in range(parts + 1)]
        out: List["torch.Tensor"] = []
        for part in self._device_iter((req.narrow(range(cut[i], cut[i + 1])) for i in range(parts)), depth=2):
            if req.dest is None:
                out += part
        return out if req.dest is None else self._mixed(req, req.dest)

    @staticmethod
    def _result(req: _Request, out):
        """what a call returns for a request: ``out``, or — with extra groups — the tuple of every group's tensor, the call's own first"""
        return out if req.also is None else tuple(g.dest for g in req.groups)

    def _mixed(self, req: _Request, out):
        """What a call returns for a request whose plans have all been collected (``out``: :meth:`_decode_request`'s): every group
        with ``mix`` entries has its tensor mixed into a new one (:meth:`_mix_device`), every group with ``compose`` its tiles composed
        into a new one (:meth:`_composed`), and every group with ``patches`` its tensor — as it then stands — packed into token
        rows (:meth:`_patchified`), which takes its place."""
        if all(g.mix is None and g.compose is None and g.patches is None for g in req.groups):
            return self._result(req, out)
        for g in req.groups:
            if g.mix is not None:
                g.dest = self._mix_device(g)
            if g.compose is not None:
                g.dest = self._composed(g)
            if g.patches is not None:
                g.dest = self._patchified(g)
        return self._result(req, req.dest)

    def _patch_geometry(self, g: _Request, n_sources: int, elements: int):
        """(dtype name, components, (width, height) of a source, rows of the output, D) of a group's patchify launch over ``n_sources``
        sources of ``elements`` elements in all — the group's outputs, or its composed canvases"""
        W, H = g.compose["size"] if g.compose is not None else g.size
        dtype = g.output.dtype if g.output else "uint8"
        nc = elements // (n_sources * W * H)
        rows = B.host_patchify_count(self.layout, dtype, nc, (W, H), n_sources, g.patches)
        return dtype, nc, (W, H), rows, nc * g.patches["repeat"] * g.patches["patch"] ** 2

    def _patch_shape(self, g: _Request, n_sources: int, rows: int, D: int):
        return (rows, D) if g.patches["length"] is None else (n_sources, g.patches["length"], D)

    def _patchified(self, g: _Request):
        """Group ``g``'s tensor as token rows (mj_patchify): one launch from ``g.dest`` — the outputs, mixed or composed where the group
        is, which every plan has finished writing — into a new tensor (T, D) or (N, L, D), on torch's current stream as
        :meth:`_composed` does it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        src = g.dest
        n = int(src.shape[0])
        dtype, nc, wh, rows, D = self._patch_geometry(g, n, src.numel())
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            dst = torch.empty(self._patch_shape(g, n, rows, D), dtype=src.dtype, device=dev)
            args = (self.layout, dtype, nc, wh, n, g.patches)
            if cur.cuda_stream:
                if src.device == dev:
                    src.record_stream(cur)      # (allocated on the stream the call was made on, which may be another)
                self.ctx.patchify(src.data_ptr(), dst.data_ptr(), *args, stream=cur.cuda_stream)
                return dst
            if getattr(self, "_mix_stream", None) is None:
                self._mix_stream = torch.cuda.Stream(device=dev)
            st = self._mix_stream
            st.wait_stream(cur)
            src.record_stream(st)
            dst.record_stream(st)
            self.ctx.patchify(src.data_ptr(), dst.data_ptr(), *args, stream=st.cuda_stream)
            cur.wait_stream(st)
        return dst

    def _patchify_host(self, g: _Request, dense: np.ndarray) -> np.ndarray:
        """Group ``g``'s array as token rows (mj_patchify): uploaded, one launch on the context's stream into a second block, downloaded"""
        n = int(dense.shape[0])
        dtype, nc, wh, rows, D = self._patch_geometry(g, n, int(dense.size))
        out = np.empty(self._patch_shape(g, n, rows, D), dtype=dense.dtype)
        src = B.DeviceBytes(np.ascontiguousarray(dense))
        try:
            dst = B.DeviceBytes(None, out.nbytes)
            try:
                self.ctx.patchify(src.ptr, dst.ptr, self.layout, dtype, nc, wh, n, g.patches)
                return dst.download(out)
            finally:
                dst.close()
        finally:
            src.close()

    def _compose_fill_bits(self, g: _Request, nc: int):
        """the element bit patterns, one per component, of a group's compose fill: its bytes — ``compose``'s own, else the group's
        ``fill``, else 0 — as the group's outputs store such a pixel (the table the resize launch stores through)"""
        fill = g.compose["fill"] if g.compose["fill"] is not None else g.fill if g.fill is not None else (0,) * nc
        if g.output is None or g.output.dtype == "uint8":
            return [int(v) for v in fill]
        mean, std = (g.output.mean, g.output.std) if g.output.mean is not None else ((0.0,) * nc, (1.0,) * nc)
        return [int(B.normalize_table(g.output.dtype, mean[c], std[c])[fill[c]]) for c in range(nc)]

    def _composed(self, g: _Request):
        """Group ``g``'s tensor composed (mj_compose): one launch from ``g.dest`` — the tiles, which every plan has finished writing —
        into a new tensor of ``len(outputs)`` canvases of ``compose``'s size, on torch's current stream as :meth:`_mix_device` does it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        src = g.dest
        dtype, nc, W, H = self._mix_geometry(g, src[0].numel())
        cw, ch = g.compose["size"]
        outputs = g.compose["outputs"]
        bits = self._compose_fill_bits(g, nc)
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            dst = torch.empty((len(outputs),) + self._shape(cw, ch, nc), dtype=src.dtype, device=dev)
            args = (self.layout, dtype, nc, (W, H), src.shape[0], (cw, ch), bits, outputs)
            if cur.cuda_stream:
                if src.device == dev:
                    src.record_stream(cur)      # (allocated on the stream the call was made on, which may be another)
                self.ctx.compose(src.data_ptr(), dst.data_ptr(), *args, stream=cur.cuda_stream)
                return dst
            if getattr(self, "_mix_stream", None) is None:
                self._mix_stream = torch.cuda.Stream(device=dev)
            st = self._mix_stream
            st.wait_stream(cur)
            src.record_stream(st)
            dst.record_stream(st)
            self.ctx.compose(src.data_ptr(), dst.data_ptr(), *args, stream=st.cuda_stream)
            cur.wait_stream(st)
        return dst

    def _compose_host(self, g: _Request, dense: np.ndarray) -> np.ndarray:
        """Group ``g``'s array composed (mj_compose): uploaded, one launch on the context's stream into a second block, downloaded"""
        dtype, nc, W, H = self._mix_geometry(g, int(dense[0].size))
        cw, ch = g.compose["size"]
        outputs = g.compose["outputs"]
        out = np.empty((len(outputs),) + tuple(self._shape(cw, ch, nc)), dtype=dense.dtype)
        src = B.DeviceBytes(dense)
        try:
            dst = B.DeviceBytes(None, out.nbytes)
            try:
                self.ctx.compose(src.ptr, dst.ptr, self.layout, dtype, nc, (W, H), dense.shape[0], (cw, ch), self._compose_fill_bits(g, nc), outputs)
                return dst.download(out)
            finally:
                dst.close()
        finally:
            src.close()

    def _mix_geometry(self, g: _Request, elements_per_output: int):
        """(dtype name, components, width, height) of a group's outputs"""
        W, H = g.size
        return (g.output.dtype if g.output else "uint8"), elements_per_output // (W * H), W, H

    def _mix_device(self, g: _Request):
        """Group ``g``'s tensor mixed (mj_mix): one launch from ``g.dest`` into a new tensor of its shape, on torch's current stream
        — the default stream has no handle the library could launch on, so there the launch goes on a side stream between two
        waits.  Every plan that wrote ``g.dest`` has been synchronised by now.  ``g.dest`` is released to the allocator by the
        caller's dropping it: the launch that reads it is on the stream it was allocated on, or recorded (``record_stream``)."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        src = g.dest
        dtype, nc, W, H = self._mix_geometry(g, src[0].numel())
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            dst = torch.empty_like(src)
            if cur.cuda_stream:
                if src.device == dev:
                    src.record_stream(cur)      # (allocated on the stream the call was made on, which may be another)
                self.ctx.mix(src.data_ptr(), dst.data_ptr(), self.layout, dtype, nc, W, H, g.mix, stream=cur.cuda_stream)
                return dst
            if getattr(self, "_mix_stream", None) is None:
                self._mix_stream = torch.cuda.Stream(device=dev)
            st = self._mix_stream
            st.wait_stream(cur)
            src.record_stream(st)
            dst.record_stream(st)
            self.ctx.mix(src.data_ptr(), dst.data_ptr(), self.layout, dtype, nc, W, H, g.mix, stream=st.cuda_stream)
            cur.wait_stream(st)
        return dst

    def _mix_host(self, g: _Request, dense: np.ndarray) -> np.ndarray:
        """Group ``g``'s array mixed (mj_mix): uploaded, one launch on the context's stream into a second block, downloaded"""
        dtype, nc, W, H = self._mix_geometry(g, int(dense[0].size))
        src = B.DeviceBytes(dense)
        try:
            dst = B.DeviceBytes(None, dense.nbytes)
            try:
                self.ctx.mix(src.ptr, dst.ptr, self.layout, dtype, nc, W, H, g.mix)
                return dst.download(np.empty_like(dense))
            finally:
                dst.close()
        finally:
            src.close()

    def _decode_request(self, req: _Request):
        """What :meth:`decode_device` returns for a checked request, decoded as one plan per kind of file — the request's
        tensor when it has one, else a list of tensors."""
        import torch
        files = req.files
        classes = req.orient_classes()
        if len(classes) > 1:
            # files turned and not (with size: turned in two ways): every class is a request of its own — the upright files the
            # one a call without orientation makes — into the same tensor, or into the same list
            merged: List[Optional["torch.Tensor"]] = [None] * len(files)
            for idxs in classes:
                part = self._decode_request(req.narrow(idxs))
                if req.dest is None:
                    for i, img in zip(idxs, part):
                        merged[i] = img
            return merged if req.dest is None else req.dest
        dev = torch.device("cuda", self.ctx.device)
        results: List[Optional["torch.Tensor"]] = [None] * len(files)
        parsed: Dict[int, ParsedJpeg] = {}
        work: List[_Work] = []
        rest: List[int] = []
        gpu_segment = self._gpu_segment_for(files)
        if gpu_segment and self.native_host:
            prep = prepare_batch_native(files, self.layout, self.base_flags, staging=self._staging_for(files))
            if isinstance(prep, PreparedBatch):                   # the everyday case: one pass, one plan
                work.append(_Work(list(range(len(files))), prep=prep))
            else:
                # files of several kinds (sampling layouts; with / without restart markers), or some the front end does not
                # take (progressive, ...): it sorts them — one native assembly per kind when its turn comes (one staging
                # buffer), the Python path for the rest
                groups_n, rest = prepare_batch_native(files, self.layout, self.base_flags, staging=self._staging_for(files), split=True)
                work += [_Work(idxs, native=True) for idxs in groups_n]
        if not work or rest:
            todo = rest if work else range(len(files))          # everything, unless the front end kept some of it
            # (first in line: what the front end left over is mostly progressive files, whose decode is a long serial chain
            # the other plans can run beside)
            work = [_Work(idxs) for idxs in _group_by_kind(files, todo, parsed, gpu_segment, index=req.index if req.views is not None else None)] + work
        # Several plans (a batch of several kinds of files): all are submitted before the first is collected, on a few
        # streams in turn, so that small plans share the GPU instead of queueing behind each other's host round trips
        # (mj_plan_sync waits for a plan's own work only).  Files handed back by the GPU scan go round again.
        streams = None
        while work:
            flying: List[_Flight] = []
            try:
                while work:
                    item = work.pop(0)
                    sub, prep = req.narrow(item.idxs), item.prep
                    if item.native:
                        prep = prepare_batch_native(sub.files, self.layout, self.base_flags, staging=self._staging_for(sub.files))
                        if not isinstance(prep, PreparedBatch):   # (declined after all: the Python path sorts these files)
                            work[:0] = [_Work(idxs) for idxs in _group_by_kind(files, item.idxs, parsed, True)]
                            continue
                    if prep is None:
                        prep = prepare_batch(sub.files, self.layout, self.base_flags | item.flags, [parsed[i] for i in item.idxs])
                    if work or flying:
                        # more than one plan: keep off the null stream, whose copies would wait for the other plans' kernels
                        if streams is None:
                            streams = [torch.cuda.Stream(device=dev) for _ in range(5)]
                        with torch.cuda.stream(streams[4]):
                            d_blob = torch.from_numpy(prep.blob).to(dev)         # (pageable source: the staging buffer is free on return)
                    else:
                        d_blob = torch.from_numpy(prep.blob).to(dev)
                    plans = self._group_plans(sub, prep, d_blob.data_ptr())      # (extra groups: the plan that decodes, then the derived ones)
                    lead = plans[0][0]
                    flight = _Flight(sub, item.idxs, prep, plans[0][1], None, d_blob, plans[1:])
                    flying.append(flight)
                    d_rgb = flight.d_rgb = lead.dest if lead.dest is not None else torch.empty(flight.plan.info.rgb_bytes, dtype=torch.uint8, device=dev)
                    cur = torch.cuda.current_stream(dev)
                    if streams is None:
                        self._wait_for_current_stream(cur)
                        flight.plan.execute(0, d_rgb.data_ptr())                 # the everyday case: one plan, the context's stream
                        for g, derived in flight.extra:
                            derived.execute(0, g.dest.data_ptr())
                    else:
                        # (streams only overlap when they sit on different hardware queues: the package asks the runtime for
                        # eight instead of four, see __init__.py)
                        st = streams[(len(flying) - 1) % 4]
                        st.wait_stream(streams[4])                               # the upload above
                        st.wait_stream(cur)                                      # (as _wait_for_current_stream, for this stream)
                        d_rgb.record_stream(st)
                        d_blob.record_stream(st)
                        flight.plan.execute(st.cuda_stream, d_rgb.data_ptr())
                        for g, derived in flight.extra:
                            g.dest.record_stream(st)
                            derived.execute(st.cuda_stream, g.dest.data_ptr())
                for flight in flying:
                    flight.sync()
                    tail, unconverged = _triage(flight.plan.read(rgb=False)["status"], flight.idxs, files, parsed, flight.req.index)
                    if tail:
                        work.append(_Work(tail))
                    if unconverged:
                        work.append(_Work(unconverged, flags=B.MJ_FLAG_NO_SYNC))
                    if req.dest is not None:                     # (the plan wrote its slots of the one tensor)
                        continue
                    views = self._views(flight.d_rgb, self._out_shapes(flight.prep, flight.req.wins, flight.req.orient, flight.req.ncomp))
                    for k, i in enumerate(flight.idxs):
                        if i not in tail and i not in unconverged:
                            results[i] = views[k]
            finally:
                for flight in flying:
                    flight.close()
        return results if req.dest is None else req.dest

    def decode_device_iter(self, batches, depth=2, size=None, dtype=None, normalize=None, mirror=None, orientation=None, resample=None,
                           mode=None, resize_to=None, place=None, fill=None, reducing_gap=None, views=None, affine=None, affine_resample=None,
                           affine_fill=None, color_ops=None, perspective=None, also=None, erase=None, mix=None, compose=None, patches=None):
        """Decode a stream of batches (an iterable of lists of file bytes) with the host work and the upload of the next
        batches overlapping the GPU work of the ones before; yields, per batch and in order, what :meth:`decode_device` returns.

        Per batch: the native host front end assembles the blob in one of ``depth + 1`` pinned buffers (host threads), the upload
        is queued on a copy stream, the plan is created (its buffer clears run on the context's setup stream), its kernels
        are queued on the context's stream behind the previous batch's, waiting for the upload by event — and only then is the
        batch ``depth`` places back collected (``mj_plan_sync`` waits for that plan's own work) and handed out.  With one batch
        in flight (round 5) the host waited for batch k's kernels before it started assembling batch k + 2, and the copy engine
        idled meanwhile: 512 x 1080p took the front end's 4.3 ms PLUS the upload's 6.1 ms per batch; with two the three —
        host threads, copy engine, GPU — run side by side and the batch takes what the slowest of them takes.  Batches the front
        end declines are decoded as :meth:`decode_device` decodes them, in place, behind everything in flight (no overlap for
        those).
        ``size=(width, height)``: one tensor per batch, as :meth:`decode_device` returns it with ``size``; ``dtype`` and
        ``normalize`` as there, for every batch; ``mirror``: None, one bool for all files, or an iterable that yields, batch by
        batch, what :meth:`decode_device` takes for that batch (one bool, or one bool per file).  ``orientation``: None, "exif" or
        an int 1..8 for every file of every batch, or an iterable that yields, batch by batch, what :meth:`decode_device` takes.
        ``resample``, ``mode`` and ``reducing_gap`` as in :meth:`decode_device`, for every batch; ``resize_to``, ``place`` and
        ``fill`` too (a list per file then has to fit every batch).  ``views``: None, or an iterable that yields, batch by batch,
        what :meth:`decode_device` takes for that batch — a list with one entry per output; ``mirror`` and the list forms of
        ``resize_to`` and ``place`` then go by view.  ``affine``: None, one matrix for every output of every batch, or an iterable
        that yields, batch by batch, what :meth:`decode_device` takes for that batch; ``affine_resample`` and ``affine_fill`` as
        there, for every batch.  ``perspective``: None, one sequence of eight coefficients for every output of every batch, or an
        iterable that yields one value per batch, as ``affine`` does; not together with ``affine``.  ``color_ops``: None, one chain for every output of every batch, or an iterable that yields, batch by
        batch, what :meth:`decode_device` takes for that batch.  ``also``: None, or an iterable that yields, batch by batch, what
        :meth:`decode_device` takes for that batch — a list with one dict per extra group; every batch is then handed out as a tuple
        of tensors, one per group.  ``erase``: None, or an iterable that yields, batch by batch, what :meth:`decode_device` takes for
        that batch — a list with one entry per output, or None.  ``mix``: None, or an iterable that yields, batch by batch, what
        :meth:`decode_device` takes for that batch; the batch is mixed when it is collected, before it is handed out.  ``compose``: None, or an
        iterable that yields, batch by batch, the dict :meth:`decode_device` takes for that batch, or None.  ``patches``: likewise None, or
        an iterable that yields one dict or None per batch; a batch with a dict is handed out as its token rows."""
        size = normalize_size(size)
        if also is not None and isinstance(also, (list, tuple)) and len(also) == 0:
            also = None                                                               # (no extra group: a call without the argument)
        if also is not None and size is None:
            raise ValueError("also needs size=(width, height): every group of outputs is one array at its own size")
        per_batch_also = iter(also) if also is not None else None
        if erase is not None and size is None:
            raise ValueError("erase needs size=(width, height): boxes are in the coordinates of the finished canvas")
        per_batch_erase = iter(erase) if erase is not None else None
        if mix is not None and size is None:
            raise ValueError("mix needs size=(width, height): the outputs of one array are mixed with each other")
        per_batch_mix = iter(mix) if mix is not None else None
        if compose is not None and size is None:
            raise ValueError("compose needs size=(width, height): the tiles are the outputs of one array")
        if isinstance(compose, dict):
            raise ValueError("compose must be None or an iterable that yields one dict or None per batch, not a dict")
        per_batch_compose = iter(compose) if compose is not None else None
        if patches is not None and size is None:
            raise ValueError("patches needs size=(width, height): the sources are the outputs of one array")
        if isinstance(patches, dict):
            raise ValueError("patches must be None or an iterable that yields one dict or None per batch, not a dict")
        per_batch_patches = iter(patches) if patches is not None else None
        normalize_color_ops(color_ops if color_ops is None or _is_chain(color_ops) else (), size)      # (what needs no file, before any work)
        per_batch_colour = iter(color_ops) if color_ops is not None and not _is_chain(color_ops) else None
        # (what needs no file, before any work: an iterable's matrices are looked at batch by batch)
        normalize_transform(affine if affine is None or _is_matrix(affine) else (1, 0, 0, 0, 1, 0),
                            perspective if perspective is None or _is_coeffs(perspective) else (1, 0, 0, 0, 1, 0, 0, 0), affine_resample, affine_fill, size, None,
                            reducing_gap)
        per_batch_affine = iter(affine) if affine is not None and not _is_matrix(affine) else None
        per_batch_perspective = iter(perspective) if perspective is not None and not _is_coeffs(perspective) else None
        if views is not None and size is None:
            raise ValueError("views needs size=(width, height): every view is resized to it (crops at their own sizes would be ragged)")
        per_batch_views = iter(views) if views is not None else None
        normalize_resample(resample, size)                                            # (what needs no file: before any work)
        normalize_reducing_gap(reducing_gap, size)
        normalize_mode(mode)
        normalize_places(resize_to, place, size)
        normalize_fill(fill, resize_to)
        turns_per_batch = not (orientation is None or isinstance(orientation, (str, int, np.integer)))
        if not turns_per_batch:
            normalize_orientation(orientation, [])                                    # (what needs no file: before any work)
        turns = iter(orientation) if turns_per_batch else None
        per_batch = mirror is not None and not isinstance(mirror, (bool, np.bool_))
        normalize_output(dtype, normalize, None if per_batch else mirror, size)      # (what needs no file: before any work)
        if per_batch and size is None:
            raise ValueError("dtype, normalize and mirror need size=(width, height)")
        flags = iter(mirror) if per_batch else None

        def requests():
            for files in batches:
                files = list(files)
                m = mirror
                if flags is not None:
                    try:
                        m = next(flags)
                    except StopIteration:
                        raise ValueError("mirror yields fewer entries than there are batches") from None
                o = orientation
                if turns is not None:
                    try:
                        o = next(turns)
                    except StopIteration:
                        raise ValueError("orientation yields fewer entries than there are batches") from None
                v = None
                if per_batch_views is not None:
                    try:
                        v = next(per_batch_views)
                    except StopIteration:
                        raise ValueError("views yields fewer entries than there are batches") from None
                t = affine
                if per_batch_affine is not None:
                    try:
                        t = next(per_batch_affine)
                    except StopIteration:
                        raise ValueError("affine yields fewer entries than there are batches") from None
                ps = perspective
                if per_batch_perspective is not None:
                    try:
                        ps = next(per_batch_perspective)
                    except StopIteration:
                        raise ValueError("perspective yields fewer entries than there are batches") from None
                c = color_ops
                if per_batch_colour is not None:
                    try:
                        c = next(per_batch_colour)
                    except StopIteration:
                        raise ValueError("color_ops yields fewer entries than there are batches") from None
                er = None
                if per_batch_erase is not None:
                    try:
                        er = next(per_batch_erase)
                    except StopIteration:
                        raise ValueError("erase yields fewer entries than there are batches") from None
                mx = None
                if per_batch_mix is not None:
                    try:
                        mx = next(per_batch_mix)
                    except StopIteration:
                        raise ValueError("mix yields fewer entries than there are batches") from None
                cp = None
                if per_batch_compose is not None:
                    try:
                        cp = next(per_batch_compose)
                    except StopIteration:
                        raise ValueError("compose yields fewer entries than there are batches") from None
                pt = None
                if per_batch_patches is not None:
                    try:
                        pt = next(per_batch_patches)
                    except StopIteration:
                        raise ValueError("patches yields fewer entries than there are batches") from None
                def none(g):
                    return g is None or (isinstance(g, (list, tuple)) and all(e is None for e in g))
                if per_batch_also is not None:
                    try:
                        a = next(per_batch_also)
                    except StopIteration:
                        raise ValueError("also yields fewer entries than there are batches") from None
                    plain = none(t) and none(ps)
                    main = dict(size=size, dtype=dtype, normalize=normalize, mirror=m, resample=resample, mode=mode, resize_to=resize_to, place=place,
                                fill=fill, reducing_gap=reducing_gap, views=v, affine=None if none(t) else t, affine_resample=None if plain else affine_resample,
                                affine_fill=None if plain else affine_fill, color_ops=c, perspective=None if none(ps) else ps, erase=er, mix=mx, compose=cp, patches=pt)
                    extra = normalize_also(a, dict(main, affine_resample=affine_resample, affine_fill=affine_fill), size)
                    if extra is not None:
                        yield self._merged_request(files, o, [main] + extra, lambda fs, **kw: self._device_request(fs, None, **kw))
                        continue
                if none(t) and none(ps):                # (a batch without a transform)
                    yield self._device_request(files, None, size, dtype, normalize, m, o, resample, mode, resize_to, place, fill, reducing_gap, v,
                                               color_ops=c, erase=er, mix=mx, compose=cp, patches=pt)
                    continue
                yield self._device_request(files, None, size, dtype, normalize, m, o, resample, mode, resize_to, place, fill, reducing_gap, v,
                                           None if none(t) else t, affine_resample, affine_fill, c, None if none(ps) else ps, er, mx, cp, pt)
        yield from self._device_iter(requests(), depth)

    def _device_iter(self, requests, depth=2):
        """:meth:`decode_device_iter` over checked requests (:meth:`_device_request`'s, or parts of one)."""
        import collections
        import torch
        dev = torch.device("cuda", self.ctx.device)
        copy_stream = torch.cuda.Stream(device=dev)
        depth = max(1, int(depth))
        pinned = [None] * (depth + 1)
        uploaded = [None] * (depth + 1)     # event behind the latest upload out of each pinned buffer
        turn = 0
        pending = collections.deque()       # the batches in flight (_Flight), oldest first

        def collect(flight):
            req = flight.req
            try:
                flight.sync()
                tail, unconverged = _triage(flight.plan.read(rgb=False)["status"], np.arange(len(req.files)), index=req.index)
                out = flight.d_rgb if req.size is not None else self._views(flight.d_rgb, self._out_shapes(flight.prep, req.wins, req.orient, req.ncomp))
            finally:
                flight.close()
            again = sorted(tail + unconverged)
            if again:                                             # only the files concerned take the long way (host parse)
                redo = self._decode_request(req.narrow(again))
                if req.size is None:
                    for i, img in zip(again, redo):
                        out[i] = img
            return self._mixed(req, out)

        try:
            for req in requests:
                files = req.files
                prep = None
                if self.gpu_segment and self.native_host and files and len(req.orient_classes()) == 1:
                    buf, turn = turn, (turn + 1) % (depth + 1)
                    need = sum(map(len, files)) + 3 * len(files) + 1024
                    if uploaded[buf] is not None:
                        uploaded[buf].synchronize()               # depth + 1 batches ago: long done
                    if pinned[buf] is None or pinned[buf].numel() < need:
                        pinned[buf] = torch.empty(need + need // 4, dtype=torch.uint8, pin_memory=True)
                    prep = prepare_batch_native(files, self.layout, self.base_flags, staging=pinned[buf].numpy())
                if not isinstance(prep, PreparedBatch):           # declined, or several plans' worth: the one-call path sorts it out
                    while pending:
                        yield collect(pending.popleft())
                    yield self._mixed(req, self._decode_request(req))
                    continue
                with torch.cuda.stream(copy_stream):
                    d_blob = pinned[buf][:prep.blob.size].to(dev, non_blocking=True)
                    uploaded[buf] = torch.cuda.Event()
                    uploaded[buf].record(copy_stream)
                plans = self._group_plans(req, prep, d_blob.data_ptr())
                lead, plan = plans[0]
                flight = _Flight(req, None, prep, plan, None, d_blob, plans[1:])
                try:
                    # (both tensors outlive the kernels that touch them: they stay in `pending` until the plan has been collected)
                    d_rgb = flight.d_rgb = lead.dest if lead.dest is not None else torch.empty(plan.info.rgb_bytes, dtype=torch.uint8, device=dev)
                    self.ctx.wait_event(uploaded[buf].cuda_event)
                    self._wait_for_current_stream(torch.cuda.current_stream(dev))
                    plan.execute(0, d_rgb.data_ptr())
                    for g, derived in flight.extra:
                        derived.execute(0, g.dest.data_ptr())
                except BaseException:
                    flight.close()
                    raise
                pending.append(flight)
                while len(pending) > depth:
                    yield collect(pending.popleft())
            while pending:
                yield collect(pending.popleft())
        finally:
            while pending:                                        # (an error, or a consumer that stopped early: nothing stays open)
                pending.popleft().close()

    def close(self):
        self.ctx.close()
