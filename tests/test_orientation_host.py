"""EXIF orientation, the host side (no GPU): tools/orient_model.py against Pillow and against brute force; the tag reader
(pyjpegdecoder_amd.exif_orientation, the specification) on APP1 segments spliced behind SOI of golden files, against Pillow's
getexif() where Pillow opens the file, and its native twin (mj_host_exif_orientations) file by file; the new keyword's checks."""
import io
import struct

import numpy as np
import pytest

from conftest import GOLDEN

SHAPES = ((5, 7), (7, 5), (1, 9), (9, 1), (29, 37), (36, 100), (1, 1), (6, 6))


def test_orient_against_brute_force():
    from tools import orient_model
    for (h, w) in SHAPES:
        for tail in ((), (3,)):
            a = np.arange(h * w * (tail[0] if tail else 1), dtype=np.int32).reshape((h, w) + tail)
            for o in range(1, 9):
                got = orient_model.orient(a, o)
                wo, ho = orient_model.oriented_size(o, w, h)
                assert got.shape == (ho, wo) + tail
                for y in range(ho):
                    for x in range(wo):
                        # where the pixel shown at (x, y) is stored: the EXIF definition, orientation by orientation
                        sx, sy = {1: (x, y), 2: (w - 1 - x, y), 3: (w - 1 - x, h - 1 - y), 4: (x, h - 1 - y), 5: (y, x),
                                  6: (y, h - 1 - x), 7: (w - 1 - y, h - 1 - x), 8: (w - 1 - y, x)}[o]
                        assert np.array_equal(got[y, x], a[sy, sx]), (o, h, w, x, y)


def test_orient_is_pillows_exif_transpose():
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    from tools import orient_model
    rng = np.random.default_rng(3)
    ops = {2: Image.FLIP_LEFT_RIGHT, 3: Image.ROTATE_180, 4: Image.FLIP_TOP_BOTTOM, 5: Image.TRANSPOSE, 6: Image.ROTATE_270,
           7: Image.TRANSVERSE, 8: Image.ROTATE_90}
    for (h, w) in SHAPES:
        for tail in ((), (3,)):
            a = rng.integers(0, 256, (h, w) + tail, dtype=np.uint8)
            for o in range(1, 9):
                img = Image.fromarray(a)
                if o in ops:
                    assert np.array_equal(np.asarray(img.transpose(ops[o])), orient_model.orient(a, o)), (o, h, w)
                exif = img.getexif()
                exif[0x0112] = o
                img.info["exif"] = exif.tobytes()
                turned = ImageOps.exif_transpose(img)
                assert np.array_equal(np.asarray(turned), orient_model.orient(a, o)), (o, h, w)


def test_stored_window_against_brute_force():
    from tools import orient_model
    for (h, w) in ((5, 7), (7, 4), (1, 6), (3, 3)):
        a = np.arange(h * w).reshape(h, w)
        for o in range(1, 9):
            shown = orient_model.orient(a, o)
            ho, wo = shown.shape
            for x in range(wo):
                for y in range(ho):
                    for ww in range(1, wo - x + 1):
                        for hh in range(1, ho - y + 1):
                            sx, sy, sw, sh = orient_model.stored_window(o, w, h, (x, y, ww, hh))
                            assert 0 <= sx and 0 <= sy and sx + sw <= w and sy + sh <= h
                            assert np.array_equal(shown[y:y + hh, x:x + ww], orient_model.orient(a[sy:sy + sh, sx:sx + sw], o))


# ---- the tag -------------------------------------------------------------------------------------------------------------------
def entry(order, tag, typ, count, value):
    return struct.pack(order + "HHI", tag, typ, count) + struct.pack(order + "HH", value, 0)


def tiff(order, entries, ifd=8, count=None, magic=42):
    head = (b"II" if order == "<" else b"MM") + struct.pack(order + "H", magic) + struct.pack(order + "I", ifd)
    body = struct.pack(order + "H", len(entries) if count is None else count) + b"".join(entries) + struct.pack(order + "I", 0)
    return head + b"\0" * max(0, ifd - 8) + body


def segment(marker, payload):
    return bytes((0xFF, marker)) + struct.pack(">H", len(payload) + 2) + payload


def exif(order, entries, **kw):
    return segment(0xE1, b"Exif\0\0" + tiff(order, entries, **kw))


OTHER = [(0x010F, 3, 1, 7), (0x0128, 3, 1, 2), (0x0213, 3, 1, 1)]     # (sorted by tag around 0x0112, as TIFF asks)
JFIF = segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
XMP = segment(0xE1, b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta/>")


def cases():
    """(name, bytes spliced behind SOI, the answer, well formed: Pillow must agree)"""
    out = []
    for order in "<>":
        for o in range(0, 10):
            want = o if 1 <= o <= 8 else 1
            out.append((f"only_{order}{o}", exif(order, [entry(order, 0x0112, 3, 1, o)]), want, 1 <= o <= 8))
        first, last = [entry(order, *OTHER[0])], [entry(order, *e) for e in OTHER[1:]]
        out.append((f"second_{order}", exif(order, first + [entry(order, 0x0112, 3, 1, 6)] + last), 6, True))
        out.append((f"last_{order}", exif(order, first + [entry(order, 0x0112, 3, 1, 8)]), 8, True))
        out.append((f"jfif_xmp_in_front_{order}", JFIF + XMP + exif(order, [entry(order, 0x0112, 3, 1, 5)]), 5, True))
        out.append((f"ifd_further_on_{order}", exif(order, [entry(order, 0x0112, 3, 1, 3)], ifd=20), 3, True))
        out.append((f"type_long_{order}", exif(order, [entry(order, 0x0112, 4, 1, 6)]), 1, False))
        out.append((f"count_two_{order}", exif(order, [entry(order, 0x0112, 3, 2, 6)]), 1, False))
        out.append((f"ifd_outside_{order}", segment(0xE1, b"Exif\0\0" + tiff(order, [entry(order, 0x0112, 3, 1, 6)])[:8].replace(
            struct.pack(order + "I", 8), struct.pack(order + "I", 4000))), 1, False))
        out.append((f"count_outside_{order}", exif(order, [entry(order, 0x0112, 3, 1, 6)], count=40), 1, False))
        out.append((f"magic_{order}", exif(order, [entry(order, 0x0112, 3, 1, 6)], magic=43), 1, False))
        out.append((f"no_tag_{order}", exif(order, [entry(order, *e) for e in OTHER]), 1, True))
    out.append(("no_exif", b"", 1, True))
    out.append(("xmp_only", JFIF + XMP, 1, True))
    out.append(("second_exif_is_ignored", exif("<", [entry("<", *OTHER[0])]) + exif("<", [entry("<", 0x0112, 3, 1, 6)]), 1, False))
    out.append(("bad_byte_order", segment(0xE1, b"Exif\0\0" + b"XX" + tiff("<", [entry("<", 0x0112, 3, 1, 6)])[2:]), 1, False))
    out.append(("short_payload", segment(0xE1, b"Exif\0\0II"), 1, False))
    return out


def golden_files():
    return [f.read_bytes() for f in sorted((GOLDEN / "files").glob("*.jpg"))[:3]]


def spliced(raw, head):
    assert raw[:2] == b"\xff\xd8"
    return raw[:2] + head + raw[2:]


def test_exif_orientation_cases():
    from pyjpegdecoder_amd import exif_orientation, parse_jpeg
    for raw in golden_files():
        for name, head, want, _ in cases():
            f = spliced(raw, head)
            assert exif_orientation(f) == want, name
            assert parse_jpeg(f, headers_only=True).exif_orientation == want, name
    assert exif_orientation(b"") == 1 and exif_orientation(b"\xff\xd8") == 1 and exif_orientation(b"not a jpeg at all") == 1


def test_a_tag_behind_the_first_sos_is_not_read():
    from pyjpegdecoder_amd import exif_orientation
    raw = golden_files()[0]
    sos = raw.index(b"\xff\xda")
    assert exif_orientation(raw[:sos] + exif("<", [entry("<", 0x0112, 3, 1, 6)]) + raw[sos:]) == 6
    assert exif_orientation(raw + exif("<", [entry("<", 0x0112, 3, 1, 6)])) == 1


def test_a_segment_cut_at_every_length():
    from pyjpegdecoder_amd import exif_orientation
    from pyjpegdecoder_amd import _binding as B
    raw = golden_files()[0]
    for order in "<>":
        head = JFIF + exif(order, [entry(order, *OTHER[0]), entry(order, 0x0112, 3, 1, 7)])
        whole = spliced(raw, head)
        cuts = [whole[:n] for n in range(len(head) + 2)]
        assert [exif_orientation(c) for c in cuts] == [1] * len(cuts)         # the segment says more bytes than there are
        assert B.exif_orientations(cuts).tolist() == [1] * len(cuts)
        assert exif_orientation(whole[:2 + len(head)] + b"\xff\xd9") == 7
        # ... and a segment whose own length stops short: the IFD then points outside it
        for n in range(8, len(head) - len(JFIF) - 2):
            short = segment(0xE1, head[len(JFIF) + 4:len(JFIF) + 4 + n])
            f = spliced(raw, JFIF + short)
            full_entries = n >= 6 + 8 + 2 + 24
            assert exif_orientation(f) == (7 if full_entries else 1), n


def test_against_pillows_getexif():
    Image = pytest.importorskip("PIL.Image")
    from pyjpegdecoder_amd import exif_orientation
    raw = (GOLDEN / "example" / "base_image.jpg").read_bytes()
    checked = 0
    for name, head, want, well_formed in cases():
        if not well_formed:
            continue
        f = spliced(raw, head)
        try:
            tag = Image.open(io.BytesIO(f)).getexif().get(0x0112)
        except Exception:
            continue
        assert (tag if tag in range(1, 9) else 1) == exif_orientation(f) == want, name
        checked += 1
    assert checked >= 20


def test_native_reader_equals_the_python_one():
    from pyjpegdecoder_amd import exif_orientation
    from pyjpegdecoder_amd import _binding as B
    rng = np.random.default_rng(11)
    raw = golden_files()[1]
    files = [spliced(raw, head) for _, head, _, _ in cases()]
    assert B.exif_orientations(files).tolist() == [exif_orientation(f) for f in files]
    mutated = []
    for k in range(600):
        base = bytearray(files[k % len(files)][:400 if k % 3 else 90])
        for _ in range(int(rng.integers(1, 4))):
            base[int(rng.integers(0, min(len(base), 120)))] = int(rng.integers(0, 256))
        mutated.append(bytes(base))
    mutated += [b"", b"\xff", b"\xff\xd8", b"\xff\xd8\xff", b"\xff\xd8\xff\xe1", b"\xff\xd8\xff\xe1\x00"]
    want = [exif_orientation(f) for f in mutated]
    for threads in (1, 16):
        got = B.exif_orientations(mutated, n_threads=threads).tolist()
        assert got == want
    assert all(1 <= v <= 8 for v in want) and len(set(want)) > 2
    assert B.exif_orientations([]).size == 0
    assert B.exif_orientations([bytearray(files[3])]).tolist() == [exif_orientation(files[3])]      # (not bytes: the Python reader)


def test_normalize_orientation():
    from pyjpegdecoder_amd.batch import normalize_orientation
    raw = golden_files()[0]
    files = [spliced(raw, exif("<", [entry("<", 0x0112, 3, 1, o)])) for o in (6, 1, 3)]
    assert normalize_orientation(None, files) is None
    assert normalize_orientation(1, files) is None
    assert normalize_orientation([1, None, 1], files) is None
    assert normalize_orientation("exif", files) == [6, 1, 3]
    assert normalize_orientation("exif", [raw, raw]) is None
    assert normalize_orientation(8, files) == [8, 8, 8]
    assert normalize_orientation([2, "exif", None], files) == [2, 1, 1]
    assert normalize_orientation(["exif", 5, "exif"], files) == [6, 5, 3]
    assert normalize_orientation(np.array([4, 1, 7]), files) == [4, 1, 7]
    for bad in (0, 9, -1, True, 2.0, "EXIF", "auto", [1, 2], [1, 2, 9], [1, 2, "x"], [1, 2, 3.0], b"exif"):
        with pytest.raises(ValueError):
            normalize_orientation(bad, files)


def test_keyword_checks_need_no_gpu(monkeypatch):
    """orientation with return_seams, and values outside the table, are ValueErrors before any GPU work."""
    from pyjpegdecoder_amd import batch
    dec = batch.BatchDecoder.__new__(batch.BatchDecoder)            # (no context: the checks come first)
    dec.layout, dec.base_flags, dec.gpu_segment, dec.gpu_segment_min_files, dec.native_host = 0, 0, True, 8, True
    raw = golden_files()[0]
    with pytest.raises(ValueError, match="return_seams"):
        dec.decode([raw], return_seams=True, orientation=6)
    for bad in (0, 9, "auto", [6, 6]):
        with pytest.raises(ValueError, match="orientation"):
            dec.decode([raw], orientation=bad)
        with pytest.raises(ValueError, match="orientation"):
            dec.decode_device([raw], orientation=bad)
        if not isinstance(bad, list):       # (a per-batch value is checked when its batch comes)
            with pytest.raises(ValueError, match="orientation"):
                list(dec.decode_device_iter([[raw]], orientation=bad))
    w, h = batch._image_dims(raw)
    if w != h:
        with pytest.raises(ValueError, match="not inside"):       # the window is checked against the ORIENTED size
            dec.decode_device([raw], rois=(0, 0, w, h), orientation=6)


def test_request_carries_orientation_through_narrow():
    from pyjpegdecoder_amd.batch import _Request
    req = _Request([b"a", b"b", b"c", b"d"], orient=[6, 1, 3, 1], size=(4, 4))
    assert req.narrow([2, 0]).orient == [3, 6] and req.narrow([2, 0]).plan_kwargs()["orientation"] == [3, 6]
    assert req.narrow([1, 3]).orient is None and "orientation" not in req.narrow([1, 3]).plan_kwargs()
    assert sorted(map(tuple, req.orient_classes())) == [(0,), (1, 3), (2,)]
    assert sorted(map(tuple, _Request(req.files, orient=req.orient).orient_classes())) == [(0, 2), (1, 3)]
    assert _Request(req.files).orient_classes() == [[0, 1, 2, 3]]
