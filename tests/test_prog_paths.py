"""The progressive stage 1's rare symbol paths on the GPU: every row of tests/prog_cases.py against what the reference made of it
(tests/golden/prog_paths.npz), coefficient store and pixels, in both layouts and in every launch form — the stream walks, the
general walk, one launch per level, bands of two and three MCU rows, refining scans split into scout + parts, first scans in
chunks, the GPU marker scan.  tests/test_prog_paths_host.py proves on the host that each row reaches its path.
Needs a real MI355X: run with `-m gpu`."""
import numpy as np
import pytest

from conftest import GOLDEN
from prog_cases import EXTRA, ROWS, row_bytes

pytestmark = pytest.mark.gpu

OK = [r for r in ROWS if not r.refused]
REFUSED = [r for r in ROWS if r.refused]
FORMS = {
    "default": {},
    "general_walk": {"MJ_PROG_FAST": "0"},
    "levels": {"MJ_PROG_BANDS": "0"},
    "two_row_bands": {"MJ_PROG_ROWS": "2"},
    "three_row_bands": {"MJ_PROG_ROWS": "3"},
    # scout + parts for every refining scan: parts that start inside an end-of-band run, bands with fewer blocks than parts
    "split_2_parts": {"MJ_PROG_SPLIT": "2", "MJ_PROG_PARTS": "2"},
    "split_8_parts": {"MJ_PROG_SPLIT": "2", "MJ_PROG_PARTS": "8"},
    "chunks_128": {"MJ_PROG_CHUNKS": "2", "MJ_PROG_CHUNK": "128"},
    "chunks_512": {"MJ_PROG_CHUNKS": "2", "MJ_PROG_CHUNK": "512"},
    "gpu_marker_scan": {},
}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "prog_paths.npz")


@pytest.fixture(scope="module")
def decs():
    from pyjpegdecoder_amd import BatchDecoder
    d = {"x": BatchDecoder(device=0, segment="host"), "rm": BatchDecoder(device=0, layout="rowmajor", segment="host"),
         "x_gs": BatchDecoder(device=0, segment="gpu", gpu_segment_min_files=1),
         "rm_gs": BatchDecoder(device=0, layout="rowmajor", segment="gpu", gpu_segment_min_files=1),
         "spec": BatchDecoder(device=0, spec_refine=True, segment="host"),
         "spec_rm": BatchDecoder(device=0, layout="rowmajor", spec_refine=True, segment="host")}
    yield d
    for v in d.values():
        v.close()


def _pair(decs, form):
    return (decs["x_gs"], decs["rm_gs"]) if form == "gpu_marker_scan" else (decs["x"], decs["rm"])


def test_the_committed_files_are_the_rows(gold):
    for r in ROWS:
        assert gold[r.name + ".jpg"].tobytes() == row_bytes(r.name), r.name


@pytest.mark.parametrize("form", list(FORMS))
def test_rows_against_the_reference(decs, gold, tune, form):
    """Every row the reference decodes, in one mixed batch per layout: the coefficient store (in the reference's order in both
    layouts: the row-major launch transposes inside the block) and the pixels."""
    for k, v in FORMS[form].items():
        tune(k, v)
    files = [row_bytes(r.name) for r in OK]
    for layout, dec in zip(("xmajor", "rowmajor"), _pair(decs, form)):
        imgs, seams = dec.decode(files, return_seams=True)
        for r, img, seam in zip(OK, imgs, seams):
            assert np.array_equal(seam["coef"], gold[r.name + ".coef"]), (form, layout, r.name)
            assert np.array_equal(seam["planes"], gold[r.name + ".planes"]), (form, layout, r.name)
            assert np.array_equal(img if layout == "xmajor" else np.swapaxes(img, 0, 1), gold[r.name + ".rgb"]), (form, layout, r.name)


@pytest.mark.parametrize("form", list(FORMS))
def test_refused_rows_raise_and_leave_the_decoder_healthy(decs, gold, tune, form):
    """The rows the reference raises on (a position behind 63, no code within 16 bits, a refining run with too few zeros, a refining
    end-of-band run past the scan's last block), one file per call: the library's exception for a damaged stream, and a healthy row decodes correctly afterwards."""
    from pyjpegdecoder_amd import CorruptedJpeg
    for k, v in FORMS[form].items():
        tune(k, v)
    for layout, dec in zip(("xmajor", "rowmajor"), _pair(decs, form)):
        for r in REFUSED:
            with pytest.raises(CorruptedJpeg):
                dec.decode([row_bytes(r.name)])
            (img,), (seam,) = dec.decode([row_bytes("R-hist")], return_seams=True)
            assert np.array_equal(seam["coef"], gold["R-hist.coef"]), (form, layout, r.name)
            assert np.array_equal(img if layout == "xmajor" else np.swapaxes(img, 0, 1), gold["R-hist.rgb"]), (form, layout, r.name)


@pytest.mark.parametrize("chunk", ["128", "512"])
def test_chunked_first_scans_settle_on_the_device(decs, tune, chunk):
    """Under chunks a conformant row needs no second decode by the host layer: the plan reports the chunked form and ends with
    device status 0 (as test_progressive_launch_forms asserts of the fixtures at 512 bytes; the rows settle at 128 bytes too —
    every status is printed).  A row whose first scans hold what no encoder writes may be handed back (MJ_ST_UNCONVERGED: the
    host layer decodes it again with the wavefront walks); its pixels are held by test_rows_against_the_reference either way.
    Only the rows that HAVE a first AC scan for the stream walks: a plan without one drops the chunked form, and so does a
    layout with a factor of 3, which the general walk decodes (F-3x) — their status would say nothing about chunks."""
    from pyjpegdecoder_amd import _binding as B
    from pyjpegdecoder_amd._parse import parse_jpeg
    from pyjpegdecoder_amd.batch import prepare_batch
    tune("MJ_PROG_CHUNKS", "2")
    tune("MJ_PROG_CHUNK", chunk)
    dec = decs["x"]

    def chunked(raw):
        p = parse_jpeg(raw)
        factors = [f for c in p.color_components.values() for f in (c.horizontal_sampling, c.vertical_sampling)]
        return any(s.spectral_start > 0 and s.bit_high == 0 for s in p.scans) and 3 not in factors
    rows = [r for r in OK if chunked(row_bytes(r.name))]
    assert {r.name[0] for r in rows} == {"F", "R"} and len(rows) == len([r for r in OK if r.name[0] in "FR"]) - 1
    for r in rows:
        prep = prepare_batch([row_bytes(r.name)], B.MJ_LAYOUT_XMAJOR, 0)
        plan = B.Plan(dec.ctx, prep.to_c(), {"prep": prep, "n_images": 1})
        try:
            assert plan.stage1_form() & B.MJ_FORM_COUNT_RESOLVED, (r.name, plan.stage1_form())
            plan.execute()
            plan.sync()
            st = int(plan.read(rgb=False)["status"][0])
            print(f"chunk {chunk} {r.name}: form {plan.stage1_form():#x} status {st}")
            if r.conformant:
                assert st == 0, (r.name, st)
            else:
                assert st in (0, B.MJ_ST_UNCONVERGED), (r.name, st)
        finally:
            plan.close()


@pytest.mark.parametrize("form", ["default", "general_walk", "levels", "split_2_parts", "split_8_parts"])
def test_refining_rows_under_spec_refine(decs, gold, tune, form):
    """spec_refine=True (negative history refined by subtraction, T.81 G.1.2.3): the rows with refining AC scans against the
    model walk's result under the same switch — committed with the goldens, since no other reference for it exists."""
    for k, v in FORMS[form].items():
        tune(k, v)
    rows = [r for r in OK if r.name.startswith("R-")]
    differ = sum(not np.array_equal(gold[r.name + ".spec_coef"], gold[r.name + ".coef"]) for r in rows)
    assert len(rows) == 10 and differ >= 5, "the switch changes the result of at least half of these rows"
    for layout, dec in (("xmajor", decs["spec"]), ("rowmajor", decs["spec_rm"])):
        _, seams = dec.decode([row_bytes(r.name) for r in rows], return_seams=True)
        for r, seam in zip(rows, seams):
            assert np.array_equal(seam["coef"], gold[r.name + ".spec_coef"]), (form, layout, r.name)


@pytest.mark.parametrize("form", list(FORMS))
def test_the_32_bit_dc_symbol_against_the_oracle(decs, tune, form):
    """A 16-bit DC code with 16 value bits, the longest symbol a stream can hold, in every form (each of them walks DC scans).
    The reference's array library refuses the sum (prog_cases.EXTRA), so this one file is held to the oracle."""
    from oracle import oracle
    for k, v in FORMS[form].items():
        tune(k, v)
    raw = row_bytes(EXTRA[0].name)
    want = oracle.decode(raw)
    for layout, dec in zip(("xmajor", "rowmajor"), _pair(decs, form)):
        (img,), (seam,) = dec.decode([raw], return_seams=True)
        assert np.array_equal(seam["coef"], want["coef"]), (form, layout)
        assert np.array_equal(img if layout == "xmajor" else np.swapaxes(img, 0, 1), want["rgb"]), (form, layout)
