#!/usr/bin/env python3
"""tests/golden/prog_paths.npz: what the REFERENCE makes of every row of tests/prog_cases.py (like tools/make_layout_goldens.py:
the reference is imported here and only here; what is committed is data).

Per row: the file's bytes (`<row>.jpg`) and either the coefficient store after the last scan, the planes and the image
(`.coef`, `.planes`, `.rgb`), or — where the reference raises — the name of its exception (`.refused`).  For the rows with
refining AC scans also the model walk's coefficients under spec_refine (`.spec_coef`): no other reference for that switch
exists.  A row whose result is not what its `refused` flag in the table says stops the tool.

Usage:  python tools/make_prog_path_goldens.py [row ...]      (no rows: all of them, the two large ones included — minutes)"""
import sys
import tempfile
import warnings
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

GOLD = ROOT / "tests" / "golden" / "prog_paths.npz"


def one(name):
    from tools import make_goldens as mg          # imports the reference as mg.jd
    import prog_cases as pc
    raw = pc.row_bytes(name)
    out = {name + ".jpg": np.frombuffer(raw, dtype=np.uint8)}
    with tempfile.NamedTemporaryFile(suffix=".jpg") as f:
        f.write(raw)
        f.flush()
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                         # (int16 sums that wrap: the point of some rows)
                dec, cap = mg.run_reference_progressive(Path(f.name))
        except Exception as exc:                                        # noqa: BLE001 — whatever the reference raises
            out[name + ".refused"] = np.frombuffer(type(exc).__name__.encode(), dtype=np.uint8)
            return name, out, f"refused ({type(exc).__name__}: {exc})"
    out[name + ".coef"] = mg.pixel_layout_to_blocks(cap["pre_idct"], dec)
    out[name + ".planes"] = cap["planes"]
    out[name + ".rgb"] = np.array(dec.image_array)
    if name.startswith("R-"):
        out[name + ".spec_coef"] = pc.walk(raw, spec_refine=True)
    return name, out, f"{len(raw)} bytes, {out[name + '.coef'].shape[0]} blocks, rgb {mg.sha(out[name + '.rgb'])[:12]}"


def main():
    import prog_cases as pc
    names = sys.argv[1:] or [r.name for r in pc.ROWS]
    out = dict(np.load(GOLD)) if GOLD.exists() and sys.argv[1:] else {}
    with ProcessPoolExecutor(8) as pool:
        for name, vec, text in pool.map(one, names):
            print(f"{name}: {text}", flush=True)
            assert (name + ".refused" in vec) == pc.ROW[name].refused, f"{name}: the table says refused={pc.ROW[name].refused}"
            out = {k: v for k, v in out.items() if not k.startswith(name + ".")}
            out.update(vec)
    np.savez_compressed(GOLD, **out)
    print(f"{len(names)} rows -> {GOLD.name}, {GOLD.stat().st_size} bytes")


if __name__ == "__main__":
    main()
