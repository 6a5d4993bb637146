#!/usr/bin/env python3
"""tests/golden/base_paths.npz: what the REFERENCE makes of every row of tests/base_cases.py (like tools/make_prog_path_goldens.py:
the reference is imported here and only here; what is committed is data).

Per row: the file's bytes (`<row>.jpg`) and either the coefficients it decoded, the image, and which MCUs hold a block whose
samples leave int16 before the reference's cast (:1573, undefined: the pixel comparison leaves those MCUs out) — `.coef`, `.rgb`,
`.mask` — or, where the reference raises, the name of its exception (`.refused`).  A row whose outcome is not what its line of the
table says, or with masked MCUs where the table allows none, stops the tool.

Usage:  python tools/make_base_path_goldens.py [row ...]      (no rows: all of them)"""
import sys
import tempfile
import warnings
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

GOLD = ROOT / "tests" / "golden" / "base_paths.npz"


def one(name):
    from tools import make_goldens as mg          # imports the reference as mg.jd
    import base_cases as bc
    raw = bc.row_bytes(name)
    out = {name + ".jpg": np.frombuffer(raw, dtype=np.uint8)}
    with tempfile.NamedTemporaryFile(suffix=".jpg") as f:
        f.write(raw)
        f.flush()
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                         # (int16 sums that wrap: the point of some rows)
                dec, cap = mg.run_reference(Path(f.name))
        except Exception as exc:                                        # noqa: BLE001 — whatever the reference raises
            out[name + ".refused"] = np.frombuffer(type(exc).__name__.encode(), dtype=np.uint8)
            return name, out, f"refused ({type(exc).__name__}: {exc})"
    coef = np.array(cap["coef"], dtype=np.int16).reshape(-1, 64)
    out[name + ".coef"] = coef
    out[name + ".rgb"] = np.array(dec.image_array)
    out[name + ".mask"] = bc.overflow_mask(coef, 6)
    return name, out, f"{len(raw)} bytes, {coef.shape[0]} blocks, {int(out[name + '.mask'].sum())} MCUs masked, rgb {mg.sha(out[name + '.rgb'])[:12]}"


def main():
    import base_cases as bc
    names = sys.argv[1:] or [r.name for r in bc.ROWS]
    out = dict(np.load(GOLD)) if GOLD.exists() and sys.argv[1:] else {}
    with ProcessPoolExecutor(8) as pool:
        for name, vec, text in pool.map(one, names):
            print(f"{name}: {text}", flush=True)
            row = bc.ROW[name]
            got = bytes(vec[name + ".refused"]).decode() if name + ".refused" in vec else ""
            assert got == row.ref, f"{name}: the table says the reference {'raises ' + row.ref if row.ref else 'decodes it'}"
            assert row.ref or row.masked or not vec[name + ".mask"].any(), f"{name}: samples leave int16 in a row that is compared whole"
            out = {k: v for k, v in out.items() if not k.startswith(name + ".")}
            out.update(vec)
    np.savez_compressed(GOLD, **out)
    print(f"{len(names)} rows -> {GOLD.name}, {GOLD.stat().st_size} bytes")
    assert GOLD.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
