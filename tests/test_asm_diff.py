"""Host only: tools/asm_diff.py on two hand-written listings (tests/golden/asm_diff_a.s, asm_diff_b.s) — a kernel that is the same
code under other label numbers and comments, a kernel that differs, and a kernel that changed its name."""
import io

from conftest import GOLDEN

A, B = str(GOLDEN / "asm_diff_a.s"), str(GOLDEN / "asm_diff_b.s")
RENAME = ["--rename", r"k_two_old\(", "k_two("]


def run(*argv):
    from tools import asm_diff
    buf = io.StringIO()
    rc = asm_diff.main(list(argv), out=buf)
    lines = buf.getvalue().splitlines()
    return rc, dict(ln.split(": ", 1) for ln in lines[:-1]), lines[-1]


def test_identical():
    """a listing against itself, and k_one against its copy with other label numbers and comments"""
    rc, rows, total = run(A, A)
    assert rc == 0 and set(rows.values()) == {"identical"} and len(rows) == 3 and total.startswith("3 kernels: 3 identical")
    rc, rows, _ = run(A, B, "--only", "k_one")
    assert rc == 0 and rows == {"k_one(int*)": "identical"}


def test_one_kernel_differs():
    rc, rows, total = run(A, B, *RENAME)
    assert rc == 1 and "1 not allowed" in total
    assert rows["k_three(int*)"] == "differs (3 -> 4 instructions; NumVgprs 2 -> 3, TotalNumSgprs 6 -> 6, ScratchSize 0 -> 0)"
    assert rows["k_one(int*)"] == rows["k_two(int*)"] == "identical"
    rc, rows, total = run(A, B, *RENAME, "--allow", "k_three")
    assert rc == 0 and rows["k_three(int*)"].endswith("[allowed]") and "0 not allowed" in total


def test_renamed_kernel():
    """without the rename map both names are unmatched; with it the kernel is found and is the same code"""
    rc, rows, _ = run(A, B, "--allow", "k_three")
    assert rc == 1 and rows["k_two_old(int*)"] == "only in A" and rows["k_two(int*)"] == "only in B"
    rc, rows, _ = run(A, B, *RENAME, "--allow", "k_three")
    assert rc == 0 and "k_two_old(int*)" not in rows and rows["k_two(int*)"] == "identical"
