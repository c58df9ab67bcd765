"""The transpose's C ABI without a device (include/spmv_hip.h "the transpose"): the three entry points are declared,
exported by the normal and the bounds-checked library and bound in capi; null arguments are refused (SPMV_ERR_INVALID, a
message that names the function, *out untouched) instead of crashing; sparse_sgemv knows --transpose.  The numpy recipe
the GPU tests take their expectation from is checked here against a dense transposition."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import _exact as E

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("spmv_csr_transpose", "spmv_csr_transpose_values", "spmv_csr_transpose_map_bytes")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_transpose_symbols_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    for name in NAMES:
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert name in _exports(capi.LIB_PATH), f"{name} not exported by {capi.LIB_PATH.name}"
        assert name in _exports(capi.CHECKED_LIB_PATH), f"{name} not exported by {capi.CHECKED_LIB_PATH.name}"
    for m in ("transpose", "transpose_values", "transpose_map_bytes"):
        assert callable(getattr(capi.CsrMatrix, m, None)), f"CsrMatrix.{m} missing"
    assert "spmv_csr_transpose any handle" in re.sub(r"\s+", " ", header), "no line in 'Limits of the layouts'"


def test_transpose_entry_points_refuse_null_arguments(pkg):
    capi = pkg.capi
    lib = capi.lib()

    def last():
        return lib.spmv_last_error().decode()

    out = C.c_void_p()
    assert lib.spmv_csr_transpose(None, 0, None, C.byref(out)) == capi.ERR_INVALID
    assert "spmv_csr_transpose" in last() and out.value is None
    dummy = C.create_string_buffer(64)                     # out = NULL is refused before `a` is looked at
    assert lib.spmv_csr_transpose(C.addressof(dummy), 0, None, None) == capi.ERR_INVALID
    assert "spmv_csr_transpose" in last()
    assert lib.spmv_csr_transpose_values(None, None, None) == capi.ERR_INVALID
    assert "spmv_csr_transpose_values" in last()
    assert lib.spmv_csr_transpose_map_bytes(None) < 0
    assert "spmv_csr_transpose_map_bytes" in last()


def test_cli_knows_transpose(pkg, tmp_path):
    p = tmp_path / "a.mtx"
    p.write_text("%%MatrixMarket matrix coordinate real general\n3 4 3\n1 1 1.5\n2 4 -2\n3 2 7\n")
    tester = str(pkg.capi.TESTER_PATH)
    r = subprocess.run([tester, "--mtx", str(p), "--transpose", "--parse-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "matrix 3 x 4, nnz 3" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([tester, "--mtx", str(p), "--transposed", "--parse-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "unknown option" in r.stderr


def host_transpose(rows, cols, rp, ci, vals):
    """The specification (include/spmv_hip.h): perm = argsort(col_idx, stable)."""
    ci = np.asarray(ci, np.int64)
    perm = np.argsort(ci, kind="stable")
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))
    t_rp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=cols))]).astype(np.int32)
    return t_rp, row_of[perm].astype(np.int32), np.asarray(vals)[perm], perm


def test_the_numpy_recipe(pkg, oracle):
    """T's rows come out sorted, T is the dense transposition, the double transpose is the row-wise stable column sort,
    and Exact data put on T and carried back to A gives Exact.expected() through a float64 scatter over A."""
    for name in sorted(E.EDGE_CASES) + list(E.SPECIAL):
        s0 = E.structure(name, pkg, oracle)
        for s in (s0, E.shuffled(s0, name)[0]):
            ident = np.arange(s.nnz, dtype=np.int64)
            t_rp, t_ci, t_pos, perm = host_transpose(s.rows, s.cols, s.rp, s.ci, ident)
            assert np.array_equal(t_pos, perm)
            st = E.Structure(s.cols, s.rows, t_rp, t_ci)
            same_row = st.row_of[1:] == st.row_of[:-1]
            assert np.all(np.diff(t_ci.astype(np.int64))[same_row] >= 0), name
            assert np.array_equal(st.row_of, s.ci[perm])
            # back again: A with every row stably sorted by column
            b_rp, b_ci, b_pos, _ = host_transpose(st.rows, st.cols, t_rp, t_ci, perm)
            order = np.lexsort((ident, s.ci, s.row_of))
            assert np.array_equal(b_rp, s.rp) and np.array_equal(b_ci, s.ci[order]) and np.array_equal(b_pos, order), name
            # Exact data on T, carried back to A's storage order
            ex = E.Exact(st, name + "/T")
            va_a = np.empty(s.nnz, np.float32)
            va_a[perm] = ex.vals()
            z = np.zeros(s.cols, np.float64)
            np.add.at(z, s.ci, va_a.astype(np.float64) * ex.x()[s.row_of].astype(np.float64))
            assert np.array_equal(z.astype(np.float32) + np.float32(0), ex.expected() + np.float32(0)), name
