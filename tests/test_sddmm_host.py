"""spmv_csr_sddmm's C ABI without a device (include/spmv_hip.h "SDDMM"): the entry point is declared, exported by the
normal and the bounds-checked library and bound in capi; CsrMatrix.sddmm exists; a null handle is refused
(SPMV_ERR_INVALID, a message that names the function) instead of crashing; the sparse_layer module imports and holds the
autograd function and its holder.  The numpy recipe the GPU tests take their expectation from is checked against a dense
product."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import _exact as E

ROOT = Path(__file__).resolve().parent.parent
NAME = "spmv_csr_sddmm"


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_sddmm_symbol_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    assert NAME in declared, f"{NAME} not declared in include/spmv_hip.h"
    assert NAME in capi.SIGNATURES, f"{NAME} not bound in capi.SIGNATURES"
    assert len(capi.SIGNATURES[NAME][1]) == 8
    assert NAME in _exports(capi.LIB_PATH), f"{NAME} not exported by {capi.LIB_PATH.name}"
    assert NAME in _exports(capi.CHECKED_LIB_PATH), f"{NAME} not exported by {capi.CHECKED_LIB_PATH.name}"
    assert callable(getattr(capi.CsrMatrix, "sddmm", None)), "CsrMatrix.sddmm missing"
    assert "spmv_csr_sddmm the same as spmv_csr_spmm" in re.sub(r"\s+", " ", header), "no line in 'Limits of the layouts'"


def test_sddmm_refuses_a_null_handle(pkg):
    capi = pkg.capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert lib.spmv_csr_sddmm(None, 4, p, 4, p, 4, p, None) == capi.ERR_INVALID
    assert NAME in lib.spmv_last_error().decode()
    assert lib.spmv_csr_sddmm(None, 0, None, 0, None, 0, None, None) == capi.ERR_INVALID
    assert NAME in lib.spmv_last_error().decode()


def test_sparse_layer_imports(pkg):
    import torch
    sl = pkg.sparse_layer
    assert issubclass(sl.SparseMatmul, torch.autograd.Function)
    assert callable(sl.SparseLayer) and sl.MAX_K == 64
    assert "sparse_layer" in pkg.__all__


def host_sddmm(s, U, X):
    """The specification in int64: out[n] = U[row(n)] . X[col(n)]."""
    return np.einsum("nc,nc->n", U[s.row_of].astype(np.int64), X[s.ci].astype(np.int64))


def test_the_numpy_recipe(pkg, oracle):
    for name in ("not_multiple_of_anything", "lengths_around_short_threshold", "trailing_empty_rows"):
        s = E.structure(name, pkg, oracle)
        rng = np.random.Generator(np.random.PCG64(len(name)))
        U = rng.integers(-4, 5, size=(s.rows, 5))
        X = rng.integers(-4, 5, size=(s.cols, 5))
        dense = U @ X.T
        assert np.array_equal(host_sddmm(s, U, X), dense[s.row_of, s.ci]), name
