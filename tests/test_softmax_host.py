"""spmv_csr_row_softmax / spmv_csr_row_softmax_backward without a device (include/spmv_hip.h "Row softmax"): both entry
points are declared, exported by the normal and the bounds-checked library and bound in capi; the CsrMatrix methods and the
sparse_attention module exist; a null handle is refused (SPMV_ERR_INVALID, a message that names the function).  The numpy
recipe the GPU tests take their expectation from (tests/_softmax.py) is checked against torch.softmax on a dense fp64
matrix masked with -Inf, and a numpy emulation of the documented fp32 order of the sums stays inside the parity bound of
the GPU tests on rows of 1 .. 120 000 entries."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _exact as E
import _softmax as SM

ROOT = Path(__file__).resolve().parent.parent
NAMES = {"spmv_csr_row_softmax": 5, "spmv_csr_row_softmax_backward": 6}      # name -> number of arguments


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_softmax_symbols_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "spmv_hip.h").read_text()
    declared = set(re.findall(r"SPMV_API[^;(]*?\b(spmv_\w+)\s*\(", header))
    capi = pkg.capi
    flat = re.sub(r"\s+", " ", header)
    for name, nargs in NAMES.items():
        assert name in declared, f"{name} not declared in include/spmv_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert len(capi.SIGNATURES[name][1]) == nargs
        assert capi.SIGNATURES[name][1][1] is C.c_float, "scale is a float"
        assert name in _exports(capi.LIB_PATH), f"{name} not exported by {capi.LIB_PATH.name}"
        assert name in _exports(capi.CHECKED_LIB_PATH), f"{name} not exported by {capi.CHECKED_LIB_PATH.name}"
    limits = flat[flat.index("Limits of the layouts"):flat.index("tests/test_gpu_limits.py")]
    assert "spmv_csr_row_softmax any handle" in limits and "spmv_csr_row_softmax_backward the same" in limits
    assert callable(getattr(capi.CsrMatrix, "row_softmax", None)), "CsrMatrix.row_softmax missing"
    assert callable(getattr(capi.CsrMatrix, "row_softmax_backward", None)), "CsrMatrix.row_softmax_backward missing"


def test_sparse_attention_imports(pkg):
    import torch
    sa = pkg.sparse_attention
    assert issubclass(sa.SparseAttentionFunction, torch.autograd.Function)
    assert callable(sa.SparseAttention) and sa.MAX_K == 64
    assert "sparse_attention" in pkg.__all__ and "sparse_layer" in pkg.__all__


def test_softmax_refuses_a_null_handle(pkg):
    capi = pkg.capi
    lib = capi.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert lib.spmv_csr_row_softmax(None, 1.0, p, p, None) == capi.ERR_INVALID
    assert "spmv_csr_row_softmax:" in lib.spmv_last_error().decode()
    assert lib.spmv_csr_row_softmax(None, 1.0, None, None, None) == capi.ERR_INVALID
    assert lib.spmv_csr_row_softmax_backward(None, 1.0, p, p, p, None) == capi.ERR_INVALID
    assert "spmv_csr_row_softmax_backward:" in lib.spmv_last_error().decode()


@pytest.mark.parametrize("scale", SM.SCALES)
def test_the_numpy_recipe_against_torch_softmax(pkg, oracle, scale):
    import torch
    for name in ("not_multiple_of_anything", "lengths_around_short_threshold", "trailing_empty_rows"):
        s = E.structure(name, pkg, oracle)
        rng = np.random.Generator(np.random.PCG64([len(name), 5]))
        scores = SM.clipped_scores(rng, s.nnz, scale)
        scores[rng.random(s.nnz) < 0.2] = -np.inf if scale > 0 else np.inf            # masked entries
        first = s.rp[:-1][np.diff(s.rp) > 0]
        scores[first] = 0.5                                                            # (no row fully masked)
        ref, D, L = SM.recipe(s.rp, scores, scale)
        dense = torch.full((s.rows, s.cols), -np.inf, dtype=torch.float64)
        dense[torch.from_numpy(s.row_of), torch.from_numpy(s.ci.astype(np.int64))] = torch.from_numpy(
            SM.scaled(scores, scale).astype(np.float64))
        full = np.flatnonzero(np.diff(s.rp) > 0)
        want = torch.softmax(dense[full], dim=1).numpy()
        got = want[np.searchsorted(full, s.row_of), s.ci]
        assert np.allclose(ref, got, rtol=1e-13, atol=0), name
        masked = np.isinf(scores)
        assert np.all(ref[masked] == 0) and np.all(ref[~masked] > 0)
        assert np.array_equal(L, np.diff(s.rp)[s.row_of])
    # the rows torch.softmax turns into NaN are NaN here too
    rp = np.array([0, 3, 6, 9, 12])
    sc = np.array([1, np.nan, 2, 1, np.inf, 2, -np.inf, -np.inf, -np.inf, 1, -np.inf, 3], np.float32)
    ref, _, _ = SM.recipe(rp, sc, 1.0)
    want = torch.softmax(torch.from_numpy(sc.astype(np.float64)).view(4, 3), dim=1).numpy().reshape(-1)
    assert np.array_equal(np.isnan(ref), np.isnan(want)) and np.isnan(ref[:9]).all()
    assert np.allclose(ref[9:], want[9:], rtol=1e-13, atol=0) and ref[10] == 0


def test_chain_lengths():
    assert [int(SM.chain(L)) for L in (1, 64, 65, 512, 513, 1024, 1025, 120_000)] == [7, 7, 8, 14, 16, 16, 17, 249]


LENGTHS = (1, 2, 3, 31, 64, 65, 127, 512, 513, 1024, 1025, 4100, 20_000, 120_000)


@pytest.mark.parametrize("scale", (1.0, 0.125, -0.5) + SM.SCALES[2:])
def test_the_documented_order_stays_inside_the_parity_bound(scale):
    worst = 0.0
    for L in LENGTHS:
        rng = np.random.Generator(np.random.PCG64([L, 11]))
        scores = SM.clipped_scores(rng, L, scale)
        ref, D, Ls = SM.recipe(np.array([0, L]), scores, scale)
        assert D.max() <= 32.0 and ref.min() >= 1e-17
        out = SM.emulate_row(scores, scale)
        ratio = np.abs(out.astype(np.float64) - ref) / SM.parity_bound(ref, D, Ls)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, f"L={L}: {ratio.max():.3g} of the bound"
    print(f"scale={scale}: the emulated order reaches {worst:.3g} of the parity bound")


def test_the_order_is_a_function_of_the_row_alone():
    """A row of L <= G entries in a group of G < 64 lanes (the levels m = G/2 .. 1 only) has the full butterfly's bits."""
    rng = np.random.Generator(np.random.PCG64(3))
    for L in (1, 2, 3, 5, 8, 13, 31, 32):
        G = 1
        while G < L:
            G *= 2
        x = np.zeros(G, np.float32)
        x[:L] = rng.random(L).astype(np.float32)
        q, lane, m = x.copy(), np.arange(G), G // 2
        while m:
            q = q + q[lane ^ m]
            m //= 2
        assert q[0].tobytes() == SM.ordered_sum(x[:L]).tobytes(), L
