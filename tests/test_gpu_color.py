"""spmv_csr_color on the device against the numpy contract of tests/_color.py, bit for bit (include/spmv_hip.h "the multicolour
ordering"), and the solver layer on top of it.

  1. color, perm, color_ptr and info[0], [1], [3], [4] equal the contract under two seeds on every shared pattern: long rows fed by
     short ones (the wavefront path), a fan, an arrow, a stencil, a 70-clique (the window of 64 colours slides), a star of 5000
     leaves, rows of exactly 31, 32 and 33 neighbour entries, a strictly upper-triangular pattern, unsorted rows with repeats, a
     diagonal matrix, nnz = 0, rows = 0 and rows = 1;
  2. the same bytes from borrowed and owned arrays, on two streams at once, from two calls; a short color_ptr fills exactly cap;
  3. every refusal leaves the outputs poisoned and the free memory where it was;
  4. end to end: solvers.multicolor, ILU(0) of P A P^T in at most `colors` levels with the contract's bits, PCG and BiCGStab through
     R.solve in at most 2/3 of the plain iterations, a second solve without allocation, refresh after a rewrite.
"""
import ctypes as C

import numpy as np
import pytest

import _color as K
import _ilu0 as G
import _trsv as T

MIB = 1 << 20
f32, f64 = np.float32, np.float64
CASES = ("generic", "stairs", "tridiagonal", "fan", "arrow", "stencil8", "clique70", "star5000", "boundary", "upper", "unsorted",
         "diagonal", "empty", "rows0", "rows1")


def _dev(gpu, a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(gpu)


def _handle(capi, n, rp, ci, va=None):
    return capi.CsrMatrix.from_host(n, n, rp, ci, np.ones(len(ci), f32) if va is None else va)


_want_cache = {}


def _want(pkg, key, seed):
    """The contract's colouring of a shared case, computed once."""
    if (key, seed) not in _want_cache:
        n, rp, ci = K.color_cases(pkg)[key]
        _want_cache[key, seed] = K.color(rp, ci, seed)
    return _want_cache[key, seed]


def _equal(got, want, what):
    color, perm, cp, info = got
    wcolor, wperm, wcp, winfo = want
    assert np.array_equal(color.cpu().numpy(), wcolor), f"{what}: color"
    assert np.array_equal(perm.cpu().numpy(), wperm), f"{what}: perm"
    assert cp.dtype == np.int32 and np.array_equal(cp, wcp), f"{what}: color_ptr"
    assert {k: info[k] for k in winfo} == winfo, f"{what}: {info}"


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", K.SEEDS)
@pytest.mark.parametrize("key", CASES)
def test_color_equals_the_contract_bit_for_bit(pkg, gpu, key, seed):
    n, rp, ci = K.color_cases(pkg)[key]
    A = _handle(pkg.capi, n, rp, ci)
    got = A.color(seed)
    _equal(got, _want(pkg, key, seed), f"{key} seed {seed:#x}")
    info = got[3]
    assert info["sweep_entries"] == (2 * ci.size if n else 0) and info["peak_bytes"] >= 12 * n
    if n:
        assert 1 <= info["launches"] <= info["rounds"], "a launch runs one round or, in one workgroup, several"
        assert K.is_proper(rp, ci, got[0].cpu().numpy())
    A.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_purity_owners_streams_calls_and_a_short_color_ptr(pkg, gpu):
    import torch
    capi = pkg.capi
    n, rp, ci = K.color_cases(pkg)["generic"]
    want = _want(pkg, "generic", 0)
    owned = _handle(capi, n, rp, ci)
    t = (_dev(gpu, rp, np.int32), _dev(gpu, ci, np.int32), torch.full((ci.size,), float("nan"), device=gpu))   # values are never read
    borrowed = capi.CsrMatrix.from_device(n, n, *t)
    _equal(owned.color(0), want, "owned")
    _equal(borrowed.color(0), want, "borrowed")
    _equal(owned.color(0), want, "a second call")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = owned.color(0, stream=s1)
    with torch.cuda.stream(s2):
        b = borrowed.color(K.SEEDS[1], stream=s2)
    torch.cuda.synchronize()
    _equal(a, want, "stream 1")
    _equal(b, _want(pkg, "generic", K.SEEDS[1]), "stream 2")
    # cap below colours + 1: exactly cap entries are filled; no perm and no color_ptr at all
    lib = capi.lib()
    color = torch.full((n,), -7, dtype=torch.int32, device=gpu)
    cp = np.full(8, -9, np.int32)
    info = (C.c_int64 * 8)()
    st = torch.cuda.current_stream().cuda_stream
    capi.check(lib.spmv_csr_color(owned._h, 0, st, color.data_ptr(), None, cp.ctypes.data, 5, info))
    assert info[0] == 14 and np.array_equal(cp[:5], want[2][:5]) and np.all(cp[5:] == -9)
    assert np.array_equal(color.cpu().numpy(), want[0])
    capi.check(lib.spmv_csr_color(owned._h, 0, st, color.data_ptr(), None, None, 0, None))
    assert np.array_equal(color.cpu().numpy(), want[0])
    owned.close()
    borrowed.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing_and_leave_the_outputs_poisoned(pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    n, rp, ci = K.color_cases(pkg)["generic"]
    A = _handle(capi, n, rp, ci)
    wide = capi.CsrMatrix.from_host(4, 5, np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros(0, f32))
    color = torch.full((n,), -7, dtype=torch.int32, device=gpu)
    perm = torch.full((n,), -8, dtype=torch.int32, device=gpu)
    cp = np.full(32, -9, np.int32)
    st = torch.cuda.current_stream().cuda_stream

    def refused(rc, start):
        assert rc == capi.ERR_INVALID, start
        msg = lib.spmv_last_error().decode()
        assert msg.startswith(start), msg

    free = []
    for _ in range(3):
        info = (C.c_int64 * 8)(*([5] * 8))
        args = (color.data_ptr(), perm.data_ptr(), cp.ctypes.data)
        refused(lib.spmv_csr_color(None, 0, st, *args, 32, info), "spmv_csr_color: null handle")
        refused(lib.spmv_csr_color(A._h, 0, st, None, perm.data_ptr(), cp.ctypes.data, 32, info), "spmv_csr_color: null d_color")
        refused(lib.spmv_csr_color(wide._h, 0, st, *args, 32, info), "spmv_csr_color: the handle is 4 x 5")
        refused(lib.spmv_csr_color(A._h, 0, st, *args, -1, info), "spmv_csr_color: cap = -1")
        refused(lib.spmv_csr_color(A._h, 0, st, *args, 0, info), "spmv_csr_color: color_ptr with cap = 0")
        if torch.cuda.device_count() > 1:                    # another current device than the handle's
            with torch.cuda.device(1):
                refused(lib.spmv_csr_color(A._h, 0, None, *args, 32, info), "spmv_csr_color")
        assert list(info) == [5] * 8
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert torch.all(color == -7) and torch.all(perm == -8) and np.all(cp == -9), "the outputs stay poisoned"
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    # colourings made again and again leave nothing behind
    held = torch.cuda.memory_allocated()
    free = []
    for _ in range(3):
        A.color(3)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    assert torch.cuda.memory_allocated() == held
    A.close()
    wide.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def _systems(pkg):
    return {"pcg": (G.symmetric_stencil(pkg), pkg.solvers.pcg), "bicgstab": (G.stencil_case(pkg, 16), pkg.solvers.bicgstab)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("pcg", "bicgstab"))
def test_multicolor_ilu0_end_to_end(pkg, gpu, kind):
    import torch
    capi, solvers = pkg.capi, pkg.solvers
    (n, rp, ci, va), solver = _systems(pkg)[kind]
    A = capi.CsrMatrix.from_host(n, n, rp, ci, va)
    R = solvers.multicolor(A)
    col, perm, cp, info = K.color(rp, ci, 0)
    assert np.array_equal(R.perm.cpu().numpy(), perm) and np.array_equal(R.color.cpu().numpy(), col) and np.array_equal(R.color_ptr, cp)
    assert R.colors == info["colors"] <= 7
    brp, bci, bva, _ = K.permute(rp, ci, va, perm, perm)
    got = R.matrix.download()
    assert np.array_equal(got[0], brp) and np.array_equal(got[1], bci) and T.same(got[2], bva) is None
    M = R.matrix.ilu0()
    assert M.trsv_plan_info("lower")["levels"] <= R.colors and M.trsv_plan_info("upper")["levels"] <= R.colors
    torch.cuda.synchronize()
    assert G.same(M.download()[2], G.factor(brp, bci, bva)) is None, "the factor of P A P^T, bit for bit"
    # the vectors: P v and back
    v = _dev(gpu, G.krylov_rhs(n, 5))
    fwd = R.forward(v)
    assert T.same(fwd.cpu().numpy(), v.cpu().numpy()[perm]) is None
    assert T.same(R.backward(fwd).cpu().numpy(), v.cpu().numpy()) is None
    # the solves
    tol = 1e-5
    b = G.krylov_rhs(n)
    d_b = _dev(gpu, b)
    x0 = torch.zeros(n, device=gpu)
    plain = solver(A, d_b, x0, tol=tol, maxiter=500)
    x1 = torch.zeros(n, device=gpu)
    res = R.solve(solver, d_b, x1, M=M, tol=tol, maxiter=500)
    r0, r1 = G.true_residual(rp, ci, va, b, x0.cpu().numpy()), G.true_residual(rp, ci, va, b, x1.cpu().numpy())
    print(f"{kind}: plain {plain.iterations} iterations, true residual {r0:.2e}; multicolour ILU(0) {res.iterations}, {r1:.2e}; "
          f"{R.colors} colours, levels {M.trsv_plan_info('lower')['levels']} / {M.trsv_plan_info('upper')['levels']}")
    assert plain.converged and res.converged
    assert 3 * res.iterations <= 2 * plain.iterations
    assert r0 <= 2 * tol and r1 <= 2 * tol
    # a second solve allocates nothing
    x1.zero_()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    again = R.solve(solver, d_b, x1, M=M, tol=tol, maxiter=500)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held
    assert again.iterations == res.iterations and G.true_residual(rp, ci, va, b, x1.cpu().numpy()) <= 2 * tol
    with pytest.raises(ValueError, match="refresh needs keep_map=True"):
        R.refresh(A)
    M.close()
    R.close()
    A.close()


@pytest.mark.gpu
def test_refresh_after_a_rewrite_gives_the_bits_of_a_fresh_build(pkg, gpu):
    import torch
    capi, solvers = pkg.capi, pkg.solvers
    n, rp, ci, va = G.generic_case()
    t = (_dev(gpu, rp, np.int32), _dev(gpu, ci, np.int32), _dev(gpu, va, f32))
    A = capi.CsrMatrix.from_device(n, n, *t)
    R = solvers.multicolor(A, keep_map=True)
    M = R.matrix.ilu0()
    perm = K.color(rp, ci, 0)[1]
    rng = np.random.default_rng(19)
    row = np.repeat(np.arange(n), np.diff(rp))
    nv = np.where(ci == row, va * f32(1.5), va * rng.uniform(0.2, 1.0, va.size).astype(f32)).astype(f32)
    t[2].copy_(_dev(gpu, nv))
    R.refresh(A)
    M.ilu0_values(R.matrix)
    torch.cuda.synchronize()
    brp, bci, bva, _ = K.permute(rp, ci, nv, perm, perm)
    assert T.same(R.matrix.download()[2], bva) is None
    assert G.same(M.download()[2], G.factor(brp, bci, bva)) is None
    fresh = solvers.multicolor(A)
    Mf = fresh.matrix.ilu0()
    torch.cuda.synchronize()
    assert G.same(M.download()[2], Mf.download()[2]) is None
    assert R.matrix.permute_map_bytes() == 4 * ci.size and fresh.matrix.permute_map_bytes() == 0
    for h in (M, Mf):
        h.close()
    R.close()
    fresh.close()
    A.close()
