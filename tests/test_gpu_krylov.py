"""GPU (-m gpu): solvers.pcg and solvers.bicgstab with the ILU(0) factor of CsrMatrix.ilu0 as their preconditioner.

Both systems have 4096 rows and 46 levels; b is standard normal (seed 2026), tol = 1e-5, x starts at 0.
  system 1 (PCG)       stencil7(16)'s pattern with 6 on the diagonal and -1 off it: symmetric positive definite
  system 2 (BiCGStab)  the library's row-scaled stencil7(16), not symmetric

The margins.  The float32 numpy twins (tests/test_ilu0_host.py, which asserts the same three properties on the host) took 45
iterations of CG and 15 of PCG on system 1, with true relative residuals of 8.4e-6 and 6.6e-6: the same counts as the probe the
margins were first derived from (45 and 15; 9.0e-6 and 6.3e-6), so they stand as derived.  PCG with ILU(0) takes at most HALF
the plain iterations: the twins measured a third, the margin is for torch's different dot-product order.  The float64 true
residual computed on the host is at most 2 tol: the recurrence residual the solvers stop on drifts from the true one by
rounding only.  On system 2 the twin took 35 iterations of BiCGStab without and 10 with ILU(0) (5.9e-6 and 4.9e-6): the test
asserts no more iterations with M than without, and the same residual bound.

The iterates.  Convergence alone passes a wrong coefficient that still converges, so x after k = 1, 2 and 4 iterations from x = 0
(maxiter = k, a tol nothing meets) is compared with the numpy twin run in float64 on the 512-row versions of both systems, with
and without M (the factor of _ilu0.factor in both).  The bound is 8 max(d(k), k 2^-23) with d(k) the FLOAT32 twin's deviation
from the float64 twin (max norm, relative to x), computed again here and never taken from the solver; the factor 8 is for torch's
order of the dot products.  tests/test_ilu0_host.py measured d(k) and shows that 1 / beta for beta and p updated with the
opposite sign leave the bound by k = 4 (deviations of 3.4e-4 .. 0.69 against bounds below 4e-6):
    pcg       without M  d = 7.4e-8, 1.6e-7, 7.7e-8     with M  d = 7.9e-8, 1.2e-7, 1.4e-7
    bicgstab  without M  d = 8.7e-8, 7.8e-8, 7.8e-8     with M  d = 1.7e-7, 1.5e-7, 1.2e-7
On an MI355X the solvers deviated by 6.6e-8 .. 1.7e-7 (each case prints d(k), the device's deviation and the bound).
solvers.multicolor(A).solve gets the same check through the permutation: the iterate it brings back against the twin run on
_color.permute's matrix and un-permuted on the host.
"""
import numpy as np
import pytest

import _color
import _ilu0 as G

f32, f64 = np.float32, np.float64
TOL = 1e-5


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _run(pkg, gpu, solver, system):
    """(iterations, converged, true residual) without and with M, from x = 0."""
    import torch
    n, rp, ci, va = system
    A = pkg.capi.CsrMatrix.from_host(n, n, rp, ci, va)
    M = A.ilu0()
    assert M.ilu0_pivot() == -1 and M.trsv_plan_info("lower")["levels"] == 46
    b = G.krylov_rhs(n)
    d_b = _dev(gpu, b)
    out = []
    for m in (None, M):
        x = torch.zeros(n, device=gpu)
        res = solver(A, d_b, x, M=m, tol=TOL, maxiter=500)
        torch.cuda.synchronize()
        assert res.state.A is A and res.state.M is m
        out.append((res.iterations, res.converged, G.true_residual(rp, ci, va, b, x.cpu().numpy())))
    M.close()
    A.close()
    return out


@pytest.mark.gpu
def test_pcg_with_ilu0_halves_the_iterations(pkg, gpu):
    (it0, ok0, res0), (it1, ok1, res1) = _run(pkg, gpu, pkg.solvers.pcg, G.symmetric_stencil(pkg))
    print(f"pcg: plain {it0} iterations, true residual {res0:.2e}; with ILU(0) {it1}, {res1:.2e}")
    assert ok0 and ok1
    assert 2 * it1 <= it0, (it0, it1)
    assert res0 <= 2 * TOL and res1 <= 2 * TOL, (res0, res1)


@pytest.mark.gpu
def test_bicgstab_with_ilu0_takes_no_more_iterations(pkg, gpu):
    (it0, ok0, res0), (it1, ok1, res1) = _run(pkg, gpu, pkg.solvers.bicgstab, G.stencil_case(pkg, 16))
    print(f"bicgstab: plain {it0} iterations, true residual {res0:.2e}; with ILU(0) {it1}, {res1:.2e}")
    assert ok0 and ok1
    assert it1 <= it0, (it0, it1)
    assert res0 <= 2 * TOL and res1 <= 2 * TOL, (res0, res1)


def _check_iterates(what, got, ref, f32_twin):
    """got, ref, f32_twin: {k: x}.  Prints d(k) beside the device's deviation and asserts the bound."""
    for k in G.KRYLOV_KS:
        d, dev = G.deviation(f32_twin[k], ref[k]), G.deviation(got[k], ref[k])
        print(f"{what} k={k}: d(k) = {d:.2e}, the device's deviation {dev:.2e}, the bound {G.krylov_bound(d, k):.2e}")
        assert np.all(np.isfinite(got[k])) and dev <= G.krylov_bound(d, k), f"{what} k={k}: {dev:.3g} against {G.krylov_bound(d, k):.3g}"


@pytest.mark.gpu
@pytest.mark.parametrize("with_m", (False, True))
@pytest.mark.parametrize("kind", ("pcg", "bicgstab"))
def test_the_iterates_are_the_float64_twins(pkg, oracle, gpu, kind, with_m):
    import torch
    system, twin = G.krylov_systems(pkg)[kind]
    n, rp, ci, va = system
    b = G.krylov_rhs(n)
    ref = G.twin_iterates(twin, system, b, with_m, f64)
    f32_twin = G.twin_iterates(twin, system, b, with_m, f32, spmv32=oracle.spmv)
    A = pkg.capi.CsrMatrix.from_host(n, n, rp, ci, va)
    M = A.ilu0() if with_m else None
    d_b = _dev(gpu, b)
    got = {}
    for k in G.KRYLOV_KS:
        x = torch.zeros(n, device=gpu)
        res = getattr(pkg.solvers, kind)(A, d_b, x, M=M, tol=G.NEVER, maxiter=k)
        torch.cuda.synchronize()
        assert res.iterations == k and not res.converged
        got[k] = x.cpu().numpy()
    _check_iterates(f"{kind} {'with' if with_m else 'without'} M", got, ref, f32_twin)
    if M is not None:
        M.close()
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("pcg", "bicgstab"))
def test_the_iterates_through_the_multicolour_ordering(pkg, oracle, gpu, kind):
    """Reordering.solve: P b and P x forward, the solver on P A P^T with its ILU(0), x brought back by backward.  The twin runs
    on _color.permute's matrix with b[perm], and its x goes back by x[perm[r]] = x_B[r]."""
    import torch
    (n, rp, ci, va), twin = G.krylov_systems(pkg)[kind]
    b = G.krylov_rhs(n)
    perm = _color.color(rp, ci)[1]
    brp, bci, bva, _ = _color.permute(rp, ci, va, perm, perm)
    system = (n, brp, bci, bva)

    def back(xs):
        out = {}
        for k, xb in xs.items():
            out[k] = np.empty_like(xb)
            out[k][perm] = xb
        return out

    ref = back(G.twin_iterates(twin, system, b[perm], True, f64))
    f32_twin = back(G.twin_iterates(twin, system, b[perm], True, f32, spmv32=oracle.spmv))
    A = pkg.capi.CsrMatrix.from_host(n, n, rp, ci, va)
    R = pkg.solvers.multicolor(A)
    assert np.array_equal(R.perm.cpu().numpy(), perm)
    M = R.matrix.ilu0()
    d_b = _dev(gpu, b)
    got = {}
    for k in G.KRYLOV_KS:
        x = torch.zeros(n, device=gpu)
        res = R.solve(getattr(pkg.solvers, kind), d_b, x, M=M, tol=G.NEVER, maxiter=k)
        torch.cuda.synchronize()
        assert res.iterations == k and not res.converged
        got[k] = x.cpu().numpy()
    _check_iterates(f"{kind} through the multicolour ordering", got, ref, f32_twin)
    M.close()
    R.close()
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("pcg", "bicgstab"))
def test_a_breakdown_stops_without_an_exception(pkg, gpu, kind):
    import torch
    solver = getattr(pkg.solvers, kind)
    Z = pkg.capi.CsrMatrix.from_host(4, 4, np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32), np.zeros(4, f32))
    b, x = _dev(gpu, np.array([1.0, -2.0, 0.5, 3.0], f32)), torch.zeros(4, device=gpu)
    res = solver(Z, b, x)
    torch.cuda.synchronize()
    assert res.converged is False and res.iterations <= 1
    assert torch.all(x == 0), "x takes no step from a breakdown"
    # b = 0 is solved by x = 0 at once
    res = solver(Z, torch.zeros(4, device=gpu), x, state=res.state)
    assert res.converged is True and res.iterations == 0
    Z.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("pcg", "bicgstab"))
def test_the_state_passed_back_plans_and_allocates_nothing_again(pkg, gpu, kind):
    import torch
    solver = getattr(pkg.solvers, kind)
    n, rp, ci, va = G.symmetric_stencil(pkg, 8)
    A = pkg.capi.CsrMatrix.from_host(n, n, rp, ci, va)
    M = A.ilu0()
    b = _dev(gpu, G.krylov_rhs(n, 7))
    x = torch.zeros(n, device=gpu)
    first = solver(A, b, x, M=M, tol=1e-3)
    assert first.converged and first.state.plans == 1
    torch.cuda.synchronize()
    held, vec = torch.cuda.memory_allocated(), [v.data_ptr() for v in first.state.vec]
    again = solver(A, b, x, M=M, tol=TOL, state=first.state)      # goes on from the x it has
    torch.cuda.synchronize()
    assert again.state is first.state and again.state.plans == 1 and again.converged
    assert [v.data_ptr() for v in again.state.vec] == vec and torch.cuda.memory_allocated() == held
    assert G.true_residual(rp, ci, va, b.cpu().numpy(), x.cpu().numpy()) <= 2 * TOL
    with pytest.raises(ValueError, match="state was made for another matrix or another preconditioner"):
        solver(A, b, x, M=None, state=first.state)
    M.close()
    A.close()
