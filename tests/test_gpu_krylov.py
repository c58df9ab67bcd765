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
"""
import numpy as np
import pytest

import _ilu0 as G

f32 = np.float32
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
