"""Stationary and Krylov iterations on a CSR handle: the downstream users of ``CsrMatrix.trsv`` and ``CsrMatrix.ilu0``.

``multicolor`` reorders a matrix by a colouring of its graph, so that its ILU(0) factor has no more levels than colours.
``gauss_seidel`` runs on A's own handle: the triangular solve reads the triangle it is asked for and never the other one, so
neither D + L nor D + U is ever formed.  ``pcg`` and ``bicgstab`` take an ILU(0) factor handle as their preconditioner and apply
it with ``ilu0_solve``.  Every step is a library launch or a torch elementwise kernel or dot product on the current stream.
"""
from __future__ import annotations

from . import capi

__all__ = ["GaussSeidel", "gauss_seidel", "Krylov", "KrylovResult", "pcg", "bicgstab", "Reordering", "multicolor"]


class GaussSeidel:
    """The plans and the two work vectors of Gauss-Seidel sweeps on one matrix: made once, reused by every sweep."""

    def __init__(self, A: "capi.CsrMatrix", symmetric: bool = False):
        if not isinstance(A, capi.CsrMatrix):
            raise TypeError("gauss_seidel: A must be a CsrMatrix")
        if A.rows != A.cols:
            raise ValueError(f"gauss_seidel: A is {A.rows} x {A.cols} (a square matrix is needed)")
        self.A, self.symmetric = A, bool(symmetric)
        A.plan(capi.SCALAR)
        A.trsv_plan("lower")
        if self.symmetric:
            A.trsv_plan("upper")
        self._r = self._d = None

    def sweep(self, b, x) -> None:
        """One sweep in place: x <- x + (D + L)^-1 (b - A x), and, symmetric, then x <- x + (D + U)^-1 (b - A x)."""
        import torch
        A = self.A
        for name, t in (("b", b), ("x", x)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != A.rows:
                raise ValueError(f"gauss_seidel: {name} must be a contiguous 1-D float32 tensor of {A.rows} elements")
        if self._r is None or self._r.device != x.device:
            self._r, self._d = torch.empty_like(x), torch.empty_like(x)
        for uplo in ("lower", "upper") if self.symmetric else ("lower",):
            A.run(capi.SCALAR, x, self._r)                 # r = A x
            torch.sub(b, self._r, out=self._r)             # r = b - A x
            A.trsv(self._r, self._d, uplo=uplo)            # d = (D + L)^-1 r
            x.add_(self._d)


def gauss_seidel(A, b, x, sweeps: int = 1, symmetric: bool = False, state: GaussSeidel | None = None) -> GaussSeidel:
    """``sweeps`` Gauss-Seidel sweeps on ``A x = b``, x updated in place.  A forward sweep is x <- x + (D + L)^-1 (b - A x) with
    SPMV_SCALAR for A x and ``trsv`` lower on A's own handle; ``symmetric=True`` adds the backward sweep with ``trsv`` upper
    (symmetric Gauss-Seidel).  The plans are made once and nothing is allocated per sweep after the first; the returned state
    can be passed back as ``state=`` to go on sweeping without planning again."""
    if isinstance(sweeps, bool) or not isinstance(sweeps, int) or sweeps < 0:
        raise ValueError(f"gauss_seidel: sweeps = {sweeps!r}")
    gs = state if state is not None else GaussSeidel(A, symmetric)
    if gs.A is not A or gs.symmetric != bool(symmetric):
        raise ValueError("gauss_seidel: state was made for another matrix or another kind of sweep")
    for _ in range(sweeps):
        gs.sweep(b, x)
    return gs


# ---- Krylov iterations: the downstream user of ``CsrMatrix.ilu0`` -----------------------------------------------------------------
def _bad(v: float) -> bool:
    """A rho or a denominator that ends the iteration: 0 or not finite."""
    return v == 0.0 or v != v or v in (float("inf"), float("-inf"))


class KrylovResult(tuple):
    """``(iterations, converged, state)``; ``state`` goes back in as ``state=`` to solve again without planning or allocating."""
    __slots__ = ()
    iterations = property(lambda self: self[0])
    converged = property(lambda self: self[1])
    state = property(lambda self: self[2])


class Krylov:
    """The plan of A and the work vectors of :func:`pcg` or :func:`bicgstab` on one matrix: made once, reused by every solve."""

    def __init__(self, what: str, A: "capi.CsrMatrix", M, b, nvec: int):
        import torch
        if not isinstance(A, capi.CsrMatrix):
            raise TypeError(f"{what}: A must be a CsrMatrix")
        if A.rows != A.cols:
            raise ValueError(f"{what}: A is {A.rows} x {A.cols} (a square matrix is needed)")
        if M is not None and (not isinstance(M, capi.CsrMatrix) or (M.rows, M.cols) != (A.rows, A.cols)):
            raise ValueError(f"{what}: M must be None or a factor handle of A's shape (A.ilu0())")
        self.what, self.A, self.M = what, A, M
        A.plan(capi.SCALAR)
        self.plans = 1                                     # how often this state planned (a state passed back in plans nothing again)
        self.vec = [torch.empty_like(b) for _ in range(nvec)]
        self.scal = torch.zeros(8, dtype=torch.float32, device=b.device)      # the dot products of one iteration, read in one copy

    def check(self, A, M, b, x):
        import torch
        if self.A is not A or self.M is not M:
            raise ValueError(f"{self.what}: state was made for another matrix or another preconditioner")
        for name, t in (("b", b), ("x", x)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != A.rows:
                raise ValueError(f"{self.what}: {name} must be a contiguous 1-D float32 tensor of {A.rows} elements")
        if b.device != self.scal.device:
            raise ValueError(f"{self.what}: state was made on another device")

    def apply(self, r, z):
        """z = M^-1 r (without M: a copy)."""
        if self.M is None:
            z.copy_(r)
        else:
            self.M.ilu0_solve(r, z)


def _krylov_args(what, tol, maxiter, rows):
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not tol > 0:
        raise ValueError(f"{what}: tol = {tol!r}")
    if maxiter is None:
        maxiter = max(2 * rows, 1)
    if isinstance(maxiter, bool) or not isinstance(maxiter, int) or maxiter < 0:
        raise ValueError(f"{what}: maxiter = {maxiter!r}")
    return float(tol), maxiter


def pcg(A, b, x, M=None, tol: float = 1e-5, maxiter=None, state: Krylov | None = None) -> KrylovResult:
    """Preconditioned conjugate gradients on ``A x = b`` (A symmetric positive definite), x updated in place from the x given.
    ``M``: a factor handle (``A.ilu0()``) applied through ``ilu0_solve``, or None.  ``A p`` is SPMV_SCALAR; vector updates and
    dot products are torch calls on the current stream.  Stops when the RECURRENCE residual has ``||r|| <= tol ||b||``: that
    costs one host read (of three dot products) per iteration.  A breakdown -- rho or p . A p is 0 or not finite -- stops with
    ``converged=False`` and no exception, before x takes the step.  Returns ``(iterations, converged, state)``."""
    import torch
    tol, maxiter = _krylov_args("pcg", tol, maxiter, getattr(A, "rows", 0))
    st = state if state is not None else Krylov("pcg", A, M, b, 4)
    st.check(A, M, b, x)
    r, z, p, q = st.vec
    sc = st.scal
    A.run(capi.SCALAR, x, r)
    torch.sub(b, r, out=r)                                 # r = b - A x
    st.apply(r, z)
    p.copy_(z)
    A.run(capi.SCALAR, p, q)
    torch.dot(r, r, out=sc[0]); torch.dot(r, z, out=sc[1]); torch.dot(p, q, out=sc[2]); torch.dot(b, b, out=sc[3])
    rr, rho, den, bb = sc[:4].tolist()
    it = 0
    while True:
        if rr <= (tol * tol) * bb and rr == rr:
            return KrylovResult((it, True, st))
        if it >= maxiter or _bad(rho) or _bad(den) or rr != rr:
            return KrylovResult((it, False, st))
        alpha = rho / den
        x.add_(p, alpha=alpha)
        r.add_(q, alpha=-alpha)
        it += 1
        st.apply(r, z)
        torch.dot(r, r, out=sc[0]); torch.dot(r, z, out=sc[1])
        torch.div(sc[1], rho, out=sc[4])                   # beta = rho_new / rho, on the device
        torch.addcmul(z, p, sc[4], out=p)                  # p = z + beta p
        A.run(capi.SCALAR, p, q)
        torch.dot(p, q, out=sc[2])
        rr, rho, den = sc[:3].tolist()                     # the one host read of the iteration


def bicgstab(A, b, x, M=None, tol: float = 1e-5, maxiter=None, state: Krylov | None = None) -> KrylovResult:
    """BiCGStab on ``A x = b`` (A square), preconditioned on the RIGHT by ``M`` (a factor handle, or None), x updated in place
    from the x given.  ``A y`` is SPMV_SCALAR, ``M^-1`` is ``ilu0_solve``; vector updates and dot products are torch calls on the
    current stream, and alpha, omega and beta stay on the device.  Stops when the RECURRENCE residual has ``||r|| <= tol ||b||``:
    one host read (of five dot products) per iteration.  A breakdown -- rho, rhat . v, t . t or omega is 0 or not finite --
    stops with ``converged=False`` and no exception; the step of such an iteration is taken with the bad coefficient set to 0,
    so x stays finite.  Returns ``(iterations, converged, state)``."""
    import torch
    tol, maxiter = _krylov_args("bicgstab", tol, maxiter, getattr(A, "rows", 0))
    st = state if state is not None else Krylov("bicgstab", A, M, b, 8)
    st.check(A, M, b, x)
    r, rhat, p, v, y, s, z, t = st.vec
    sc = st.scal
    A.run(capi.SCALAR, x, r)
    torch.sub(b, r, out=r)
    rhat.copy_(r)
    p.zero_(); v.zero_()
    torch.dot(r, r, out=sc[0]); torch.dot(b, b, out=sc[5])
    rr, bb = sc[0].item(), sc[5].item()
    sc[5:8] = 1.0                                          # rho, alpha, omega of the step before the first
    it = 0
    rho = den = tt = omega = 1.0
    zero = torch.zeros((), dtype=torch.float32, device=b.device)

    def guarded(num, d):                                   # num / d, or 0 where d is 0 or the quotient is not finite
        qv = num / d
        return torch.where(torch.isfinite(qv) & (d != 0), qv, zero)

    while True:
        if rr <= (tol * tol) * bb and rr == rr:
            return KrylovResult((it, True, st))
        if it >= maxiter or _bad(rho) or _bad(den) or _bad(tt) or _bad(omega) or rr != rr:
            return KrylovResult((it, False, st))
        it += 1
        torch.dot(rhat, r, out=sc[1])                      # rho_new
        beta = guarded(sc[1] * sc[6], sc[5] * sc[7])       # (rho_new / rho) (alpha / omega)
        p.sub_(v * sc[7])                                  # p = r + beta (p - omega v)
        torch.addcmul(r, p, beta, out=p)
        st.apply(p, y)
        A.run(capi.SCALAR, y, v)
        torch.dot(rhat, v, out=sc[2])
        sc[6] = guarded(sc[1], sc[2])                      # alpha
        torch.addcmul(r, v, -sc[6], out=s)                 # s = r - alpha v
        st.apply(s, z)
        A.run(capi.SCALAR, z, t)
        torch.dot(t, t, out=sc[3]); torch.dot(t, s, out=sc[4])
        sc[7] = guarded(sc[4], sc[3])                      # omega
        x.addcmul_(y, sc[6]).addcmul_(z, sc[7])            # x += alpha y + omega z
        torch.addcmul(s, t, -sc[7], out=r)                 # r = s - omega t
        torch.dot(r, r, out=sc[0])
        sc[5] = sc[1]
        rr, rho, den, tt, ts, _, _, omega = sc.tolist()    # the one host read of the iteration
        if rr == 0.0:                                      # (s vanished: t . t = 0 is no breakdown then)
            tt = omega = 1.0


# ---- the multicolour ordering: the downstream user of ``CsrMatrix.color`` and ``CsrMatrix.permute`` ----------------------------
class Reordering:
    """P A P^T by a colouring of A's graph (:func:`multicolor`): ``matrix`` (a handle of its own), ``perm`` (row r of ``matrix`` is
    row ``perm[r]`` of A), ``color``, ``color_ptr`` (numpy: where every colour starts in ``perm``) and ``colors``.  No stored entry
    joins two rows of a colour, so each triangle of ``matrix`` has at most ``colors`` levels."""

    def __init__(self, A: "capi.CsrMatrix", seed: int = 0, keep_map: bool = False):
        if not isinstance(A, capi.CsrMatrix):
            raise TypeError("multicolor: A must be a CsrMatrix")
        if A.rows != A.cols:
            raise ValueError(f"multicolor: A is {A.rows} x {A.cols} (a square matrix is needed)")
        self.color, self.perm, self.color_ptr, self.info = A.color(seed)
        self.colors = self.info["colors"]
        self.keep_map = bool(keep_map)
        self.matrix = A.permute(self.perm, self.perm, keep_map=self.keep_map)
        self._b = self._x = None
        self._states = {}

    def _vector(self, who, v, out):
        import torch
        if out is None and isinstance(v, torch.Tensor):
            out = torch.empty_like(v)
        for name, t in (("v", v), ("out", out)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != self.matrix.rows:
                raise ValueError(f"multicolor: {who}: {name} must be a contiguous 1-D float32 tensor of {self.matrix.rows} elements")
        return out

    def forward(self, v, out=None):
        """P v: ``out[r] = v[perm[r]]``, a vector of A's order brought into ``matrix``'s."""
        out = self._vector("forward", v, out)
        return capi.permute_vector(self.perm, v, out, inverse=False)

    def backward(self, v, out=None):
        """P^T v: ``out[perm[r]] = v[r]``, a vector of ``matrix``'s order brought back into A's."""
        out = self._vector("backward", v, out)
        return capi.permute_vector(self.perm, v, out, inverse=True)

    def solve(self, solver, b, x, M=None, **kw):
        """``solver(self.matrix, P b, P x, M=M, **kw)`` (:func:`pcg` or :func:`bicgstab`; ``M``: ``self.matrix.ilu0()`` or None), then x
        brought back in place.  The two work vectors and the solver's state are kept across calls.  Returns the solver's result."""
        import torch
        self._vector("solve", b, x)
        if self._b is None or self._b.device != b.device:
            self._b, self._x = torch.empty_like(b), torch.empty_like(b)
        self.forward(b, self._b)
        self.forward(x, self._x)
        key = (solver, id(M))
        if key in self._states and "state" not in kw:
            kw["state"] = self._states[key]
        res = solver(self.matrix, self._b, self._x, M=M, **kw)
        self._states = {key: res.state}
        self.backward(self._x, x)
        return res

    def refresh(self, A: "capi.CsrMatrix") -> None:
        """``matrix``'s values again from the values A holds now (``permute_values``); needs ``keep_map=True``."""
        if not self.keep_map:
            raise ValueError("multicolor: refresh needs keep_map=True")
        self.matrix.permute_values(A)

    def close(self) -> None:
        self._states = {}
        self._b = self._x = None
        if self.matrix is not None:
            self.matrix.close()
            self.matrix = None


def multicolor(A, seed: int = 0, keep_map: bool = False) -> Reordering:
    """Colour A's graph (``A.color(seed)``) and build P A P^T with the rows of one colour contiguous.  ``R.matrix.ilu0()`` then has at
    most ``R.colors`` levels in each triangle, and ``R.solve(pcg, b, x, M=M)`` solves the original system through it."""
    return Reordering(A, seed, keep_map)
