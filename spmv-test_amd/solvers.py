"""Stationary iterations on a CSR handle: the downstream user of ``CsrMatrix.trsv``.

``gauss_seidel`` runs on A's own handle: the triangular solve reads the triangle it is asked for and never the other one, so
neither D + L nor D + U is ever formed.  Every step is a library launch or a torch elementwise kernel on the current stream.
"""
from __future__ import annotations

from . import capi

__all__ = ["GaussSeidel", "gauss_seidel"]


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
