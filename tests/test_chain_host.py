"""CPU: the carriers and programs of tests/_chain.py, before tests/test_gpu_chain.py relies on them.

  carriers     every carrier pushed through its builder's numpy model returns `out` with the values bit for bit, on every
               (builder, structure) pair the GPU tests use, with the integer and the subnormal data of _exact.Exact
  exactness    Exact.int_sums asserts sum |k m| <= EXACT_LIMIT per row for the SpMV data and for every SpMM column; the SDDMM
               data states its own bound: a GPU session never meets an inexact expectation
  programs     every program evaluates on the host; the patterns of (A + B) C and A C + B C agree, and so do (A B)^T and
               B^T A^T; the empty results are empty; the oversized row is oversized
  wrong        a carrier with a decoy kept, or with the two sides' values exchanged, is told apart by the comparison
"""
import numpy as np
import pytest

import _chain as H
import _exact as E
import _spgemm


@pytest.mark.parametrize("kind,name", H.CASES)
def test_the_carrier_reproduces_the_target(pkg, oracle, kind, name):
    c = H.carrier(kind, name, pkg, oracle)
    st = E.structure(name, pkg, oracle)
    assert (c.out.rows, c.out.cols) == (st.rows, st.cols)
    if kind in ("threshold", "topk"):
        assert c.out is st and (c._n_decoys > 0 or st.nnz == 0 and kind == "topk"), "no decoys"
    else:
        assert c.base.nnz <= st.nnz and not np.any((np.diff(c.out.ci) <= 0) & (c.out.row_of[1:] == c.out.row_of[:-1]))
    if kind == "sum-grown":
        assert c.out.nnz > c.base.nnz or c.base.nnz == st.rows * st.cols
    _, problems = H.exact_problems(c, f"{name}/{kind}")        # (expected() asserts the exactness condition)
    for label, vals, _, _ in problems:
        got = c.result(vals)
        bad = H.same(got[2], (c.out.rp, c.out.ci, c.out_vals(vals)))
        assert got[:2] == (st.rows, st.cols) and bad is None, f"{kind}/{name}/{label}: {bad}"
        assert not np.isnan(got[2][2]).any()


def test_product_carriers_land_in_every_class(pkg, oracle):
    """The terms of a row of the product carrier are the target row's entries: the structures reach every class of
    SPMV_SPGEMM_CLASS_SLOTS (64, 512, 4096, 32768) and none needs the oversized route."""
    slots = (64, 512, 4096, 32768)
    seen = set()
    for name in H.STRUCTURES:
        lengths = np.diff(E.structure(name, pkg, oracle).rp)
        assert lengths.max(initial=0) <= slots[-1]
        seen |= set(np.searchsorted(slots, lengths[lengths > 0], side="left").tolist())
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("name", sorted(set(H.SPMM_ON)))
@pytest.mark.parametrize("kind", H.KINDS)
def test_spmm_data_is_exact(pkg, oracle, kind, name):
    ex, _ = H.exact_problems(H.carrier(kind, name, pkg, oracle), f"{name}/{kind}/spmm")
    for k in H.SPMM_K + H.SPMM_COLS_K:
        M, want = H.spmm_problem(ex, k, 5)                       # int_sums asserts the condition column by column
        assert want.shape == (ex.s.rows, k) and np.abs(M).max() <= 4


@pytest.mark.parametrize("name", H.SDDMM_ON)
def test_sddmm_data_is_exact(pkg, oracle, name):
    s = E.structure(name, pkg, oracle)
    for k in H.SDDMM_K:
        U, X, want = H.sddmm_problem(s, k, 7)
        assert np.abs(U).max() <= 4 and np.abs(X).max() <= 4 and 16 * k <= E.EXACT_LIMIT
        assert np.array_equal(want.astype(np.int64), np.einsum("nk,nk->n", U[s.row_of], X[s.ci]))


@pytest.mark.parametrize("name", H.PROGRAMS)
def test_every_program_evaluates_on_the_host(name):
    p = H.programs()[name]
    env = p.host
    for step, _, _, _ in p.steps:
        m, n, (rp, ci, va) = env[step]
        assert len(rp) == m + 1 and rp[0] == 0 and rp[-1] == len(ci) == len(va), step
        assert ci.size == 0 or (ci.min() >= 0 and ci.max() < n), step
    for a, b in p.equal_patterns:
        assert env[a][:2] == env[b][:2] and H.same_pattern(env[a][2], env[b][2]), f"{name}: the patterns of {a} and {b} differ"
        assert len(env[a][2][1]) > 1000
    for z in p.empty:
        assert len(env[z][2][1]) == 0, f"{name}: {z} is not empty"
    if not p.empty:
        assert all(len(env[s[0]][2][1]) > 0 for s in p.steps), f"{name}: a step came out empty"


def test_the_program_list_is_the_fixed_one():
    assert tuple(H.programs()) == H.PROGRAMS
    p = H.programs()["oversized_then_selected"]
    row = _spgemm.terms(p.leaves["A"][2], p.leaves["B"][2])[0]
    assert np.bincount(row).max() > 32768, "no row takes the oversized route"
    small = H.programs()["aat_topk"]
    assert np.bincount(_spgemm.terms(small.leaves["A"][2], small.host["T"][2])[0]).max() <= 32768
    a = H.programs()["a_plus_at"].leaves["A"]
    s = E.Structure(a[0], a[1], a[2][0], a[2][1])
    same_row = s.row_of[1:] == s.row_of[:-1]
    step = np.diff(s.ci.astype(np.int64))[same_row]
    assert s.rows == s.cols and np.diff(s.rp).max() == H.LONG_ROW and (step < 0).any() and (step == 0).any(), "unsorted, with repeats"
    assert np.isnan(a[2][2]).any() and np.isinf(a[2][2]).any()


@pytest.mark.parametrize("kind,wrong", [("threshold", "decoy_kept"), ("topk", "decoy_kept"), ("sum", "swapped_split")])
def test_a_wrong_carrier_is_told_apart(pkg, oracle, kind, wrong):
    st = E.structure("lengths_around_short_threshold", pkg, oracle)
    right, bad = H.Carrier(kind, st, "wrong"), H.Carrier(kind, st, "wrong", wrong=wrong)
    ex, problems = H.exact_problems(right, "wrong")
    vals = problems[0][1]
    want = (right.out.rp, right.out.ci, right.out_vals(vals))
    assert H.same(right.result(vals)[2], want) is None
    assert H.same(bad.result(vals)[2], want) is not None
    if wrong == "decoy_kept":                                          # and the decoy poisons its row's sum
        m, n, (rp, ci, va) = bad.result(vals)
        y = np.add.reduceat(np.concatenate([va * ex.x()[ci], [0]]), np.minimum(rp[:-1], len(va)))[:m]
        assert np.isnan(y[np.diff(rp) > 0]).sum() == 1
