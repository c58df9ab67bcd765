"""CPU: the carriers and programs of tests/_chain.py, before tests/test_gpu_chain.py relies on them.

  carriers     every carrier pushed through its builder's numpy model returns `out` with the values bit for bit, on every
               (builder, structure) pair the GPU tests use, with the integer and the subnormal data of _exact.Exact
  exactness    Exact.int_sums asserts sum |k m| <= EXACT_LIMIT per row for the SpMV data and for every SpMM column; the SDDMM
               data states its own bound: a GPU session never meets an inexact expectation
  programs     every program evaluates on the host; the patterns of (A + B) C and A C + B C agree, and so do (A B)^T and
               B^T A^T; the empty results are empty; the oversized row is oversized
  wrong        a carrier with a decoy kept, or with the two sides' values exchanged, is told apart by the comparison
  new kinds    the permuted and the factor carriers likewise, with their own wrong variants (the inverse convention, an unstable
               order among repeats, a lower diagonal other than 1); permute(transpose(A)) and transpose(permute(A)) agree byte
               for byte, (P A Q^T)(Q B R^T) and P (A B) R^T in their patterns
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


def _rows_ascend(s, strictly):
    step = np.diff(s.ci.astype(np.int64))[s.row_of[1:] == s.row_of[:-1]]
    return bool(np.all(step > 0 if strictly else step >= 0))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("kind,name", H.NEW_CASES)
def test_a_permuted_or_factor_carrier_reproduces_its_out(pkg, oracle, kind, name):
    """The model of the carrier's builder returns `out` with the values strictly bit for bit, for the integer and the subnormal
    data; `out` is the target's rows sorted (permuted) or the mirrored square structure (factor)."""
    c = H.carrier(kind, name, pkg, oracle)
    st = E.structure(name, pkg, oracle)
    if kind in H.PERMUTED_KINDS:
        assert (c.out.rows, c.out.cols) == (st.rows, st.cols) and np.array_equal(c.out.rp, st.rp) and _rows_ascend(c.out, False)
        assert np.array_equal(np.sort(c.out.row_of * max(st.cols, 1) + c.out.ci), np.sort(st.row_of * max(st.cols, 1) + st.ci))
        (_, _, _, kw), = c.steps
        assert kw["via_transpose"] == (kind == "permuted-via-transpose")
        if st.rows > 100 and st.nnz > 100:                         # the parent is neither the target nor sorted
            assert not np.array_equal(c._p_rp, st.rp) or np.ptp(np.diff(st.rp)) == 0
            assert not _rows_ascend(E.Structure(st.rows, st.cols, c._p_rp, c._p_ci), False)
    else:
        n = max(st.rows, st.cols)
        assert (c.out.rows, c.out.cols) == (n, n) and _rows_ascend(c.out, True) and c._diag.size == n
        lower = c.out.ci <= c.out.row_of
        assert np.all(lower) if kind == "factor-lower" else np.all(c.out.ci >= c.out.row_of)
        if (kind, name) != ("factor-lower", "lengths_around_short_threshold"):     # (400 rows: mirrored down, its rows are short)
            assert (np.diff(c.out.rp) > 32).sum() > 0, "no row takes the wavefront path of the factor kernel"
    _, problems = H.exact_problems(c, f"{name}/{kind}")
    for label, vals, _, _ in problems:
        got = c.result(vals)
        want = (c.out.rp, c.out.ci, c.out_vals(vals))
        assert got[:2] == (c.out.rows, c.out.cols), f"{kind}/{name}/{label}"
        assert all(np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32)) for g, w in zip(got[2], want)), \
            f"{kind}/{name}/{label}: {H.same(got[2], want)}"
        if kind in H.FACTOR_KINDS:                                 # ILU(0) of such a matrix is the matrix
            assert np.array_equal(_bits(got[2][2]), _bits(c.leaves(vals)["A"][2][2]))
            if kind == "factor-lower":
                assert np.all(got[2][2][c._diag] == 1)


def test_the_mirrored_structures_hold_the_long_rows():
    """What DESIGN.md states of the factor kinds' structures: rows above SPMV_ILU0_SERIAL_MAX in every one of them."""
    import _ilu0
    for name in H.FACTOR_ON:
        for kind in H.FACTOR_KINDS:
            lengths = np.diff(H.carrier(kind, name).out.rp)
            print(f"{name} {kind}: {int((lengths > _ilu0.SERIAL_MAX).sum())} rows above SERIAL_MAX, the longest {int(lengths.max())}")
    upper = {name: np.diff(H.carrier("factor-upper", name).out.rp) for name in H.FACTOR_ON}
    assert (upper["lengths_around_short_threshold"] > _ilu0.SERIAL_MAX).sum() == 363
    assert upper["not_multiple_of_anything"].max() == 3458 and upper["long_row_between_short_rows"].max() == 20000


@pytest.mark.parametrize("form", ["plain", "shuffled"])
@pytest.mark.parametrize("name", ["lengths_around_short_threshold", "not_multiple_of_anything", "long_row_between_short_rows",
                                  "single_element", "all_rows_empty"])
def test_the_permuted_model_sorts_the_targets_rows(name, form):
    """_color.permute on the carrier's operands: the target's row_ptr and each row's columns sorted, repeats kept; with the
    target's own columns shuffled and repeated too."""
    st = E.structure(name)
    if form == "shuffled":
        st = E.shuffled(st, name)[0]
    c = H.Carrier("permuted", st, name + form)
    vals = np.arange(1, st.nnz + 1, dtype=np.float32)
    m, n, (rp, ci, va) = c.result(vals)
    assert (m, n) == (st.rows, st.cols) and np.array_equal(rp, st.rp)
    want_ci = st.ci[np.lexsort((st.ci, st.row_of))]
    assert np.array_equal(ci, want_ci) and np.array_equal(va, vals)
    if form == "shuffled" and st.nnz > 100:
        assert not _rows_ascend(c.out, True), "no repeats"


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


@pytest.mark.parametrize("kind,name", [c for c in H.consumer_cases(sorted(set(H.SPMM_ON))) if c[0] not in H.KINDS])
def test_spmm_data_is_exact_on_the_new_kinds(pkg, oracle, kind, name):
    ex = H.exact_on(H.carrier(kind, name, pkg, oracle), f"{name}/{kind}/spmm")
    for k in H.SPMM_K + H.SPMM_COLS_K:
        M, want = H.spmm_problem(ex, k, 5)
        assert want.shape == (ex.s.rows, k) and np.abs(M).max() <= 4


@pytest.mark.parametrize("kind,wrong", [("permuted", "inverse"), ("permuted", "unstable"), ("permuted-via-transpose", "inverse"),
                                        ("factor-lower", "diagonal_not_one")])
def test_a_wrong_new_carrier_is_told_apart(pkg, oracle, kind, wrong):
    """The inverse convention of the permutations, another order among a row's repeats, and a lower diagonal other than 1 (the
    factor is then not the matrix): each differs from the right carrier's `out` in the comparison the GPU tests make."""
    st = E.structure("lengths_around_short_threshold", pkg, oracle)
    if kind in H.PERMUTED_KINDS:
        st = E.shuffled(st, "wrong")[0]                                # repeats, which "unstable" needs
    right, bad = H.Carrier(kind, st, "wrong"), H.Carrier(kind, st, "wrong", wrong=wrong)
    for label, vals, _, _ in H.exact_problems(right, "wrong")[1]:
        want = (right.out.rp, right.out.ci, right.out_vals(vals))
        assert H.same(right.result(vals)[2], want) is None
        differs = H.same(bad.result(vals)[2], want)
        assert differs is not None, f"{kind}/{wrong}/{label}"
        if wrong == "unstable":                                    # the pattern is the same: only values among repeats moved
            assert H.same_pattern(bad.result(vals)[2], want) and "vals" in differs


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
    for a, b in p.equal_bytes:
        assert H.same(env[a][2], env[b][2]) is None, f"{name}: {a} and {b}: {H.same(env[a][2], env[b][2])}"
    for z in p.empty:
        assert len(env[z][2][1]) == 0, f"{name}: {z} is not empty"
    if not p.empty:
        assert all(len(env[s[0]][2][1]) > 0 for s in p.steps), f"{name}: a step came out empty"


def test_colour_of_a_product_on_the_host():
    """S = A A^T + I is sorted with one diagonal entry per row; its colouring is proper and needs fewer colours than rows; the
    multicolour ordering leaves both triangles of B with at most `colors` levels; the factor and the solve are finite."""
    import _color
    import _ilu0
    import _trsv
    c = H.colour_of_a_product()
    m, n, (rp, ci, va) = c["env"]["S"]
    col, perm, cptr, info = c["color"]
    assert m == n == 257 and _ilu0.is_sorted(rp, ci) and np.all(_trsv.diagonal(rp, ci)[1] == 1)
    assert _color.is_proper(rp, ci, col) and 2 <= info["colors"] < 128 and len(cptr) == info["colors"] + 1
    assert np.array_equal(np.sort(perm), np.arange(257)) and not np.array_equal(perm, np.arange(257))
    _, _, (brp, bci, bva) = c["env"]["B"]
    assert _ilu0.is_sorted(brp, bci) and len(bci) == len(ci) > 2000
    for uplo in _trsv.UPLOS:
        assert _color.depth(brp, bci, uplo) <= info["colors"] < _color.depth(rp, ci, uplo), uplo
    assert np.all(np.isfinite(c["env"]["M"][2][2])) and np.all(np.isfinite(c["z"])) and np.abs(c["z"]).max() > 0


@pytest.mark.parametrize("name", H.SOLVED)
def test_the_solved_programs_have_square_steps_with_both_triangles(name):
    p = H.programs()[name]
    square = [s for s, _, _, _ in p.steps if p.host[s][0] == p.host[s][1]]
    assert len(square) == len(p.steps) >= 2
    for s in square:
        for mat in (p.host[s], H.host_step("select_topk", [p.host[s]], k=H.SOLVED_K)):
            tri, b = H.triangles(mat)
            for uplo, (lp, od, x) in tri.items():
                assert len(lp) > 2 and np.array_equal(np.sort(od), np.arange(mat[0])) and x.shape == b.shape, (s, uplo)


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
