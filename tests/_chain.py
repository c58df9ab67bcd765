"""Carriers and programs: how the tests put known data on a handle that a builder made, and how they chain builders (host
only, numpy).  The builders are spmv_csr_transpose, _select_topk / _select_threshold, _spgemm, _add, _permute and _ilu0; their
contracts in numpy are test_transpose_host.host_transpose, tests/_select.py, tests/_spgemm.py, tests/_add.py, _color.permute and
_ilu0.factor, and nothing here computes an expectation in any other way.

A matrix is (rows, cols, (row_ptr, col_idx, vals)), as in _spgemm.py and _add.py.  A step is (name, op, operand names,
keywords) with op one of OPS; host_step runs one through its numpy model and run_host a list of them over named leaves.

A carrier turns a target structure (tests/_exact.py) and values on it into the operands of one builder such that the builder's
contract returns the target's pattern with exactly those values:

  sum        the target's nonzeros split at random into two disjoint patterns A and B, C = 1 A + 1 B: fl(1 v) = v
  sum-grown  C = 1 A + 0 G with A the whole target and G further positions whose values are NaN: a side whose coefficient is 0
             has no terms, so the new positions are +0 and G's NaNs are never read
  product    C = S B: B holds the even-numbered entries of the target's row i in its row 2 i and the odd-numbered ones in
             row 2 i + 1, S the entries (i, 2 i) and (i, 2 i + 1) of value 1: fma(1, v, +0) = v, and a row has as many terms as
             the target's row has entries
  threshold  the parent is the target with decoys mixed into its rows (empty ones too); the decoys' values are NaN and their
             scores lie below the threshold (or are NaN), the target's at or above it
  topk       k is the longest row; decoys sit only in rows of that length, score below every entry of the target or tie the
             lowest from behind the row's last entry (a tie goes to the earlier position)
  permuted   p and q are random permutations of the rows and the columns; the parent holds the target's row r in its row p[r],
             every column c relabelled q[c], the entries of a row in random storage order; C = permute(P, p, q) is the target
             with every row stably sorted by column, repeats in the parent's order.  Values travel as bits.
             permuted-via-transpose: the same operands through SPMV_PERMUTE_VIA_TRANSPOSE, the same bytes
  factor-upper, factor-lower
             with n = max(rows, cols) every entry (i, j) of the target mirrored to (min, max) (lower: (max, min)), the diagonal
             added, repeats merged, rows sorted; for factor-lower the diagonal values are 1.  C = ilu0(A) is A itself bit for
             bit: an upper-triangular row has no position with col < i, a lower-triangular row divides by a pivot of 1 and
             has no update.  base and out are that square structure

Where a row of the target repeats a column, sum and product merge the repeats into one entry: `base` is the target with the
repeats merged, the values live on base, and the first repeat carries the value while the others carry +0 (v + 0 = v).  `out`
is the structure the builder must return: base, or base and the +0 positions of sum-grown, or the target itself for select
(which keeps repeats).  Exact data (tests/_exact.py) goes on base; +0 entries add nothing to a row's sum while x is finite.
"""
import functools

import numpy as np

import _add
import _color
import _exact as E
import _ilu0
import _select
import _spgemm
import _trsv
from test_transpose_host import host_transpose

f32 = np.float32
OPS = ("transpose", "select_topk", "select_threshold", "spgemm", "add", "permute", "ilu0")
THIRD = float(f32(1) / f32(3))
KINDS = ("threshold", "topk", "product", "sum", "sum-grown")
PERMUTED_KINDS = ("permuted", "permuted-via-transpose")
FACTOR_KINDS = ("factor-upper", "factor-lower")
ALL_KINDS = KINDS + PERMUTED_KINDS + FACTOR_KINDS
# the structures the factor kinds run on: mirrored, they still hold rows above SPMV_ILU0_SERIAL_MAX
FACTOR_ON = ("lengths_around_short_threshold", "not_multiple_of_anything", "long_row_between_short_rows")
# the structures of _exact every path runs on, per builder; the product of the 120 000-entry row is the oversized route, which
# the program "oversized_then_selected" covers once
STRUCTURES = ("wave_pipe_thresholds", "rows_near_64", "odd_last_chunk", "stencil7_32", "wide_window", "long_row_between_short_rows",
              "rows_exactly_chunk_aligned", "chunk_ends_on_row_boundary_then_empties", "all_rows_empty", "leading_empty_rows",
              "trailing_empty_rows", "single_element", "lengths_around_short_threshold", "not_multiple_of_anything")
CASES = [(k, n) for k in KINDS for n in STRUCTURES] + [(k, "one_row_spanning_30_chunks") for k in KINDS if k != "product"]
NEW_CASES = [(k, n) for k in PERMUTED_KINDS for n in STRUCTURES + ("one_row_spanning_30_chunks",)] + \
            [(k, n) for k in FACTOR_KINDS for n in FACTOR_ON]
# the structures the other consumers run on
SPMM_ON = ("wave_pipe_thresholds", "not_multiple_of_anything", "leading_empty_rows")
SDDMM_ON = ("wave_pipe_thresholds", "lengths_around_short_threshold")
VALS16_ON = ("odd_last_chunk", "long_row_between_short_rows")
SPMM_K, SPMM_COLS_K, SDDMM_K = (1, 4, 17), (65, 130), (3, 16, 64)


def consumer_cases(on):
    """(kind, structure) of one of the other consumers: every kind on the consumer's structures, the factor kinds on theirs."""
    return [(k, n) for k in KINDS + PERMUTED_KINDS for n in on] + [(k, FACTOR_ON[0]) for k in FACTOR_KINDS]


# ---- the builders on the host ----------------------------------------------------------------------------------------------------
def host_step(builder, mats, **kw):
    """One builder through its numpy model: (rows, cols, (row_ptr, col_idx, vals))."""
    if builder == "transpose":
        (m, n, (rp, ci, va)), = mats
        t = host_transpose(m, n, rp, ci, np.asarray(va, f32))
        return n, m, (t[0], np.asarray(t[1], np.int32), np.asarray(t[2], f32))
    if builder == "select_topk":
        (m, n, (rp, ci, va)), = mats
        return m, n, _select.host_select_topk(m, rp, ci, va, kw["k"], kw.get("score"), kw.get("abs", False))[:3]
    if builder == "select_threshold":
        (m, n, (rp, ci, va)), = mats
        return m, n, _select.host_select_threshold(m, rp, ci, va, kw["threshold"], kw.get("score"), kw.get("abs", False))[:3]
    if builder == "spgemm":
        a, b = mats
        assert a[1] == b[0]
        return a[0], b[1], _spgemm.spgemm(a[2], b[2])[:3]
    if builder == "add":
        a, b = mats
        assert a[:2] == b[:2]
        return a[0], a[1], _add.add(a[2], b[2], kw.get("alpha", 1.0), kw.get("beta", 1.0), kw.get("op", "union"), cols=a[1])[:3]
    if builder == "permute":
        (m, n, (rp, ci, va)), = mats
        return m, n, _color.permute(rp, ci, va, row_perm=kw.get("row_perm"), col_perm=kw.get("col_perm"), cols=n)[:3]
    if builder == "ilu0":
        (m, n, (rp, ci, va)), = mats
        assert m == n
        return m, n, (np.asarray(rp, np.int32), np.asarray(ci, np.int32), _ilu0.factor(rp, ci, va))
    raise KeyError(builder)


def run_host(leaves, steps):
    """Every step's result by name (the leaves included)."""
    env = dict(leaves)
    for name, op, operands, kw in steps:
        env[name] = host_step(op, [env[o] for o in operands], **kw)
    return env


def same(got, want):
    """None, or what differs first: _spgemm.same (bit for bit; a NaN matches any NaN)."""
    return _spgemm.same(got, want)


def same_pattern(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- carriers ----------------------------------------------------------------------------------------------------------------
def _rp(row, rows):
    return np.concatenate([[0], np.cumsum(np.bincount(row, minlength=rows))]).astype(np.int32)


def _merged(st):
    """The target with the repeats of a row merged (rows ascending), the entry of every nonzero, and whether it is the entry's
    first nonzero in storage order."""
    width = max(st.cols, 1)
    key = st.row_of * width + st.ci.astype(np.int64)
    entries, e = np.unique(key, return_inverse=True)
    first_pos = np.full(entries.size, st.nnz, np.int64)
    np.minimum.at(first_pos, e, np.arange(st.nnz, dtype=np.int64))
    first = np.zeros(st.nnz, bool)
    first[first_pos] = True
    return E.Structure(st.rows, st.cols, _rp(entries // width, st.rows), entries % width), e, first


class Carrier:
    """kind, target, base (where the values live), out (what the builder must return), steps (one step named "C"), and
    leaves(vals on base) -> the operands; out_vals(vals on base) -> the values on out."""

    def __init__(self, kind, target, seed_name, wrong=None):
        assert kind in ALL_KINDS
        self.kind, self.target, self.wrong = kind, target, wrong
        self._diag = None
        seed_kind = "permuted" if kind in PERMUTED_KINDS else kind          # both routes get the same operands
        self.rng = np.random.default_rng([sum(map(ord, seed_name)) * 7919 + len(seed_name), ALL_KINDS.index(seed_kind)])
        getattr(self, "_" + kind.replace("-", "_"))()
        # the pattern the model returns for these operands is the expectation; on a right carrier it is `out`
        zeros = np.zeros(self.base.nnz, f32)
        got = run_host(self.leaves(zeros), self.steps)["C"]
        if wrong is None:
            assert (got[0], got[1]) == (self.out.rows, self.out.cols) and same_pattern(got[2], (self.out.rp, self.out.ci)), kind

    def result(self, vals):
        return run_host(self.leaves(vals), self.steps)["C"]

    def out_vals(self, vals):
        if self.kind == "factor-lower":
            return self._unit_diagonal(vals, f32(1))
        if self._out_from_base is None:
            return np.asarray(vals, f32)
        v = np.zeros(self.out.nnz, f32)
        v[self._out_from_base] = vals
        return v

    # values on the target's nonzeros: the entry's value on its first nonzero, +0 on the repeats
    def _on_target(self, vals):
        return np.where(self._first, np.asarray(vals, f32)[self._entry], f32(0)).astype(f32) if self.target.nnz else np.zeros(0, f32)

    def _sub(self, mask, tv):
        st = self.target
        return st.rows, st.cols, (_rp(st.row_of[mask], st.rows), st.ci[mask], tv[mask])

    # -- sum ---------------------------------------------------------------------------------------------------------------------
    def _sum(self):
        st = self.target
        self.base, self._entry, self._first = _merged(st)
        self.out, self._out_from_base = self.base, None
        self._mask = self.rng.random(st.nnz) < 0.5
        self.steps = [("C", "add", ("A", "B"), dict(alpha=1.0, beta=1.0, op="union"))]

    def _sum_grown(self):
        st = self.target
        self.base, self._entry, self._first = _merged(st)
        extra = st.nnz // 4 + st.rows // 8 + 3
        g_row = np.sort(self.rng.integers(0, st.rows, extra))
        g_col = self.rng.integers(0, st.cols, extra)
        self._g = (st.rows, st.cols, (_rp(g_row, st.rows), g_col.astype(np.int32), np.full(extra, np.nan, f32)))
        width = max(st.cols, 1)
        base_key = self.base.row_of * width + self.base.ci
        keys = np.union1d(base_key, g_row * width + g_col)
        self.out = E.Structure(st.rows, st.cols, _rp(keys // width, st.rows), keys % width)
        self._out_from_base = np.searchsorted(keys, base_key)
        self.steps = [("C", "add", ("A", "G"), dict(alpha=1.0, beta=0.0, op="union"))]

    # -- product -----------------------------------------------------------------------------------------------------------------
    def _product(self):
        st = self.target
        self.base, self._entry, self._first = _merged(st)
        self.out, self._out_from_base = self.base, None
        local = np.arange(st.nnz, dtype=np.int64) - st.rp[:-1].astype(np.int64)[st.row_of]
        self._b_row = 2 * st.row_of + (local & 1)
        self._b_order = np.lexsort((np.arange(st.nnz), self._b_row))
        self.steps = [("C", "spgemm", ("S", "B"), {})]

    # -- select ------------------------------------------------------------------------------------------------------------------
    def _parent(self, decoys_per_row, t_score, d_score_of):
        """The target's nonzeros with decoys_per_row[r] decoys mixed into row r; d_score_of(slot == row length) -> scores."""
        st, rng = self.target, self.rng
        self.base = self.out = st
        self._out_from_base = None
        lengths = np.diff(st.rp).astype(np.int64)
        d_row = np.repeat(np.arange(st.rows, dtype=np.int64), decoys_per_row)
        slot = (rng.random(d_row.size) * (lengths[d_row] + 1)).astype(np.int64)          # before entry `slot` of the row
        local = np.arange(st.nnz, dtype=np.int64) - st.rp[:-1].astype(np.int64)[st.row_of]
        place = np.concatenate([local.astype(np.float64), slot - 0.5])
        row = np.concatenate([st.row_of, d_row])
        order = np.lexsort((rng.random(row.size), place, row))
        self._is_target = (np.arange(row.size) < st.nnz)[order]
        self._p_rp = _rp(row, st.rows)
        self._p_ci = np.concatenate([st.ci.astype(np.int64), rng.integers(0, st.cols, d_row.size)])[order].astype(np.int32)
        d_score = d_score_of(slot == lengths[d_row])
        if self.wrong == "decoy_kept" and d_score.size:
            d_score[d_score.size // 2] = f32(9.0)
        self._score = np.concatenate([t_score, d_score]).astype(f32)[order]
        self._n_decoys = int(d_row.size)

    def _threshold(self):
        st, rng = self.target, self.rng
        low = np.array([0.25, -1.0, np.nan, -np.inf, np.nextafter(f32(0.5), f32(0))], f32)
        per_row = rng.integers(0, 3, st.rows)
        per_row[st.rows // 2] += 1                                     # at least one decoy, whatever the draw
        self._parent(per_row, rng.choice(np.array([0.5, 1.0, 3.0, np.inf], f32), st.nnz),
                     lambda last: rng.choice(low, last.size))
        self.steps = [("C", "select_threshold", ("P",), dict(threshold=0.5, score=self._score))]

    def _topk(self):
        st, rng = self.target, self.rng
        lengths = np.diff(st.rp)
        longest = int(lengths.max()) if st.rows else 0
        per_row = np.where(lengths == longest, rng.integers(1, 4, st.rows), 0) if longest else np.zeros(st.rows, np.int64)
        low = np.array([0.5, -1.0, np.nan, -np.inf], f32)

        def d_score(last):
            s = rng.choice(low, last.size)
            s[last & (rng.random(last.size) < 0.5)] = f32(1.0)        # ties the target's lowest score from behind its last entry
            return s
        self._parent(per_row, rng.choice(np.array([1.0, 2.0, 7.0], f32), st.nnz), d_score)
        self.steps = [("C", "select_topk", ("P",), dict(k=max(longest, 1), score=self._score))]

    # -- permute -----------------------------------------------------------------------------------------------------------------
    def _permuted(self, via_transpose=False):
        st, rng = self.target, self.rng
        p, q = rng.permutation(st.rows), rng.permutation(st.cols)
        parent_row = p[st.row_of]
        order = np.lexsort((rng.random(st.nnz), parent_row))            # the parent's storage order, of the target's nonzeros
        pos = np.empty(st.nnz, np.int64)
        pos[order] = np.arange(st.nnz)                                  # where the parent stores the target's nonzero t
        self._p_rp = _rp(parent_row, st.rows)
        self._p_ci = q[st.ci.astype(np.int64)][order].astype(np.int32) if st.nnz else np.zeros(0, np.int32)
        # every row stably sorted by column, repeats in the parent's order ("unstable": in the reverse of it)
        by = np.lexsort((-pos if self.wrong == "unstable" else pos, st.ci, st.row_of))
        self.base = self.out = E.Structure(st.rows, st.cols, st.rp, st.ci[by])
        self._out_from_base = None
        self._pos_of_out = pos[by]
        if self.wrong == "inverse":                                     # "new index perm[r] holds old index r"
            p, q = _color.inverse(p), _color.inverse(q)
        self.steps = [("C", "permute", ("P",), dict(row_perm=p.astype(np.int32), col_perm=q.astype(np.int32),
                                                    via_transpose=via_transpose))]

    def _permuted_via_transpose(self):
        self._permuted(via_transpose=True)

    # -- ilu0 --------------------------------------------------------------------------------------------------------------------
    def _factor(self, lower):
        st = self.target
        n = max(st.rows, st.cols)
        i, j = st.row_of, st.ci.astype(np.int64)
        lo, hi = np.minimum(i, j), np.maximum(i, j)
        d = np.arange(n, dtype=np.int64)
        keys = np.unique(np.concatenate([(hi * n + lo) if lower else (lo * n + hi), d * n + d]))
        self.base = self.out = E.Structure(n, n, _rp(keys // n, n), keys % n)
        self._out_from_base = None
        self._diag = np.flatnonzero(self.base.row_of == self.base.ci)
        self.steps = [("C", "ilu0", ("A",), {})]

    def _factor_upper(self):
        self._factor(False)

    def _factor_lower(self):
        self._factor(True)

    def _unit_diagonal(self, vals, one):
        v = np.array(vals, f32)
        v[self._diag] = one
        return v

    # -- the operands ------------------------------------------------------------------------------------------------------------
    def leaves(self, vals):
        st = self.target
        if self.kind in PERMUTED_KINDS:
            pv = np.empty(st.nnz, f32)
            pv[self._pos_of_out] = np.asarray(vals, f32)
            return {"P": (st.rows, st.cols, (self._p_rp, self._p_ci, pv))}
        if self.kind in FACTOR_KINDS:
            b = self.base
            va = np.asarray(vals, f32)
            if self.kind == "factor-lower":
                va = self._unit_diagonal(vals, f32(2) if self.wrong == "diagonal_not_one" else f32(1))
            return {"A": (b.rows, b.cols, (b.rp, b.ci, va))}
        if self.kind in ("threshold", "topk"):
            pv = np.full(self._is_target.size, np.nan, f32)
            pv[self._is_target] = np.asarray(vals, f32)
            return {"P": (st.rows, st.cols, (self._p_rp, self._p_ci, pv))}
        tv = self._on_target(vals)
        if self.kind == "sum":
            a, b = self._sub(self._mask, tv), self._sub(~self._mask, tv)
            if self.wrong == "swapped_split":             # the values of the two sides exchanged where both have an entry
                n = min(a[2][2].size, b[2][2].size)
                va, vb = a[2][2].copy(), b[2][2].copy()
                va[:n], vb[:n] = b[2][2][:n], a[2][2][:n]
                a, b = (a[0], a[1], (a[2][0], a[2][1], va)), (b[0], b[1], (b[2][0], b[2][1], vb))
            return {"A": a, "B": b}
        if self.kind == "sum-grown":
            return {"A": self._sub(np.ones(st.nnz, bool), tv), "G": self._g}
        s = (st.rows, 2 * st.rows, (2 * np.arange(st.rows + 1, dtype=np.int32), np.arange(2 * st.rows, dtype=np.int32),
                                    np.ones(2 * st.rows, f32)))
        o = self._b_order
        return {"S": s, "B": (2 * st.rows, st.cols, (_rp(self._b_row, 2 * st.rows), st.ci[o], tv[o]))}


@functools.lru_cache(maxsize=None)
def carrier(kind, name, pkg=None, oracle=None):
    return Carrier(kind, E.structure(name, pkg, oracle), name)


def exact_on(c, seed_name, scaled=True):
    """_exact.Exact on the carrier's base.  factor-lower: the diagonal's k is 1 and no row is scaled, so that vals() holds the 1
    the carrier needs there and the integer sums stay exact."""
    ex = E.Exact(c.base, seed_name, scaled=scaled and c.kind != "factor-lower")
    if c.kind == "factor-lower":
        ex.k[c._diag] = 1
    return ex


def exact_problems(c, seed_name):
    """Exact data on the carrier's base: the Exact and [(label, vals on base, x, expected y)] (integer and subnormal).

    factor-lower, subnormal: the diagonal is 1 among values k 2^-75, so row i holds one term m_i 2^-74 beside terms that are
    multiples of 2^-149 and sum to less than 2^-125 in magnitude.  A partial sum without the diagonal term is such a multiple,
    exact; one with it (m_i != 0) is m_i 2^-74 plus less than 2^-125, which rounds back to m_i 2^-74 (half an ulp is at least
    2^-98).  So in every order y_i = m_i 2^-74 where m_i != 0 and the exact sum of the other terms where m_i = 0."""
    ex = exact_on(c, seed_name)
    sub_vals, sub_want = ex.sub_vals(), None
    if c.kind == "factor-lower":
        on_diag = np.zeros(c.base.nnz, bool)
        on_diag[c._diag] = True
        sub_vals = c._unit_diagonal(sub_vals, f32(1))
        others = ex.int_sums(keep=~on_diag)
        assert np.abs(others).max(initial=0) < 1 << 24
        sub_want = np.where(ex.m != 0, np.ldexp(ex.m.astype(np.float64), E.SUB_X_EXP),
                            np.ldexp(others.astype(np.float64), E.SUB_VAL_EXP + E.SUB_X_EXP)).astype(f32)
    else:
        sub_want = ex.sub_expected()
    return ex, [("int", ex.vals(), ex.x(), ex.expected()), ("subnormal", sub_vals, ex.sub_x(), sub_want)]


def spmm_problem(ex, k, seed):
    """Integer X (cols x k, int64) and the expected Y (rows x k, fp32) on ex's structure; int_sums asserts, column by column,
    that sum |k m| stays within _exact.EXACT_LIMIT units of the row's scale."""
    M = np.random.default_rng([seed, k]).integers(-4, 5, size=(ex.s.cols, k)).astype(np.int64)
    want = np.stack([ex.expected(ex.int_sums(m=M[:, c])) for c in range(k)], axis=1) if k else np.zeros((ex.s.rows, 0), f32)
    return M, want


def sddmm_problem(s, k, seed):
    """Integer U (rows x k) and X (cols x k) in [-4, 4] and the int64 U[row] . X[col] of every nonzero of s; the exactness
    condition: sum |u x| <= 16 k per nonzero, within _exact.EXACT_LIMIT, so every partial sum of every order is an fp32 number."""
    rng = np.random.default_rng([seed, k, 1])
    U = rng.integers(-4, 5, size=(s.rows, k)).astype(np.int64)
    X = rng.integers(-4, 5, size=(s.cols, k)).astype(np.int64)
    assert 16 * k <= E.EXACT_LIMIT
    want = np.zeros(s.nnz, np.int64)
    for c in range(k):                                                 # column by column: no nnz x k temporary
        want += U[s.row_of, c] * X[s.ci, c]
    return U, X, want.astype(f32)


# ---- programs ----------------------------------------------------------------------------------------------------------------
LONG_ROW = 5000


def leaf(seed, rows, cols, max_len=40, long_row=0, special=0.02):
    """Unsorted rows of 0 .. max_len entries with repeats (_spgemm.random_matrix), optionally one row of long_row entries;
    values from _spgemm.spread with the bit patterns of _add.SPECIAL mixed in."""
    rng = np.random.default_rng(seed)
    m, n, (rp, ci, va) = _spgemm.random_matrix(rng, rows, cols, max_len)
    if long_row and rows and cols:
        r = rows // 2
        lists = [ci[rp[i]:rp[i + 1]] for i in range(rows)]
        lists[r] = rng.integers(0, cols, long_row)
        m, n, (rp, ci, va) = _spgemm.from_rows(cols, lists, rng)
    va = va.copy()
    hit = rng.random(va.size) < special
    va[hit] = _add.SPECIAL[rng.integers(0, _add.SPECIAL.size, int(hit.sum()))]
    return m, n, (rp, ci, va)


def _band(rows, cols, half):
    centre = (np.arange(rows, dtype=np.int64) * cols) // max(rows, 1)
    lists = [np.arange(max(c - half, 0), min(c + half + 1, cols)) for c in centre]
    return _spgemm.from_rows(cols, lists, np.random.default_rng(41), values=lambda rng, n: np.ones(n, f32))


def _columns(seed, rows, cols, max_len, lo, hi, step=1):
    """A leaf whose columns are lo, lo + step, ... below hi."""
    m, n, (rp, ci, va) = leaf(seed, rows, cols, max_len)
    span = max((hi - lo + step - 1) // step, 1)
    return m, n, (rp, (lo + step * (ci.astype(np.int64) % span)).astype(np.int32), va)


def _empty(rows, cols):
    return rows, cols, (np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, f32))


class Program:
    def __init__(self, name, leaves, steps, equal_patterns=(), empty=(), equal_bytes=()):
        self.name, self.leaves, self.steps = name, leaves, steps
        self.equal_patterns, self.empty, self.equal_bytes = tuple(equal_patterns), tuple(empty), tuple(equal_bytes)

    @functools.cached_property
    def host(self):
        """Every step's result on the host, computed once and left unchanged."""
        return run_host(self.leaves, self.steps)


def _perm(seed, n):
    return np.random.default_rng(seed).permutation(n).astype(np.int32)


def identity(n):
    """I of order n."""
    return n, n, (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, f32))


def _feed(z, partner, sq, rows, cols):
    """An empty rows x cols handle `z` fed to every builder; `partner` has z's shape, `sq` is cols x rows."""
    return [(z + "_same", "permute", (z,), {}),
            (z + "_moved", "permute", (z,), dict(row_perm=_perm(3130 + rows, rows), col_perm=_perm(3131 + cols, cols))),
            (z + "_moved_by_transposes", "permute", (z,), dict(row_perm=_perm(3132 + rows, rows), via_transpose=True)),
            (z + "_x_sq", "spgemm", (z, sq), {}), ("sq_x_" + z, "spgemm", (sq, z), {}),
            (z + "_or_p", "add", (z, partner), dict(alpha=THIRD, beta=3.0, op="union")),
            ("p_minus_" + z, "add", (partner, z), dict(alpha=THIRD, beta=3.0, op="minus")),
            ("p_and_" + z, "add", (partner, z), dict(alpha=THIRD, beta=3.0, op="intersect")),
            (z + "_or_" + z, "add", (z, z), dict(op="union")),
            (z + "_top3", "select_topk", (z,), dict(k=3)), (z + "_ge0", "select_threshold", (z,), dict(threshold=0.0, abs=True)),
            (z + "_T", "transpose", (z,), {}), (z + "_T_x_" + z, "spgemm", (z + "_T", z), {})]


@functools.lru_cache(maxsize=None)
def programs():
    """The fixed list, by name."""
    mix = dict(alpha=THIRD, beta=3.0)
    out = [
        Program("a_plus_at", {"A": leaf(3101, 257, 257, long_row=LONG_ROW)},
                [("T", "transpose", ("A",), {}), ("C", "add", ("A", "T"), dict(mix, op="union"))]),
        Program("aat_topk", {"A": leaf(3102, 257, 193)},
                [("T", "transpose", ("A",), {}), ("P", "spgemm", ("A", "T"), {}), ("K", "select_topk", ("P",), dict(k=8, abs=True))]),
        Program("pattern_algebra", {"A": leaf(3103, 257, 193, long_row=LONG_ROW), "band": _band(257, 193, 2),
                                    "M": leaf(3104, 257, 193, 150, special=0.0), "N": leaf(3105, 257, 193, 12, special=0.0)},
                [("S", "select_topk", ("A",), dict(k=6)), ("U", "add", ("S", "band"), dict(op="union")),
                 ("I", "add", ("U", "M"), dict(alpha=1.0, beta=0.0, op="intersect")),
                 ("D", "add", ("I", "N"), dict(op="minus"))]),
        Program("distributive", {"A": leaf(3106, 257, 193), "B": leaf(3107, 257, 193), "C": leaf(3108, 193, 257)},
                [("AB", "add", ("A", "B"), dict(mix, op="union")), ("L", "spgemm", ("AB", "C"), {}),
                 ("AC", "spgemm", ("A", "C"), {}), ("BC", "spgemm", ("B", "C"), {}), ("R", "add", ("AC", "BC"), dict(op="union"))],
                equal_patterns=[("L", "R")]),
        Program("transpose_of_product", {"A": leaf(3109, 257, 193), "B": leaf(3110, 193, 257)},
                [("P", "spgemm", ("A", "B"), {}), ("PT", "transpose", ("P",), {}), ("BT", "transpose", ("B",), {}),
                 ("AT", "transpose", ("A",), {}), ("Q", "spgemm", ("BT", "AT"), {})], equal_patterns=[("PT", "Q")]),
        Program("threshold_transposed", {"A": leaf(3111, 257, 193, long_row=LONG_ROW)},
                [("S", "select_threshold", ("A",), dict(threshold=0.5, abs=True)), ("T", "transpose", ("S",), {})]),
        # (g) an empty result in the middle: an empty intersection (even against odd columns), a product without terms (a's
        # columns name empty rows of b), and leaves with m = 0 and n = 0
        Program("empty_intersection", {"A": _columns(3112, 257, 257, 40, 0, 257, 2), "B": _columns(3113, 257, 257, 40, 1, 257, 2),
                                       "SQ": leaf(3114, 257, 257, 20)},
                [("Z", "add", ("A", "B"), dict(mix, op="intersect"))] + _feed("Z", "A", "SQ", 257, 257), empty=("Z",)),
        Program("product_without_terms", {"A": _columns(3115, 257, 193, 40, 0, 100),
                                          "B": _rows_from(100, leaf(3116, 93, 257, 40)), "P0": leaf(3117, 257, 257, 20)},
                [("Z", "spgemm", ("A", "B"), {})] + _feed("Z", "P0", "P0", 257, 257), empty=("Z",)),
        Program("no_rows", {"Z": _empty(0, 193), "P0": _empty(0, 193), "SQ": _empty(193, 0)},
                _feed("Z", "P0", "SQ", 0, 193), empty=("Z",)),
        Program("no_columns", {"Z": _empty(257, 0), "P0": _empty(257, 0), "SQ": _empty(0, 257)},
                _feed("Z", "P0", "SQ", 257, 0), empty=("Z",)),
        Program("self_operands", {"A": leaf(3119, 257, 257, 24)},
                [("T", "transpose", ("A",), {}), ("C", "add", ("A", "T"), dict(mix, op="union")),
                 ("CC", "spgemm", ("C", "C"), {}), ("C2", "add", ("C", "C"), dict(mix, op="union"))]),
        # (i) a row of 1500 entries over rows of 0 .. 60: more than 32768 terms on 3001 columns
        Program("oversized_then_selected", {"A": leaf(3120, 257, 193, long_row=1500), "B": leaf(3121, 193, 3001, 60)},
                [("P", "spgemm", ("A", "B"), {}), ("K", "select_topk", ("P",), dict(k=5, abs=True))]),
        # permute(transpose(A), q, p) and transpose(permute(A, p, q)): the same pattern and the same bytes (repeats stay in A's
        # storage order on both ways)
        Program("permute_commutes", {"A": leaf(3122, 257, 193, long_row=LONG_ROW)},
                [("T", "transpose", ("A",), {}), ("L", "permute", ("T",), dict(row_perm=_perm(3123, 193), col_perm=_perm(3124, 257))),
                 ("B", "permute", ("A",), dict(row_perm=_perm(3124, 257), col_perm=_perm(3123, 193))), ("R", "transpose", ("B",), {})],
                equal_patterns=[("L", "R")], equal_bytes=[("L", "R")]),
        # (P A Q^T) (Q B R^T) against P (A B) R^T: the same pattern; the sums of a row take their terms in another order
        Program("permuted_product", {"A": leaf(3125, 257, 193), "B": leaf(3126, 193, 257)},
                [("PA", "permute", ("A",), dict(row_perm=_perm(3127, 257), col_perm=_perm(3128, 193))),
                 ("PB", "permute", ("B",), dict(row_perm=_perm(3128, 193), col_perm=_perm(3129, 257), via_transpose=True)),
                 ("L", "spgemm", ("PA", "PB"), {}), ("P", "spgemm", ("A", "B"), {}),
                 ("R", "permute", ("P",), dict(row_perm=_perm(3127, 257), col_perm=_perm(3129, 257)))], equal_patterns=[("L", "R")]),
    ]
    return {p.name: p for p in out}


@functools.lru_cache(maxsize=None)
def colour_of_a_product():
    """P = A A^T, S = P + I (sorted, with a diagonal), the colouring of S, B = permute(S, perm, perm), M = ILU(0) of B and
    z = U^-1 L^-1 r, all on the host: leaves, env (T, P, S, B, M), color (colour, perm, color_ptr, info), r, z."""
    leaves = {"A": leaf(3140, 257, 193, 6, special=0.0), "I": identity(257)}
    env = run_host(leaves, [("T", "transpose", ("A",), {}), ("P", "spgemm", ("A", "T"), {}), ("S", "add", ("P", "I"), dict(op="union"))])
    rp, ci, _ = env["S"][2]
    coloring = _color.color(rp, ci)
    perm = coloring[1]
    env["B"] = host_step("permute", [env["S"]], row_perm=perm, col_perm=perm)
    env["M"] = host_step("ilu0", [env["B"]])
    r = _trsv.rhs(257, np.random.default_rng(3141))
    return dict(leaves=leaves, env=env, color=coloring, r=r, z=_ilu0.apply(*env["M"][2], r))


SOLVED = ("a_plus_at", "self_operands")          # the programs whose square steps are planned and solved, and a top-k of each
SOLVED_K = 5


def triangles(mat):
    """{uplo: (level_ptr, order, the UNIT solve's x)} of a square matrix by tests/_trsv.py, and the right-hand side."""
    n, _, (rp, ci, va) = mat
    b = _trsv.rhs(n, np.random.default_rng(3142))
    out = {}
    for uplo in _trsv.UPLOS:
        lev = _trsv.levels(rp, ci, uplo)
        out[uplo] = _trsv.order(lev) + (_trsv.solve(rp, ci, va, b, uplo, unit=True, lev=lev),)
    return out, b


def _rows_from(first, mat):
    """mat's rows moved down by `first` empty rows."""
    m, n, (rp, ci, va) = mat
    return m + first, n, (np.concatenate([np.zeros(first, np.int32), rp]).astype(np.int32), ci, va)


PROGRAMS = ("a_plus_at", "aat_topk", "pattern_algebra", "distributive", "transpose_of_product", "threshold_transposed",
            "empty_intersection", "product_without_terms", "no_rows", "no_columns", "self_operands", "oversized_then_selected",
            "permute_commutes", "permuted_product")
