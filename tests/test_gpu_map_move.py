"""The one strided move behind spmv_csr_transpose_gather, _permute_gather, _select_gather and _select_scatter
(csrc/kernels_map.hip), at the array lengths where a word-per-lane kernel can go wrong: 0, 1, kBlock - 1, kBlock, kBlock + 1
and 2 kBlock + 3 nonzeros of the parent.  Every maker's map is worked out in numpy from the parent's pattern, and the moved
words are compared bit for bit: NaN payloads, +-0 and +-Inf among them.  count is 1 and 3, the stride of a dst of several
arrays the array's length and the length + 5; dst starts 7 words into a poisoned buffer (4-byte aligned, no more), and the
whole buffer is compared, so the words before it, behind it and in the gaps must be poison still.  A select handle (k = 1)
has fewer nonzeros than its parent: its scatter leaves every word that is not in the map as it was.  A second select parent
with two nonzeros in each of n rows puts the HANDLE's count on the same lengths.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_BLOCK = 256                                       # csrc/spmv_internal.hpp kBlock
LENGTHS = (0, 1, K_BLOCK - 1, K_BLOCK, K_BLOCK + 1, 2 * K_BLOCK + 3)
COLS, GUARD, POISON = 16, 7, -0x21524111            # 0xdeadbeef as int32
SPECIALS = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001], np.uint32)


def parent(nnz, rng, lengths=None):
    """(rows, row_ptr, col_idx, score): rows of 1, 2, 3, 1, ... nonzeros (or `lengths`) that hold nnz in all, three empty
    rows where nnz = 0; sorted distinct columns; distinct scores."""
    if lengths is None:
        lengths = []
        while sum(lengths) < nnz:
            lengths.append(min(len(lengths) % 3 + 1, nnz - sum(lengths)))
        lengths = lengths or [0, 0, 0]
    ci = np.concatenate([np.sort(rng.choice(COLS, size=n, replace=False)) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return len(lengths), rp, ci, rng.permutation(len(ci)).astype(np.float32)


def words(n, rng):
    w = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    w[:min(n, len(SPECIALS))] = SPECIALS[:n]
    return rng.permutation(w).view(np.int32)


def check_move(torch, gpu, rng, call, who, n_src, n_dst, expect):
    """call(src, dst) at count 1 (1-D) and 3 (strides n and n + 5); expect(s, d) applies the move to numpy arrays."""
    for count, pad in ((1, 0), (3, 0), (3, 5)):
        src_h = words(count * (n_src + pad), rng)
        want = np.full(2 * GUARD + count * (n_dst + pad), POISON, np.int32)
        for c in range(count):
            expect(src_h[c * (n_src + pad):][:n_src], want[GUARD + c * (n_dst + pad):][:n_dst])
        src_d = torch.zeros(len(src_h), dtype=torch.int32, device=gpu)      # (from_numpy of no words has stride 0)
        src_d.copy_(torch.from_numpy(src_h.copy()))
        buf = torch.full((len(want),), POISON, dtype=torch.int32, device=gpu)
        if count == 1:
            src, dst = src_d[:n_src], buf[GUARD:GUARD + n_dst]
        else:
            src = src_d.view(count, n_src + pad)[:, :n_src]
            dst = buf[GUARD:GUARD + count * (n_dst + pad)].view(count, n_dst + pad)[:, :n_dst]
        call(src, dst)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got, want), f"{who}, count {count}, stride n + {pad}: differs at words {np.flatnonzero(got != want)[:8]}"


@pytest.mark.parametrize("nnz", LENGTHS)
def test_every_makers_move_bit_for_bit(pkg, gpu, nnz):
    import torch
    capi = pkg.capi
    rng = np.random.Generator(np.random.PCG64(100 + nnz))
    rows, rp, ci, score = parent(nnz, rng)
    dev = [torch.from_numpy(a).to(gpu) for a in (rp, ci, score)]
    a = capi.CsrMatrix.from_device(rows, COLS, *dev)
    row_perm, col_perm = rng.permutation(rows).astype(np.int32), rng.permutation(COLS).astype(np.int32)
    made = []
    try:
        # the transpose: the positions stably sorted by column
        t = a.transpose(keep_map=True)
        made.append(t)
        t_map = np.argsort(ci, kind="stable")

        def gather(m):
            def expect(s, d):
                d[:] = s[m]
            return expect
        check_move(torch, gpu, rng, t.transpose_gather, "transpose_gather", nnz, nnz, gather(t_map))
        # the permutation, by both routes: row r is the parent's row row_perm[r] by (new column, position)
        inv_col = np.argsort(col_perm)
        order = [np.arange(rp[o], rp[o + 1]) for o in row_perm]
        b_map = np.concatenate([p[np.argsort(inv_col[ci[p]], kind="stable")] for p in order] + [np.zeros(0, np.int64)]).astype(np.int64)
        for via in (False, True):
            b = a.permute(torch.from_numpy(row_perm).to(gpu), torch.from_numpy(col_perm).to(gpu), keep_map=True, via_transpose=via)
            made.append(b)
            check_move(torch, gpu, rng, b.permute_gather, f"permute_gather (via_transpose={via})", nnz, nnz, gather(b_map))
        # the selection, k = 1: the position of every nonempty row's largest score
        parents = [(a, rp, score)]
        if nnz:
            rows2, rp2, ci2, score2 = parent(2 * nnz, rng, [2] * nnz)              # (the handle's count on the same lengths)
            dev2 = [torch.from_numpy(x).to(gpu) for x in (rp2, ci2, score2)]
            a2 = capi.CsrMatrix.from_device(rows2, COLS, *dev2)
            made.append(a2)
            parents.append((a2, rp2, score2))
        for p, prp, psc in parents:
            s = p.select_topk(1, keep_map=True)
            made.append(s)
            s_map = np.array([prp[r] + np.argmax(psc[prp[r]:prp[r + 1]]) for r in range(len(prp) - 1) if prp[r + 1] > prp[r]], np.int64)
            assert s.nnz == len(s_map) and (p.nnz < 4 or s.nnz < p.nnz)
            check_move(torch, gpu, rng, s.select_gather, "select_gather", p.nnz, s.nnz, gather(s_map))

            def scatter(src, d, m=s_map):
                d[m] = src
            check_move(torch, gpu, rng, s.select_scatter, "select_scatter", s.nnz, p.nnz, scatter)
    finally:
        torch.cuda.synchronize()
        for h in reversed(made):
            h.close()
        a.close()


def test_transpose_and_permute_gather_refuse_a_host_tensor(pkg, gpu):
    """A tensor that is not on the device never reaches the kernel as a host pointer: ValueError, as select_gather's."""
    import torch
    capi = pkg.capi
    rng = np.random.Generator(np.random.PCG64(3))
    rows, rp, ci, score = parent(5, rng)
    dev = [torch.from_numpy(x).to(gpu) for x in (rp, ci, score)]
    a = capi.CsrMatrix.from_device(rows, COLS, *dev)
    t, b = a.transpose(keep_map=True), a.permute(keep_map=True)
    try:
        on_host, on_dev = torch.zeros(5, dtype=torch.float32), torch.zeros(5, dtype=torch.float32, device=gpu)
        for who, fn in (("transpose_gather", t.transpose_gather), ("permute_gather", b.permute_gather)):
            for src, dst in ((on_host, on_dev), (on_dev, on_host)):
                with pytest.raises(ValueError, match="^" + who):
                    fn(src, dst)
        with pytest.raises(ValueError, match="^permute_gather"):
            b.permute_gather(on_host)
    finally:
        t.close()
        b.close()
        a.close()
