"""spmv_csr_permute, its companions and spmv_permute_vector on the device against the numpy contract of tests/_color.py, bit for bit
(include/spmv_hip.h "the multicolour ordering").

  1. row_ptr, col_idx, vals as bits (a NaN payload and -0.0 among them) and the map equal the contract for rows of 0, 1, 63, 64, 65,
     4095 and 4096 entries through the direct route, with a row of 4097 entries (the call switches to the route via the transpose),
     and on a rectangular pattern -- by rows, by columns, both and neither -- and again with the route via the transpose forced;
  2. a bad permutation is refused with its index in the message, nothing left allocated;
  3. permute_values after a rewrite and permute_gather inside a replayed graph; permute_vector there and back;
  4. one map per handle: the other makers' companions refuse B, and B's refuse the others' handles;
  5. B through SPMV_SCALAR equals the serial chain on B's own arrays, and the permuted result of A where only rows moved;
  6. the tester executable colours, permutes and factors a file.
"""
import ctypes as C

import numpy as np
import pytest

import _color as K
import _ilu0 as G
import _trsv as T

MIB = 1 << 20
f32 = np.float32
MODES = ("both", "rows", "cols", "identity")


def _dev(gpu, a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(gpu)


_case_cache = {}


def _case(key):
    """(rows, cols, rp, ci, va, row_perm, col_perm) of a shared case, made once."""
    if key not in _case_cache:
        if key == "rectangular":
            rows, cols, rp, ci, va = K.rectangular_case()
        else:
            rows, cols, rp, ci, va = K.lengths_case(longest=int(key))
        rng = np.random.default_rng(41)
        _case_cache[key] = (rows, cols, rp, ci, va, rng.permutation(rows).astype(np.int32), rng.permutation(cols).astype(np.int32))
    return _case_cache[key]


def _download(B):
    import torch
    torch.cuda.synchronize()
    return B.download()


def _map_of(B, gpu):
    """B's map, read through permute_gather of the positions themselves."""
    import torch
    src = torch.arange(B.nnz, dtype=torch.int32, device=gpu)
    return B.permute_gather(src).cpu().numpy().astype(np.uint32)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ("4096", "4097", "rectangular"))
def test_permute_equals_the_contract_through_both_routes(pkg, gpu, key, mode):
    capi = pkg.capi
    rows, cols, rp, ci, va, rperm, cperm = _case(key)
    rperm = rperm if mode in ("both", "rows") else None
    cperm = cperm if mode in ("both", "cols") else None
    assert np.diff(rp).max() == (11 if key == "rectangular" else int(key))
    A = capi.CsrMatrix.from_host(rows, cols, rp, ci, va)
    want = K.permute(rp, ci, va, rperm, cperm, cols=cols)
    d_r = None if rperm is None else _dev(gpu, rperm)
    d_c = None if cperm is None else _dev(gpu, cperm)
    for via in (False, True):
        B = A.permute(d_r, d_c, keep_map=True, via_transpose=via)
        assert (B.rows, B.cols, B.nnz) == (rows, cols, ci.size)
        got = _download(B)
        what = f"{key} {mode} via_transpose={via}"
        assert np.array_equal(got[0], want[0]), f"{what}: row_ptr"
        assert np.array_equal(got[1], want[1]), f"{what}: col_idx"
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), f"{what}: vals as bits"
        assert np.array_equal(_map_of(B, gpu), want[3]), f"{what}: map"
        assert B.permute_map_bytes() == 4 * ci.size
        B.close()
    bare = A.permute(d_r, d_c)
    assert bare.permute_map_bytes() == 0 and np.array_equal(_download(bare)[1], want[1])
    bare.close()
    A.close()


@pytest.mark.gpu
def test_the_special_values_keep_their_bits(pkg, gpu):
    rows, cols, rp, ci, va, rperm, cperm = _case("4096")
    bits = va.view(np.uint32)
    assert 0x7FC01234 in bits and 0x80000000 in bits
    A = pkg.capi.CsrMatrix.from_host(rows, cols, rp, ci, va)
    B = A.permute(_dev(gpu, rperm), _dev(gpu, cperm))
    got = _download(B)[2].view(np.uint32)
    assert np.sum(got == 0x7FC01234) == np.sum(bits == 0x7FC01234) and np.sum(got == 0x80000000) == np.sum(bits == 0x80000000)
    B.close()
    A.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_bad_permutation_is_refused_with_its_index(pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    rows, cols, rp, ci, va, rperm, cperm = _case("rectangular")
    A = capi.CsrMatrix.from_host(rows, cols, rp, ci, va)
    st = torch.cuda.current_stream().cuda_stream
    free = []
    for _ in range(3):
        for side, good, n in (("d_row_perm", rperm, rows), ("d_col_perm", cperm, cols)):
            for at, value, index in ((5, int(good[2]), 5), (0, -1, 0), (0, n, 0)):
                bad = good.copy()
                bad[at] = value
                d_bad = _dev(gpu, bad)
                for flags in (0, capi.PERMUTE_VIA_TRANSPOSE):
                    out = C.c_void_p(77)
                    args = (d_bad.data_ptr(), None) if side == "d_row_perm" else (None, d_bad.data_ptr())
                    assert lib.spmv_csr_permute(A._h, *args, flags, st, C.byref(out)) == capi.ERR_INVALID
                    msg = lib.spmv_last_error().decode()
                    assert msg.startswith(f"spmv_csr_permute: {side} is no permutation") and f"index {index} " in msg, msg
                    assert out.value == 77, "*out is untouched"
        out = C.c_void_p(77)
        assert lib.spmv_csr_permute(A._h, None, None, 4, st, C.byref(out)) == capi.ERR_INVALID
        assert lib.spmv_last_error().decode().startswith("spmv_csr_permute: flags = 0x4")
        assert lib.spmv_csr_permute(A._h, None, None, 0, st, None) == capi.ERR_INVALID
        assert out.value == 77
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    A.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_values_and_gather_in_a_replayed_graph(pkg, gpu):
    import torch
    capi = pkg.capi
    rows, cols, rp, ci, va, rperm, cperm = _case("rectangular")
    t = (_dev(gpu, rp, np.int32), _dev(gpu, ci, np.int32), _dev(gpu, va, f32))
    A = capi.CsrMatrix.from_device(rows, cols, *t)
    B = A.permute(_dev(gpu, rperm), _dev(gpu, cperm), keep_map=True)
    bmap = K.permute(rp, ci, va, rperm, cperm, cols=cols)[3]
    src = torch.zeros((2, ci.size), dtype=torch.int32, device=gpu)
    dst = torch.full((2, ci.size), -1, dtype=torch.int32, device=gpu)
    rng = np.random.default_rng(42)

    def rewrite():
        nv = rng.standard_normal(va.size).astype(f32)
        nv.view(np.uint32)[3] = 0x7FC00077
        ns = rng.integers(-2 ** 31, 2 ** 31 - 1, (2, ci.size)).astype(np.int32)
        t[2].copy_(_dev(gpu, nv))
        src.copy_(_dev(gpu, ns))
        return nv, ns

    nv, ns = rewrite()
    B.permute_values(A)
    B.permute_gather(src, dst)
    assert np.array_equal(_download(B)[2].view(np.uint32), nv[bmap].view(np.uint32))
    assert np.array_equal(dst.cpu().numpy(), ns[:, bmap])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        B.permute_values(A)
        B.permute_gather(src, dst)
    nv, ns = rewrite()
    dst.fill_(-1)
    g.replay()
    assert np.array_equal(_download(B)[2].view(np.uint32), nv[bmap].view(np.uint32)), "from a replayed graph"
    assert np.array_equal(dst.cpu().numpy(), ns[:, bmap])
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info()[0]]
    for _ in range(3):
        B.permute_values(A)
        B.permute_gather(src, dst)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert max(abs(f - free[0]) for f in free[1:]) <= 2 * MIB, f"free device memory per round: {free}"
    B.close()
    A.close()


@pytest.mark.gpu
def test_permute_vector_there_and_back(pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    n = 5003
    perm = np.random.default_rng(43).permutation(n).astype(np.int32)
    v = np.random.default_rng(44).standard_normal(n).astype(f32)
    v.view(np.uint32)[7] = 0x7FC00055
    v[8] = f32(-0.0)
    d_p, d_v = _dev(gpu, perm), _dev(gpu, v)
    fwd = capi.permute_vector(d_p, d_v)
    assert np.array_equal(fwd.cpu().numpy().view(np.uint32), v[perm].view(np.uint32))
    back = capi.permute_vector(d_p, fwd, inverse=True)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), v.view(np.uint32))
    inv = torch.full((n,), 9.0, device=gpu)
    capi.permute_vector(d_p, d_v, inv, inverse=True)
    want = np.empty(n, f32)
    want[perm] = v
    assert np.array_equal(inv.cpu().numpy().view(np.uint32), want.view(np.uint32))
    st = torch.cuda.current_stream().cuda_stream
    poisoned = torch.full((n,), 9.0, device=gpu)
    for src, dst in ((d_v.data_ptr(), d_v.data_ptr()), (poisoned.data_ptr(), poisoned.data_ptr() + 4 * (n // 2))):
        assert lib.spmv_permute_vector(d_p.data_ptr(), n - n // 2, 0, src, dst, st) == capi.ERR_INVALID
        assert lib.spmv_last_error().decode().startswith("spmv_permute_vector: src and dst overlap")
    assert lib.spmv_permute_vector(d_p.data_ptr(), n, 2, d_v.data_ptr(), poisoned.data_ptr(), st) == capi.ERR_INVALID
    assert torch.all(poisoned == 9.0)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_map_per_handle(pkg, gpu):
    import torch
    capi = pkg.capi
    lib = capi.lib()
    n, rp, ci, va = G.generic_case()
    A = capi.CsrMatrix.from_host(n, n, rp, ci, va)
    perm = _dev(gpu, np.random.default_rng(45).permutation(n).astype(np.int32))
    B, bare, Tr = A.permute(perm, perm, keep_map=True), A.permute(perm, perm), A.transpose(keep_map=True)
    wide = capi.CsrMatrix.from_host(4, 5, np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros(0, f32))
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(ci.size, device=gpu)
    before = _download(B)[2].copy()

    def refused(rc, start):
        assert rc == capi.ERR_INVALID, start
        msg = lib.spmv_last_error().decode()
        assert msg.startswith(start), msg

    p = buf.data_ptr()
    refused(lib.spmv_csr_transpose_values(B._h, A._h, st), "spmv_csr_transpose_values: the handle has no map")
    refused(lib.spmv_csr_transpose_gather(B._h, 1, p, 0, p, 0, st), "spmv_csr_transpose_gather: the handle has no map")
    refused(lib.spmv_csr_select_values(B._h, A._h, st), "spmv_csr_select_values: the handle has no map")
    refused(lib.spmv_csr_select_gather(B._h, 1, p, 0, p, 0, st), "spmv_csr_select_gather: the handle has no map")
    refused(lib.spmv_csr_spgemm_values(B._h, A._h, A._h, st), "spmv_csr_spgemm_values: the handle has no plan")
    refused(lib.spmv_csr_add_values(B._h, A._h, A._h, 1.0, 1.0, st), "spmv_csr_add_values: the handle has no plan")
    refused(lib.spmv_csr_ilu0_values(B._h, A._h, st), "spmv_csr_ilu0_values: the handle is no factor handle")
    for h in (A, bare, Tr):
        refused(lib.spmv_csr_permute_values(h._h, A._h, st), "spmv_csr_permute_values: the handle has no map")
        refused(lib.spmv_csr_permute_gather(h._h, 1, p, 0, p, 0, st), "spmv_csr_permute_gather: the handle has no map")
        assert h.permute_map_bytes() == 0
    refused(lib.spmv_csr_permute_values(B._h, B._h, st), "spmv_csr_permute_values: a is b itself")
    refused(lib.spmv_csr_permute_values(B._h, None, st), "spmv_csr_permute_values: null argument")
    refused(lib.spmv_csr_permute_values(B._h, wide._h, st), "spmv_csr_permute_values: a is 4 x 5")
    refused(lib.spmv_csr_permute_gather(B._h, 0, p, 0, p, 0, st), "spmv_csr_permute_gather: count = 0")
    refused(lib.spmv_csr_permute_gather(B._h, 1, None, 0, p, 0, st), "spmv_csr_permute_gather: null array")
    refused(lib.spmv_csr_permute_gather(B._h, 1, p + 2, 0, p, 0, st), "spmv_csr_permute_gather: src and dst must be 4-byte aligned")
    refused(lib.spmv_csr_permute_gather(B._h, 1, p, -1, p, 0, st), "spmv_csr_permute_gather: src_stride = -1")
    refused(lib.spmv_csr_permute_gather(B._h, 2, p, 0, p, ci.size - 1, st), "spmv_csr_permute_gather: dst_stride")
    torch.cuda.synchronize()
    assert np.array_equal(_download(B)[2].view(np.uint32), before.view(np.uint32)) and torch.all(buf == 0)
    for h in (B, bare, Tr, wide, A):
        h.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_permuted_handle_runs_through_scalar(pkg, gpu, oracle):
    import torch
    capi = pkg.capi
    n, rp, ci, va = G.generic_case()
    A = capi.CsrMatrix.from_host(n, n, rp, ci, va)
    perm = np.random.default_rng(46).permutation(n).astype(np.int32)
    d_p = _dev(gpu, perm)
    x = np.random.default_rng(47).standard_normal(n).astype(f32)
    d_x = _dev(gpu, x)
    y_a = torch.empty(n, device=gpu)
    A.plan(capi.SCALAR)
    A.run(capi.SCALAR, d_x, y_a)
    # rows only: every row keeps its terms in their order, so B x is the permuted A x exactly
    B = A.permute(d_p, None)
    B.plan(capi.SCALAR)
    y_b = torch.empty(n, device=gpu)
    B.run(capi.SCALAR, d_x, y_b)
    assert T.same(y_b.cpu().numpy(), y_a.cpu().numpy()[perm]) is None
    # rows and columns: the same terms in another order -- the serial chain on B's own arrays, with x permuted too
    P = A.permute(d_p, d_p)
    P.plan(capi.SCALAR)
    brp, bci, bva, _ = K.permute(rp, ci, va, perm, perm)
    d_px = capi.permute_vector(d_p, d_x)
    P.run(capi.SCALAR, d_px, y_b)
    assert T.same(y_b.cpu().numpy(), oracle.spmv(brp, bci, bva, x[perm])) is None
    for h in (B, P, A):
        h.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tester_executable_colours_permutes_and_factors_a_file(pkg, gpu, tmp_path):
    import subprocess
    n, rp, ci, va = G.stencil_case(pkg, 8)
    with open(tmp_path / "A.mtx", "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{n} {n} {ci.size}\n")
        row = np.repeat(np.arange(n), np.diff(rp))
        for r, c, v in zip(row, ci, va):
            f.write(f"{r + 1} {c + 1} {float(v)!r}\n")
    out = tmp_path / "B.mtx"
    run = subprocess.run([str(pkg.capi.TESTER_PATH), "--mtx", str(tmp_path / "A.mtx"), "--color", "--seed", "0", "--ilu0", "--out", str(out)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    col, perm, cp, info = K.color(rp, ci, 0)
    assert f"colors={info['colors']} rounds={info['rounds']}" in run.stdout, run.stdout
    brp, bci, bva, _ = K.permute(rp, ci, va, perm, perm)
    assert f"levels lower={K.depth(brp, bci, 'lower')} upper={K.depth(brp, bci, 'upper')}" in run.stdout, run.stdout
    assert "color check ok" in run.stdout and out.exists()
