"""The row sums of SPMV_TILED and SPMV_ADAPTIVE on the device against the numpy statement of their order
(tests/_tiled_order.py), bit for bit and row for row: raw uint32 views, no tolerance, no row left out.

How the kernels issue their LDS reads (one word or a batch ahead of the adds, a tree through the LDS crossbar or through DPP
row shifts) must not show in y: the order of every addition is fixed.  The values are general fp32 numbers of mixed exponents
and signs, so another order changes the low bits (tests/test_tiled_order_host.py shows that on these very problems).

Two problems per workgroup size (tests/_tiled_order.py, Problem):
  lengths  rows of 0, 1, 15..18, 31..33 nonzeros, of 16 B - 1 .. 16 B + 1 and twice that for the long loop's batch B = 4, and of
           511..513, 575..577, 639..641, each at every phase 0..33 of the pad words;
  chunks   a row that fills a chunk, heads of every class, a two-term fix-up, chunks in which block - 1, block, block + 1 and
           2 block + 3 rows of 1..8 nonzeros begin (the second and third trip over a chunk's segments; also moved by 1 and
           33 words), more 16-lane segments than one round of groups takes and fewer, rows whose products are all -0.0 and
           rows that hold +Inf or -Inf beside finite rows, and a ragged last chunk.
Each runs at SPMV_TILED_BLOCK = 256, 512 and 1024 through the 16-bit body, the 32-bit body (SPMV_COL16=0), the sorted body
(SPMV_SORTED_FROM=1 with SPMV_BLOCKS=0), the 16-bit body over block lists (SPMV_SORTED_FROM=1), SPMV_ADAPTIVE and the
persistent form of the 32-bit body (SPMV_PERSIST=1).
"""
import re

import numpy as np
import pytest

import _tiled_order as TO

pytestmark = pytest.mark.gpu

MODES = {
    # name: (variant, environment, what plan_describe must say: field -> "most" (all but the ragged last chunk) | "none")
    "col16": ("tiled", {"SPMV_SORTED_FROM": "0"}, {"col16_chunks": "most", "sorted_chunks": "none"}),
    "col32": ("tiled", {"SPMV_COL16": "0", "SPMV_SORTED_FROM": "0"}, {"col16_chunks": "none", "sorted_chunks": "none"}),
    # (a chunk marked for the sorted body takes a block list first where its columns allow one, unless SPMV_BLOCKS=0)
    "sorted": ("tiled", {"SPMV_SORTED_FROM": "1", "SPMV_BLOCKS": "0"}, {"sorted_chunks": "most"}),
    "blocks": ("tiled", {"SPMV_SORTED_FROM": "1"}, {"block_list_chunks": "most"}),
    "adaptive": ("adaptive", {}, {}),
    # (the persistent 32-bit body: resident workgroups that walk their XCD's chunks, the row sums one word at a time)
    "persist": ("tiled", {"SPMV_PERSIST": "1"}, {"col16_chunks": "none", "sorted_chunks": "none"}),
}


def _field(plan, name):
    m = re.search(rf"\b{name}=(\d+)", plan)
    assert m, (name, plan)
    return int(m.group(1))


@pytest.fixture(scope="module")
def device_problem(pkg, gpu):
    """The device copy of a problem, made once per (case, block)."""
    import torch
    made = {}

    def get(case, block):
        if (case, block) not in made:
            P = TO.problem(case, block)
            made[case, block] = (P, [torch.from_numpy(a).to(gpu) for a in (P.rp, P.ci, P.va, P.x)])
        return made[case, block]
    return get


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("block", [256, 512, 1024])
@pytest.mark.parametrize("case", TO.CASES)
def test_row_sums_have_the_documented_order(pkg, gpu, device_problem, monkeypatch, case, block, mode):
    import torch
    capi = pkg.capi
    vname, env, says = MODES[mode]
    for k in ("SPMV_TILED_BLOCK", "SPMV_COL16", "SPMV_SORTED_FROM", "SPMV_PERSIST", "SPMV_MAXPASS", "SPMV_AUTOTUNE", "SPMV_BLOCKS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SPMV_TILED_BLOCK", str(block))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    P, (d_rp, d_ci, d_va, d_x) = device_problem(case, block)
    v = capi.VARIANTS[vname]
    A = capi.CsrMatrix.from_device(P.rows, P.cols, d_rp, d_ci, d_va)
    try:
        A.plan(v)
        plan = A.plan_describe(v)
        run_block = _field(plan, "block")
        if vname == "tiled":
            assert run_block == block, plan
        chunks = _field(plan, "chunks")
        assert chunks == -(-P.nnz // (16 * run_block)), plan
        for name, how in says.items():
            n = _field(plan, name)
            # (the ragged last chunk always takes the 32-bit body)
            assert (n == 0) if how == "none" else (n >= chunks - 1), (name, how, plan)
        if mode == "persist":
            assert _field(plan, "persist") == 1, plan
        y = torch.full((P.rows,), float("nan"), dtype=torch.float32, device=gpu)
        A.run(v, d_x, y)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
    finally:
        A.close()
    want, _, classes = P.want(16 * run_block)
    print(f"{case} block={run_block} {mode}: {P.rows} rows, {P.nnz} nonzeros, short/16-lane/wavefront segments {classes}; {plan}")
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (f"{bad.size} of {P.rows} rows differ from the documented order in a bit; first rows {bad[:6]} of lengths "
                           f"{[P.lengths[b] for b in bad[:6]]}: {got[bad[:6]]} against {want[bad[:6]]}")
