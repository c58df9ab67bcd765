#!/usr/bin/env python3
"""Record tests/golden/map_refusals.json: what the companions of the derived handles answer to a bad argument -- the five
strided moves (spmv_csr_transpose_gather, _select_gather, _select_scatter, _add_gather, _permute_gather), the five refreshes
(_transpose_values, _select_values, _permute_values, _spgemm_values, _add_values) and the five _map_bytes / _plan_bytes.

Needs a device and the built library.  The golden is recorded ONCE, from the commit before the one that put the handle's
position map into one struct and the argument checks of these calls into one function each, and is never re-recorded from a
later tree: tests/test_gpu_map_refusals.py replays the same cases and holds the library to every status and every
spmv_last_error text, so the order in which the checks fire is pinned too.  Usage:  python tests/golden/make_map_refusals.py

The setup is as small as a refusal allows (a refused call launches nothing): make_attention_refusals.py's pattern of 8 x 8
with 20 nonzeros as A, a second 8 x 8 pattern with 18 as A2, and HANDLES: T = A^T, S = A's top 2 per row, B = A permuted (by
the direct route, Bt through the transposes), Cadd = A + A2, Cmul = A A2, each with its map or plan and again without
(the names that end in 0), and R, 4 x 5, for the shapes.  Per call, every single corruption of corruptions() (what the call's
checks can see: every handle of another maker among them) and every pair of them on different arguments.  A _bytes call has
one argument: it is asked about every handle, and a count of bytes is recorded as (count, the call's name).  Everything goes
through raw ctypes, below the Python wrappers' own checks.  The file's encoding is make_attention_refusals.py's.

What is not recorded: the wrong-current-device refusal (it needs a second device) and spmv_csr_permute_values' null-d_vals
refusal (no entry point makes a handle with nonzeros and no values).
"""
import itertools
import sys
from pathlib import Path

import numpy as np

import make_attention_refusals as A

HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "map_refusals.json"

N, COUNT, PAD = A.N, 2, 3
INT64_MAX = 2 ** 63 - 1
POISON = -0x21524111                               # 0xdeadbeef as int32
HANDLES = ("A", "A2", "T", "T0", "S", "S0", "B", "B0", "Bt", "Bt0", "Cadd", "Cadd0", "Cmul", "Cmul0", "R")
ROW_PERM = np.array([3, 0, 7, 1, 6, 2, 5, 4], np.int32)
COL_PERM = np.array([5, 2, 0, 7, 4, 1, 6, 3], np.int32)
ALPHA, BETA = 2.0, 3.0
# key -> (kind, the handle of the accepted call, the handles the call accepts at all, side of add_gather)
CALLS = {
    "transpose_gather": ("move", "T", ("T",), None), "select_gather": ("move", "S", ("S",), None),
    "select_scatter": ("move", "S", ("S",), None), "add_gather/a": ("move", "Cadd", ("Cadd",), 0),
    "add_gather/b": ("move", "Cadd", ("Cadd",), 1), "permute_gather": ("move", "B", ("B", "Bt"), None),
    "permute_gather/via": ("move", "Bt", ("B", "Bt"), None),
    "transpose_values": ("values", "T", ("T",), None), "select_values": ("values", "S", ("S",), None),
    "permute_values": ("values", "B", ("B", "Bt"), None), "permute_values/via": ("values", "Bt", ("B", "Bt"), None),
    "spgemm_values": ("values2", "Cmul", ("Cmul",), None), "add_values": ("values2", "Cadd", ("Cadd",), None),
    "transpose_map_bytes": ("bytes", None, (), None), "select_map_bytes": ("bytes", None, (), None),
    "permute_map_bytes": ("bytes", None, (), None), "spgemm_plan_bytes": ("bytes", None, (), None),
    "add_plan_bytes": ("bytes", None, (), None),
}


def prefix(key):
    return "spmv_csr_" + key.split("/")[0]


def patterns():
    """{name: (rows, cols, row_ptr, col_idx, vals)} of A, A2 and R; the values are small distinct integers."""
    out = {}
    rp, ci = A.pattern()
    out["A"] = (N, N, rp, ci, np.arange(1, len(ci) + 1, dtype=np.float32))
    for name, rows, cols, lengths, seed in (("A2", N, N, [2, 3, 0, 4, 1, 3, 2, 3], 6), ("R", 4, 5, [2, 0, 3, 1], 7)):
        rng = np.random.Generator(np.random.PCG64(seed))
        ci = np.concatenate([np.sort(rng.choice(cols, size=n, replace=False)) for n in lengths]).astype(np.int32)
        rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        out[name] = (rows, cols, rp, ci, np.arange(2, len(ci) + 2, dtype=np.float32))
    return out


def dense(rows, cols, rp, ci, va):
    d = np.zeros((rows, cols), np.float64)
    for r in range(rows):
        d[r, ci[rp[r]:rp[r + 1]]] = va[rp[r]:rp[r + 1]]
    return d


def expected_maps():
    """What the makers must have built, from numpy alone: {handle: positions of A per entry of the handle}, and for Cadd
    {"Cadd/a": [(entry of C, position of A)], "Cadd/b": the same for A2}."""
    p = patterns()
    _, _, rp, ci, va = p["A"]
    maps = {"T": np.argsort(ci, kind="stable")}
    keep = []
    for r in range(N):
        pos = np.arange(rp[r], rp[r + 1])
        keep += sorted(pos[np.argsort(-va[pos], kind="stable")[:2]])
    maps["S"] = np.array(keep, np.int64)
    inv_col = np.argsort(COL_PERM)
    order = []
    for r in range(N):
        pos = np.arange(rp[ROW_PERM[r]], rp[ROW_PERM[r] + 1])
        order += list(pos[np.argsort(inv_col[ci[pos]], kind="stable")])
    maps["B"] = maps["Bt"] = np.array(order, np.int64)
    _, _, rp2, ci2, _ = p["A2"]
    e, ta, tb = 0, [], []
    for r in range(N):
        ca, cb = list(ci[rp[r]:rp[r + 1]]), list(ci2[rp2[r]:rp2[r + 1]])
        for c in sorted(set(ca) | set(cb)):
            if c in ca:
                ta.append((e, rp[r] + ca.index(c)))
            if c in cb:
                tb.append((e, rp2[r] + cb.index(c)))
            e += 1
    maps["Cadd/a"], maps["Cadd/b"], maps["Cadd/nnz"] = ta, tb, e
    return maps


def sizes(key, nnz):
    """(words of one src array, words of one dst array) of a move; nnz: {handle: nnz}."""
    return {"transpose_gather": (nnz["A"], nnz["T"]), "select_gather": (nnz["A"], nnz["S"]), "select_scatter": (nnz["S"], nnz["A"]),
            "add_gather/a": (nnz["Cadd"], nnz["A"]), "add_gather/b": (nnz["Cadd"], nnz["A2"]),
            "permute_gather": (nnz["A"], nnz["B"]), "permute_gather/via": (nnz["A"], nnz["Bt"])}[key]


def good(key, nnz):
    """The arguments of an accepted call, flat: what a corruption replaces entries of.  A pointer is a byte offset from its
    buffer, or None for a null pointer; a handle is a name of HANDLES, None, or "self" (the call's first handle)."""
    kind, h, _, side = CALLS[key]
    if kind == "move":
        n_src, n_dst = sizes(key, nnz)
        st = dict(h=h, count=COUNT, src=0, src_stride=n_src + PAD, dst=0, dst_stride=n_dst + PAD)
        if side is not None:
            st["side"] = side
        return st
    if kind == "values":
        return dict(h=h, a="A")
    if kind == "values2":
        return dict(h=h, a="A", b="A2")
    return dict(h="A")


def corruptions(key, nnz):
    """[(name, argument, value)]: every one alone makes the call a refusal (a _bytes call: an answer)."""
    kind, h, accepted, side = CALLS[key]
    if kind == "bytes":
        return [("h=null", "h", None)] + [(f"h={x}", "h", x) for x in HANDLES]
    out = [("h=null", "h", None)] + [(f"h={x}", "h", x) for x in HANDLES if x not in accepted]
    if kind == "move":
        _, n_dst = sizes(key, nnz)
        big = INT64_MAX // 4 // COUNT + 1
        if side is not None:
            out += [("side=-1", "side", -1), ("side=2", "side", 2)]
        out += [("count=0", "count", 0), ("count=-1", "count", -1), ("src=null", "src", None), ("src+2B", "src", 2),
                ("dst=null", "dst", None), ("dst+2B", "dst", 2), ("src_stride=-1", "src_stride", -1), ("src_stride>max", "src_stride", big),
                ("dst_stride=-1", "dst_stride", -1), ("dst_stride>max", "dst_stride", big), ("dst_stride<n", "dst_stride", n_dst - 1)]
        return out
    # a parent: null, the handle itself, another shape, the right shape with other nonzeros
    out += [("a=null", "a", None), ("a=self", "a", "self"), ("a=R", "a", "R"), ("a=A2", "a", "A2")]
    if kind == "values2":
        out += [("b=null", "b", None), ("b=self", "b", "self"), ("b=R", "b", "R"), ("b=A", "b", "A")]
    return out


def cases(key, nnz):
    """[(case name, {argument: value})]: the single corruptions, then every pair on two different arguments."""
    one = corruptions(key, nnz)
    out = [(n, {a: v}) for n, a, v in one]
    if CALLS[key][0] != "bytes":
        for (n0, a0, v0), (n1, a1, v1) in itertools.combinations(one, 2):
            if a0 != a1:
                out.append((n0 + " " + n1, {a0: v0, a1: v1}))
    return out


class Fixture:
    """The handles and the device buffers of the setup; invoke() makes one raw call."""

    def __init__(self, capi, dev):
        import torch
        self.capi, self.lib, self.torch, self.dev = capi, capi.lib(), torch, dev
        self.host = patterns()
        self.arrays = {k: tuple(torch.from_numpy(x).to(dev) for x in v[2:]) for k, v in self.host.items()}
        H = self.handles = {k: capi.CsrMatrix.from_device(v[0], v[1], *self.arrays[k]) for k, v in self.host.items()}
        rperm, cperm = torch.from_numpy(ROW_PERM).to(dev), torch.from_numpy(COL_PERM).to(dev)
        for z, keep in (("", True), ("0", False)):
            H["T" + z] = H["A"].transpose(keep_map=keep)
            H["S" + z] = H["A"].select_topk(2, keep_map=keep)
            H["B" + z] = H["A"].permute(rperm, cperm, keep_map=keep)
            H["Bt" + z] = H["A"].permute(rperm, cperm, keep_map=keep, via_transpose=True)
            H["Cadd" + z] = H["A"].add(H["A2"], keep_plan=keep)           # (1 A + 1 A2: the refresh changes the values)
            H["Cmul" + z] = H["A"].spgemm(H["A2"], keep_plan=keep)
        assert sorted(H) == sorted(HANDLES)
        self.nnz = {k: h.nnz for k, h in H.items()}
        words = COUNT * (max(self.nnz.values()) + PAD) + 2 * PAD
        rng = np.random.Generator(np.random.PCG64(11))
        src = rng.integers(0, 2 ** 32, size=words, dtype=np.uint64).astype(np.uint32)
        src[:8] = [0x7fc00001, 0xffc12345, 0x7f800001, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001]
        self.src_host = src.view(np.int32)
        self.src = torch.from_numpy(self.src_host.copy()).to(dev)
        self.dst = torch.full((words,), POISON, dtype=torch.int32, device=dev)
        self.stream = capi._stream_handle()
        self.vals_before = self.own_values()

    def own_values(self):
        self.torch.cuda.synchronize()
        return {k: h.download()[2].view(np.int32).copy() for k, h in self.handles.items()}

    def invoke(self, key, changes=()):
        """(status, spmv_last_error text) of the call of `key` on good(key) with `changes` applied; a _bytes call that
        answers a count: (count, the call's name)."""
        kind, _, _, side = CALLS[key]
        st = dict(good(key, self.nnz), **dict(changes))
        handle = lambda name: None if name is None else self.handles[st["h"] or CALLS[key][1] if name == "self" else name]._h   # noqa: E731
        at = lambda buf, off: None if off is None else buf.data_ptr() + off       # noqa: E731
        fn = getattr(self.lib, prefix(key))
        if kind == "bytes":
            n = fn(handle(st["h"]))
            return (n, prefix(key)) if n >= 0 else (n, self.lib.spmv_last_error().decode())
        args = [handle(st["h"])]
        if kind == "move":
            args += ([st["side"]] if side is not None else []) + [st["count"], at(self.src, st["src"]), st["src_stride"],
                                                                  at(self.dst, st["dst"]), st["dst_stride"]]
        else:
            args.append(handle(st["a"]))
            if kind == "values2":
                args.append(handle(st["b"]))
            if key == "add_values":
                args += [ALPHA, BETA]
        status = fn(*args, self.stream)
        return status, (self.lib.spmv_last_error().decode() if status != self.capi.OK else "")

    def outputs_untouched(self):
        """No refused call wrote: the moves' dst is poison still, and every handle holds the values it held."""
        now = self.own_values()
        return bool((self.dst == POISON).all()) and all(np.array_equal(now[k], v) for k, v in self.vals_before.items())

    def accepted_calls_exact(self):
        """Every uncorrupted call is accepted and writes what numpy says, bit for bit (the moves: dst whole, the words
        between and behind the arrays poison still)."""
        torch, maps = self.torch, expected_maps()
        for key, (kind, h, _, side) in CALLS.items():
            if kind != "move":
                continue
            status, text = self.invoke(key)
            assert status == self.capi.OK, f"{prefix(key)} refused the uncorrupted call: {text}"
            torch.cuda.synchronize()
            n_src, n_dst = sizes(key, self.nnz)
            want = np.full(self.dst.numel(), POISON, np.int32)
            for c in range(COUNT):
                s, d = self.src_host[c * (n_src + PAD):][:n_src], want[c * (n_dst + PAD):][:n_dst]
                if key == "select_scatter":
                    d[maps["S"]] = s
                elif side is not None:
                    for e, p in maps["Cadd/a" if side == 0 else "Cadd/b"]:
                        d[p] = s[e]
                else:
                    d[:] = s[maps[h]]
            got = self.dst.cpu().numpy()
            assert np.array_equal(got, want), f"{key}: dst differs from numpy's at {np.flatnonzero(got != want)[:8]}"
            self.dst.fill_(POISON)
        # the one-parent refreshes: arbitrary words (NaN payloads, -0, infinities among them) through the map
        va = self.arrays["A"][2]
        saved = va.clone()
        words = self.src_host[:self.nnz["A"]]
        va.copy_(torch.from_numpy(words.copy()).to(self.dev).view(torch.float32))
        for key, (kind, h, _, _) in CALLS.items():
            if kind != "values":
                continue
            status, text = self.invoke(key)
            assert status == self.capi.OK, f"{prefix(key)} refused the uncorrupted call: {text}"
            torch.cuda.synchronize()
            got = self.handles[h].download()[2].view(np.int32)
            assert np.array_equal(got, words[maps[h]]), f"{key}: the values differ from numpy's"
        va.copy_(saved)
        # the two-parent refreshes: small integers, exact in any order
        da, db = dense(*self.host["A"]), dense(*self.host["A2"])
        for key, want in (("spgemm_values", da @ db), ("add_values", ALPHA * da + BETA * db)):
            h = self.handles[CALLS[key][1]]
            rp, ci, _ = h.download()
            assert h.nnz == np.count_nonzero(want) and (key != "add_values" or h.nnz == maps["Cadd/nnz"])
            status, text = self.invoke(key)
            assert status == self.capi.OK, f"{prefix(key)} refused the uncorrupted call: {text}"
            torch.cuda.synchronize()
            got = h.download()[2]
            rows = np.repeat(np.arange(h.rows), np.diff(rp))
            assert np.array_equal(got.view(np.int32), want[rows, ci].astype(np.float32).view(np.int32)), f"{key}: the values differ"
        torch.cuda.synchronize()

    def close(self):
        for k in reversed(HANDLES):
            self.handles[k].close()


def read_golden(nnz):
    return A.read_golden(GOLDEN, prefix, {key: [n for n, _ in cases(key, nnz)] for key in CALLS})


def main():
    sys.path.insert(0, str(HERE.parent.parent))
    import __graft_entry__ as ge
    import torch
    capi = ge.load_package().capi
    fx = Fixture(capi, torch.device("cuda:0"))
    results = {}
    for key in CALLS:
        rec = results[key] = {}
        for name, changes in cases(key, fx.nnz):
            rec[name] = fx.invoke(key, changes)
            assert CALLS[key][0] == "bytes" or rec[name][0] != capi.OK, f"{prefix(key)} accepted {name}"
    assert fx.outputs_untouched(), "a refused call wrote to an output"
    fx.accepted_calls_exact()
    fx.close()
    A.write_golden(results, GOLDEN, prefix)
    print(f"{GOLDEN.name}: {sum(len(r) for r in results.values())} cases, {GOLDEN.stat().st_size} bytes")


if __name__ == "__main__":
    main()
