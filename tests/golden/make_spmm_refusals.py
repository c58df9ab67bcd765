#!/usr/bin/env python3
"""Record tests/golden/spmm_refusals.json: what the six SpMM / SDDMM run calls and spmv_csr_spmm_plan_cols answer to a bad
argument.

Needs a device and the built library.  The golden is recorded ONCE, from the commit before the one that merged the argument
checks of the six run calls into one description, and is never re-recorded from a later tree:
tests/test_gpu_spmm_refusals.py replays the same cases and holds the library to every status and every spmv_last_error
text, so the order in which the checks fire is pinned too.  Usage:  python tests/golden/make_spmm_refusals.py

The setup is as small as a refusal allows (a refused call launches nothing): make_attention_refusals.py's pattern of 8 x 8
with 20 nonzeros in three handles, one never planned, one with spmm_plan only, one with spmm_plan_cols(130).  The narrow and
_16 calls run at k = 8, ld = 8 on the handle with the narrow plan, the _cols calls at k = 130, ld = 136 on the third.  The
calls that take a dtype are recorded at two of them each (CALLS), since the alignment and the byte-offset bound follow it.
Per call, every single corruption of corruptions() (what the call's checks can see) and every pair of them on different
arguments.  Everything goes through raw ctypes, below the Python wrappers' own checks.  The file's encoding is
make_attention_refusals.py's.
"""
import itertools
import sys
from pathlib import Path

import make_attention_refusals as A

HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "spmm_refusals.json"

N, NNZ, K, LD, K_COLS, LD_COLS, MAX_K_COLS = A.N, 20, 8, 8, 130, 136, 65536
INT64_MAX = 2 ** 63 - 1
# key -> (C call after "spmv_csr_", product, column tiles, dtype argument or None for the fp32-only calls)
CALLS = {
    "spmm": ("spmm", "spmm", False, None), "sddmm": ("sddmm", "sddmm", False, None),
    "spmm_16/bf16": ("spmm_16", "spmm", False, 1), "sddmm_16/fp16": ("sddmm_16", "sddmm", False, 2),
    "spmm_cols/fp32": ("spmm_cols", "spmm", True, 0), "spmm_cols/fp16": ("spmm_cols", "spmm", True, 2),
    "sddmm_cols/fp32": ("sddmm_cols", "sddmm", True, 0), "sddmm_cols/bf16": ("sddmm_cols", "sddmm", True, 1),
    "spmm_plan_cols": ("spmm_plan_cols", "plan", True, None),
}
MATRICES = {"spmm": ("X", "Y"), "sddmm": ("U", "X")}       # in C argument order, each as (pointer, ld); SDDMM's `out` follows


def prefix(key):
    return "spmv_csr_" + CALLS[key][0]


def good(key):
    """The arguments of an accepted call, flat: what a corruption replaces entries of.  A pointer is a byte offset from its
    buffer, or None for a null pointer."""
    _, product, cols, dtype = CALLS[key]
    if product == "plan":
        return dict(h="cols", k_max=K_COLS)
    st = dict(h="cols" if cols else "narrow", k=K_COLS if cols else K)
    if dtype is not None:
        st["dtype"] = dtype
    for m in MATRICES[product]:
        st["p." + m], st["ld." + m] = 0, LD_COLS if cols else LD
    if product == "sddmm":
        st["p.out"] = 0
    return st


def corruptions(key):
    """[(name, argument, {entry: value})]: every one alone makes the call a refusal."""
    name, product, cols, dtype = CALLS[key]
    out = [("h=null", "h", dict(h=None))]
    if product == "plan":
        return out + [(f"k_max={v}", "k_max", dict(k_max=v)) for v in (0, -3, MAX_K_COLS + 1)]
    out.append(("unplanned", "h", dict(h="unplanned")))
    if cols:
        out.append(("narrow-plan", "h", dict(h="narrow")))
    if dtype is not None:
        out += [(f"dtype={v}", "dtype", dict(dtype=v)) for v in (-1, 3) + ((0,) if name.endswith("_16") else ())]
    a, b = MATRICES[product]
    k, es = good(key)["k"], 2 if dtype else 4
    wide = MAX_K_COLS + 1 if cols else 65
    out += [("k=0", "k", dict(k=0)), (f"k={wide}", "k", {"k": wide, "ld." + a: wide, "ld." + b: wide})]
    if cols:
        out.append((f"k={K_COLS + 1}", "k", dict(k=K_COLS + 1)))          # (beyond the plan; ld 136 still holds it)
    for m in (a, b):
        out += [(f"ld{m}<k", "ld." + m, {"ld." + m: k - 1}), (f"ld{m}>max", "ld." + m, {"ld." + m: INT64_MAX // es // N + 1}),
                (f"{m}=null", "p." + m, {"p." + m: None}), (f"{m}+1", "p." + m, {"p." + m: es}), (f"{m}+2", "p." + m, {"p." + m: 2 * es})]
    if product == "sddmm":
        out += [("out=null", "p.out", {"p.out": None}), ("out+2B", "p.out", {"p.out": 2})]
    return out


def cases(key):
    """[(case name, {entry: value})]: the single corruptions, then every pair on two different arguments (the second's
    entries over the first's)."""
    one = corruptions(key)
    out = [(n, c) for n, _, c in one]
    for (n0, a0, c0), (n1, a1, c1) in itertools.combinations(one, 2):
        if a0 != a1:
            out.append((n0 + " " + n1, dict(c0, **c1)))
    return out


class Fixture:
    """The handles and the device buffers of the setup; invoke() makes one raw call."""

    def __init__(self, capi, dev):
        import torch
        self.capi, self.lib, self.torch = capi, capi.lib(), torch
        rp, ci = A.pattern()
        assert len(ci) == NNZ
        self.keep = (torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev), torch.ones(NNZ, dtype=torch.float32, device=dev))
        self.handles = {state: capi.CsrMatrix.from_device(N, N, *self.keep) for state in ("unplanned", "narrow", "cols")}
        self.handles["narrow"].spmm_plan()
        self.handles["cols"].spmm_plan_cols(K_COLS)
        # (a row more than the matrices have: a pointer moved by two elements still points into its buffer)
        kinds = {None: torch.float32, 0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
        self.ins = {d: torch.ones((N + 1, LD_COLS), dtype=t, device=dev) for d, t in kinds.items()}
        self.outs = {d: torch.full((N + 1, LD_COLS), float("nan"), dtype=t, device=dev) for d, t in kinds.items()}
        self.outs["out"] = torch.full((NNZ + 1,), float("nan"), dtype=torch.float32, device=dev)
        self.stream = capi._stream_handle()

    def output(self, key):
        """The buffer that an accepted call of `key` writes (None: spmm_plan_cols writes none)."""
        _, product, _, dtype = CALLS[key]
        return {"spmm": self.outs[dtype], "sddmm": self.outs["out"], "plan": None}[product]

    def invoke(self, key, changes=()):
        """(status, spmv_last_error text) of the call of `key` on good(key) with `changes` applied."""
        name, product, _, dtype = CALLS[key]
        st = dict(good(key), **dict(changes))
        at = lambda buf, off: None if off is None else buf.data_ptr() + off       # noqa: E731
        args = [None if st["h"] is None else self.handles[st["h"]]._h]
        if product == "plan":
            args.append(st["k_max"])
        else:
            args += ([st["dtype"]] if dtype is not None else []) + [st["k"]]
            for m in MATRICES[product]:
                args += [at(self.outs[dtype] if m == "Y" else self.ins[dtype], st["p." + m]), st["ld." + m]]
            if product == "sddmm":
                args.append(at(self.outs["out"], st["p.out"]))
        status = getattr(self.lib, "spmv_csr_" + name)(*args, self.stream)
        return status, (self.lib.spmv_last_error().decode() if status != self.capi.OK else "")

    def outputs_untouched(self):
        self.torch.cuda.synchronize()
        return all(bool(self.torch.isnan(t).all()) for t in self.outs.values())

    def accepted_calls_write(self):
        """Every uncorrupted call is accepted, and each run call writes to its output."""
        for key in CALLS:
            status, text = self.invoke(key)
            assert status == self.capi.OK, f"{prefix(key)} refused the uncorrupted call: {text}"
            self.torch.cuda.synchronize()
            out = self.output(key)
            if out is not None:
                assert not bool(self.torch.isnan(out).all()), f"the accepted {prefix(key)} wrote nothing"
                out.fill_(float("nan"))

    def close(self):
        for a in self.handles.values():
            a.close()


def read_golden():
    return A.read_golden(GOLDEN, prefix, {key: [n for n, _ in cases(key)] for key in CALLS})


def main():
    sys.path.insert(0, str(HERE.parent.parent))
    import __graft_entry__ as ge
    import torch
    capi = ge.load_package().capi
    fx = Fixture(capi, torch.device("cuda:0"))
    results = {}
    for key in CALLS:
        rec = results[key] = {}
        for name, changes in cases(key):
            rec[name] = fx.invoke(key, changes)
            assert rec[name][0] != capi.OK, f"{prefix(key)} accepted {name}"
    assert fx.outputs_untouched(), "a refused call wrote to an output"
    fx.accepted_calls_write()
    fx.close()
    A.write_golden(results, GOLDEN, prefix)
    print(f"{GOLDEN.name}: {sum(len(r) for r in results.values())} cases, {GOLDEN.stat().st_size} bytes")


if __name__ == "__main__":
    main()
