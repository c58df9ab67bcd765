#!/usr/bin/env python3
"""Record tests/golden/attention_refusals.json: what the nine spmv_csr_attention_* calls answer to a bad argument.

Needs a device and the built library.  The golden is recorded ONCE, from the commit before the one that rewrote the
argument checks, and is never re-recorded from a later tree: tests/test_gpu_attention_refusals.py replays the same cases and
holds the library to every status and every spmv_last_error text, so the order in which the checks fire is pinned too.
Usage:  python tests/golden/make_attention_refusals.py

The setup is as small as a refusal allows (a refused call launches nothing): a pattern of 8 queries x 8 keys with 20
nonzeros and its transpose, both planned for 4 heads; k = kv = 8, every ld 8, 4 query heads, group = 2; a second pair of
handles that was never planned.  Per call, every single corruption of corruptions() (what the call's checks can see) and
every pair of them on different arguments.  Everything goes through raw ctypes, below the Python wrappers' own checks.
"""
import ctypes as C
import itertools
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "attention_refusals.json"
PREFIX = "spmv_csr_attention_"

N, W, LD, HEADS, GROUP, SCALE = 8, 8, 8, 4, 2, 0.25
INT64_MAX = 2 ** 63 - 1
# the C argument order of a pass after (handle, [hs], [group], scale, k): a matrix is (pointer, ld), a vector a pointer
PASSES = {
    "forward": dict(transposed=False, order=("Q", "K", "kv", "V", "O", "stats"), outputs=("O", "stats")),
    "backward_q": dict(transposed=False, order=("Q", "K", "kv", "V", "O", "dO", "stats", "delta", "dQ"), outputs=("delta", "dQ")),
    "backward_kv": dict(transposed=True, order=("Q", "K", "kv", "V", "dO", "stats", "delta", "dK", "dV"), outputs=("dK", "dV")),
}
MODES = ("one", "heads", "gqa")
CALLS = [(p, m) for m in MODES for p in PASSES]
VECTORS = {"stats": 2, "delta": 1}          # floats per query; also the unit of the head stride
FIELD = dict(Q="q", K="k", V="v", O="o", dO="d_o", stats="stats", delta="delta", dQ="dq", dK="dk", dV="dv")   # of spmv_attn_heads_t


def call_name(pas, mode):
    return pas + {"one": "", "heads": "_heads", "gqa": "_gqa"}[mode]


def good(pas):
    """The arguments of an accepted call, flat: what a corruption replaces one entry of."""
    st = dict(h="planned", hs="given", heads=HEADS, reserved=0, group=GROUP, scale=SCALE, k=W, kv=W)
    for x in PASSES[pas]["order"]:
        if x == "kv":
            continue
        st["p." + x] = 0                                   # byte offset from the buffer; None: a null pointer
        st["hs." + x] = N * (VECTORS[x] if x in VECTORS else LD)
        if x not in VECTORS:
            st["ld." + x] = LD
    return st


def corruptions(pas, mode):
    """[(name, argument, value)]: every one alone makes the call a refusal."""
    order = [x for x in PASSES[pas]["order"] if x != "kv"]
    out = [("h=null", "h", None), ("unplanned", "h", "unplanned")]
    if mode != "one":
        out += [("hs=null", "hs", None), ("heads=0", "heads", 0), ("heads=65536", "heads", 65536), ("reserved=1", "reserved", 1),
                ("heads=8", "heads", 2 * HEADS)]           # (beyond the plan)
    if mode == "gqa":
        out += [(f"group={g}", "group", g) for g in (0, -1, 3)]
    if mode != "one":
        for x in order:
            unit = VECTORS.get(x, 4)
            out.append((f"hs.{x}<0", "hs." + x, -unit))
            if unit > 1:
                out.append((f"hs.{x}%{unit}", "hs." + x, good(pas)["hs." + x] + unit // 2))
            if x in PASSES[pas]["outputs"]:
                out.append((f"hs.{x}<w", "hs." + x, 0 if x in VECTORS else 4))
        out.append(("hs.Q>max", "hs.Q", INT64_MAX // 4 // HEADS // 4 * 4 + 4))
    out += [("k=0", "k", 0), ("k=65", "k", 65), ("kv=0", "kv", 0), ("kv=65", "kv", 65),
            ("scale=inf", "scale", float("inf")), ("scale=nan", "scale", float("nan"))]
    for x in order:
        if x in VECTORS:
            out += [(f"{x}=null", "p." + x, None), (f"{x}+{VECTORS[x] * 2}", "p." + x, VECTORS[x] * 2)]
        else:
            out += [(f"ld{x}<w", "ld." + x, 4), (f"ld{x}>max", "ld." + x, INT64_MAX // 4 // N + 1),
                    (f"{x}=null", "p." + x, None), (f"{x}+4", "p." + x, 4)]
    return out


def cases(pas, mode):
    """[(case name, {argument: value})]: the single corruptions, then every pair on two different arguments."""
    one = corruptions(pas, mode)
    out = [(n, {a: v}) for n, a, v in one]
    for (n0, a0, v0), (n1, a1, v1) in itertools.combinations(one, 2):
        if a0 != a1:
            out.append((n0 + " " + n1, {a0: v0, a1: v1}))
    return out


def pattern():
    lengths = np.array([3, 0, 4, 2, 3, 1, 4, 3])
    rng = np.random.Generator(np.random.PCG64(5))
    ci = np.concatenate([np.sort(rng.choice(N, size=int(n), replace=False)) for n in lengths]).astype(np.int32)
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), ci


class Fixture:
    """The handles and the device buffers of the setup; invoke() makes one raw call."""

    def __init__(self, capi, dev):
        import torch
        self.capi, self.lib, self.torch = capi, capi.lib(), torch
        rp, ci = pattern()
        self.keep = (torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev), torch.zeros(len(ci), dtype=torch.float32, device=dev))
        self.handles = {}
        for state in ("planned", "unplanned"):
            a = capi.CsrMatrix.from_device(N, N, *self.keep)
            t = a.transpose(keep_map=False)
            if state == "planned":
                a.attention_plan_heads(HEADS)
                t.attention_plan_heads(HEADS)
            self.handles[state] = (a, t)
        shape = lambda x: (HEADS, N, VECTORS[x]) if x in VECTORS else (HEADS, N, LD)       # noqa: E731
        self.ins = {x: torch.ones(shape(x), dtype=torch.float32, device=dev) for x in ("Q", "K", "V", "O", "dO", "stats", "delta")}
        self.outs = {x: torch.full(shape(x), float("nan"), dtype=torch.float32, device=dev) for x in ("O", "stats", "delta", "dQ", "dK", "dV")}
        self.stream = capi._stream_handle()

    def invoke(self, pas, mode, changes=()):
        """(status, spmv_last_error text) of call_name(pas, mode) on good(pas) with `changes` applied."""
        st = dict(good(pas), **dict(changes))
        spec = PASSES[pas]
        args = [None if st["h"] is None else self.handles[st["h"]][spec["transposed"]]._h]
        if mode != "one":
            hs = self.capi.AttnHeads(heads=st["heads"], reserved=st["reserved"],
                                     **{FIELD[x]: st["hs." + x] for x in spec["order"] if x != "kv"})
            args.append(C.byref(hs) if st["hs"] else None)
        if mode == "gqa":
            args.append(st["group"])
        args += [st["scale"], st["k"]]
        for x in spec["order"]:
            if x == "kv":
                args.append(st["kv"])
                continue
            buf = self.outs[x] if x in spec["outputs"] else self.ins[x]
            args.append(None if st["p." + x] is None else buf.data_ptr() + st["p." + x])
            if x not in VECTORS:
                args.append(st["ld." + x])
        args.append(self.stream)
        status = getattr(self.lib, "spmv_csr_attention_" + call_name(pas, mode))(*args)
        return status, (self.lib.spmv_last_error().decode() if status != self.capi.OK else "")

    def outputs_untouched(self):
        self.torch.cuda.synchronize()
        return all(bool(self.torch.isnan(t).all()) for t in self.outs.values())

    def close(self):
        for a, t in self.handles.values():
            t.close()
            a.close()


def write_golden(results, golden=GOLDEN, prefix=lambda call: PREFIX + call):
    """results: {call: {case name: (status, text)}} in the order of CALLS and cases().  The file keeps it whole in little
    space.  "messages": the distinct (status, text), the call's name (prefix(call)) at the start of a text written as "@".
    Per call, "singles": {corruption: message index}; "pairs": a digit per pair of cases() in order, 0 or 1 where the pair
    answers what its first or its second corruption answers alone, 2 where it answers something else, which "others" lists
    by name."""
    messages, calls = [], {}

    def index(call, status, text):
        assert text.startswith(prefix(call)) and "@" not in text
        m = [status, "@" + text[len(prefix(call)):]]
        if m not in messages:
            messages.append(m)
        return messages.index(m)

    for call, rec in results.items():
        single = {n: index(call, *r) for n, r in rec.items() if " " not in n}
        digits, others = "", {}
        for n, r in rec.items():
            if " " in n:
                a, b = n.split(" ")
                digits += "0" if r == rec[a] else "1" if r == rec[b] else "2"
                if digits[-1] == "2":
                    others[n] = index(call, *r)
        calls[call] = dict(singles=single, pairs=[digits[i:i + 120] for i in range(0, len(digits), 120)], others=others)
    body = ",\n".join(f" {json.dumps(c)}: {json.dumps(rec, separators=(',', ':'))}" for c, rec in calls.items())
    rows = ",\n".join(" " + json.dumps(m) for m in messages)
    golden.write_text('{"messages": [\n' + rows + '],\n"calls": {\n' + body + "\n}}\n")
    assert read_golden(golden, prefix, {c: list(rec) for c, rec in results.items()}) == results


def read_golden(golden=GOLDEN, prefix=lambda call: PREFIX + call, names=None):
    """{call: {case name: (status, text)}} of the file, every case spelled out.  names: {call: its case names in order}
    (the nine attention calls' by default)."""
    g = json.loads(golden.read_text())
    names = names or {call_name(pas, mode): [n for n, _ in cases(pas, mode)] for pas, mode in CALLS}
    out = {}
    for call, all_names in names.items():
        rec = g["calls"][call]
        msg = lambda i: (g["messages"][i][0], prefix(call) + g["messages"][i][1][1:])       # noqa: E731
        res = out[call] = {n: msg(i) for n, i in rec["singles"].items()}
        pairs = [n for n in all_names if " " in n]
        digits = "".join(rec["pairs"])
        assert len(digits) == len(pairs)
        for n, d in zip(pairs, digits):
            res[n] = msg(rec["others"][n]) if d == "2" else res[n.split(" ")[int(d)]]
    return out


def main():
    sys.path.insert(0, str(HERE.parent.parent))
    import __graft_entry__ as ge
    import torch
    capi = ge.load_package().capi
    fx = Fixture(capi, torch.device("cuda:0"))
    results = {}
    for pas, mode in CALLS:
        rec = results[call_name(pas, mode)] = {}
        for name, changes in cases(pas, mode):
            rec[name] = fx.invoke(pas, mode, changes)
            assert rec[name][0] != capi.OK, f"{call_name(pas, mode)} accepted {name}"
    assert fx.outputs_untouched(), "a refused call wrote to an output"
    for pas, mode in CALLS:
        status, text = fx.invoke(pas, mode)
        assert status == capi.OK, f"{call_name(pas, mode)} refused the uncorrupted call: {text}"
    torch.cuda.synchronize()
    fx.close()
    write_golden(results)
    print(f"{GOLDEN.name}: {sum(len(r) for r in results.values())} cases, {GOLDEN.stat().st_size} bytes")


if __name__ == "__main__":
    main()
