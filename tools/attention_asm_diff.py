#!/usr/bin/env python3
"""tools/attention_asm_diff.py OLD.s NEW.s [NEW2.s ...] -- do the kernels of two builds of a kernel file have the same code?

Both files are device assembly of one csrc/*.hip file (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S, the Makefile's
other flags), OLD at an earlier commit, NEW at this one.  Where the file has been split since, name every part: OLD is
compared against the union of their kernels, and a kernel must not appear in two of them.  The text of every kernel (from
its .globl line to the next kernel's: the instruction stream, the .amdhsa_ block, the .set lines of its resource counts) is compared after what only
names it is normalised: the kernel's own symbol becomes a placeholder, the function numbers in local labels (.LBB12_3,
.Lfunc_end12) and in the comments that name a loop (Header=BB12_3, Child Loop BB12_5) are dropped: they count the kernels
before this one in the file (so do the blanks that align a label's comment), and the lines that only lead in the next
kernel (.section, .text, its .protected line) or pad the text behind a file's last kernel are left out: which kernel
follows changes when a file is split.

Which kernel of NEW is which of OLD is read off the mangled symbol itself (c++filt does not know every element type): a
k_attn_* kernel is its name, V, VEC, its element type (float where the symbol has none, as before the 16-bit calls) and
whether AttnBias is among its arguments.  So k_attn_X_bias<V, VEC, E>(..., AttnBias), the twin kernels of before, and
k_attn_X<V, VEC, E, AttnBias>(..., AttnBias), one template with a trailing argument pack, are the same kernel, and so are
k_attn_X<V, VEC, E>(...) and k_attn_X<V, VEC, E>(...) with an empty pack.  The kernels of kernels_spmm.hip and
kernels_sddmm.hip are read the same way: k_spmm_rows, k_spmm_pieces, k_sddmm_rows and k_sddmm_pieces are their name, V, VEC and
element type (float where the symbol has none, as before the 16-bit calls, whose argument struct was no template either), and
k_spmm_combine its name and element type; SpMM's three kernels may end in a TILED flag (the instantiations of the _cols call),
and a kernel without the flag, as before that call, is the one with TILED = false.  SDDMM's two kernels may end in a COLS flag
in the same way (the kernels of its _cols call), and k_sddmm_cols_rows<VEC, E> and k_sddmm_cols_pieces<VEC, E>, the twin kernels
of before, are k_sddmm_rows<16, VEC, E, COLS> and k_sddmm_pieces<16, VEC, E, COLS>.  The run kernels of kernels_adaptive.hip --
k_tiled16, k_sorted, k_adaptive, k_tiled_mixed -- are their name, their integer and boolean template arguments and the element
type of the matrix values (float where the symbol has none, as before spmv_csr_run_vals16); what follows the template
arguments in the symbol, the argument list, spells the values' pointer through the template parameter since then and is not
part of the key.  Any other symbol is its own key.
Exit status 0: every kernel of OLD is in NEW with the same text."""
import re
import sys

ELEMENTS = {None: "float", "f": "float", "NS_4bf16E": "bf16", "DF16_": "fp16"}
# the trailing flag of SpMM's and of SDDMM's kernels (the instantiations of their _cols calls; absent before those)
TILED = {None: "", "0": "", "1": ", TILED"}
COLS = {None: "", "0": "", "1": ", COLS"}
ATTN = re.compile(r"_ZN4spmv12_GLOBAL__N_1\d+(k_attn_[a-z_]+?)(?:_bias)?ILi(\d+)ELb([01])E(f|NS_4bf16E|DF16_)?(?:J(?:NS_8AttnBiasE)?E)?EEv")
GROUPS = re.compile(r"_ZN4spmv12_GLOBAL__N_1\d+(k_(?:spmm|sddmm)_(?:rows|pieces))ILi(\d+)ELb([01])E(f|NS_4bf16E|DF16_)?(?:Lb([01])E)?EEv")
# (the lines that lead in the next kernel, or pad the text behind a file's last one)
NEXT = re.compile(r"\t\.text$|\t\.(?:protected|weak|hidden)\t\w+ +; -- Begin function |\t\.p2alignl 6, 3212836864$|\t\.fill 256, 4, 3212836864$")
TILED_RUN = re.compile(r"_ZN4spmv\d+(k_tiled16|k_sorted|k_adaptive|k_tiled_mixed)I((?:L[ib]\d+E)+)(f|NS_4bf16E|DF16_)?EEv")
SDDMM_COLS = re.compile(r"_ZN4spmv12_GLOBAL__N_1\d+k_sddmm_cols_(rows|pieces)ILb([01])E(f|NS_4bf16E|DF16_)EEv")     # (the twins of before)
COMBINE = re.compile(r"_ZN4spmv12_GLOBAL__N_1\d+(k_spmm_combine)(?:I(f|NS_4bf16E|DF16_)(?:Lb([01])E)?E)?E")


def key(symbol: str) -> str:
    m = GROUPS.match(symbol)
    if m:
        flag = (COLS if "sddmm" in m.group(1) else TILED)[m.group(5)]
        return f"{m.group(1)}<{m.group(2)}, {'true' if m.group(3) == '1' else 'false'}, {ELEMENTS[m.group(4)]}{flag}>"
    m = SDDMM_COLS.match(symbol)
    if m:
        return f"k_sddmm_{m.group(1)}<16, {'true' if m.group(2) == '1' else 'false'}, {ELEMENTS[m.group(3)]}, COLS>"
    m = COMBINE.match(symbol)
    if m:
        return f"{m.group(1)}<{ELEMENTS[m.group(2)]}{TILED[m.group(3)]}>"
    m = TILED_RUN.match(symbol)
    if m:
        args = [a[1:] if a[0] == "i" else ("true" if a[1:] == "1" else "false") for a in re.findall(r"L([ib]\d+)E", m.group(2))]
        return f"{m.group(1)}<{', '.join(args)}, {ELEMENTS[m.group(3)]}>"
    m = ATTN.match(symbol)
    if not m:
        return symbol
    bias = ", AttnBias" if "NS_8AttnBiasE" in symbol else ""
    return f"{m.group(1)}<{m.group(2)}, {'true' if m.group(3) == '1' else 'false'}, {ELEMENTS[m.group(4)]}{bias}>"


def kernels(path: str) -> dict:
    text = open(path).read()
    text = text.split("\t.amdgpu_metadata")[0].split("\t.type\t__hip_cuid_")[0]      # (the unit's id hashes its path)
    text = text.split("\t.section\t.AMDGPU.gpr_maximums")[0]       # (the file's trailer, after the last kernel)
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    text = re.sub(r"\bBB\d+_(?=\d)", "BB_", text)
    text = re.sub(r"(?m)^(\.LBB_\d+:) +;", r"\1 ;", text)      # (the comment's column moves with the label's length)
    out = {}
    for chunk in re.split(r"(?m)^(?=\t\.globl\t_Z)", text)[1:]:
        symbol = re.match(r"\t\.globl\t(\w+)", chunk).group(1)
        chunk = re.sub(r"\b" + symbol + r"\b", "{kernel}", chunk)
        assert key(symbol) not in out, key(symbol)
        out[key(symbol)] = "\n".join(l for l in chunk.splitlines() if not l.startswith("\t.section\t.text") and not NEXT.match(l))
    return out


def main() -> int:
    old, new = kernels(sys.argv[1]), {}
    for path in sys.argv[2:]:
        more = kernels(path)
        twice = [n for n in more if n in new]
        assert not twice, f"{path}: in an earlier NEW file too: {twice}"
        new.update(more)
    missing = [n for n in old if n not in new]
    differ = [n for n in old if n in new and old[n] != new[n]]
    extra = [n for n in new if n not in old]
    print(f"{len(old)} kernels before, {len(new)} now: {len(old) - len(missing) - len(differ)} identical, {len(differ)} differ, "
          f"{len(missing)} missing, {len(extra)} new")
    for n in differ + missing + extra:
        print(("differs: " if n in differ else "missing: " if n in missing else "new: ") + n)
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main())
