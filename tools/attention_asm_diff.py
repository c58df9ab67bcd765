#!/usr/bin/env python3
"""tools/attention_asm_diff.py OLD.s NEW.s -- do the fp32 kernels of two builds of a kernel file have the same code?

Both files are device assembly of one csrc/*.hip file (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S, the Makefile's
other flags), OLD at an earlier commit, NEW at this one.  The text of every kernel (from its .globl line to the next
kernel's: the instruction stream, the .amdhsa_ block, the .set lines of its resource counts) is compared after the names
are normalised: a symbol is demangled, the element type that fused attention's kernels gained as a last template argument is
dropped where it is float (k_attn_fwd_rows<1, true, float>(GroupRows, AttnArgsT<float>) is k_attn_fwd_rows<1, true>(GroupRows,
AttnArgs) of before), the function numbers in local labels (.LBB12_3, .Lfunc_end12) and in the comments that name a loop
(Header=BB12_3, Child Loop BB12_5) are dropped: they count the kernels before this one in the file (so do the blanks that align a
label's comment), and the .section lines that only
name the next kernel are left out.  Kernels of NEW on another element type or with a bias (k_attn_*_bias) are new code and
are counted, not compared.  Exit status 0: every kernel of OLD is in NEW with the same text."""
import re
import subprocess
import sys


def canonical(name: str) -> str:
    name = name.replace("spmv::(anonymous namespace)::", "")
    name = name.replace("spmv::AttnArgsT<float>", "spmv::AttnArgs")
    name = re.sub(r"<(\d+), (true|false), float>", r"<\1, \2>", name)
    name = re.sub(r"spmv::Pointers2<float>", "spmv::Pointers2", name)
    return name


def kernels(path: str) -> dict:
    text = open(path).read()
    text = text.split("\t.amdgpu_metadata")[0].split("\t.type\t__hip_cuid_")[0]      # (the unit's id hashes its path)
    text = text.split("\t.section\t.AMDGPU.gpr_maximums")[0]       # (the file's trailer, after the last kernel)
    syms = sorted(set(re.findall(r"\b_Z\w+", text)), key=len, reverse=True)
    plain = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.splitlines()
    table = dict(zip(syms, (canonical(p) for p in plain)))
    text = re.sub(r"\b_Z\w+", lambda m: "{" + table[m.group(0)] + "}", text)
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    text = re.sub(r"\bBB\d+_(?=\d)", "BB_", text)
    text = re.sub(r"(?m)^(\.LBB_\d+:) +;", r"\1 ;", text)      # (the comment's column moves with the label's length)
    out = {}
    for chunk in re.split(r"(?m)^(?=\t\.globl\t\{)", text)[1:]:
        name = re.match(r"\t\.globl\t\{(.*?)\} ", chunk).group(1)
        out[name] = "\n".join(l for l in chunk.splitlines() if not l.startswith("\t.section\t.text"))
    return out


def main() -> int:
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    other = [n for n in new if re.search(r"spmv::bf16|_Float16|DF16_", n)]
    missing = [n for n in old if n not in new]
    differ = [n for n in old if n in new and old[n] != new[n]]
    biased = [n for n in new if n not in old and re.search(r"k_attn_\w+_bias[<I]", n)]
    extra = [n for n in new if n not in old and n not in other and n not in biased]
    print(f"{len(old)} kernels before, {len(new)} now: {len(old) - len(missing) - len(differ)} identical, {len(differ)} differ, "
          f"{len(missing)} missing, {len(biased)} new with a bias, {len([n for n in other if n not in old and n not in biased])} new on "
          f"16-bit elements, {len(extra)} other new ones")
    for n in differ + missing + extra:
        print(("differs: " if n in differ else "missing: " if n in missing else "new: ") + n)
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main())
