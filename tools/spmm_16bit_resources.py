#!/usr/bin/env python3
"""tools/spmm_16bit_resources.py [LOG ...] -- every bf16 and fp16 kernel of csrc/kernels_spmm.hip and csrc/kernels_sddmm.hip
beside its fp32 twin.

Compiles the two files' device code for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage (or reads
the remarks of such compiles from the LOGs) and prints, per kernel<V, VEC>, as fp32/bf16/fp16: VGPRs, waves per SIMD, SGPRs,
scratch bytes per lane and the registers the compiler spilled (SGPRs into vector lanes / VGPRs to scratch).  It is the table
of profiles/spmm_16bit_resources.md.  Exit status 1 if an instantiation has scratch.  A compile, not a run: it needs no device."""
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "spmv-test_amd" / "csrc"
ELEMENTS = {"f": "fp32", "NS_4bf16E": "bf16", "DF16_": "fp16"}
FILES = ("kernels_spmm.hip", "kernels_sddmm.hip")


def remarks() -> str:
    if len(sys.argv) > 1:
        return "".join(Path(p).read_text() for p in sys.argv[1:])
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    out = ""
    for f in FILES:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden",
               f"-I{ROOT / 'include'}", f"-I{CSRC}", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
               str(CSRC / f), "-o", os.devnull]
        out += subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    return out


def main() -> int:
    table, order = {}, []
    for block in re.split(r"remark: Function Name: ", remarks())[1:]:
        m = re.match(r"\S*?\d+(k_(?:spmm|sddmm)_(?:rows|pieces))ILi(\d+)ELb([01])E(f|DF16_|NS_4bf16E)E", block)
        c = re.match(r"\S*?\d+(k_spmm_combine)I(f|DF16_|NS_4bf16E)E", block)
        if m:
            row, e = f"{m.group(1)}<{m.group(2)}, {'true' if m.group(3) == '1' else 'false'}>", ELEMENTS[m.group(4)]
        elif c:
            row, e = c.group(1), ELEMENTS[c.group(2)]
        else:
            continue
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))      # noqa: E731
        if row not in order:
            order.append(row)
        table[(row, e)] = dict(vgpr=get("VGPRs"), sgpr=get("TotalSGPRs"), scratch=get("ScratchSize [bytes/lane]"),
                               waves=get("Occupancy [waves/SIMD]"), spill=f"{get('SGPRs Spill')}/{get('VGPRs Spill')}")
    if not order:
        print("no k_spmm_* or k_sddmm_* kernel found")
        return 1
    print("| kernel<V, VEC> | VGPRs f32/bf16/fp16 | waves / SIMD f32/bf16/fp16 | SGPRs f32/bf16/fp16 | scratch | spills bf16, fp16 (S/V) |")
    print("|---|---|---|---|---|---|")
    join = lambda xs: "/".join(str(x) for x in xs)      # noqa: E731
    scratch = raised = lower = 0
    for row in order:
        r = [table[(row, e)] for e in ELEMENTS.values()]
        scratch += sum(x["scratch"] > 0 for x in r[1:])
        raised += sum(x["waves"] > r[0]["waves"] for x in r[1:])
        lower += sum(x["waves"] < r[0]["waves"] for x in r[1:])
        print(f"| {row} | {join(x['vgpr'] for x in r)} | {join(x['waves'] for x in r)} | {join(x['sgpr'] for x in r)} | "
              f"{join(x['scratch'] for x in r)} | {r[1]['spill']}, {r[2]['spill']} |")
    print(f"\n{2 * len(order)} 16-bit instantiations: {raised} above their fp32 twin's waves per SIMD, {lower} below, {scratch} with scratch")
    return 1 if scratch else 0


if __name__ == "__main__":
    sys.exit(main())
