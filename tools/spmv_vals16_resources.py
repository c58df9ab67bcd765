#!/usr/bin/env python3
"""tools/spmv_vals16_resources.py [LOG] -- every bf16 and fp16 run kernel of csrc/kernels_adaptive.hip beside its fp32 twin.

Compiles the file's device code for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage (or reads the
remarks of such a compile from LOG) and prints, per kernel as fp32/bf16/fp16: VGPRs, scratch bytes per lane, waves per SIMD
and the registers the compiler spilled.  The kernels are named by tools/attention_asm_diff.py's key.  It is the table of
profiles/spmv_vals16_resources.md.  Exit status 1 if a 16-bit instantiation has scratch where its twin has none, or fewer
waves.  A compile, not a run: it needs no device."""
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "spmv-test_amd" / "csrc"
sys.path.insert(0, str(ROOT / "tools"))
from attention_asm_diff import key  # noqa: E402

ELEMENTS = ("float", "bf16", "fp16")


def remarks() -> str:
    if len(sys.argv) > 1:
        return Path(sys.argv[1]).read_text()
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden",
           f"-I{ROOT / 'include'}", f"-I{CSRC}", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           str(CSRC / "kernels_adaptive.hip"), "-o", os.devnull]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stderr


def main() -> int:
    table, order = {}, []
    for block in re.split(r"remark: Function Name: ", remarks())[1:]:
        m = re.match(r"(\w+)<(.*), (float|bf16|fp16)>$", key(block.split()[0]))
        if not m:
            continue
        row = f"{m.group(1)}<{m.group(2)}>"
        get = lambda k: int(re.search(re.escape(k) + r": (\d+)", block).group(1))      # noqa: E731
        if row not in order:
            order.append(row)
        table[row, m.group(3)] = dict(vgpr=get("VGPRs"), scratch=get("ScratchSize [bytes/lane]"), waves=get("Occupancy [waves/SIMD]"),
                                      spill=f"{get('SGPRs Spill')}/{get('VGPRs Spill')}")
    join = lambda xs: "/".join(str(x) for x in xs)      # noqa: E731
    print("| kernel | VGPRs f32/bf16/fp16 | scratch bytes f32/bf16/fp16 | waves / SIMD f32/bf16/fp16 | spills bf16, fp16 (S/V) |")
    print("|---|---|---|---|---|")
    n = missed = 0
    for row in order:
        if (row, "bf16") not in table:
            continue                                   # the persistent forms: fp32 only
        r = [table[row, e] for e in ELEMENTS]
        n += 2
        missed += sum(x["scratch"] > r[0]["scratch"] or x["waves"] < r[0]["waves"] for x in r[1:])
        print(f"| `{row}` | {join(x['vgpr'] for x in r)} | {join(x['scratch'] for x in r)} | {join(x['waves'] for x in r)} | "
              f"{r[1]['spill']}, {r[2]['spill']} |")
    print(f"\n{n} 16-bit instantiations: {missed} with more scratch or fewer waves per SIMD than their fp32 twin")
    return 1 if missed or not n else 0


if __name__ == "__main__":
    sys.exit(main())
