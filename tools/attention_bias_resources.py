#!/usr/bin/env python3
"""tools/attention_bias_resources.py [LOG] -- every biased kernel of csrc/kernels_attention.hip beside its unbiased twin.

Compiles the file's device code for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage (or reads the
remarks of such a compile from LOG) and prints, per kernel<V, VEC>, as fp32/bf16/fp16 with the twin's figure in brackets
(k_attn_X_bias<V, VEC> is the row of the instantiations k_attn_X<V, VEC, E, AttnBias>, its twin k_attn_X<V, VEC, E>):
VGPRs, waves per SIMD, SGPRs, scratch bytes per lane, scalar registers kept in vector lanes, LDS bytes per block.  It is the
last table of profiles/lane_group_resource_usage.md, and what kBiasEarly and bias_waves in the kernel file were read off.
Exit status 1 if a _bias kernel has scratch; a kernel below its twin's waves or with scalar registers in vector lanes is
marked and counted, not refused ("Known gaps").  A compile, not a run: it needs no device."""
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "spmv-test_amd" / "csrc"
ELEMENTS = {"f": "fp32", "NS_4bf16E": "bf16", "DF16_": "fp16"}


def remarks() -> str:
    if len(sys.argv) > 1:
        return Path(sys.argv[1]).read_text()
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden",
           f"-I{ROOT / 'include'}", f"-I{CSRC}", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           str(CSRC / "kernels_attention.hip"), "-o", os.devnull]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stderr


def main() -> int:
    table = {}
    for block in re.split(r"remark: Function Name: ", remarks())[1:]:
        m = re.match(r"\S*?\d+(k_attn_[a-z_]+)ILi(\d+)ELb([01])E(f|DF16_|NS_4bf16E)(?:J(NS_8AttnBiasE)?E)?E", block)
        if not m:
            continue
        name = m.group(1) + ("_bias" if m.group(5) else "")
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))      # noqa: E731
        table[(name, int(m.group(2)), m.group(3) == "1", ELEMENTS[m.group(4)])] = dict(
            vgpr=get("VGPRs"), sgpr=get("TotalSGPRs"), scratch=get("ScratchSize [bytes/lane]"), waves=get("Occupancy [waves/SIMD]"),
            lanes=get("SGPRs Spill") + get("VGPRs Spill"), lds=get("LDS Size [bytes/block]"))
    names = sorted({n for n, _, _, _ in table if n.endswith("_bias")})
    if not names:
        print("no k_attn_* kernel with a bias found")
        return 1
    print("| kernel<V, VEC> | VGPRs (twin's) | waves / SIMD (twin's) | SGPRs | scratch | SGPRs in vector lanes | LDS bytes |")
    print("|---|---|---|---|---|---|---|")
    below = lanes = scratch = total = 0
    join = lambda xs: "/".join(str(x) for x in xs)      # noqa: E731
    for name in names:
        for V in (1, 2, 4, 8, 16, 32):
            for vec in (True, False):
                ours = [table[(name, V, vec, e)] for e in ELEMENTS.values()]
                twin = [table[(name[:-5], V, vec, e)] for e in ELEMENTS.values()]
                total += len(ours)
                low = sum(o["waves"] < t["waves"] for o, t in zip(ours, twin))
                below, lanes, scratch = below + low, lanes + sum(o["lanes"] > 0 for o in ours), scratch + sum(o["scratch"] > 0 for o in ours)
                print(f"| {name}<{V}, {'true' if vec else 'false'}> | {join(o['vgpr'] for o in ours)} ({join(t['vgpr'] for t in twin)}) | "
                      f"{join(o['waves'] for o in ours)} ({join(t['waves'] for t in twin)}){' **below**' if low else ''} | "
                      f"{join(o['sgpr'] for o in ours)} | {join(o['scratch'] for o in ours)} | {join(o['lanes'] for o in ours)} | "
                      f"{join(o['lds'] for o in ours)} |")
    print(f"\n{total} _bias instantiations: {below} below their twin's waves per SIMD, {lanes} with scalar registers in vector lanes, "
          f"{scratch} with scratch")
    return 1 if scratch else 0


if __name__ == "__main__":
    sys.exit(main())
