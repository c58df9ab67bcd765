#!/usr/bin/env python3
"""tools/select_resources.py [LOG] -- registers, LDS and scratch of every kernel of csrc/kernels_select.hip and of the move through
the map that its companions launch (csrc/kernels_map.hip).

Compiles the files' device code for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage (or reads the
remarks of such a compile from LOG) and prints one row per instantiation: VGPRs, AGPRs, waves per SIMD, SGPRs, scratch bytes
per lane, registers spilled, LDS bytes per block.  profiles/select_resources.md is its output.  Exit status 1 if a kernel
has scratch.  A compile, not a run: it needs no device."""
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "spmv-test_amd" / "csrc"
NAMES = {"k_sel_cutILb0E": "k_sel_cut<false> (top-k: cut and count)", "k_sel_cutILb1E": "k_sel_cut<true> (threshold: count)",
         "k_sel_compact": "k_sel_compact", "k_map_moveILb0ELb0E": "k_map_move<false, false> (gather, values)",
         "k_map_moveILb1ELb0E": "k_map_move<true, false> (scatter)"}


def remarks() -> str:
    if len(sys.argv) > 1:
        return Path(sys.argv[1]).read_text()
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden",
           f"-I{ROOT / 'include'}", f"-I{CSRC}", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]
    return "".join(subprocess.run(cmd + [str(CSRC / name), "-o", os.devnull], capture_output=True, text=True, check=True).stderr
                   for name in ("kernels_select.hip", "kernels_map.hip"))


def main() -> int:
    rows = {}
    for block in re.split(r"remark: Function Name: ", remarks())[1:]:
        mangled = block.split()[0]
        label = next((v for k, v in NAMES.items() if k in mangled), None)
        if label is None:
            continue
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))      # noqa: E731
        rows[label] = (get("VGPRs"), get("AGPRs"), get("Occupancy [waves/SIMD]"), get("TotalSGPRs"), get("ScratchSize [bytes/lane]"),
                       get("SGPRs Spill") + get("VGPRs Spill"), get("LDS Size [bytes/block]"))
    if len(rows) != len(NAMES):
        print(f"expected {len(NAMES)} kernels, found {sorted(rows)}")
        return 1
    print("| kernel | VGPRs | AGPRs | waves / SIMD | SGPRs | scratch bytes / lane | registers spilled | LDS bytes / block |")
    print("|---|---|---|---|---|---|---|---|")
    for label in NAMES.values():
        print(f"| {label} | " + " | ".join(str(v) for v in rows[label]) + " |")
    scratch = [label for label, r in rows.items() if r[4] or r[5]]
    print(f"\n{len(rows)} instantiations, {len(scratch)} with scratch or spills" + (f": {scratch}" if scratch else ""))
    return 1 if scratch else 0


if __name__ == "__main__":
    sys.exit(main())
