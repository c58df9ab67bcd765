#!/usr/bin/env python3
"""tools/color_resources.py -- registers, LDS and scratch of every kernel of csrc/kernels_color.hip and csrc/kernels_permute.hip, and
of the gather through the map that spmv_csr_permute_values and _permute_gather launch (csrc/kernels_map.hip).

Compiles the files' device code for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage and prints one row
per kernel: VGPRs, AGPRs, waves per SIMD by registers, SGPRs, scratch bytes per lane, registers spilled, LDS bytes per block.
profiles/color_resources.md is its output.  Exit status 1 if a kernel has scratch.  A compile, not a run: it needs no device."""
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "spmv-test_amd" / "csrc"
NAMES = {
    "kernels_color.hip": {"k_color_round": "k_color_round (a grid over the list of one round)",
                          "k_color_small": "k_color_small (one workgroup, round after round)", "k_color_iota": "k_color_iota"},
    "kernels_permute.hip": {"k_perm_invert": "k_perm_invert", "k_perm_verify": "k_perm_verify", "k_perm_lengths": "k_perm_lengths",
                            "k_perm_rankILi8E": "k_perm_rank<8> (rows of at most 8 entries)",
                            "k_perm_rankILi64E": "k_perm_rank<64> (rows of 9 .. 64 entries)",
                            "k_perm_bitonic": "k_perm_bitonic (rows of 65 .. 4096 entries)", "k_perm_relabel": "k_perm_relabel",
                            "k_perm_compose": "k_perm_compose", "k_perm_vector": "k_perm_vector"},
    "kernels_map.hip": {"k_map_moveILb0ELb1E": "k_map_move<false, true> (the gather of a transpose or permute map)"},
}


def remarks(name: str) -> str:
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden",
           f"-I{ROOT / 'include'}", f"-I{CSRC}", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           str(CSRC / name), "-o", os.devnull]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stderr


def main() -> int:
    rows = {}
    for name, kernels in NAMES.items():
        for block in re.split(r"remark: Function Name: ", remarks(name))[1:]:
            mangled = block.split()[0]
            label = next((v for k, v in kernels.items() if k in mangled), None)
            if label is None:
                continue
            get = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))      # noqa: E731
            rows[label] = (get("VGPRs"), get("AGPRs"), get("Occupancy [waves/SIMD]"), get("TotalSGPRs"), get("ScratchSize [bytes/lane]"),
                           get("SGPRs Spill") + get("VGPRs Spill"), get("LDS Size [bytes/block]"))
    labels = [label for kernels in NAMES.values() for label in kernels.values()]
    if len(rows) != len(labels):
        print(f"expected {len(labels)} kernels, found {sorted(rows)}")
        return 1
    print("| kernel | VGPRs | AGPRs | waves / SIMD by registers | SGPRs | scratch bytes / lane | registers spilled | LDS bytes / block |")
    print("|---|---|---|---|---|---|---|---|")
    for label in labels:
        print(f"| {label} | " + " | ".join(str(v) for v in rows[label]) + " |")
    scratch = [label for label, r in rows.items() if r[4] or r[5]]
    print(f"\n{len(rows)} kernels, {len(scratch)} with scratch or spills" + (f": {scratch}" if scratch else ""))
    return 1 if scratch else 0


if __name__ == "__main__":
    sys.exit(main())
