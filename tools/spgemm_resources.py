#!/usr/bin/env python3
"""tools/spgemm_resources.py [LOG] -- registers, LDS and scratch of every kernel of csrc/kernels_spgemm.hip.

Compiles the file's device code for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage (or reads the
remarks of such a compile from LOG) and prints one row per instantiation: VGPRs, AGPRs, waves per SIMD by registers, SGPRs,
scratch bytes per lane, registers spilled, LDS bytes per block (dynamic LDS: as the launches size it).  profiles/spgemm_resources.md is its output.  Exit status 1 if a kernel
has scratch.  A compile, not a run: it needs no device."""
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "spmv-test_amd" / "csrc"
NAMES = {"k_spg_bound": "k_spg_bound (terms per row of A)",
         "k_spg_symILi64ELi4ELb0E": "k_spg_sym<64, 4, count>", "k_spg_symILi64ELi4ELb1E": "k_spg_sym<64, 4, write>",
         "k_spg_symILi512ELi4ELb0E": "k_spg_sym<512, 4, count>", "k_spg_symILi512ELi4ELb1E": "k_spg_sym<512, 4, write>",
         "k_spg_symILi4096ELi4ELb0E": "k_spg_sym<4096, 4, count>", "k_spg_symILi4096ELi4ELb1E": "k_spg_sym<4096, 4, write>",
         "k_spg_symILi32768ELi1ELb0E": "k_spg_sym<32768, 1, count>", "k_spg_symILi32768ELi1ELb1E": "k_spg_sym<32768, 1, write>",
         "k_spg_big_sort": "k_spg_big_sort (oversized rows)", "k_spg_big_write": "k_spg_big_write (oversized rows)",
         "k_spg_total": "k_spg_total",
         "k_spg_numILi64ELi4E": "k_spg_num<64, 4>", "k_spg_numILi512ELi4E": "k_spg_num<512, 4>",
         "k_spg_numILi4096ELi1E": "k_spg_num<4096, 1>", "k_spg_numILi16384ELi1E": "k_spg_num<16384, 1>"}
# LDS of k_spg_sym and k_spg_num is dynamic (the compile reports 0): bytes per workgroup as the launches size it
DYNAMIC_LDS = {"k_spg_sym<64, 4": 1024, "k_spg_sym<512, 4": 8192, "k_spg_sym<4096, 4": 65536, "k_spg_sym<32768, 1": 131072,
               "k_spg_num<64, 4>": 6144, "k_spg_num<512, 4>": 20480, "k_spg_num<4096, 1>": 33792, "k_spg_num<16384, 1>": 132096}


def remarks() -> str:
    if len(sys.argv) > 1:
        return Path(sys.argv[1]).read_text()
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden",
           f"-I{ROOT / 'include'}", f"-I{CSRC}", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           str(CSRC / "kernels_spgemm.hip"), "-o", os.devnull]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stderr


def main() -> int:
    rows = {}
    for block in re.split(r"remark: Function Name: ", remarks())[1:]:
        mangled = block.split()[0]
        label = next((v for k, v in NAMES.items() if k in mangled), None)
        if label is None:
            continue
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))      # noqa: E731
        lds = next((v for k, v in DYNAMIC_LDS.items() if label.startswith(k)), get("LDS Size [bytes/block]"))
        rows[label] = (get("VGPRs"), get("AGPRs"), get("Occupancy [waves/SIMD]"), get("TotalSGPRs"), get("ScratchSize [bytes/lane]"),
                       get("SGPRs Spill") + get("VGPRs Spill"), lds)
    if len(rows) != len(NAMES):
        print(f"expected {len(NAMES)} kernels, found {sorted(rows)}")
        return 1
    print("| kernel | VGPRs | AGPRs | waves / SIMD by registers | SGPRs | scratch bytes / lane | registers spilled | LDS bytes / block |")
    print("|---|---|---|---|---|---|---|---|")
    for label in NAMES.values():
        print(f"| {label} | " + " | ".join(str(v) for v in rows[label]) + " |")
    scratch = [label for label, r in rows.items() if r[4] or r[5]]
    print(f"\n{len(rows)} instantiations, {len(scratch)} with scratch or spills" + (f": {scratch}" if scratch else ""))
    return 1 if scratch else 0


if __name__ == "__main__":
    sys.exit(main())
