#!/usr/bin/env python3
"""tools/spmm_cols_resources.py -- the table of profiles/spmm_cols_resources.md: VGPRs, SGPRs, waves per SIMD, scratch and
spills of every instantiation that spmv_csr_spmm_cols and spmv_csr_sddmm_cols launch, beside the V = 16 kernels of the narrow
entry points.  A compile (hipcc -Rpass-analysis=kernel-resource-usage with the Makefile's flags), not a run.

    python tools/spmm_cols_resources.py > table.md          # exit status 1 if a new instantiation uses scratch or spills
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import attention_asm_diff as D  # noqa: E402

PKG = ROOT / "spmv-test_amd"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden",
         f"-I{ROOT / 'include'}", f"-I{PKG / 'csrc'}", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]


def remarks(source):
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, str(source), "-o", f"{tmp}/out.s"], capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def main():
    bad = 0
    print("| kernel | | VGPRs | AGPRs | SGPRs | waves / SIMD | scratch bytes / lane | VGPR spills |\n|---|---|---|---|---|---|---|---|")
    for source in ("kernels_spmm.hip", "kernels_sddmm.hip"):
        for symbol, r in remarks(PKG / "csrc" / source).items():
            n = D.key(symbol)
            new = n.endswith((", TILED>", ", COLS>"))      # (the instantiations of the _cols calls)
            if not (new or re.match(r"k_(spmm|sddmm)_(rows|pieces)<16,", n) or n.startswith("k_spmm_combine")):
                continue
            bad += new and (r["ScratchSize [bytes/lane]"] != "0" or r["VGPRs Spill"] != "0" or r["SGPRs Spill"] != "0")
            print(f"| `{n}` | {'new' if new else 'narrow twin'} | {r['VGPRs']} | {r['AGPRs']} | {r['TotalSGPRs']} | "
                  f"{r['Occupancy [waves/SIMD]']} | {r['ScratchSize [bytes/lane]']} | {r['VGPRs Spill']} |")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
