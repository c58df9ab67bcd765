"""CPU: the UNMODIFIED reference tester (src/tester.cpp + test/main.cpp) compiles against include/kernel.hpp and links
against libspmv_launchers.so -- the drop-in claim at the link level.  build() compiles and links it where the reference
sources lie (oracle/Makefile, target _ref/ref_tester; nothing of the reference is copied into the repository), and this
test checks that binary.  Skipped where build() had no reference sources to compile."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "oracle" / "_ref" / "ref_tester"


def test_unmodified_reference_tester_links_against_our_launchers(pkg):
    if not EXE.exists():        # (checked after `pkg`: that fixture runs build() where nothing is built yet)
        pytest.skip("oracle/_ref/ref_tester not built (no reference sources at build time)")
    out = subprocess.run(["nm", "-u", str(EXE)], capture_output=True, text=True).stdout
    for sym in ("_Z15cublas_gemv_gpuiiPfS_S_", "_Z12wsp_gemv_gpuiiPfS_S_i", "_Z12asp_gemv_gpuiiPfS_S_i",
                "_Z13awsp_gemv_gpuiiPfS_S_i", "_Z17awsp_ref_gemv_gpuiiPfS_S_"):
        assert sym in out
    # the launchers it resolves are this package's
    ldd = subprocess.run(["ldd", str(EXE)], capture_output=True, text=True).stdout
    found = [l.split("=>")[1].split("(")[0].strip() for l in ldd.splitlines() if "libspmv_launchers.so" in l and "=>" in l]
    assert found and Path(found[0]).resolve() == pkg.capi.LAUNCHERS_PATH.resolve(), ldd
    # without a GPU the first launcher must stop the process the way CUDA_CHECK does (kernel.hpp:21-28)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "start to launch cublas kernel" in r.stdout and "HIP error" in r.stderr
