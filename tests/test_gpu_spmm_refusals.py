"""What the six SpMM / SDDMM run calls and spmv_csr_spmm_plan_cols answer to a bad argument, exactly: every status and every
spmv_last_error text of tests/golden/spmm_refusals.json, which tests/golden/make_spmm_refusals.py recorded from the library
before the argument checks of the six run calls were merged into one description.  The cases are every single bad argument
a call can see and every pair of them, so the order in which the checks fire is held too.  A refused call launches nothing:
the outputs, NaN before, are NaN after; the same calls without a bad argument are accepted and write.
"""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import make_spmm_refusals as R  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_refusal_is_the_recorded_one(pkg, gpu):
    calls = R.read_golden()
    assert list(calls) == list(R.CALLS)
    fx = R.Fixture(pkg.capi, gpu)
    try:
        wrong, n = [], 0
        for key, want in calls.items():
            cases = R.cases(key)
            assert [name for name, _ in cases] == list(want), f"{key}: the cases are not the recorded ones"
            for name, changes in cases:
                got = fx.invoke(key, changes)
                n += 1
                if got != want[name]:
                    wrong.append(f"{key} [{name}]: {got}, recorded {want[name]}")
        assert n == sum(len(c) for c in calls.values()) and n > 1000
        assert not wrong, f"{len(wrong)} of {n} refusals differ, the first: " + "\n".join(wrong[:10])
        assert fx.outputs_untouched(), "a refused call wrote to an output"
        fx.accepted_calls_write()
    finally:
        fx.torch.cuda.synchronize()
        fx.close()
