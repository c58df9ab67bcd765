"""What the nine spmv_csr_attention_* calls answer to a bad argument, exactly: every status and every spmv_last_error text
of tests/golden/attention_refusals.json, which tests/golden/make_attention_refusals.py recorded from the library before the
argument checks of the nine calls were merged into one description per pass.  The cases are every single bad argument a
call can see and every pair of them, so the order in which the checks fire is held too.  A refused call launches nothing:
the outputs, NaN before, are NaN after; the same calls without a bad argument are accepted.
"""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import make_attention_refusals as R  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_refusal_is_the_recorded_one(pkg, gpu):
    capi = pkg.capi
    calls = R.read_golden()
    assert sorted(calls) == sorted(R.call_name(p, m) for p, m in R.CALLS)
    fx = R.Fixture(capi, gpu)
    try:
        wrong, n = [], 0
        for pas, mode in R.CALLS:
            want = calls[R.call_name(pas, mode)]
            cases = R.cases(pas, mode)
            assert [name for name, _ in cases] == list(want), f"{R.call_name(pas, mode)}: the cases are not the recorded ones"
            for name, changes in cases:
                got = fx.invoke(pas, mode, changes)
                n += 1
                if got != want[name]:
                    wrong.append(f"{R.call_name(pas, mode)} [{name}]: {got}, recorded {want[name]}")
        assert n == sum(len(c) for c in calls.values()) and n > 10000
        assert not wrong, f"{len(wrong)} of {n} refusals differ, the first: " + "\n".join(wrong[:10])
        assert fx.outputs_untouched(), "a refused call wrote to an output"
        for pas, mode in R.CALLS:
            status, text = fx.invoke(pas, mode)
            assert status == capi.OK, f"{R.call_name(pas, mode)} refused the uncorrupted call: {text}"
        assert not fx.outputs_untouched(), "the accepted calls wrote nothing"
    finally:
        fx.torch.cuda.synchronize()
        fx.close()
