"""What the companions of the derived handles answer to a bad argument, exactly: the five strided moves (_transpose_gather,
_select_gather, _select_scatter, _add_gather, _permute_gather), the five refreshes (_transpose_values, _select_values,
_permute_values, _spgemm_values, _add_values) and the five _map_bytes / _plan_bytes.  Every status and every spmv_last_error
text of tests/golden/map_refusals.json, which tests/golden/make_map_refusals.py recorded from the library before the handle's
position map became one struct and these calls' checks one function each.  The cases are every single bad argument a call
can see, every handle of another maker and every pair of them, so the order in which the checks fire is held too.  A refused
call launches nothing: the moves' dst, poison before, is poison after, and every handle keeps its values; the same calls
without a bad argument are accepted and write what numpy says, bit for bit.
"""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import make_map_refusals as R  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_refusal_is_the_recorded_one(pkg, gpu):
    fx = R.Fixture(pkg.capi, gpu)
    try:
        calls = R.read_golden(fx.nnz)
        assert list(calls) == list(R.CALLS)
        wrong, n = [], 0
        for key, want in calls.items():
            cases = R.cases(key, fx.nnz)
            assert [name for name, _ in cases] == list(want), f"{key}: the cases are not the recorded ones"
            for name, changes in cases:
                got = fx.invoke(key, changes)
                n += 1
                if got != want[name]:
                    wrong.append(f"{key} [{name}]: {got}, recorded {want[name]}")
        assert n == sum(len(c) for c in calls.values()) and n > 1000
        assert not wrong, f"{len(wrong)} of {n} answers differ, the first: " + "\n".join(wrong[:10])
        assert fx.outputs_untouched(), "a refused call wrote to an output"
        fx.accepted_calls_exact()
    finally:
        fx.torch.cuda.synchronize()
        fx.close()
