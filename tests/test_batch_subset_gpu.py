"""A launch on a subset of a step's branches under the batch hint computes the bits of the full launch's rows -- per kernel, through
``ops`` and the C ABI, no models (cases: tests/batch_subset_spec.py; that the hint is decisive for them: tests/test_batch_subset_host.py).

Every case runs the launch on T rows of B branches, then on the contiguous copy of the last B - 1 branches' rows inside
``with ops.batch_hint(B, B - 1)``.  Rows per case: the full launch against the fp64 / fp32 reference of that kernel's existing check at
``gpu_checks.KTOL`` (two equally wrong results do not pass); subset == the full launch's rows with ``torch.equal`` -- outputs, records
and statistics alike; and one informational row saying whether the subset WITHOUT the hint coincides (attention: an asserted row, its
planner does not read the hint).  No tolerance between the two launches.
"""
import pytest

import batch_subset_spec as bss
import gpu_checks as gc

pytestmark = pytest.mark.gpu


def _assert_all(results):
    for r in results:
        print(f"{'ok  ' if r['ok'] else 'FAIL'} {r['name']}: {r['err']:.3e} (l2 {r.get('l2', float('nan')):.3e}, tol {r['tol']:.1e})")
    bad = [f"{r['name']}: err {r['err']:.3e} (l2 {r.get('l2', float('nan')):.3e}) > tol {r['tol']:.1e}" for r in results if not r["ok"]]
    assert not bad, "\n".join(bad)
    assert results


@pytest.mark.parametrize("line", bss.GEMM_LINES)
def test_gemm_family(line):
    rows = gc.check_subset_gemm(line)
    _assert_all(rows)
    assert any(not r.get("skipped") for r in rows)   # a line must not pass because every case was skipped


def test_groupnorm_one_call():
    _assert_all(gc.check_subset_groupnorm())


def test_groupnorm_two_phase_and_from_gemm_records():
    _assert_all(gc.check_subset_groupnorm_two_phase_and_records())


def test_attention():
    _assert_all(gc.check_subset_attention())


def test_attention_pnp_replay_launch():
    _assert_all(gc.check_subset_attention_pnp())


def test_step_kernels_with_branch_indices():
    _assert_all(gc.check_subset_step_kernels())


def test_layernorm_and_softmax_rows():
    _assert_all(gc.check_subset_layernorm_softmax())


def test_zz_batch_hint_is_restored():
    """Last in the module: a plain launch plans as un-hinted again."""
    _assert_all(gc.check_subset_hint_restored())
