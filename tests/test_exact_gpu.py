"""GEMM families and attention kernels bit for bit on exact data (``gpu_checks.check_gemm_exact`` / ``check_attention_exact``).

The inputs are chosen so that the exact result is representable at every intermediate step: the expected output is known to the last
bit whatever the summation order, every row's tolerance is 0 and its ``err`` is the number of differing elements.  The GEMM rows pin
the rounding contract of the epilogue, fp16(fp16(acc + bias + rowvec) + R), on every family and then each family against the naive
kernel; the attention rows show that every key position is read once, from its own V row, and counted once in the denominator.  The
builders and their conditions are checked on the CPU by tests/test_exact_host.py, the family each GEMM launch names by
tests/test_gemm_plan_host.py, the kernel instantiation each attention launch names by tests/test_attention_plan_host.py.
"""
import os

import pytest

import gpu_checks as gc

pytestmark = pytest.mark.gpu


def _assert_all(results):
    if os.environ.get("ANYV2V_PRINT_ROWS", "0") == "1":
        for r in results:
            print(f"{'ok  ' if r['ok'] else 'FAIL'} {r['name']}: {r['err']:.3e} (tol {r['tol']:.1e})")
    bad = [f"{r['name']}: err {r['err']:.3e} > tol {r['tol']:.1e}" for r in results if not r["ok"]]
    assert not bad, "\n".join(bad)
    assert results
    assert all(r["tol"] == 0.0 for r in results)


@pytest.mark.parametrize("variant", ["tile reg", "tile glds", "naive"])
def test_exact_gemm_128_row_tile_and_naive_kernels(variant):
    rows = gc.check_gemm_exact((variant,))
    _assert_all(rows)
    assert not any(r.get("skipped") for r in rows)


def test_exact_gemm_persistent_pingpong_single_wave_stream_k():
    rows = gc.check_gemm_exact(("persistent",))
    _assert_all(rows)
    # a forced kernel must not pass because every one of its cases was skipped
    for fam, _bits in gc.PERSISTENT_FAMILIES:
        assert any(f"[{fam}]" in r["name"] and not r.get("skipped") for r in rows), fam


def test_exact_gemm_split_k_both_forms():
    rows = gc.check_gemm_exact(("split-K",))
    _assert_all(rows)
    assert len(rows) == 2 and not any(r.get("skipped") for r in rows)


def test_exact_gemm_conv_lds_patch_kernel():
    rows = gc.check_gemm_exact(("LDS patch",))
    _assert_all(rows)
    assert len(rows) == 3 and not any(r.get("skipped") for r in rows)


def test_exact_gemm_weight_stationary():
    rows = gc.check_gemm_exact(("weight-stationary",))
    _assert_all(rows)
    assert len(rows) == 3 and not any(r.get("skipped") for r in rows)


def test_exact_gemm_every_family_equals_the_naive_kernel():
    rows = gc.check_gemm_exact(("cross-family",))
    _assert_all(rows)
    for fam in ["128-row reg", "128-row glds", "LDS patch"] + [f for f, _bits in gc.PERSISTENT_FAMILIES]:
        assert any(f"[{fam}]" in r["name"] and not r.get("skipped") for r in rows), fam


@pytest.mark.parametrize("kernel", gc.XA_KERNELS)
def test_exact_attention_every_key_once(kernel):
    rows = gc.check_attention_exact((kernel,))
    _assert_all(rows)
    assert not any(r.get("skipped") for r in rows)
    assert any("selection" in r["name"] for r in rows)
