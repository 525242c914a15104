"""Kernels on operands whose rows lie more than 2^32 bytes apart, every call through ``anyv2v_amd.ops``.

Each case runs the plain ("near") launch against the float64 / fp32 reference of that kernel's edge check, then once per operand with
that operand inside a large allocation (``gpu_checks._FarBuffer``): its last row starts 2^32 bytes or more behind the pointer the
kernel gets, the pointer lies 4 GiB into the allocation, and every place a 32-bit image of a row offset points to holds other data.
The far result must equal the near result bit for bit -- the same launch on the same data, only the addresses differ -- unless the far
layout legitimately runs another kernel (the flash-attention kernels' K / V limit: those rows compare with the reference and say so).
No case expects a fault: a truncated offset stays inside the allocation and shows as a failing row.  No row may skip on a 288 GB part.
"""
import os
import time

import pytest

import gpu_checks as gc

pytestmark = pytest.mark.gpu


def _assert_all(results):
    if os.environ.get("ANYV2V_PRINT_ROWS", "0") == "1":
        for r in results:
            print(f"{'ok  ' if r['ok'] else 'FAIL'} {r['name']}: {r['err']:.3e} (l2 {r.get('l2', float('nan')):.3e}, tol {r['tol']:.1e})")
        for k, v in gc.FAR_PEAK.items():
            print(f"peak {v / 2 ** 30:.2f} GiB  {k}")
        gc.FAR_PEAK.clear()
    bad = [f"{r['name']}: err {r['err']:.3e} (l2 {r.get('l2', float('nan')):.3e}) > tol {r['tol']:.1e}" for r in results if not r["ok"]]
    assert not bad, "\n".join(bad)
    assert results
    assert gc.far_skipped(results) == 0


@pytest.mark.parametrize("family", [f[0] for f in gc.FAR_GEMM_FAMILIES])
def test_far_gemm(family):
    _assert_all(gc.check_far_gemm(family))


def test_far_fused_feed_forward():
    _assert_all(gc.check_far_ff_fused())


@pytest.mark.parametrize("kernel", gc.FAR_ATTN_KERNELS)
def test_far_attention(kernel):
    rows = gc.check_far_attention(kernel)
    _assert_all(rows)
    if kernel in ("4-wave flash", "shared-softmax 4-wave"):     # the far K / V rows beyond the flash kernels' limit ran, on the fallback
        assert sum("64-bit fallback" in r["name"] for r in rows) >= 2
    if kernel == "4-wave flash":     # both sides of the limit ran: at it on the flash kernel (bit-equal to near), 8 elements past it on the fallback
        assert sum("limit+8" in r["name"] and "64-bit fallback" in r["name"] for r in rows) == 2
        assert sum("via limit ==" in r["name"] for r in rows) == 2


def test_attention_with_a_negative_key_stride_takes_the_64_bit_kernels():
    _assert_all(gc.check_attention_negative_kv_seq())


def test_attention_beyond_the_flash_limit_with_more_than_65535_batch_elements_takes_the_generic_kernel():
    _assert_all(gc.check_attention_wide_exit_to_generic())


@pytest.mark.parametrize("entry", gc.FAR_NORM_ENTRIES)
def test_far_norms_on_a_source_past_2_31_elements(entry):
    _assert_all(gc.check_far_norm(entry))


@pytest.mark.parametrize("case", gc.FAR_LAYOUT_CASES)
def test_far_layout_and_elementwise(case):
    _assert_all(gc.check_far_layout(case))


@pytest.mark.parametrize("which", ["silu", "add"])
def test_far_flat_kernels_past_2_31_elements(which):
    _assert_all(gc.check_far_flat(which))
