"""What the kernels do NEXT TO their operands, every call through the C ABI.

Each case runs twice with the same flags: on plain tensors and with every operand -- inputs and outputs -- carved out of a larger
tensor whose every other element holds a NaN bit pattern (``gpu_checks._framed``).  Three rows per case: the framed result against
the fp32 / float64 reference of that kernel's existing check (``gpu_checks.KTOL`` unless the kernel documents fp16 rounding points);
framed result == plain result bit for bit (the launch plan depends on shapes, flags and alignment only, so a difference means a
masked-off read reached a stored value); the frames of all framed outputs bit-intact (no store outside the logical output).  Every
framed operand lies inside one allocation and no case expects a fault: a violation shows as a failing row.
"""
import os

import pytest

import gpu_checks as gc

pytestmark = pytest.mark.gpu


def _assert_all(results):
    if os.environ.get("ANYV2V_PRINT_ROWS", "0") == "1":
        for r in results:
            print(f"{'ok  ' if r['ok'] else 'FAIL'} {r['name']}: {r['err']:.3e} (l2 {r.get('l2', float('nan')):.3e}, tol {r['tol']:.1e})")
    bad = [f"{r['name']}: err {r['err']:.3e} (l2 {r.get('l2', float('nan')):.3e}) > tol {r['tol']:.1e}" for r in results if not r["ok"]]
    assert not bad, "\n".join(bad)
    assert results


@pytest.mark.parametrize("variant", ["reg", "glds", "naive"])
def test_edges_gemm_128_row_tile_kernel(variant):
    _assert_all(gc.check_edges_gemm_tile((variant,)))


@pytest.mark.parametrize("variant", ["reg", "glds", "naive"])
def test_edges_conv_and_temporal_conv(variant):
    _assert_all(gc.check_edges_conv((variant,)))


def test_edges_gemm_persistent_pingpong_single_wave_stream_k():
    rows = gc.check_edges_gemm_persistent()
    _assert_all(rows)
    # a forced kernel must not pass because every one of its cases was skipped
    for fam, _bits in gc.PERSISTENT_FAMILIES:
        assert any(fam in r["name"] and not r.get("skipped") for r in rows), fam


def test_edges_split_k_with_poisoned_workspace():
    _assert_all(gc.check_edges_splitk())


def test_edges_conv_lds_patch_kernel():
    _assert_all(gc.check_edges_conv_lds_patch())


def test_edges_gemm_weight_stationary_and_layernorm_fold():
    _assert_all(gc.check_edges_gemm_ws())


def test_edges_fused_feed_forward():
    _assert_all(gc.check_edges_ff_fused())


def test_edges_attention_flash_pnp_temporal():
    _assert_all(gc.check_edges_attention())


def test_edges_attention_8_wave_blocks():
    _assert_all(gc.check_edges_attention_8wave())


def test_edges_attention_small_loop_bias_and_generic():
    _assert_all(gc.check_edges_attention_small())


def test_edges_elementwise_and_step_kernels():
    _assert_all(gc.check_edges_elementwise())


def test_edges_layout_kernels():
    _assert_all(gc.check_edges_layout())


def test_edges_softmax_rows_and_timestep_embedding():
    _assert_all(gc.check_edges_softmax_timestep())
