"""The fused temporal QKV + attention kernel (``anyv2v_amd/csrc/tattn_fused.hip``, ``anyv2v_temporal_qkv_attn_f16``) on the GPU, through
``ops.temporal_qkv_attn`` -- the entry point itself, below and above the row count from which the model takes it.

 * small shapes (one strip; strips that are no multiple of the waves of a block; strips across the batch boundary) against an fp64
   reference of the same fp16 operands at the project's kernel tolerance ``KTOL``: LayerNorm -> QKV -> softmax(Q K^T / 8) V in
   float64, no intermediate rounding (the kernel rounds QKV to fp16 once, as the GEMM it replaces stores them);
 * from 32 768 rows -- where the two launches it replaces run the weight-stationary LayerNorm-fold GEMM and the short attention
   kernel -- ``torch.equal`` with those two launches: seeded data and rows with a large offset (``x + 30``) for the LayerNorm;
 * a batch-hinted subset, operands inside poisoned frames, and the wiring in ``unet.py`` (switch on against switch off).
"""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

C, HEADS, F = 320, 5, 16
EPS = 1e-5


@pytest.fixture(scope="module")
def gc():
    import gpu_checks
    return gpu_checks


@pytest.fixture(scope="module")
def ops():
    from anyv2v_amd import ops as o
    return o


@pytest.fixture(scope="module")
def weights(ops):
    """One folded projection for every case: (W', b', c1) of ``ops.ln_fold`` and the fp64 operands of the reference."""
    g = torch.Generator().manual_seed(1234)
    w = (torch.randn(3 * C, C, generator=g) / C ** 0.5).half().cuda()
    gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).half().cuda()
    beta = (0.2 * torch.randn(C, generator=g)).half().cuda()
    return ops.ln_fold(w, None, gamma, beta)


def _x(B, HW, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * F * HW, C, generator=g) * (1.0 + 0.5 * torch.rand(B * F * HW, 1, generator=g)) + offset
    return x.half().cuda()


def _two_launches(ops, x, weights, B, HW):
    """Today's form: LayerNorm-folded QKV GEMM, then the strided temporal attention."""
    w, b, c1 = weights
    qkv = ops.gemm(x, w, bias=b, ln=(c1, EPS))
    o = torch.empty((x.shape[0], C), dtype=torch.float16, device=x.device)
    st = (F * HW, 1, HW)
    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, batch=B * HW, heads=HEADS, Sq=F, Sk=F, inner=HW, q_strides=st,
                  kv_strides=st, scale=0.125)
    return o


def _fused(ops, x, weights, B, HW, out=None):
    w, b, c1 = weights
    return ops.temporal_qkv_attn(x, w, b, c1, EPS, B=B, F=F, HW=HW, heads=HEADS, scale=0.125, out=out)


def _ref64(x, weights, B, HW):
    w, b, _c1 = weights
    x64 = x.double()
    mean = x64.mean(1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(1, keepdim=True)
    qkv = (x64 - mean) / torch.sqrt(var + EPS) @ w.double().t() + b.double()
    # rows (b, f, pixel) -> sequences (b, pixel, head) of F frames
    t = qkv.view(B, F, HW, 3, HEADS, 64).permute(3, 0, 2, 4, 1, 5)   # [3][B][HW][heads][F][64]
    q, k, v = t[0], t[1], t[2]
    p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
    o = p @ v                                                          # [B][HW][heads][F][64]
    return o.permute(0, 3, 1, 2, 4).reshape(B * F * HW, C)


@pytest.mark.parametrize("B,HW,offset", [(1, 2, 0.0), (1, 10, 0.0), (2, 6, 0.0), (2, 6, 30.0)],
                         ids=["one_strip", "strips_not_multiple_of_waves", "across_batch_boundary", "row_offset_30"])
def test_small_shapes_against_fp64(gc, ops, weights, B, HW, offset):
    x = _x(B, HW, 100 + HW, offset)
    o = _fused(ops, x, weights, B, HW)
    torch.cuda.synchronize()
    r = gc._res(f"temporal_qkv_attn B{B} HW{HW} +{offset}", o, _ref64(x, weights, B, HW), gc.KTOL)
    print(r)
    assert r["ok"], r


@pytest.fixture(scope="module")
def big(ops, weights):
    """B = 3, HW = 2048 (98 304 rows; one branch = 32 768 rows, the smallest shape at which the reference launches take the
    weight-stationary path): input, the fused output and the two-launch output of the full batch, computed once."""
    x = _x(3, 2048, 7)
    x[5::97] += 30.0   # some rows far off zero: the LayerNorm fold subtracts mean x column sums
    fused = _fused(ops, x, weights, 3, 2048)
    two = _two_launches(ops, x, weights, 3, 2048)
    torch.cuda.synchronize()
    return x, fused, two


def test_supported_at_the_tested_shapes(ops, big):
    assert ops.temporal_qkv_attn_supported(F * 2048, C, HEADS, F, 2048, big[0])
    assert ops.ln_gemm_supported(F * 2048, C, 3 * C, hinted=False)


def test_one_branch_bit_equal_to_two_launches(ops, weights, big):
    """B = 1, HW = 2048: 32 768 rows."""
    x = big[0][:F * 2048].contiguous()
    fused = _fused(ops, x, weights, 1, 2048)
    two = _two_launches(ops, x, weights, 1, 2048)
    assert torch.equal(fused, two)
    assert torch.equal(fused, big[1][:F * 2048])   # a row's result does not depend on what else is in the launch


def test_ragged_last_round_bit_equal(ops, weights):
    """B = 1, HW = 2050: 1025 strips on 48 ranges of 22 -- the last range is short, and 22 strips are no multiple of 8 waves."""
    x = _x(1, 2050, 11, offset=30.0)
    assert torch.equal(_fused(ops, x, weights, 1, 2050), _two_launches(ops, x, weights, 1, 2050))


def test_three_branches_bit_equal(big):
    assert torch.equal(big[1], big[2])


def test_batch_hinted_subset(ops, weights, big):
    """[negative, editing] under the batch hint (3, 2): the same rows of the full launch, bit for bit, from either form."""
    x, fused, _two = big
    n = x.shape[0] // 3
    with ops.batch_hint(3, 2):
        sub = _fused(ops, x[n:], weights, 2, 2048)
        sub_two = _two_launches(ops, x[n:], weights, 2, 2048)
    assert torch.equal(sub, fused[n:])
    assert torch.equal(sub_two, fused[n:])


def test_framed_operands(gc, ops, weights, big):
    """``x`` and ``O`` as interior windows of poisoned buffers: same bits, and nothing outside the output window is written (a read
    outside the input window would bring NaN into the result)."""
    x, fused, _two = big
    n = x.shape[0] // 3
    _xb, xv, _xf = gc._framed_like(x[n:])
    ob, ov, of = gc._framed(2 * n, C)
    with ops.batch_hint(3, 2):
        _fused(ops, xv, weights, 2, 2048, out=ov)
    torch.cuda.synchronize()
    assert torch.equal(ov, fused[n:])
    assert gc._frame_intact(ob, of)


def test_wiring_switch_on_equals_off(ops, monkeypatch):
    """One TransformerTemporalModel at 320 channels, HW = 2048, B = 1: both self-attentions take the fused kernel with the switch on,
    none with it off, and the block output is the same."""
    from anyv2v_amd import unet
    model = unet.TransformerTemporalModel(HEADS, 64, C, 32)
    g = torch.Generator().manual_seed(99)
    for name, prm in model.named_parameters():
        if prm.dim() == 1:
            v = (1.0 if name.endswith("weight") else 0.0) + 0.1 * torch.randn(prm.shape, generator=g)
        else:
            v = torch.randn(prm.shape, generator=g) / prm.shape[-1] ** 0.5
        prm.data.copy_(v.half())
    model = model.cuda()
    for m in model.modules():
        if m is not model and hasattr(m, "pack"):
            m.pack()
    HW = 2048
    M = F * HW
    ctx = types.SimpleNamespace(B=1, F=F, stats=torch.empty(ops.gn_scratch_floats(M, F * HW, 32), dtype=torch.float32, device="cuda"))
    x = _x(1, HW, 5)
    calls = []
    real = ops.temporal_qkv_attn
    monkeypatch.setattr(ops, "temporal_qkv_attn", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setenv("ANYV2V_TATTN_FUSED", "1")
    on = model.run(ctx, x, 32, 64)
    assert len(calls) == 2
    monkeypatch.setenv("ANYV2V_TATTN_FUSED", "0")
    off = model.run(ctx, x, 32, 64)
    torch.cuda.synchronize()
    assert len(calls) == 2
    assert torch.isfinite(on.float()).all() and torch.equal(on, off)
