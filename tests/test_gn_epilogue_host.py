"""GroupNorm statistics from the GEMM epilogue (ABI 105): the host side, no GPU.

The record rule the kernels implement, restated in a few lines of torch: one record (K, sum(x - K), sum((x - K)^2)) per 16 rows x
channel group about the record's first element, moved to one pivot per (statistics group, channel group) exactly.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from anyv2v_amd import _lib, ops
from anyv2v_amd.ops import gemm_gn_stats_floats, gn_launches, gn_stats_floats, groupnorm_from_stats  # noqa: F401  (new in ABI 105)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KTOL = 2e-3   # the kernel-level bound of tests/gpu_checks.py: max |diff| / max |ref| and relative L2


def _records(x16, groups):
    """[M, C] fp16 -> records [M / 16, groups, 3] in fp32, as the GEMM epilogue writes them."""
    M, C = x16.shape
    x = x16.float().view(M // 16, 16, groups, C // groups).permute(0, 2, 1, 3).reshape(M // 16, groups, -1)
    K = x[:, :, 0]
    d = x - K[:, :, None]
    return torch.stack([K, d.sum(-1), (d * d).sum(-1)], -1)


def _fold(rec, rows_per_group, n_rec):
    """records -> (mean, var) per (statistics group, channel group): s += s_i + n_i d, q += q_i + 2 d s_i + n_i d^2, d = K_i - K."""
    R, G, _ = rec.shape
    per = rows_per_group // 16
    rec = rec.view(R // per, per, G, 3)
    K = rec[:, 0, :, 0]
    s = torch.zeros_like(K)
    q = torch.zeros_like(K)
    for i in range(per):   # ascending row order, fp32 throughout
        d = rec[:, i, :, 0] - K
        s = s + (rec[:, i, :, 1] + n_rec * d)
        q = q + (rec[:, i, :, 2] + (2 * d * rec[:, i, :, 1] + n_rec * d * d))
    n = per * n_rec
    m = s / n
    return K + m, (q / n - m * m).clamp_min(0)


def _groupnorm_from_records(x16, rows_per_group, groups, eps=1e-5):
    M, C = x16.shape
    mean, var = _fold(_records(x16, groups), rows_per_group, 16 * (C // groups))
    cg = C // groups
    mean = mean.repeat_interleave(cg, 1).repeat_interleave(rows_per_group, 0)
    rstd = torch.rsqrt(var + eps).repeat_interleave(cg, 1).repeat_interleave(rows_per_group, 0)
    return (x16.float() - mean) * rstd


def _reference(x16, rows_per_group, groups, eps=1e-5):
    M, C = x16.shape
    x = x16.double().view(M // rows_per_group, rows_per_group, C).permute(0, 2, 1)
    return F.group_norm(x, groups, eps=eps).permute(0, 2, 1).reshape(M, C)


@pytest.mark.parametrize("case", ["random", "mean=1000sigma", "constant groups"])
def test_record_folding_rule_matches_group_norm(case):
    g = torch.Generator().manual_seed(3)
    M, C, rpg, groups = 4 * 1024, 320, 1024, 32
    x = torch.randn((M, C), generator=g)
    if case == "mean=1000sigma":
        x = 0.25 * x + 250.0   # fp16 spacing at 250 is 0.125 = sigma / 2: the stored values still spread, |mean| = 1000 sigma
    if case == "constant groups":
        x = (torch.randn((M // rpg, 1, groups, 1), generator=g) * 30).expand(M // rpg, rpg, groups, C // groups).reshape(M, C)
    x16 = x.half()
    got, ref = _groupnorm_from_records(x16, rpg, groups).double(), _reference(x16, rpg, groups)
    mx = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))
    l2 = float((got - ref).norm() / ref.norm().clamp_min(1e-12))
    print(f"{case}: max {mx:.3e} l2 {l2:.3e}")
    if case == "constant groups":
        assert float(got.abs().max()) == 0.0 and float(ref.abs().max()) == 0.0   # x - mean is exactly 0: the output is beta
    else:
        assert mx <= KTOL and l2 <= KTOL
    if case == "mean=1000sigma":   # what the pivot is for: the same sums about 0 lose the variance
        xf = x16.float().view(M // rpg, rpg, groups, C // groups)
        s, q = xf.sum((1, 3)), (xf * xf).sum((1, 3))
        n = rpg * (C // groups)
        var0 = q / n - (s / n) ** 2
        var = xf.double().var((1, 3), unbiased=False)
        assert float(((var0 - var).abs() / var).max()) > 10 * KTOL


def test_gemm_desc_mirrors_the_header():
    hdr = open(os.path.join(ROOT, "include", "anyv2v_hip.h")).read()
    body = hdr[hdr.index("typedef struct AnyV2VGemmDesc {"):hdr.index("} AnyV2VGemmDesc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        names.append(re.findall(r"[A-Za-z_0-9]+", first)[-1])
        names += [r.strip().lstrip("*") for r in rest]
    assert names == [n for n, _t in _lib.GemmDesc._fields_]
    assert names[-4:] == ["gn_stats", "gn_stats_floats", "gn_rows_per_group", "gn_groups"]
    assert names.index("reserved0") == len(names) - 5   # appended: the existing fields keep their offsets
    assert _lib.GemmDesc.gn_stats.offset == _lib.GemmDesc.reserved0.offset + 4
    assert int(re.search(r"#define ANYV2V_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 105
    for sym in ("anyv2v_gemm_gn_stats_floats", "anyv2v_gemm_gn_launches", "anyv2v_groupnorm_stats_floats",
                "anyv2v_groupnorm_apply_stats_f16"):
        assert sym in _lib.SYMBOLS


def test_switch_parses_and_is_off_by_default():
    assert ops._parse_switch(None) is False and ops._parse_switch("0") is False and ops._parse_switch("") is False
    assert ops._parse_switch("1") is True and ops._parse_switch(" 1 ") is True
    assert ops._parse_switch("yes") is False   # like the other switches of ops.py: "1" or nothing
    if os.environ.get("ANYV2V_GN_EPILOGUE") is None:
        assert ops.GN_EPILOGUE is False


def test_record_buffer_size_matches_the_layout():
    assert gn_stats_floats(196608, 4096, 32) == 3 * 12288 * 32 + 3 * 48 * 256 * 32
    assert gn_stats_floats(960, 60, 32) == 0 and gn_stats_floats(960, 960, 32) > 0   # HW = 60: 4-D no, 5-D (16 frames) yes


class _Ctx:
    pass


def _run_blocks(monkeypatch, switch):
    """One ResnetBlock2D and one TemporalConvLayer on the CPU emulation of the ops; returns the new entry points that were hit."""
    import cpu_ops_emulation as emu
    from anyv2v_amd import unet
    emu.install(monkeypatch)
    monkeypatch.setattr(ops, "GN_EPILOGUE", switch)
    hit = []
    real_gemm = ops.gemm

    def gemm(*a, gn=None, **k):
        if gn is not None:
            hit.append("gemm(gn=)")
        return real_gemm(*a, **k)

    def query(*a, rows_per_group, groups=32, **k):
        hit.append("gemm_gn_stats_floats")
        return 1

    def from_stats(x, gamma, beta, stats, rows_per_group, *, groups=32, eps=1e-5, silu=False, out=None):
        hit.append("groupnorm_from_stats")
        return emu.groupnorm(x, gamma, beta, None, rows_per_group, groups=groups, eps=eps, silu=silu, out=out)
    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(ops, "gemm_gn_stats_floats", query)
    monkeypatch.setattr(ops, "groupnorm_from_stats", from_stats)
    monkeypatch.setattr(unet, "_gn_records",
                        lambda ctx, M, rpg, g: torch.empty(1) if ops.GN_EPILOGUE and getattr(ctx, "fp", None) is None else None)
    torch.manual_seed(0)
    Fr, H, W, C = 2, 4, 4, 64
    ctx = _Ctx()
    ctx.F, ctx.fp, ctx.stats = Fr, None, None
    ctx.temb_all = (0.1 * torch.randn(1, C)).half()
    res = unet.ResnetBlock2D(C, C, 32, 32)
    tcl = unet.TemporalConvLayer(C, 32)
    for blk in (res, tcl):
        for p in blk.parameters():
            p.data = (0.05 * torch.randn(p.shape)).half()
        for m in blk.modules():
            if hasattr(m, "pack"):
                m.pack()
    x = torch.randn(Fr * H * W, C).half()
    y = res.run(ctx, x, None, H, W)
    return hit, tcl.run(ctx, y, H, W)


def test_unet_never_calls_the_new_entry_points_with_the_switch_off(monkeypatch):
    hit_off, z_off = _run_blocks(monkeypatch, False)
    assert hit_off == []
    hit_on, z_on = _run_blocks(monkeypatch, True)
    # conv1 -> norm2, and temporal conv i -> norm i + 1 for i = 1..3: four (query, launch, apply) triples
    assert hit_on.count("gemm_gn_stats_floats") == hit_on.count("gemm(gn=)") == hit_on.count("groupnorm_from_stats") == 4
    assert torch.isfinite(z_on.float()).all() and torch.equal(z_on, z_off)   # the emulation computes the same either way
