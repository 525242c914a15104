"""GroupNorm statistics from the GEMM epilogue (ABI 105, ``ANYV2V_GN_EPILOGUE``) on the GPU, every call through the C ABI.

Kernel rows: every (producer, shape) of the conv1 -> norm2 and temporal-conv chains at the four UNet levels, 16 frames, B = 1 and
B = 3 row counts, plus the levels of one odd latent size (40 x 24).  Reference: ``F.group_norm`` (+ SiLU) in fp32 on the same fp16
GEMM output; bound ``gpu_checks.KTOL`` on max |diff| / max |ref| and on the relative L2, as ``check_norms``.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FRAMES = 16
LEVELS = [(320, 64, 64), (640, 32, 32), (1280, 16, 16), (1280, 8, 8)]
ODD_LEVELS = [(320, 40, 24), (640, 20, 12), (1280, 10, 6)]   # a 40 x 24 latent: HW = 960, 240, 60


def _rows():
    rows = []
    for B in (1, 3):
        for C, H, W in LEVELS:
            rows.append((f"conv1->norm2 {C}@{H}x{W} B{B}", "conv", C, H, W, B))
            rows.append((f"temporal {C}@{H}x{W} B{B}", "temporal", C, H, W, B))
    for C, H, W in ODD_LEVELS:
        rows.append((f"conv1->norm2 {C}@{H}x{W} B1", "conv", C, H, W, 1))
        rows.append((f"temporal {C}@{H}x{W} B1", "temporal", C, H, W, 1))
    return rows


ROWS = _rows()
SPLIT_K = "the launch is planned split-K (tiles cannot fill the CUs, long K loop): the reduce kernel finishes it, no tile to take records of"
# rows the library may decline, by name, with the reason.  Only split-K plans and the odd-size row whose statistics group (HW = 60)
# is not a whole number of 16-row records; never the 64x64 / 32x32 B = 3 rows.
DECLINED = {
    "conv1->norm2 1280@10x6 B1": "4-D statistics group of HW = 60 rows: not a whole number of 16-row records",
    "conv1->norm2 1280@16x16 B1": SPLIT_K,
    "conv1->norm2 1280@8x8 B1": SPLIT_K,
    "conv1->norm2 1280@8x8 B3": SPLIT_K,
    "temporal 1280@8x8 B1": SPLIT_K,
    "temporal 1280@10x6 B1": SPLIT_K,
    "conv1->norm2 640@20x12 B1": SPLIT_K,
}
NEVER_DECLINED = {n for n, _k, _C, H, _W, B in ROWS if B == 3 and H in (64, 32)}


def _producer(kind, C, H, W, B, shift=0.0, seed=0):
    """(a, w, kwargs of ops.gemm, rows_per_group of the consumer norm)"""
    from anyv2v_amd import ops
    g = torch.Generator(device="cuda").manual_seed(seed)
    HW, M = H * W, B * FRAMES * H * W
    taps = 9 if kind == "conv" else 3
    a = torch.randn((M, C), generator=g, device="cuda", dtype=torch.float32).half()
    w = (torch.randn((C, taps * C), generator=g, device="cuda", dtype=torch.float32) / (taps * C) ** 0.5).half()
    bias = (0.1 * torch.randn(C, generator=g, device="cuda") + shift).half()
    if kind == "conv":
        temb = (0.1 * torch.randn((B, C), generator=g, device="cuda")).half()
        kw = dict(bias=bias, rowvec=temb, rowvec_div=FRAMES * HW, mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0, 0), M=M)
        return a, w, kw, HW
    kw = dict(bias=bias, mode=ops.MODE_TEMPORAL, temporal=(FRAMES, HW))
    return a, w, kw, FRAMES * HW


def _reference(c16, rows_per_group, gamma, beta):
    M, C = c16.shape
    x = c16.float().view(M // rows_per_group, rows_per_group, C).permute(0, 2, 1)
    y = F.group_norm(x, 32, gamma.float(), beta.float(), 1e-5)
    return F.silu(y).permute(0, 2, 1).reshape(M, C)


def _err(got, ref):
    d = (got.float() - ref).abs()
    return float(d.max() / ref.abs().max().clamp_min(1e-6)), float(d.norm() / ref.norm().clamp_min(1e-12))


def _affine(C):
    g = torch.Generator(device="cuda").manual_seed(7)
    return (1 + 0.2 * torch.randn(C, generator=g, device="cuda")).half(), (0.2 * torch.randn(C, generator=g, device="cuda")).half()


@pytest.mark.parametrize("shifted", [False, True], ids=["plain", "mean=1000sigma"])
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_gemm_records_then_apply_matches_group_norm(row, shifted):
    """GEMM-with-records + apply-from-records vs F.group_norm (+ SiLU) in fp32 on the same fp16 GEMM output; the query says yes
    and the launch is counted (or the row is listed in DECLINED); output bit-equal to the launch without records; records
    bit-equal run to run; distance to the two-launch form printed and gated."""
    from anyv2v_amd import ops
    from gpu_checks import KTOL
    name, kind, C, H, W, B = row
    shift = 0.0
    if shifted:   # a bias of 1000 x the spread of the unshifted output: the case the pivoted sums exist for
        a, w, kw, _ = _producer(kind, C, H, W, B)
        shift = 1000.0 * float(ops.gemm(a, w, **kw).float().std())
    a, w, kw, rpg = _producer(kind, C, H, W, B, shift=shift)
    M = kw.get("M", a.shape[0])
    gamma, beta = _affine(C)
    n = ops.gemm_gn_stats_floats(a, w, rows_per_group=rpg, groups=32, **kw)
    print(f"[gn-epilogue] {name} shifted={shifted}: query -> {n} floats")
    if name in DECLINED:
        assert name not in NEVER_DECLINED
        assert n == 0, f"{name} is listed as declined ({DECLINED[name]}) but the query answers {n}: remove it from the list"
        with pytest.raises(Exception, match="gn_stats"):   # a launch on a declined plan is an error, never a silent fallback
            ops.gemm(a, w, gn=(torch.empty(ops.gn_stats_floats(M, 16, 32), device="cuda"), rpg, 32), **kw)
        return
    assert n == 3 * (M // 16) * 32 > 0, f"{name}: the query declined a row that must emit statistics"
    plain = ops.gemm(a, w, **kw)
    rec = torch.full((ops.gn_stats_floats(M, rpg, 32),), float("nan"), device="cuda")
    ops.gn_launches(reset=True)
    c = ops.gemm(a, w, gn=(rec, rpg, 32), **kw)
    assert ops.gn_launches(reset=True) == 1, "the launch did not emit statistics"
    assert torch.equal(c, plain), "the fp16 output changed with gn_stats set"
    assert torch.isfinite(rec[:n]).all(), "records missing"
    y = ops.groupnorm_from_stats(c, gamma, beta, rec, rpg, silu=True)
    rec2 = torch.full_like(rec, float("nan"))
    c2 = ops.gemm(a, w, gn=(rec2, rpg, 32), **kw)
    y2 = ops.groupnorm_from_stats(c2, gamma, beta, rec2, rpg, silu=True)
    assert torch.equal(rec[:n], rec2[:n]) and torch.equal(y, y2), "two runs differ"
    ref = _reference(c, rpg, gamma, beta)
    mx, l2 = _err(y, ref)
    stats = torch.empty(ops.gn_scratch_floats(M, rpg, 32), device="cuda")
    two = ops.groupnorm(c, gamma, beta, stats, rpg, silu=True)
    dmx, dl2 = _err(y, two.float())
    print(f"[gn-epilogue] {name} shifted={shifted}: vs F.group_norm max {mx:.3e} l2 {l2:.3e}; vs two-launch form max {dmx:.3e} l2 {dl2:.3e}")
    assert mx <= KTOL and l2 <= KTOL, f"{name}: max {mx:.3e} l2 {l2:.3e} > {KTOL}"
    assert dmx <= KTOL and dl2 <= KTOL, f"{name}: distance to the two-launch form {dmx:.3e} / {dl2:.3e} > {KTOL}"


@pytest.mark.parametrize("row", [r for r in ROWS if r[0] in NEVER_DECLINED], ids=[r[0] for r in ROWS if r[0] in NEVER_DECLINED])
def test_two_branch_launch_under_batch_hint_is_bit_equal(row):
    """Rows [T/3, T) of the three-branch launch vs the two-branch launch under batch_hint(3, 2): T/3 is not a multiple of the 192-
    or 128-row tiles, the records must not depend on the tile origin."""
    from anyv2v_amd import ops
    name, kind, C, H, W, _B = row
    a, w, kw, rpg = _producer(kind, C, H, W, 3)
    gamma, beta = _affine(C)
    T = a.shape[0]
    rec3 = torch.empty(ops.gn_stats_floats(T, rpg, 32), device="cuda")
    c3 = ops.gemm(a, w, gn=(rec3, rpg, 32), **kw)
    y3 = ops.groupnorm_from_stats(c3, gamma, beta, rec3, rpg, silu=True)
    kw2 = dict(kw)
    if "M" in kw2:
        kw2["M"] = 2 * T // 3
        kw2["rowvec"] = kw["rowvec"][1:].contiguous()
    a2 = a[T // 3:].contiguous()
    with ops.batch_hint(3, 2):
        assert ops.gemm_gn_stats_floats(a2, w, rows_per_group=rpg, groups=32, **kw2) > 0
        rec2 = torch.empty(ops.gn_stats_floats(2 * T // 3, rpg, 32), device="cuda")
        c2 = ops.gemm(a2, w, gn=(rec2, rpg, 32), **kw2)
        y2 = ops.groupnorm_from_stats(c2, gamma, beta, rec2, rpg, silu=True)
    n2 = 3 * (2 * T // 3 // 16) * 32
    assert torch.equal(c2, c3[T // 3:])
    assert torch.equal(rec2[:n2], rec3[n2 // 2:n2 // 2 + n2]), "records depend on the tile origin"
    assert torch.equal(y2, y3[T // 3:])


def test_residual_launch_records_describe_the_stored_sum():
    """Records are taken of the stored output, i.e. after the residual add (both tile kernels)."""
    from anyv2v_amd import ops
    from gpu_checks import KTOL
    for C, H, W, B in ((320, 64, 64, 1), (640, 32, 32, 1)):
        a, w, kw, rpg = _producer("temporal", C, H, W, B)
        res = (3.0 * torch.randn(a.shape, device="cuda")).half()
        gamma, beta = _affine(C)
        assert ops.gemm_gn_stats_floats(a, w, residual=res, rows_per_group=rpg, **kw) > 0
        rec = torch.empty(ops.gn_stats_floats(a.shape[0], rpg, 32), device="cuda")
        c = ops.gemm(a, w, residual=res, gn=(rec, rpg, 32), **kw)
        assert torch.equal(c, ops.gemm(a, w, residual=res, **kw))
        mx, l2 = _err(ops.groupnorm_from_stats(c, gamma, beta, rec, rpg, silu=True), _reference(c, rpg, gamma, beta))
        print(f"[gn-epilogue] residual temporal {C}@{H}x{W}: max {mx:.3e} l2 {l2:.3e}")
        assert mx <= KTOL and l2 <= KTOL


# ------------------------------------------------------------------------------------------------ whole model, switch on
@pytest.fixture
def switch_on(monkeypatch):
    from anyv2v_amd import ops
    monkeypatch.setattr(ops, "GN_EPILOGUE", True)
    asked = {"yes": 0, "no": 0}
    query = ops.gemm_gn_stats_floats

    def counting(*a, **k):
        n = query(*a, **k)
        asked["yes" if n > 0 else "no"] += 1
        return n
    monkeypatch.setattr(ops, "gemm_gn_stats_floats", counting)
    ops.gn_launches(reset=True)
    return asked


def _assert_all(results):
    for r in results:
        print(f"{'PASS' if r['ok'] else 'FAIL'} {r['name']}: err {r['err']:.3e} (tol {r['tol']:.1e})")
    bad = [r["name"] for r in results if not r["ok"]]
    assert not bad, bad


def _expected_launches_per_forward(native):
    """What one B = 3 forward at 16 f x 64x64 must emit, from the block structure: one launch per ResnetBlock2D (conv1 -> norm2)
    and three per TemporalConvLayer (conv i -> norm i + 1), minus the ResNets of the 8x8 level -- the last down block, the mid
    block and the first up block -- whose conv1 is the kernel row listed as split-K above ("conv1->norm2 1280@8x8 B3"); the
    temporal convolutions of that level emit (row "temporal 1280@8x8 B3")."""
    from anyv2v_amd.unet import ResnetBlock2D, TemporalConvLayer
    assert DECLINED["conv1->norm2 1280@8x8 B3"] == SPLIT_K and "temporal 1280@8x8 B3" not in DECLINED
    resnets = sum(isinstance(m, ResnetBlock2D) for m in native.modules())
    temporal = sum(isinstance(m, TemporalConvLayer) for m in native.modules())
    at_8x8 = len(native.down_blocks[-1].resnets) + len(native.mid_block.resnets) + len(native.up_blocks[0].resnets)
    return resnets - at_8x8 + 3 * temporal


def test_full_width_forward_launch_count_and_graph_replay(switch_on):
    """One three-branch forward of the full-width model at the benchmarked size with the switch on: the getter shows the launch
    count the block structure gives; the forward captured into a HIP graph and replayed is bit-equal to the eager one; the
    prediction stays within the kernel bound of the switch-off forward (same fp16 GEMM outputs, another fp32 summation order
    in the covered GroupNorms)."""
    import gpu_checks as gc
    from anyv2v_amd import ops
    from anyv2v_amd.utils import capture_hip_graph
    m = gc.full_models("full", 1234, want=("native",))
    native = m["native"]
    inp = gc.config1_inputs(m["ocfg"], 3, FRAMES, 64)
    inp16 = {k: (v.half() if v.is_floating_point() else v) for k, v in inp.items()}
    kw = gc._cond_kw(inp16, "cuda", torch.float16)
    smp = inp16["sample"].to("cuda").contiguous()
    with torch.no_grad():
        native(smp, 981, **kw)   # prepares the clip context: every buffer exists before the counted forward and the capture
        ops.gn_launches(reset=True)
        switch_on["yes"] = switch_on["no"] = 0
        tok_eager = native.forward_tokens(smp, 981, kw["fps"], kw["image_latents"], kw["image_embeddings"],
                                          kw["encoder_hidden_states"]).clone()
        launches, expected = ops.gn_launches(reset=True), _expected_launches_per_forward(native)
        print(f"[gn-epilogue] full 3 x 16 f x 64x64 forward: launches {launches}, expected {expected}, query yes {switch_on['yes']} "
              f"no {switch_on['no']}")
        assert launches == expected == switch_on["yes"]
        ctx = native._ctx
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture_hip_graph(g):
            tok_graph = native._forward_core(ctx, smp)
        g.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(tok_eager[:, :4].float()).all()
        assert torch.equal(tok_graph[:, :4], tok_eager[:, :4]), "HIP-graph replay differs from the eager forward"   # (columns 4..7: padding)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(tok_graph[:, :4], tok_eager[:, :4]), "second replay differs"
        del g
        assert ops.gn_launches(reset=True) == expected   # the capture enqueued the same launches once more; replays do not count
        ops.GN_EPILOGUE = False   # (the fixture's monkeypatch restores the attribute)
        native._ctx = type(ctx)()  # a fresh clip context for the other setting
        tok_off = native.forward_tokens(smp, 981, kw["fps"], kw["image_latents"], kw["image_embeddings"],
                                        kw["encoder_hidden_states"])
        assert ops.gn_launches(reset=True) == 0, "switch off, but a launch emitted statistics"
        mx, l2 = _err(tok_eager[:, :4], tok_off[:, :4].float())
        print(f"[gn-epilogue] full forward, switch on vs off: max {mx:.3e} l2 {l2:.3e}")
        native._ctx = type(ctx)()


def test_full_width_config1_step_with_the_switch_on(switch_on):
    """The full-width model at config 1's size vs the fp32 CPU oracle (calibrated bound, reused) -- and the new pair really runs."""
    import gpu_checks as gc
    from anyv2v_amd import ops
    _assert_all(gc.check_n1_config1("full", 8, 32))
    launches = ops.gn_launches(reset=True)
    print(f"[gn-epilogue] full config 1: query yes {switch_on['yes']} no {switch_on['no']}, launches {launches}")
    # (several forwards of different batch / injection states at 8 f x 32x32; the count per forward is asserted from the block
    #  structure in test_full_width_forward_launch_count_and_graph_replay)
    assert launches == switch_on["yes"] > 0


def test_two_branch_steps_bit_equal_full_width_with_the_switch_on(switch_on):
    """[negative, editing] steps under batch_hint(3, 2) (replayed source features, HIP graphs) bit-equal to those branches of the
    three-branch steps, with conv1 / the temporal convolutions emitting the statistics of their consumers."""
    import gpu_checks as gc
    from anyv2v_amd import ops
    _assert_all(gc.check_source_cache("full", 16, 32, n_steps=4))
    launches = ops.gn_launches(reset=True)
    print(f"[gn-epilogue] source cache full 16 f x 256^2: query yes {switch_on['yes']}, launches {launches}")
    assert launches > 0 and switch_on["yes"] > 0
