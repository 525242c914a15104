"""The exact-data builders of tests/gpu_checks.py (check_gemm_exact, check_attention_exact) on the CPU: the conditions that make the
expected outputs exact hold for every case, the references agree with an independent evaluation, and the comparisons can fail."""
import pytest
import torch
import torch.nn.functional as F

import gpu_checks as gc
from anyv2v_amd import ops

GEMM_SPECS = gc.exact_gemm_specs()
ATTN_SPECS = gc.exact_attention_specs()
ATTN_CASES = [(s, p) for s in ATTN_SPECS for p in gc.exact_attention_patterns(s)]


@pytest.mark.parametrize("name", list(GEMM_SPECS))
def test_gemm_case_conditions(name):
    spec = GEMM_SPECS[name]
    case = gc.exact_gemm_case(spec)
    c = gc.exact_gemm_conditions(case)
    assert case["r"] == (8 if case["K"] <= 4096 else 4)          # the ranges the data is meant to have: nothing had to shrink
    assert c["abs_bound"] < 2 ** 18                               # every partial sum in any order is exact in fp32
    assert c["vmax"] <= 32768                                     # no fp16 overflow
    assert c["unrepresentable"] >= 0.25                           # the first rounding is a real one ...
    assert c["ties"] >= 1                                         # ... and meets an exact tie
    if spec["res"]:
        assert c["single_differs"] >= 0.01                        # rounding once, after the residual, is visibly another result
    # the operands are what the builder says: integers / multiples of 2^-4 in range, exactly representable in fp16
    for key, lim, step in (("a0", case["r"], 1.0), ("a1", case["r"], 1.0), ("w", case["r"], 1.0), ("bias", 32, 16.0), ("rowvec", 32, 16.0),
                           ("res", 64, 16.0)):
        t = case[key]
        if t is not None:
            t = t.double() * step
            assert t.dtype == torch.float64 and bool((t == t.round()).all()) and float(t.abs().max()) <= lim * step
    assert (case["rowvec"] is not None) == bool(spec["rowvec_div"]) and (case["res"] is not None) == spec["res"]


def _gemm_fp32(case):
    """The contract evaluated in fp32 torch ops from the fp16 operands, independently of the builder's float64 path."""
    spec = case["spec"]
    a = case["a0"].float() if case["a1"] is None else torch.cat([case["a0"], case["a1"]], 1).float()
    ci, N, M = a.shape[1], spec["N"], spec["M"]
    w = case["w"].float()
    if spec["mode"] == ops.MODE_LINEAR:
        v = a @ w.t()
    elif spec["mode"] == ops.MODE_CONV2D:
        n, H, W, Ho, Wo, stride, up, asym = spec["geo"]
        x = a.view(n, H, W, ci).permute(0, 3, 1, 2)
        if up:
            x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
        x = F.pad(x, (0, 1, 0, 1)) if asym else F.pad(x, (1, 1, 1, 1))
        cols = F.unfold(x, 3, stride=stride)                                   # [n, ci * 9, Ho * Wo], rows (channel, tap)
        wk = w.view(N, 9, ci).permute(0, 2, 1).reshape(N, ci * 9)             # packed [N, tap, channel] -> (channel, tap)
        v = (wk @ cols).permute(0, 2, 1).reshape(M, N)
    else:
        B, Fr, HW = spec["geo"]
        x = F.pad(a.view(B, Fr, HW, ci), (0, 0, 0, 0, 1, 1))                   # one zero frame before and after
        v = sum(x[:, t:t + Fr].reshape(M, ci) @ w[:, t * ci:(t + 1) * ci].t() for t in range(3))
    v = v + case["bias"].float()
    if case["rowvec"] is not None:
        v = v + case["rowvec"].float()[torch.arange(M) // spec["rowvec_div"]]
    if spec["act"] == ops.ACT_F32OUT:
        return v
    h = v.half()
    return h if case["res"] is None else (h.float() + case["res"].float()).half()


@pytest.mark.parametrize("name", list(GEMM_SPECS))
def test_gemm_reference_agrees_with_fp32_evaluation_bit_for_bit(name):
    case = gc.exact_gemm_case(GEMM_SPECS[name])
    got = _gemm_fp32(case)
    assert got.dtype == case["want"].dtype and torch.equal(got, case["want"])
    if GEMM_SPECS[name]["act"] == ops.ACT_F32OUT:
        assert torch.equal(case["want"].double(), case["v"])                    # the fp32 output holds the exact value


@pytest.mark.parametrize("name", [n for n, s in GEMM_SPECS.items() if s["res"]])
def test_single_rounding_fails_the_exact_comparison(name):
    case = gc.exact_gemm_case(GEMM_SPECS[name])
    row = gc._count_row("single rounding", case["single"] != case["want"])
    assert not row["ok"] and row["err"] >= 0.01 * case["want"].numel() and row["tol"] == 0.0
    assert gc._count_row("contract", case["want"].clone() != case["want"])["ok"]


def test_every_family_has_a_launch_and_the_cross_shape():
    launches = gc.exact_gemm_launches()
    assert {l[0] for l in launches} == set(gc.XG_GROUPS) - {"cross-family"}
    for fam, _bits in gc.PERSISTENT_FAMILIES:
        assert any(l[1] == fam and l[6] is None for l in launches), fam
        assert any(l[1] == fam and l[6] is None and l[2] == gc.XG_CROSS for l in launches), fam
    assert all(l[2] in GEMM_SPECS for l in launches)
    assert {l[2] for l in launches} == set(GEMM_SPECS)                          # no spec is built and never launched


def test_tie_detector():
    v = torch.tensor([2049.0, 2050.0, 2051.0, 128.0625, 128.125, 0.0, -4097.0, -4098.0, 4100.0], dtype=torch.float64)
    assert gc._fp16_tie(v).tolist() == [True, False, True, True, False, False, False, True, False]


# ---- attention
def _ids(cases):
    return [f"{s['kernel']}: {s['name']}, {p}" for s, p in cases]


def _some_elements(spec):
    """All batch elements where fp32 SDPA on the CPU is cheap; the first, a middle one of another branch and the last otherwise."""
    b = spec["batch"]
    return list(range(b)) if b * spec["heads"] * spec["Sq"] * spec["Sk"] <= 4e6 else sorted({0, b // 2 + 1, b - 1})


@pytest.mark.parametrize("spec,pattern", ATTN_CASES, ids=_ids(ATTN_CASES))
def test_attention_expectation_follows_from_fp32_sdpa(spec, pattern):
    case = gc.exact_attention_case(spec, pattern)
    b, h, Sq, Sk, d = spec["batch"], spec["heads"], spec["Sq"], spec["Sk"], spec["d"]
    only = _some_elements(spec)
    o = gc.exact_attention_sdpa(case, only).half()                              # [len(only), Sq, C]
    want = case["want"].view(b, Sq, h * d)[only]
    bad = gc.exact_attention_bad(dict(case, want=want), o)
    assert not bool(bad.any()), int(bad.sum())
    assert torch.equal(case["rows"].sort().values, case["rows"].unique())       # no output row is written twice
    for t in (case["q"], case["k"], case["v"]):
        assert t.dtype == torch.float16 and bool(torch.isfinite(t).all())
    if pattern == "counting":
        assert Sk <= 1024 and bool((want == 1.0).all())
        assert sorted(set(case["key_c"].reshape(-1).tolist())) == case["keys"]  # every key of the sweep holds a value somewhere
        assert {0, Sk - 1} <= set(case["keys"]) and all(k in case["keys"] for t in range(0, Sk - 15, 16) for k in (t, t + 15))
    if pattern == "causal edge":
        assert sorted(set(case["key_c"].reshape(-1).tolist())) == case["keys"]
        assert all(k in case["keys"] for k in (0, 63, 64, 65) if k < Sk) and all(k in case["keys"] for k in (95, 96, 97) if k < Sk)
        assert bool((want == 0).any()) and bool((want != 0).any())


SELECTION = [(s, p) for s, p in ATTN_CASES if p == "selection"]


@pytest.mark.parametrize("spec,pattern", SELECTION, ids=_ids(SELECTION))
def test_selection_is_exactly_one_hot_and_reaches_every_key(spec, pattern):
    case = gc.exact_attention_case(spec, pattern)
    b, h, Sq, Sk, d = spec["batch"], spec["heads"], spec["Sq"], spec["Sk"], spec["d"]
    pi = case["pi"]                                                             # [batch, heads, Sq]
    assert tuple(pi.shape) == (b, h, Sq) and int(pi.min()) >= 0 and int(pi.max()) < Sk
    assert pi.unique().numel() == Sk                                            # every key index is a target in this launch
    if spec["causal"]:
        assert bool((pi <= torch.arange(Sq)).all())                             # ... and a visible one
    gain = gc.exact_attention_gain(case["scale"])
    assert 2 * gain * case["scale"] * 1.4426950408889634 >= 160 > gain * case["scale"] * 1.4426950408889634
    rq, rkv, i, iq, n_kv, Mq, Mk = gc._xa_layout(spec)
    for e in _some_elements(spec):
        q = case["q"][rq[iq[e]]].float().view(Sq, h, d).transpose(0, 1)        # [h, Sq, d]
        k = case["k"][rkv[iq[e] // spec["kv_div"]]].float().view(Sk, h, d).transpose(0, 1)
        s = case["scale"] * (q @ k.transpose(1, 2))
        if case["bias"] is not None:
            s = s + case["bias"]
        if spec["causal"]:
            s = s.masked_fill(torch.arange(Sk)[None, :] > torch.arange(Sq)[:, None], float("-inf"))
        p = torch.softmax(s, -1)
        assert torch.equal(p, F.one_hot(pi[e], Sk).float())
    if spec["qk_mod"]:   # three streams: the branches share pi and each expects ITS OWN V row
        m = spec["qk_mod"]
        want = case["want"].view(b, Sq, h * d)
        assert torch.equal(pi[:m], pi[m:2 * m]) and torch.equal(pi[:m], pi[2 * m:])
        assert not torch.equal(want[:m], want[m:2 * m]) and not torch.equal(want[:m], want[2 * m:]) and not torch.equal(want[m:2 * m], want[2 * m:])
    if case["bias"] is not None:
        assert tuple(case["bias"].shape) == (h, Sq, Sk) and not torch.equal(pi[0, 0], pi[0, 1])   # another permutation per head


SHIFTED = SELECTION[:3] + [c for c in SELECTION if c[0]["kernel"] == "generic"][-3:]   # flash kernels; generic with and without the naive flag


@pytest.mark.parametrize("spec,pattern", SHIFTED, ids=_ids(SHIFTED))
def test_a_v_row_shifted_by_one_key_fails_the_selection(spec, pattern):
    case = gc.exact_attention_case(spec, pattern)
    rq, rkv, i, iq, n_kv, Mq, Mk = gc._xa_layout(spec)
    v = case["v"].clone()
    key = int(case["pi"][0, 0, 0])
    v[rkv[0, key]] = case["v"][rkv[0, (key + 1) % spec["Sk"]]]                  # key's V row read from its neighbour
    o = gc.exact_attention_sdpa(dict(case, v=v), [0]).half()
    want = case["want"].view(spec["batch"], spec["Sq"], -1)[[0]]
    bad = gc.exact_attention_bad(dict(case, want=want), o)
    assert bool(bad.any()) and not bool(gc.exact_attention_bad(dict(case, want=want), gc.exact_attention_sdpa(case, [0]).half()).any())


def test_counting_sees_a_dropped_and_a_doubled_key():
    """At Sk <= 1024 neither Sk / (Sk - 1) nor Sk / (Sk + 1) rounds to 1.0 in fp16."""
    for Sk in sorted({s["Sk"] for s, p in ATTN_CASES if p == "counting"} | {1024}):
        for l in (Sk - 1, Sk + 1):
            assert float(torch.tensor(Sk / l, dtype=torch.float64).half()) != 1.0, (Sk, l)


def test_every_kernel_has_its_shapes():
    assert {s["kernel"] for s in ATTN_SPECS} == set(gc.XA_KERNELS)
    assert all("selection" in gc.exact_attention_patterns(s) for s in ATTN_SPECS)
    assert {s["kernel"] for s, p in ATTN_CASES if p == "causal edge"} == {"whole-sequence MFMA", "96-key loop", "generic"}
    # every instantiation behind a kernel's name has a shape of its own (tests/test_attention_plan_host.py plans each spec and holds
    # ``instantiation`` against the planner's answer, and this set against the planner's list)
    for kernel in gc.XA_KERNELS:
        assert {s["instantiation"] for s in ATTN_SPECS if s["kernel"] == kernel} == set(gc.ATTN_KERNEL_INSTANTIATIONS[kernel]), kernel
