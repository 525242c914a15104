"""The cases of tests/batch_subset_spec.py on the CPU: every GEMM and GroupNorm case is planned three times by the host planner programs
(tests/gemm_plan_main.cpp, tests/norm_plan_main.cpp, built with the host compiler under the address and undefined-behaviour sanitizers
and run as their own processes) -- the full launch (T rows, hint 1 / 1), the subset under the hint (T - r rows, hint B / (B - 1)) and the
subset without it -- and every attention case twice by tests/attention_plan_main.cpp.  Asserted per case:

 * consistent: the hinted subset has the full launch's split-K factor, its weight-stationary decision, its GroupNorm rows per chunk;
 * sharp: where the spec says so, the un-hinted subset differs from the full launch in the named word, so tests/test_batch_subset_gpu.py
   has a reason to fail if the hint were ignored; every line of the table has a sharp spec, or is `origin` only by design;
 * origin: the subset's first row r is no multiple of the tile height of the family the full launch takes (GroupNorm: the chunk does
   not divide the rows of a group), so the subset's rows sit at another tile / chunk origin than in the full launch.

The three plans of every case are printed.  No GPU.
"""
import json
import os
import shutil
import subprocess

import pytest

import batch_subset_spec as bss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anyv2v_amd", "csrc")

# rows of a tile (or strip) of each family: the origin condition
TILE_ROWS = {"big": 192, "sw": 192, "sw_streamk": 192, "swh": 192, "mfma128": 128, "ws": 32, "ws_ln": 32}


def _build(tmp, name):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp / f"{name}_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", f"{name}_plan_main.cpp"), os.path.join(CSRC, f"{name}_plan.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    plans = [json.loads(line) for line in out.stdout.splitlines()]
    assert len(plans) == len(lines)
    return plans


@pytest.fixture(scope="module")
def gemm_plans(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("bs_gemm"), "gemm")
    lines = []
    for s in bss.GEMM_SPECS:
        T, S = s["B"] * s["r"], (s["B"] - 1) * s["r"]
        lines += [bss.gemm_plan_line(s, T), bss.gemm_plan_line(s, S, hint=T), bss.gemm_plan_line(s, S)]
    p = bss.HINT_PROBE
    probe = f"mode=0 M={p['M']} N={p['N']} C0={p['K']} gn_groups=32 gn_rpg={p['M']} flags={bss.LDS_DMA}"
    lines += [probe, probe + f" hint={p['M'] * 3 // 2}"]
    plans = _run(exe, lines)
    return {s["name"]: plans[3 * i:3 * i + 3] for i, s in enumerate(bss.GEMM_SPECS)}, plans[-2:]


@pytest.fixture(scope="module")
def norm_plans(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("bs_norm"), "norm")
    lines = []
    for s in bss.NORM_SPECS:
        B, nf = s["B"], s["per_branch"] * s["B"]
        ns = nf - s["per_branch"]
        lines += [bss.norm_plan_line(s, nf), bss.norm_plan_line(s, ns, B, B - 1), bss.norm_plan_line(s, ns)]
    plans = _run(exe, lines)
    return {s["name"]: plans[3 * i:3 * i + 3] for i, s in enumerate(bss.NORM_SPECS)}


def _words(p):
    return f"family {p['family']} nf {p['nf']} splits {p['splits']} tiles {p['tiles']} grid {p['grid']}" + (f" pp_mf {p['pp_mf']}" if p["family"] == "pp" else "")


def _differs(word, full, other):
    if word == "splits":
        return full["splits"] != other["splits"]
    if word == "family":
        return full["family"] != other["family"] and full["splits"] == other["splits"] == 1
    if word == "nf":
        return full["family"] == other["family"] == "mfma128" and full["nf"] != other["nf"] and full["splits"] == other["splits"] == 1
    raise AssertionError(word)


@pytest.mark.parametrize("spec", bss.GEMM_SPECS, ids=[s["name"] for s in bss.GEMM_SPECS])
def test_gemm_case_is_consistent_sharp_and_off_origin(gemm_plans, spec):
    full, hinted, own = gemm_plans[0][spec["name"]]
    print(f"[batch-subset] {spec['name']} (line '{spec['line']}', r = {spec['r']} x {spec['B']}):\n    full     {_words(full)}\n    hinted   {_words(hinted)}"
          f"\n    unhinted {_words(own)}\n    sharp in: {spec['sharp'] or 'nothing (origin only)'}")
    assert full["status"] == hinted["status"] == own["status"] == 0, (full, hinted, own)
    forced = bss.FORCED_FAMILY_OF.get(spec["name"])
    if forced == "sw_streamk":
        # stream-K is reachable by a forced flag only (ops.GEMM_FLAGS defaults to 0), and a hinted launch with the flag must plan another family
        assert full["family"] == "sw_streamk" and hinted["family"] != "sw_streamk" and hinted["sk_blocks"] == 0 and spec["gpu_skip"]
        return
    assert not spec["gpu_skip"]
    # consistent
    assert hinted["splits"] == full["splits"], "the hinted subset does not inherit the split-K factor"
    assert (hinted["family"] in ("ws", "ws_ln")) == (full["family"] in ("ws", "ws_ln")), "the weight-stationary decision differs under the hint"
    if full["splits"] > 1:
        assert hinted["family"] == full["family"], "a split plan is inherited with its family"
    if forced is not None:
        assert full["family"] == hinted["family"] == forced and (forced != "pp" or hinted["pp_mf"] == full["pp_mf"])
    if spec["ln"]:
        assert full["family"] == hinted["family"] == "ws_ln"
    # sharp
    if spec["sharp"] is not None:
        assert _differs(spec["sharp"], full, own), f"not sharp in '{spec['sharp']}': the un-hinted subset plans like the full launch"
    # origin
    tile = 64 * full["pp_mf"] if full["family"] == "pp" else TILE_ROWS[full["family"]]
    assert spec["r"] % tile != 0, f"the subset starts on a tile boundary of the {full['family']} kernel ({tile} rows)"


def test_every_table_line_has_a_sharp_gemm_case():
    assert {s["line"] for s in bss.GEMM_SPECS} == set(bss.GEMM_LINES)
    for line in bss.GEMM_LINES:
        sharp = [s["name"] for s in bss.GEMM_SPECS if s["line"] == line and s["sharp"]]
        assert sharp or line in bss.GEMM_ORIGIN_LINES, line
    # one case each for linear, conv 3x3 and temporal on the 128-row split-K line
    assert {s["mode"] for s in bss.GEMM_SPECS if s["line"] == "128-row split-K" and s["sharp"] == "splits"} == {0, 1, 2}
    # every row with bias; rowvec, residual, two sources, GELU and GEGLU at least once
    assert all("bias" in s["epi"] or s["ln"] or s["act"] == bss.ACT_GEGLU for s in bss.GEMM_SPECS)
    assert any("rowvec" in s["epi"] for s in bss.GEMM_SPECS) and any("res" in s["epi"] for s in bss.GEMM_SPECS)
    assert any(s["C1"] for s in bss.GEMM_SPECS) and {bss.ACT_GELU, bss.ACT_GEGLU} <= {s["act"] for s in bss.GEMM_SPECS}
    assert any(s["B"] == 2 and s["sharp"] == "splits" for s in bss.GEMM_SPECS) and any(s["B"] == 2 for s in bss.NORM_SPECS)
    assert bss.FF_SPEC["r"] % 32 != 0


def test_weight_stationary_case_straddles_the_row_threshold():
    s = next(s for s in bss.GEMM_SPECS if s["line"] == "weight-stationary")
    assert s["B"] * s["r"] >= 32768 > (s["B"] - 1) * s["r"] and s["C0"] == 320


def test_hint_probe_tells_the_two_plans_apart(gemm_plans):
    plain, hinted = gemm_plans[1]
    print(f"[batch-subset] hint probe: plain {_words(plain)} records {plain['gn_records']}; hinted {_words(hinted)} records {hinted['gn_records']}")
    assert plain["splits"] > 1 and not plain["gn_records"] and hinted["splits"] == 1 and hinted["gn_records"]


@pytest.mark.parametrize("spec", bss.NORM_SPECS, ids=[s["name"] for s in bss.NORM_SPECS])
def test_groupnorm_case_is_consistent_sharp_and_off_origin(norm_plans, spec):
    full, hinted, own = norm_plans[spec["name"]]
    w = lambda p: f"nsg {p['nsg']} rpb {p['rpb']} nchunks {p['nchunks']} rows_chunk {p['rows_chunk']}"
    print(f"[batch-subset] {spec['name']} (rows/group {spec['rpg']}):\n    full     {w(full)}\n    hinted   {w(hinted)}\n    unhinted {w(own)}\n    sharp in: rows_chunk")
    assert full["status"] == hinted["status"] == own["status"] == 0
    assert (hinted["rows_chunk"], hinted["nchunks"], hinted["rpb"]) == (full["rows_chunk"], full["nchunks"], full["rpb"])
    assert own["rows_chunk"] != full["rows_chunk"], "not sharp: the un-hinted subset chunks like the full launch"
    assert spec["rpg"] % full["rows_chunk"] != 0 and spec["rpg"] % full["rpb"] != 0
    # the two-phase entry points size their partial sums by the same plan
    assert hinted["partial_floats"] * full["nsg"] == full["partial_floats"] * hinted["nsg"]


def test_groupnorm_records_case_folds(norm_plans):
    s = bss.NORM_RECORDS
    rec = bss.NORM_RECORDS["rpg"] // 16
    assert s["rpg"] % 16 == 0 and rec > 256 and rec % 2 == 1 and (s["per_branch"] * s["rpg"]) % 128 != 0   # folded in runs of 2, the last run one record


@pytest.fixture(scope="module")
def attn_plans(tmp_path_factory):
    import torch

    import gpu_checks as gc
    exe = _build(tmp_path_factory.mktemp("bs_attn"), "attention")
    meta = lambda rows, cols: torch.empty(rows, cols, dtype=torch.float16, device="meta")
    lines, names = [], []
    for s in bss.ATTN_SPECS:
        C = s["heads"] * s["d"]
        for batch in (s["batch"], s["batch"] - s["sub"]):
            Mq, Mk, inner, qst, kst = gc._bs_attn_layout(s, batch, s["Sq"], s["Sk"])
            if s["kv_div"] == 1 and s["Sq"] == s["Sk"]:
                m = meta(Mq, 3 * C)
                q, k, v = m[:, :C], m[:, C:2 * C], m[:, 2 * C:]
            else:
                kv = meta(Mk, 2 * C)
                q, k, v = meta(Mq, C), kv[:, :C], kv[:, C:]
            extra = {} if s["d"] == 64 else dict(scale=s["d"] ** -0.5, head_dim=s["d"])
            lines.append(gc.attn_plan_words(q, k, v, meta(Mq, C), batch=batch, heads=s["heads"], Sq=s["Sq"], Sk=s["Sk"], inner=inner, q_strides=qst,
                                            kv_strides=kst, kv_div=s["kv_div"], **extra))
        names.append(s["name"])
    for s in bss.ATTN_PNP_SPECS:
        e, C = s["per_branch"], 64 * s["heads"]
        M3, _mk, inner, st, _ = gc._bs_attn_layout(s, 3 * e, s["S"], s["S"])
        m3, src, m2 = meta(M3, 3 * C), meta(M3 // 3, 2 * C), meta(2 * M3 // 3, 3 * C)
        kw = dict(heads=s["heads"], Sq=s["S"], Sk=s["S"], inner=inner, q_strides=st, kv_strides=st)
        lines.append(gc.attn_plan_words(m3[:, :C], m3[:, C:2 * C], m3[:, 2 * C:], meta(M3, C), batch=3 * e, qk_mod=e, **kw))
        lines.append(gc.attn_plan_words(src[:, :C], src[:, C:], m2[:, 2 * C:], meta(2 * M3 // 3, C), batch=2 * e, qk_mod=e, **kw))
        names.append(s["name"])
    plans = _run(exe, lines)
    return {n: plans[2 * i:2 * i + 2] for i, n in enumerate(names)}


@pytest.mark.parametrize("spec", bss.ATTN_SPECS + bss.ATTN_PNP_SPECS, ids=[s["name"] for s in bss.ATTN_SPECS + bss.ATTN_PNP_SPECS])
def test_attention_case_takes_the_kernels_it_names(attn_plans, spec):
    full, sub = attn_plans[spec["name"]]
    print(f"[batch-subset] {spec['name']}: full {full['name']} grid {full['grid']}; subset {sub['name']} grid {sub['grid']}")
    assert full["status"] == sub["status"] == 0
    assert (full["name"], sub["name"]) == (spec["full"], spec["subset"])
    if full["kernel"] == "short":   # units = batch x heads, four to a block: the subset's first unit sits inside a block
        first = (spec["sub"] if "sub" in spec else spec["per_branch"]) * spec["heads"]
        assert first % 4 != 0
    if full["kernel"] == "flash" and "sub" in spec:
        assert spec["Sq"] % (128 if full["waves"] == 4 else 256) != 0   # a ragged last query tile per (element, head)
