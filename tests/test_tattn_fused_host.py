"""The plan of the fused temporal QKV + attention kernel (anyv2v_amd/csrc/tattn_plan.cpp) on the CPU: what it covers, from where it
pays, how the (head, strip range) pairs are dealt to the blocks and how much LDS a block takes.  The plan is plain C++; this test
builds it with the host compiler under the address and undefined-behaviour sanitizers next to tests/tattn_plan_main.cpp, runs that
program once as its own process, and holds ``ops.temporal_qkv_attn_supported`` against it on the same cases.  No GPU.
"""
import json
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anyv2v_amd", "csrc")

# (name, rows_per_branch, B, C, heads, F, HW, supported, pays)
CASES = [
    ("bench_b3", 16 * 4096, 3, 320, 5, 16, 4096, 1, 1),
    ("bench_b1", 16 * 4096, 1, 320, 5, 16, 4096, 1, 1),
    ("f15", 15 * 4096, 1, 320, 5, 15, 4096, 0, 0),
    ("f17", 17 * 4096, 1, 320, 5, 17, 4096, 0, 0),
    ("hw_odd", 16 * 4095, 1, 320, 5, 16, 4095, 0, 0),
    ("hw_even_small", 16 * 2, 1, 320, 5, 16, 2, 1, 0),
    ("c312", 16 * 4096, 1, 312, 5, 16, 4096, 0, 0),
    ("heads4", 16 * 4096, 1, 320, 4, 16, 4096, 0, 0),
    ("rows_32768", 32768, 1, 320, 5, 16, 2048, 1, 1),          # the threshold itself: HW = 2048
    ("rows_32736", 32736, 2, 320, 5, 16, 2046, 1, 0),          # the largest even HW below it
    ("rows_32767", 32767, 1, 320, 5, 16, 2048, 0, 0),          # 32 767 rows are not F x HW for any HW: not a temporal token matrix
    ("ragged", 16 * 2050, 1, 320, 5, 16, 2050, 1, 1),
    ("tiny_b2", 16 * 6, 2, 320, 5, 16, 6, 1, 0),
    ("rows_mismatch", 16 * 4096, 1, 320, 5, 16, 2048, 0, 0),
    ("too_many_rows", 16 * 4096, 40000, 320, 5, 16, 4096, 0, 0),   # B x F x HW >= 2^31
]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("tattn_plan") / "tattn_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "tattn_plan_main.cpp"),
                    os.path.join(CSRC, "tattn_plan.cpp"), "-o", exe], check=True)
    text = "".join(f"{c[1]} {c[2]} {c[3]} {c[4]} {c[5]} {c[6]}\n" for c in CASES)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    return {c[0]: json.loads(line) for c, line in zip(CASES, lines)}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_eligibility(plans, case):
    name, _rows, _B, _C, _heads, _F, _HW, supported, pays = case
    got = plans[name]
    assert (got["supported"], got["pays"]) == (supported, pays), got


@pytest.mark.parametrize("case", [c for c in CASES if c[7]], ids=[c[0] for c in CASES if c[7]])
def test_grid_covers_every_strip_once_and_lds_fits(plans, case):
    name, _rows, B, _C, heads, _F, HW = case[:7]
    got = plans[name]
    assert got["covered"] == 1, got
    assert got["nstrips"] == B * HW // 2
    assert got["grid"] == 8 * got["px"] * heads <= 256 and got["px"] * heads <= 32      # at most the 32 CUs of an XCD
    assert 8 * got["px"] * got["spr"] >= got["nstrips"]
    assert 0 < got["lds_bytes"] <= 160 * 1024
    # W slab + b' + c1 + one Q | K patch per wave
    assert got["lds_bytes"] == 192 * 320 * 2 + 192 * 2 + 192 * 4 + 8 * 16 * 136 * 2


def test_hand_worked_plans(plans):
    # B = 3, HW = 4096: 6144 strips on 8 x 6 = 48 ranges of 128; 240 blocks
    assert {k: plans["bench_b3"][k] for k in ("nstrips", "px", "spr", "grid")} == dict(nstrips=6144, px=6, spr=128, grid=240)
    # B = 1, HW = 2050: 1025 strips, ceil(1025 / 48) = 22 per range
    assert {k: plans["ragged"][k] for k in ("nstrips", "spr")} == dict(nstrips=1025, spr=22)


class _Cuda:
    """Stands for a GPU tensor: the predicate reads ``is_cuda`` only."""
    is_cuda = True


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_python_predicate_agrees_with_the_plan(plans, case, monkeypatch):
    from anyv2v_amd import ops
    monkeypatch.delenv("ANYV2V_TATTN_FUSED", raising=False)
    monkeypatch.setattr(ops, "TATTN_FUSED_DEFAULT", "1")   # the agreement is about shapes, whatever the shipped default
    monkeypatch.setattr(ops, "FORCE_NAIVE", False)
    monkeypatch.setattr(ops, "USE_GLDS", True)
    monkeypatch.setattr(ops, "GEMM_FLAGS", 0)
    monkeypatch.setattr(ops, "ATTN_FLAGS", 0)
    name, rows, B, C, heads, F, HW = case[:7]
    got = plans[name]
    if name == "too_many_rows":   # a launch-size limit: the predicate sees one branch's rows, the entry point refuses the launch
        return
    assert ops.temporal_qkv_attn_supported(rows, C, heads, F, HW, _Cuda()) == bool(got["supported"] and got["pays"])
    assert ops.temporal_qkv_attn_supported(rows, C, heads, F, HW) == bool(got["supported"] and got["pays"])


def test_python_predicate_switches(monkeypatch):
    from anyv2v_amd import ops
    monkeypatch.setattr(ops, "TATTN_FUSED_DEFAULT", "1")
    monkeypatch.setattr(ops, "FORCE_NAIVE", False)
    monkeypatch.setattr(ops, "USE_GLDS", True)
    monkeypatch.setattr(ops, "GEMM_FLAGS", 0)
    monkeypatch.setattr(ops, "ATTN_FLAGS", 0)
    monkeypatch.delenv("ANYV2V_TATTN_FUSED", raising=False)
    args = (16 * 4096, 320, 5, 16, 4096)
    assert ops.temporal_qkv_attn_supported(*args, _Cuda())
    assert not ops.temporal_qkv_attn_supported(*args, torch.zeros(4, 320, dtype=torch.float16))     # a CPU tensor
    monkeypatch.setenv("ANYV2V_TATTN_FUSED", "0")
    assert not ops.temporal_qkv_attn_supported(*args, _Cuda())
    monkeypatch.setenv("ANYV2V_TATTN_FUSED", "1")
    assert ops.temporal_qkv_attn_supported(*args, _Cuda())
    monkeypatch.setattr(ops, "FORCE_NAIVE", True)
    assert not ops.temporal_qkv_attn_supported(*args, _Cuda())
    monkeypatch.setattr(ops, "FORCE_NAIVE", False)
    monkeypatch.setattr(ops, "USE_GLDS", False)
    assert not ops.temporal_qkv_attn_supported(*args, _Cuda())


def test_constants_mirror_the_plan_header():
    from anyv2v_amd import ops
    hdr = open(os.path.join(CSRC, "tattn_plan.h")).read()
    assert f"constexpr int TATTN_MIN_ROWS = {ops.TATTN_MIN_ROWS};" in hdr
