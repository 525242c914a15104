"""The GroupNorm launch planner (anyv2v_amd/csrc/norm_plan.cpp) on the CPU: block size, chunking, apply partition, record folding and the
three buffer-size rules.  The planner is plain C++; this test builds it with the host compiler under the address and undefined-behaviour
sanitizers, next to tests/norm_plan_main.cpp, runs that program once as its own process and compares the plans with

 * a table worked out BY HAND from `gn_plan` of norm.hip as it stood before the planner existed (commit 25a6953) -- each row says how;
 * that commit's own answers: tests/norm_plan_recorded.json holds what its anyv2v_groupnorm_partial_floats (= nsg * nchunks * G * 2, so
   the chunk count) returned for SWEEP under three batch hints, written by `python tests/test_norm_plan_host.py --record LIB` with LIB the
   library built from that commit (no GPU needed: the call only plans);
 * invariants over the same sweep: the chunks and the apply blocks cover a statistics group exactly, the fields that decide the order of
   the additions do not depend on the occupancy, the scratch buffer has room for the pivots behind the partial sums.

No GPU.
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anyv2v_amd", "csrc")
RECORDED = os.path.join(ROOT, "tests", "norm_plan_recorded.json")
RECORDED_AT = "25a6953"   # the commit whose library wrote RECORDED

HINTS = [(1, 1), (3, 2), (2, 3)]
SWEEP_C = [8, 64, 320, 640, 1280, 1920, 2560]
SWEEP_ROWS = [1, 2, 7, 13, 64, 127, 257, 1021, 4099, 16384, 65536 + 37]
SWEEP_NSG = [1, 2, 3, 8, 16, 48]
SWEEP_G = [4, 8, 32]


def sweep():
    """(C, rows_per_group, nsg, G): every (C, rows) pair with 4 of the 18 (nsg, G) pairs, rotating so that each pair meets each C and
    short and long groups.  C = 8 with G = 32 is no valid GroupNorm: the recorded answer is -1, and must stay -1."""
    pairs = [(nsg, G) for nsg in SWEEP_NSG for G in SWEEP_G]
    out = []
    for ci, C in enumerate(SWEEP_C):
        for ri, rows in enumerate(SWEEP_ROWS):
            i = ci * len(SWEEP_ROWS) + ri
            out += [(C, rows) + pairs[(4 * i + 5 * k) % len(pairs)] for k in range(4)]
    return out


SWEEP = sweep()


def record(lib_path):
    lib = ctypes.CDLL(lib_path)
    lib.anyv2v_groupnorm_partial_floats.restype = ctypes.c_int64
    rows = []
    for C, rpg, nsg, G in SWEEP:
        got = []
        for num, den in HINTS:
            assert lib.anyv2v_set_batch_hint(num, den) == 0
            got.append(int(lib.anyv2v_groupnorm_partial_floats(nsg * rpg, rpg, G, C)))
        rows.append([C, rpg, nsg, G, got])
    lib.anyv2v_set_batch_hint(1, 1)
    with open(RECORDED, "w") as f:
        f.write('{"commit": "%s", "what": "anyv2v_groupnorm_partial_floats(nsg * rows, rows, G, C) under batch hints %s",\n "rows": [\n' %
                (RECORDED_AT, " ".join(f"{n}/{d}" for n, d in HINTS)))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n]}\n")
    print(f"{len(rows)} shapes -> {RECORDED}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# The hand table.  gn_plan at 25a6953, for C = C0 + C1, V = C / 8 and r = rows_per_group:
#   rpb = max(256 / V, 1); threads = max(V rpb, 64, G); nsg_h = max(hinted rows / r, 1)
#   cap8 = ceil(r / (8 rpb))                                    ("at least 8 row iterations per thread")
#   n0 = min(ceil(1536 / nsg_h), cap8, 256); rows_chunk = ceil(r / n0); nchunks = ceil(r / rows_chunk); lds = 8 rpb C
#   b0 = max(min(slots / nsg, cap8), 1); rows_block = ceil(r / b0); bps = ceil(r / rows_block)
# Unless a row says otherwise: one source, one statistics group, G = 32, hint 1/1, 1792 slots (7 blocks x 256 CUs), aligned sources.
def plan(V, rpb, threads, nchunks, rows_chunk, lds, bps, rows_block, **more):
    return dict(V=V, rpb=rpb, threads=threads, nchunks=nchunks, rows_chunk=rows_chunk, lds=lds, bps=bps, rows_block=rows_block, **more)


def fails(message):
    return dict(status=-1, message=message)


C320 = dict(V=40, rpb=6, threads=240, lds=15360)   # 256 / 40 = 6 rows side by side; 6 x 320 x 8 bytes
# (C0, C1, rows_per_group, nsg, G) of the eight cases of gpu_checks.check_groupnorm_plan_edges -> the row below that plans it
EDGE_ROWS = {(320, 0, 4099, 2, 32): "edge_4099", (640, 0, 1021, 3, 32): "edge_1021", (320, 0, 65536 + 37, 1, 32): "edge_cap_ragged",
             (1280, 640, 12289, 2, 32): "edge_two_sources", (2560, 0, 2053, 2, 32): "edge_v320_2053", (2560, 0, 1024, 2, 32): "edge_v320_1024",
             (8, 0, 3001, 2, 4): "edge_c8_3001", (8, 0, 70001, 1, 8): "edge_c8_70001"}

ROWS = [
    # ---- the eight shapes of check_groupnorm_plan_edges ----
    # V = 40: rpb 6, 240 threads.  2 groups: 1536 / 2 = 768 > cap8 = ceil(4099 / 48) = 86 -> 86 chunks of ceil(4099 / 86) = 48 rows, and
    # ceil(4099 / 48) = 86 again.  1792 / 2 = 896 slots > 86 -> 86 blocks of 48 rows.  (The row the issue worked out.)
    ("edge_4099", "C0=320 rows=4099 nsg=2", plan(40, 6, 240, 86, 48, 15360, 86, 48, nsg=2, partial_floats=2 * 86 * 32 * 2)),
    # V = 80: rpb 3, 240 threads; 3 groups: 512 > cap8 = ceil(1021 / 24) = 43 -> rows_chunk = ceil(1021 / 43) = 24, 43 chunks; 597 slots > 43
    ("edge_1021", "C0=640 rows=1021 nsg=3", plan(80, 3, 240, 43, 24, 15360, 43, 24)),
    # 1536 and cap8 = ceil(65573 / 48) = 1367 are both over the 256-chunk cap: rows_chunk = ceil(65573 / 256) = 257, ceil(65573 / 257) = 256
    # chunks, the last one of 65573 - 255 x 257 = 38 rows.  1792 slots > cap8 -> 1367 blocks of ceil(65573 / 1367) = 48 rows
    ("edge_cap_ragged", "C0=320 rows=65573", plan(40, 6, 240, 256, 257, 15360, 1367, 48)),
    # V = 240: rpb 1, 240 threads; 768 < cap8 = ceil(12289 / 8) = 1537, over the cap: rows_chunk = ceil(12289 / 256) = 49 -> ceil(12289 / 49) =
    # 251 chunks.  896 slots < cap8: rows_block = ceil(12289 / 896) = 14 -> ceil(12289 / 14) = 878 blocks, the last one of 11 rows
    ("edge_two_sources", "C0=1280 C1=640 rows=12289 nsg=2", plan(240, 1, 240, 251, 49, 15360, 878, 14)),
    # V = 320 > 256: one row per block, 320 threads; min(768, cap8 = ceil(2053 / 8) = 257) is over the cap: rows_chunk = ceil(2053 / 256) = 9 ->
    # ceil(2053 / 9) = 229 chunks.  min(896, 257) = 257 -> rows_block = ceil(2053 / 257) = 8 -> 257 blocks
    ("edge_v320_2053", "C0=2560 rows=2053 nsg=2", plan(320, 1, 320, 229, 9, 20480, 257, 8)),
    ("edge_v320_1024", "C0=2560 rows=1024 nsg=2", plan(320, 1, 320, 128, 8, 20480, 128, 8)),       # cap8 = 128 on both passes: 8 rows each
    # V = 1: 256 rows side by side; cap8 = ceil(3001 / 2048) = 2 -> 2 chunks and 2 blocks of ceil(3001 / 2) = 1501 rows; lds 256 x 8 x 8
    ("edge_c8_3001", "C0=8 rows=3001 nsg=2 G=4", plan(1, 256, 256, 2, 1501, 16384, 2, 1501)),
    # cap8 = ceil(70001 / 2048) = 35 -> rows_chunk = ceil(70001 / 35) = 2001 -> ceil(70001 / 2001) = 35
    ("edge_c8_70001", "C0=8 rows=70001 G=8", plan(1, 256, 256, 35, 2001, 16384, 35, 2001)),
    # ---- its two batch-hint cases: 8 groups of 16 x 1024 rows ----
    # 1536 / 8 = 192 < cap8 = ceil(16384 / 48) = 342 -> rows_chunk = ceil(16384 / 192) = 86 -> ceil(16384 / 86) = 191 chunks (not 192).
    # 1792 / 8 = 224 slots -> rows_block = ceil(16384 / 224) = 74 -> ceil(16384 / 74) = 222 blocks
    ("hint_plain", "C0=320 rows=16384 nsg=8", plan(40, 6, 240, 191, 86, 15360, 222, 74)),
    # hinted as 8 x 3 / 2 = 12 groups: 1536 / 12 = 128 chunks of 128 rows; the apply partition sees the true 8 groups
    ("hint_3_2", "C0=320 rows=16384 nsg=8 num=3 den=2", plan(40, 6, 240, 128, 128, 15360, 222, 74)),
    # ---- the 1536-block target against cap8: C = 320, 4608 = 96 x 48 rows, cap8 = 96 ----
    ("target_above_cap8", "C0=320 rows=4608 nsg=15", dict(nchunks=96, rows_chunk=48, **C320)),     # ceil(1536 / 15) = 103 > 96
    ("target_at_cap8", "C0=320 rows=4608 nsg=16", dict(nchunks=96, rows_chunk=48, **C320)),        # 1536 / 16 = 96
    # ceil(1536 / 17) = 91 < 96: rows_chunk = ceil(4608 / 91) = 51 -> ceil(4608 / 51) = 91
    ("target_below_cap8", "C0=320 rows=4608 nsg=17", dict(nchunks=91, rows_chunk=51, **C320)),
    # the hint counts whole groups and never fewer than one: 65573 x 2 / 3 rows are 0 groups -> 1, the plan of edge_cap_ragged
    ("hint_below_one_group", "C0=320 rows=65573 num=2 den=3", plan(40, 6, 240, 256, 257, 15360, 1367, 48)),
    # 3 groups hinted as 2: a target of 768 instead of 512, but cap8 = ceil(12000 / 48) = 250 decides either way: 250 chunks of 48 rows
    ("hint_2_3_cap8_decides", "C0=320 rows=12000 nsg=3 num=2 den=3", dict(nchunks=250, rows_chunk=48)),
    # 48 groups, 4099 rows: 1536 / 48 = 32 -> rows_chunk = ceil(4099 / 32) = 129 -> 32 chunks; hinted 3/2 as 72: ceil(1536 / 72) = 22 ->
    # ceil(4099 / 22) = 187 -> 22; hinted 2/3 as 32: 48 -> ceil(4099 / 48) = 86 -> ceil(4099 / 86) = 48
    ("hint_48_plain", "C0=320 rows=4099 nsg=48", dict(nchunks=32, rows_chunk=129, partial_floats=98304)),
    ("hint_48_3_2", "C0=320 rows=4099 nsg=48 num=3 den=2", dict(nchunks=22, rows_chunk=187, partial_floats=67584)),
    ("hint_48_2_3", "C0=320 rows=4099 nsg=48 num=2 den=3", dict(nchunks=48, rows_chunk=86, partial_floats=147456)),
    # more hinted groups than target blocks: ceil(1536 / 2000) = 1 chunk of all 64 rows (cap8 = ceil(64 / 48) = 2 would allow 2, as it does
    # for 48 groups: 32 > 2 -> 2 chunks of 32).  1792 / 2000 = 0 slots per group -> 1 block
    ("target_one_chunk", "C0=320 rows=64 nsg=2000", plan(40, 6, 240, 1, 64, 15360, 1, 64)),
    ("target_cap8_two", "C0=320 rows=64 nsg=48", plan(40, 6, 240, 2, 32, 15360, 2, 32)),            # 1792 / 48 = 37 > 2
    # ---- "at least 8 row iterations": 48 rows are one chunk and one block, 49 rows two of ceil(49 / 2) = 25 ----
    ("cap8_48", "C0=320 rows=48", plan(40, 6, 240, 1, 48, 15360, 1, 48)),
    ("cap8_49", "C0=320 rows=49", plan(40, 6, 240, 2, 25, 15360, 2, 25)),
    ("cap8_1", "C0=320 rows=1", plan(40, 6, 240, 1, 1, 15360, 1, 1)),
    # ---- the 256-chunk cap: cap8 = 256 at 12288 = 256 x 48 rows; one row more: cap8 = 257 -> 256 -> rows_chunk 49 -> 251 chunks ----
    ("cap256_at", "C0=320 rows=12288", plan(40, 6, 240, 256, 48, 15360, 256, 48)),
    ("cap256_past", "C0=320 rows=12289", plan(40, 6, 240, 251, 49, 15360, 257, 48)),              # the apply pass has no such cap: ceil(12289 / 48)
    # ---- block sizes ----
    ("v128", "C0=1024 rows=64", plan(128, 2, 256, 4, 16, 16384, 4, 16)),                            # cap8 = 64 / 16
    # V x (256 / V) is smallest at V = 129 (one row of 129 vectors): the floors at 64 threads and at G <= 64 threads cannot bind
    ("v129", "C0=1032 rows=64 G=8", plan(129, 1, 129, 8, 8, 8256, 8, 8, gn_threads=129)),
    ("v256", "C0=2048 rows=64", plan(256, 1, 256, 8, 8, 16384, 8, 8)),
    ("v257", "C0=2056 rows=64 G=8", plan(257, 1, 257, 8, 8, 16448, 8, 8)),
    # the widest row: 1024 threads, 64 KiB of LDS exactly (so "LDS reduction buffer too large" cannot fire after "C too large")
    ("v1024", "C0=8192 rows=8", plan(1024, 1, 1024, 1, 8, 65536, 1, 8, gn_threads=1024)),
    ("g64", "C0=512 rows=64 G=64", plan(64, 4, 256, 2, 32, 16384, 2, 32, gn_threads=256)),         # cap8 = ceil(64 / 32)
    # ---- the apply partition: C = 320, 2 groups of 4099 rows, cap8 = 86 ----
    ("slots_past_cap", "C0=320 rows=4099 nsg=2 slots=174", dict(bps=86, rows_block=48, nchunks=86, rows_chunk=48)),     # 87 > 86
    ("slots_at_cap", "C0=320 rows=4099 nsg=2 slots=172", dict(bps=86, rows_block=48, nchunks=86, rows_chunk=48)),
    # 171 / 2 = 85 < 86: rows_block = ceil(4099 / 85) = 49 -> ceil(4099 / 49) = 84 blocks, the last one of 32 rows; the chunks stay
    ("slots_below_cap", "C0=320 rows=4099 nsg=2 slots=171", dict(bps=84, rows_block=49, nchunks=86, rows_chunk=48)),
    ("slots_below_one", "C0=320 rows=4099 nsg=2 slots=1", dict(bps=1, rows_block=4099, nchunks=86, rows_chunk=48)),     # 1 / 2 = 0 -> 1
    ("slots_2048", "C0=320 rows=16384 nsg=8 slots=2048", dict(bps=256, rows_block=64, nchunks=191, rows_chunk=86)),     # 2048 / 8
    # ---- every check, in the order it is made ----
    ("bad_c0", "C0=0 rows=8", fails("groupnorm: bad C0/C1")),
    ("bad_c1", "C0=64 C1=-8 rows=8", fails("groupnorm: bad C0/C1")),
    ("c0_mod_8", "C0=60 rows=8 G=4", fails("groupnorm: C0/C1 must be multiples of 8 (60,0)")),
    ("c1_mod_8", "C0=64 C1=4 rows=8 G=4", fails("groupnorm: C0/C1 must be multiples of 8 (64,4)")),
    ("g_0", "C0=64 rows=8 G=0", fails("groupnorm: bad group count 0 for C=64")),
    ("g_65", "C0=520 rows=8 G=65", fails("groupnorm: bad group count 65 for C=520")),
    ("g_no_divisor", "C0=64 rows=8 G=48", fails("groupnorm: bad group count 48 for C=64")),
    ("g_no_divisor_of_sum", "C0=64 C1=8 rows=8", fails("groupnorm: bad group count 32 for C=72")),
    ("rows_0", "C0=64 rows=0 M=8", fails("groupnorm: M % rows_per_group != 0")),
    ("m_mod_rows", "C0=64 rows=8 M=9", fails("groupnorm: M % rows_per_group != 0")),
    ("unaligned", "C0=64 rows=8 aligned=0", fails("groupnorm: pointers must be 16-byte aligned")),
    ("unaligned_after_shape", "C0=64 rows=8 M=9 aligned=0", fails("groupnorm: M % rows_per_group != 0")),
    ("c_too_large", "C0=8200 rows=8 G=8", fails("groupnorm: C too large (8200)")),
    ("unaligned_before_c", "C0=8200 rows=8 G=8 aligned=0", fails("groupnorm: pointers must be 16-byte aligned")),
    # 2^21 rows of 1024 vectors are 2^31 vectors; one row fewer plans: cap 256 -> rows_chunk = ceil((2^21 - 1) / 256) = 8192 -> 256 chunks
    ("group_too_large", "C0=8192 rows=2097152", fails("groupnorm: stat group too large (2147483648 vectors)")),
    ("group_largest", "C0=8192 rows=2097151", dict(nchunks=256, rows_chunk=8192, rpb=1)),
    # a failed plan has no partial sums; the other two sizes do not plan
    ("sizes_of_no_plan", "C0=64 rows=9 M=8", dict(status=-1, partial_floats=-1, scratch_floats=0, stats_floats=0)),
    # ---- the sizes: [nsg][1 + 256][G][2]; 3 floats per (16 rows, G) + 3 x 256 folded records per (group, G); [nsg][nchunks][G][2] ----
    ("sizes", "C0=64 rows=4096 nsg=2", dict(scratch_floats=2 * 257 * 32 * 2, stats_floats=3 * 512 * 32 + 3 * 2 * 256 * 32, nchunks=16,
                                            partial_floats=2 * 16 * 32 * 2)),                          # V = 8: rpb 32, cap8 = 4096 / 256 = 16
    ("sizes_abi_test", "C0=64 rows=8 nsg=8", dict(partial_floats=8 * 32 * 2, nchunks=1)),             # (tests/test_abi_config_dist.py)
    ("stats_rows_mod_16", "C0=64 rows=24 nsg=2", dict(status=0, stats_floats=0)),
]

# The records plan: nrec = r / 16 records of n_gemm = 16 C / G values; above 256, runs of run = ceil(nrec / 256) records, nruns = ceil(nrec
# / run), the last of nrec - (nruns - 1) run records; the folded records behind the GEMM's 3 (M / 16) G floats.  C = 64, G = 32: n_gemm = 32.
def rec(nrec, fold, run, nruns, n_rec, n_last, nsg=2):
    return dict(rec=dict(status=0, message="", nrec=nrec, fold=fold, run=run, nruns=nruns, n_gemm=32.0, n_rec=n_rec, n_last=n_last,
                         folded_at=3 * nsg * nrec * 32))


ROWS += [
    ("rec_16", "C0=64 rows=16 nsg=2", rec(1, False, 1, 1, 32.0, 32.0)),
    ("rec_at_cap", "C0=64 rows=4096 nsg=2", rec(256, False, 1, 256, 32.0, 32.0)),
    ("rec_257", "C0=64 rows=4112 nsg=2", rec(257, True, 2, 129, 64.0, 32.0)),          # 128 runs of 2 and one record
    ("rec_512", "C0=64 rows=8192 nsg=2", rec(512, True, 2, 256, 64.0, 64.0)),
    ("rec_513", "C0=64 rows=8208 nsg=2", rec(513, True, 3, 171, 96.0, 96.0)),          # 171 full runs of 3
    ("rec_514", "C0=64 rows=8224 nsg=2", rec(514, True, 3, 172, 96.0, 32.0)),          # 171 runs of 3 and one record
    ("rec_rows_mod_16", "C0=64 rows=24 nsg=2", dict(rec=dict(status=-1, message="groupnorm_apply_stats: rows_per_group must be a multiple of 16 (24)",
                                                             nrec=0, fold=False, run=0, nruns=0, n_gemm=0.0, n_rec=0.0, n_last=0.0, folded_at=0))),
]
HAND = len(ROWS)

SLOTS = [1, 1792, 2048, 10 ** 6]
ROWS += [(f"sweep C{C} r{r} x{nsg} G{G} hint {num}/{den} slots {slots}", f"C0={C} rows={r} nsg={nsg} G={G} num={num} den={den} slots={slots}", None)
         for C, r, nsg, G in SWEEP for num, den in HINTS for slots in SLOTS]
REC_SWEEP = [(C, 16 * k, nsg, G) for k in (1, 2, 255, 256, 257, 258, 511, 512, 513, 514, 1000, 4096, 4097, 65535, 65536, 65537)
             for C, G in ((64, 32), (320, 32), (2560, 4), (8, 8)) for nsg in (1, 3)]
ROWS += [(f"records C{C} r{r} x{nsg} G{G}", f"C0={C} rows={r} nsg={nsg} G={G}", None) for C, r, nsg, G in REC_SWEEP]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("norm_plan") / "norm_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "norm_plan_main.cpp"),
                    os.path.join(CSRC, "norm_plan.cpp"), "-o", exe], check=True)
    names = [r[0] for r in ROWS]
    assert len(set(names)) == len(names)
    out = subprocess.run([exe], input="".join(r[1] + "\n" for r in ROWS), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(ROWS)
    return {name: json.loads(line) for name, line in zip(names, lines)}


@pytest.mark.parametrize("name,words,want", ROWS[:HAND], ids=[r[0] for r in ROWS[:HAND]])
def test_plan(plans, name, words, want):
    got = plans[name]
    if "status" not in want and "rec" not in want:
        assert got["status"] == 0, got
    assert {k: got[k] for k in want} == want, (words, got)


def test_hand_rows_cover_the_gpu_plan_edge_cases():
    import gpu_checks as gc
    assert {c[:5] for c in gc.GN_PLAN_EDGE_CASES} == set(EDGE_ROWS) and len(gc.GN_PLAN_EDGE_CASES) == 8
    for (C0, C1, rows, nsg, G), name in EDGE_ROWS.items():
        words = dict(w.split("=") for w in dict((r[0], r[1]) for r in ROWS[:HAND])[name].split())
        assert (int(words["C0"]), int(words.get("C1", 0)), int(words["rows"]), int(words.get("nsg", 1)), int(words.get("G", 32))) == (C0, C1, rows, nsg, G)
    assert gc.GN_PLAN_HINT_CASE == (8, 16 * 1024, 320)   # hint_plain / hint_3_2


def _sweep_plan(plans, C, r, nsg, G, num, den, slots):
    return plans[f"sweep C{C} r{r} x{nsg} G{G} hint {num}/{den} slots {slots}"]


def test_planner_reproduces_the_recorded_chunk_counts(plans):
    with open(RECORDED) as f:
        recorded = json.load(f)
    assert recorded["commit"] == RECORDED_AT and [tuple(r[:4]) for r in recorded["rows"]] == SWEEP and len(SWEEP) >= 300
    differ = 0
    for C, r, nsg, G, want in recorded["rows"]:
        got = [_sweep_plan(plans, C, r, nsg, G, num, den, 1792)["partial_floats"] for num, den in HINTS]
        assert got == want, (C, r, nsg, G, got, want)
        differ += len(set(want)) > 1
    assert differ >= 20   # the hints move the chunking of a good part of the sweep


def test_sweep_invariants(plans):
    planned = 0
    for C, r, nsg, G in SWEEP:
        for num, den in HINTS:
            across = [_sweep_plan(plans, C, r, nsg, G, num, den, slots) for slots in SLOTS]
            p = across[0]
            if C % G:
                assert all(q["status"] == -1 and q["partial_floats"] == -1 for q in across)
                continue
            planned += 1
            for q in across:
                assert q["status"] == 0 and q["nsg"] == nsg and q["threads"] == q["gn_threads"] == max(q["V"] * q["rpb"], 64, G) <= 1024, q
                # the order of the additions does not depend on the occupancy
                assert [q[k] for k in ("rpb", "nchunks", "rows_chunk", "lds", "partial_floats")] == \
                    [p[k] for k in ("rpb", "nchunks", "rows_chunk", "lds", "partial_floats")], (p, q)
                # chunks and apply blocks cover the group, none of them empty
                assert q["nchunks"] <= 256 and q["nchunks"] * q["rows_chunk"] >= r > (q["nchunks"] - 1) * q["rows_chunk"], q
                assert q["bps"] * q["rows_block"] >= r > (q["bps"] - 1) * q["rows_block"], q
                assert q["lds"] == q["rpb"] * C * 8 <= 65536
                # the scratch buffer holds the partial sums and, behind them, the pivots of the sharded form (ops._groupnorm_sharded)
                assert q["partial_floats"] == nsg * q["nchunks"] * G * 2
                assert q["partial_floats"] + nsg * G <= q["scratch_floats"] == nsg * G * 2 * 257
    assert planned >= 3 * 250


def test_records_plan_invariants(plans):
    for C, r, nsg, G in REC_SWEEP:
        got = plans[f"records C{C} r{r} x{nsg} G{G}"]
        p = got["rec"]
        assert got["status"] == 0 and p["status"] == 0, got
        nrec, run, nruns = p["nrec"], p["run"], p["nruns"]
        assert nrec == r // 16 and p["fold"] == (nrec > 256) and (p["fold"] or (run, nruns) == (1, nrec))
        assert (nruns - 1) * run < nrec <= nruns * run and nruns <= 256
        assert p["n_gemm"] == 16 * (C // G) and p["n_rec"] == run * p["n_gemm"]
        assert p["n_rec"] * (nruns - 1) + p["n_last"] == r * (C // G)          # every value of a channel group, once
        assert p["folded_at"] == 3 * (nsg * r // 16) * G
        assert got["stats_floats"] == p["folded_at"] + 3 * nsg * 256 * G >= p["folded_at"] + 3 * nsg * nruns * G


def test_ops_scratch_size_is_the_librarys(plans):
    from anyv2v_amd import _lib, ops
    lib = _lib.load()
    for C, r, nsg, G in SWEEP[::7]:
        want = plans[f"sweep C{C} r{r} x{nsg} G{G} hint 1/1 slots 1792"]["scratch_floats"]
        assert ops.gn_scratch_floats(nsg * r, r, G) == lib.anyv2v_groupnorm_scratch_floats(nsg * r, r, G) == want
    assert ops.gn_scratch_floats(64, 1) == 64 * 32 * 2 * 257
    with open(ops.__file__) as f:
        src = f.read()
    assert "257" not in src and "GN_MAX_CHUNKS" not in src   # the chunk cap is written down once, in norm_plan.h


def test_library_plans_like_the_stand_alone_build(plans):
    """The library's anyv2v_groupnorm_partial_floats (norm.hip -> norm_plan.o, built by hipcc) against the g++ build of the same file."""
    from anyv2v_amd import _lib
    lib = _lib.load()
    try:
        for num, den in HINTS:
            assert lib.anyv2v_set_batch_hint(num, den) == 0
            for C, r, nsg, G in SWEEP[::5]:
                assert lib.anyv2v_groupnorm_partial_floats(nsg * r, r, G, C) == _sweep_plan(plans, C, r, nsg, G, num, den, 1)["partial_floats"]
    finally:
        lib.anyv2v_set_batch_hint(1, 1)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_norm_plan_host.py --record LIB"
    record(sys.argv[2])
    sys.exit(0)
