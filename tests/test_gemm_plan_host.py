"""The GEMM launch planner (anyv2v_amd/csrc/gemm_plan.cpp) on the CPU: which kernel family, tile width, split-K factor, grid and
tile order a descriptor gets.  The planner is plain C++; this test builds it with the host compiler under the address and
undefined-behaviour sanitizers, next to tests/gemm_plan_main.cpp, runs that program once as its own process and compares the plans
with a table worked out BY HAND from the rules of the dispatch code the planner replaced (gemm_impl / dispatch<MODE> of gemm.hip as it was
then, and the eligibility helpers of gemm_ws.hip / gemm_sw.hip / gemm_swh.hip) -- each row says how.  No GPU.

Every row: flags = 2 (LDS-DMA staging) unless it says otherwise, a 128 MiB workspace, 16-byte aligned fake pointers,
hinted rows = M, ldc = N.  nk = K-tiles of 64 = taps x (C0 + C1) / 64; tb = 192 x 320 tiles; tm = 128-row tiles; the split-K rules see
min(workspace, 64 MiB) = 67 108 864 bytes.
"""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anyv2v_amd", "csrc")

CONV64 = "mode=1 Hi=64 Wi=64 Ho=64 Wo=64 stride=1"   # 3x3 stride 1 at 64 x 64: M a multiple of 4096
CONV8 = "mode=1 Hi=8 Wi=8 Ho=8 Wo=8 stride=1"
SHAPE = ("a GEGLU / fp32-output / register-staged launch or a shape the record layout does not cover (N % 160 = 0, "
         "N / gn_groups dividing 40, M and gn_rows_per_group multiples of 16)")
GN = "gn_groups=32 gn_rpg=4096"

# (name, descriptor, expected fields of the plan)
ROWS = [
    # ---- the rows the refactoring set out with ----
    # tb = 1024 x 1 = 4 full rounds of 256 -> fills; one N-tile -> classic tile order
    ("conv64_320", f"{CONV64} M=196608 N=320 C0=320 flags=2",
     dict(family="big", splits=1, tiles=1024, grid=256, raster=[0, 0, 0, 0, 0], gn_records=False, gn_decline=SHAPE)),
    # nk = 180, tb = 16 x 4 = 64: sp = min(256 / 64, 8, 180 / 12) = 4, 64 x 4 = 256 >= 224, 4 x 3072 x 1280 x 4 B = 62.9 MB fits
    ("conv8_3072", f"{CONV8} M=3072 N=1280 C0=1280 flags=2",
     dict(tilesN=4, tiles=64, family="big", splits=4, grid=256, gn_records=False, gn_decline="a split-K plan")),
    # tb = 6 x 4 = 24: sp = 8 gives 192 < 224 work items -> 128-row kernel; t4 = 80 would split -> NF 5; tm = 8 x 8 = 64,
    # sp = min(ceil(512 / 64), 8, 180 / 8) = 8
    ("conv8_1024", f"{CONV8} M=1024 N=1280 C0=1280 flags=2", dict(family="mfma128", nf=5, splits=8, tilesN=8, tiles=64, grid=512)),
    # nk = 80, tb = 64: sp = min(4, 8, 80 / 12 = 6) = 4
    ("ffdown_3072", "mode=0 M=3072 N=1280 C0=5120 flags=2", dict(tilesN=4, tiles=64, family="big", splits=4, grid=256)),
    # K = 320 Linear, N = 6 slabs of 160, 196608 >= 32768 rows
    ("qkv_ws", "mode=0 M=196608 N=960 C0=320 flags=2",
     dict(family="ws", tilesN=6, grid=256, gn_records=False, gn_decline="the weight-stationary kernel")),
    # bit9: not weight-stationary; tb = 342 x 3 = 1026, 5 rounds, 1026 x 4 >= 5 x 256 x 3 -> fills
    ("qkv_no_ws", "mode=0 M=65536 N=960 C0=320 flags=514", dict(family="big", splits=1, tiles=1026, grid=256, raster=[0, 0, 0, 0, 0])),
    # 256 x 16 tiles, 16 N-tiles >= 8 and >= 512 tiles: 8 x 4 super-tiles, 256 / 8 = 32 x 16 / 4 = 4 of them
    ("geglu_up", "mode=0 M=49152 N=5120 C0=640 act=3 flags=2",
     dict(family="big", splits=1, tilesN=16, tiles=4096, grid=256, raster=[8, 4, 32, 4, 0], gn_records=False, gn_decline=SHAPE)),
    # ldc % 8 != 0 -> not `fast`; one thread per output: 196608 x 4 / 256 blocks
    ("conv_out", f"{CONV64} M=196608 N=4 C0=320 ldc=4 flags=2",
     dict(family="naive", grid=3072, gn_records=False, gn_decline="the naive kernel")),

    # ---- one row per remaining exit, derived from the same source the same way ----
    # bit17, dispatch's ping-pong arm: 256-row tiles 768 / (3 x 256) = 1.0, 192-row 1024 / (4 x 256) = 1.0: 1.0 + 0.02 >= 1.0 -> mf 4
    ("pp_mf4", f"{CONV64} M=196608 N=320 C0=320 flags={2 | 1 << 17}",
     dict(family="pp", pp_mf=4, tilesN=1, tiles=768, grid=256, gn_decline="the ping-pong kernel")),
    # M = 49152: 256-row tiles 192 / 256 = 0.75, 192-row tiles 256 / 256 = 1.0 -> mf 3 (plan: tb = 256 fills, unsplit)
    ("pp_mf3", f"{CONV64} M=49152 N=320 C0=320 flags={2 | 1 << 17}", dict(family="pp", pp_mf=3, tiles=256, grid=256)),
    # bit19 forces the 192-row tile, bit20 the 256-row one
    ("pp_bit19", f"{CONV64} M=196608 N=320 C0=320 flags={2 | 1 << 17 | 1 << 19}", dict(family="pp", pp_mf=3, tiles=1024, grid=256)),
    ("pp_bit20", f"{CONV64} M=49152 N=320 C0=320 flags={2 | 1 << 17 | 1 << 20}", dict(family="pp", pp_mf=4, tiles=192, grid=192)),
    # bit18 forbids it; a split plan never takes it (conv8_3072 splits 4)
    ("pp_bit18", f"{CONV64} M=196608 N=320 C0=320 flags={2 | 1 << 17 | 1 << 18}", dict(tilesN=1, tiles=1024, grid=256, family="big", splits=1)),
    ("pp_split", f"{CONV8} M=3072 N=1280 C0=1280 flags={2 | 1 << 17}", dict(tilesN=4, tiles=64, grid=256, family="big", splits=4)),
    # bit21, av_gemm_sw_eligible: N % 320 = 0, act 0, nk = 45 >= 2; av_gemm_sw_launch: 1024 tiles on 256 blocks, one N-tile
    ("sw", f"{CONV64} M=196608 N=320 C0=320 flags={2 | 1 << 21}",
     dict(family="sw", tilesN=1, tiles=1024, grid=256, raster=[0, 0, 0, 0, 0], gn_decline="the one-wave-per-SIMD kernel")),
    # GEGLU Linear without residual / rowvec is eligible; the same raster block as the persistent kernel's
    ("sw_geglu", f"mode=0 M=49152 N=5120 C0=640 act=3 flags={2 | 1 << 21}", dict(family="sw", tiles=4096, grid=256, raster=[8, 4, 32, 4, 0])),
    # bits 13-15 = 2: rast_gm 4 (gn 8, sm 256 / 4, sn 16 / 8), bit16: N-fastest; code 1: classic
    ("raster_forced", f"mode=0 M=49152 N=5120 C0=640 act=3 flags={2 | 2 << 13 | 1 << 16}", dict(tiles=4096, grid=256, family="big", raster=[4, 8, 64, 2, 1])),
    ("raster_classic", f"mode=0 M=49152 N=5120 C0=640 act=3 flags={2 | 1 << 13}", dict(tiles=4096, grid=256, family="big", raster=[0, 0, 0, 0, 0])),
    # bit22 forbids the round-6 kernels
    ("sw_bit22", f"{CONV64} M=196608 N=320 C0=320 flags={2 | 1 << 21 | 1 << 22 | 1 << 27 | 1 << 28}", dict(tiles=1024, grid=256, family="big", splits=1)),
    # bit27, av_gemm_sw_sk_blocks(force): U = 1024 x 45 units in [1024, 2^22] -> 256 blocks; 2 x 256 x 192 x 320 x 4 B = 125.8 MB <= 128 MiB
    ("sk_forced", f"{CONV64} M=196608 N=320 C0=320 flags={2 | 1 << 27}",
     dict(family="sw_streamk", sk_blocks=256, grid=256, tiles=1024, gn_decline="the stream-K kernel")),
    # forced on a tiny launch: 1 tile x 10 K-tiles = 10 units < 1024 -> U / 4 = 2 blocks
    ("sk_forced_small", f"mode=0 M=192 N=320 C0=640 flags={2 | 1 << 27}", dict(family="sw_streamk", sk_blocks=2, grid=2, tiles=1)),
    # bit26 only allows it: 1024 tiles are 4 full rounds (efficiency 1.0 >= 0.9) -> the default plan
    ("sk_allowed_full", f"{CONV64} M=196608 N=320 C0=320 flags={2 | 1 << 26}", dict(tiles=1024, grid=256, family="big", splits=1)),
    # 342 tiles on 2 rounds: 342 / 512 = 0.67 < 0.9 -> taken
    ("sk_allowed_pays", f"{CONV64} M=65536 N=320 C0=320 flags={2 | 1 << 26}", dict(grid=256, family="sw_streamk", sk_blocks=256, tiles=342)),
    # never for a batch-hinted launch; never when the workspace is too small (64 MiB < 125.8 MB)
    ("sk_hinted", f"{CONV64} M=196608 N=320 C0=320 hint=294912 flags={2 | 1 << 27}", dict(tiles=1024, grid=256, family="big", splits=1)),
    ("sk_small_ws", f"{CONV64} M=196608 N=320 C0=320 ws_mib=64 flags={2 | 1 << 27}", dict(tiles=1024, grid=256, family="big", splits=1)),
    # bit28, av_gemm_swh_eligible: stride 1, "same", Wi = 64, N % 320 = 0, act 0; 1024 tiles on 256 blocks
    ("swh_64", f"{CONV64} M=196608 N=320 C0=320 flags={2 | 1 << 28}",
     dict(family="swh", tilesN=1, tiles=1024, grid=256, raster=[0, 0, 0, 0, 0], gn_decline="the LDS-patch convolution kernel")),
    # Wi = 8 is not covered -> the default plan
    ("swh_8", f"{CONV8} M=3072 N=1280 C0=1280 flags={2 | 1 << 28}", dict(tilesN=4, tiles=64, grid=256, family="big", splits=4)),
    # bit2: no persistent kernel -> 128-row; N = 320 is no multiple of 128 -> NF 5; tm = 1536 x 2 >= 384 -> unsplit
    ("bit2_conv", f"{CONV64} M=196608 N=320 C0=320 flags=6", dict(family="mfma128", nf=5, splits=1, tilesN=2, tiles=3072, grid=3072)),
    # bit2 also keeps the weight-stationary kernel out (gemm_impl: flags & (512 | 4 | 1)); N = 960: NF 5, 6 x 1536 tiles
    ("bit2_ws", "mode=0 M=196608 N=960 C0=320 flags=6", dict(family="mfma128", nf=5, splits=1, tilesN=6, tiles=9216, grid=9216)),
    # bit3: the persistent kernel although 24 tiles do not fill; bit3 also switches its split-K off (flags & (16 | 8))
    ("bit3", f"{CONV8} M=1024 N=1280 C0=1280 flags=10", dict(family="big", splits=1, tiles=24, grid=24)),
    # bit4: no split-K: tb = 64 neither fills nor is forced -> 128-row, t4 = 240 would split -> NF 5, tm = 24 x 8
    ("bit4", f"{CONV8} M=3072 N=1280 C0=1280 flags=18", dict(family="mfma128", nf=5, splits=1, tiles=192, grid=192)),
    # bit11: NF 4 where conv8_1024 picks 5: tm = 8 x 10 = 80, sp = min(ceil(512 / 80) = 7, 8, 22) = 7
    ("bit11", f"{CONV8} M=1024 N=1280 C0=1280 flags={2 | 2048}", dict(family="mfma128", nf=4, splits=7, tilesN=10, tiles=80, grid=560)),
    # N = 640, nk = 5, M = 4096 < 32768 (not weight-stationary), tb = 22 x 2 = 44 does not fill, nk < 72: 128-row unsplit; mt = 32,
    # t4 = 160 <= 256 and no split in sight -> prefers NF 4; bit12 keeps NF 5
    ("nf_default", "mode=0 M=4096 N=640 C0=320 flags=2", dict(family="mfma128", nf=4, splits=1, tilesN=5, tiles=160, grid=160)),
    ("bit12", f"mode=0 M=4096 N=640 C0=320 flags={2 | 4096}", dict(family="mfma128", nf=5, splits=1, tilesN=4, tiles=128, grid=128)),
    # bit10: weight-stationary below its row threshold; without it the row above
    ("bit10", f"mode=0 M=4096 N=640 C0=320 flags={2 | 1024}", dict(family="ws", tilesN=4, grid=256)),
    # K = 512 (ws_slab_cols): GEGLU 128-column slabs; plain launches 64-column slabs for N = 512 only
    ("ws_512_geglu", "mode=0 M=196608 N=2560 C0=512 act=3 flags=2", dict(grid=256, family="ws", tilesN=20)),
    ("ws_512_plain", "mode=0 M=196608 N=512 C0=512 flags=2", dict(grid=256, family="ws", tilesN=8)),
    ("ws_512_qkv", "mode=0 M=196608 N=1536 C0=512 flags=2", dict(splits=1, tilesN=12, tiles=18432, grid=18432, family="mfma128", nf=4)),   # 1536 % 320, % 160 != 0
    # the batch hint decides the weight-stationary threshold: 24576 x 3 / 2 = 36864 >= 32768
    ("ws_hinted", "mode=0 M=24576 N=960 C0=320 hint=36864 flags=2", dict(tilesN=6, grid=256, family="ws")),
    ("ws_unhinted", "mode=0 M=24576 N=960 C0=320 flags=2", dict(tilesN=3, tiles=384, grid=256, family="big", splits=1)),   # tb = 128 x 3 = 384: 2 rounds, 75 %
    # ln_c1: only the weight-stationary kernel, at any row count and whatever bit9 says
    ("ln", "mode=0 M=196608 N=960 C0=320 ln=1 flags=2", dict(status=0, family="ws_ln", tilesN=6, grid=256, gn_decline="the LayerNorm-fold kernel")),
    ("ln_small", "mode=0 M=1024 N=960 C0=320 ln=1 flags=514", dict(tilesN=6, grid=256, status=0, family="ws_ln")),
    ("ln_512_geglu", "mode=0 M=196608 N=2560 C0=512 act=3 ln=1 flags=2", dict(grid=256, status=0, family="ws_ln", tilesN=20)),
    # unsupported: C0 = 640; a residual; C0 = 512 without GEGLU; register staging (flags 0)
    ("ln_c0", "mode=0 M=196608 N=960 C0=640 ln=1 flags=2", dict(status=-2, gn_decline="the LayerNorm-fold kernel")),
    ("ln_res", "mode=0 M=196608 N=960 C0=320 ln=1 R=1 flags=2", dict(status=-2)),
    ("ln_512_plain", "mode=0 M=196608 N=512 C0=512 ln=1 flags=2", dict(status=-2)),
    ("ln_no_dma", "mode=0 M=196608 N=960 C0=320 ln=1 flags=0", dict(status=-2)),
    # no workspace bytes / no workspace: conv8_3072 cannot split -> 128-row (as bit4)
    ("ws_0_bytes", f"{CONV8} M=3072 N=1280 C0=1280 ws_mib=0 flags=2", dict(family="mfma128", nf=5, splits=1, grid=192)),
    ("ws_null", f"{CONV8} M=3072 N=1280 C0=1280 ws_null=1 flags=2", dict(family="mfma128", nf=5, splits=1, grid=192)),
    # 32 MiB: neither the persistent kernel's 62.9 MB nor the 128-row kernel's 3 x 3072 x 1280 x 4 B = 47.2 MB fit
    ("ws_32", f"{CONV8} M=3072 N=1280 C0=1280 ws_mib=32 flags=2", dict(nf=5, tiles=192, grid=192, family="mfma128", splits=1)),
    # 64 MiB and 256 MiB plan alike (split_ws_bytes caps at 64 MiB)
    ("ws_64_a", f"{CONV8} M=3072 N=1280 C0=1280 ws_mib=64 flags=2", dict(family="big", splits=4, grid=256)),
    ("ws_256_a", f"{CONV8} M=3072 N=1280 C0=1280 ws_mib=256 flags=2", dict(family="big", splits=4, grid=256)),
    ("ws_64_b", f"{CONV8} M=1024 N=1280 C0=1280 ws_mib=64 flags=2", dict(family="mfma128", nf=5, splits=8, grid=512)),
    ("ws_256_b", f"{CONV8} M=1024 N=1280 C0=1280 ws_mib=256 flags=2", dict(family="mfma128", nf=5, splits=8, grid=512)),
    # batch hint 3 / 2, the reference launch splits and the launch's own rows would not: the workspace rule is the one that gets
    # HARDER with fewer rows (fewer tiles -> a larger factor -> more partial tiles).  Linear, N = 128 (NF 4, one column tile, no
    # persistent kernel), nk = 72, bit9, a 32 MiB workspace (33 554 432 B).  Own rows 8705: tm = 69, sp = min(ceil(512 / 69) = 8, 8, 9) = 8,
    # 8 x 8705 x 128 x 4 B = 35.7 MB does not fit -> unsplit, 69 blocks.  Reference rows 13057: tm = 103, sp = ceil(512 / 103) = 5,
    # 5 x 13057 x 128 x 4 B = 33.4 MB fits -> 5 splits, which the hinted launch takes on its own 69 tiles: 345 blocks.
    ("hint_ws_own", "mode=0 M=8705 N=128 C0=4608 ws_mib=32 flags=514",
     dict(family="mfma128", nf=4, splits=1, tilesN=1, tiles=69, grid=69, raster=[0, 0, 0, 0, 0])),
    ("hint_ws_ref", "mode=0 M=13057 N=128 C0=4608 ws_mib=32 flags=514", dict(family="mfma128", nf=4, splits=5, tiles=103, grid=515)),
    ("hint_ws_hinted", "mode=0 M=8705 N=128 C0=4608 hint=13057 ws_mib=32 flags=514",
     dict(family="mfma128", nf=4, splits=5, tilesN=1, tiles=69, grid=345, gn_decline="a split-K plan")),
    # both split, differently: reference rows 6144 -> tb = 32 x 4 = 128, sp = 2, 256 work items, 62.9 MB: persistent, 2 splits.  The
    # launch's own 4096 rows: tb = 22 x 4 = 88, 2 x 88 = 176 < 224 -> 128-row, tm = 32 x 8 = 256, sp = ceil(512 / 256) = 2.  The hinted
    # launch takes the REFERENCE plan (family and factor) on its own tiles: 88 x 2 blocks.
    ("hint_own", f"{CONV8} M=4096 N=1280 C0=1280 flags=2", dict(family="mfma128", nf=5, splits=2, tilesN=8, tiles=256, grid=512)),
    ("hint_ref_splits", f"{CONV8} M=4096 N=1280 C0=1280 hint=6144 flags=2", dict(family="big", splits=2, tilesN=4, tiles=88, grid=176)),
    # the reverse: N = 160 (no persistent kernel), nk = 45: own rows 11008 -> tm = 86 <= 128 pays, sp = min(ceil(512 / 86) = 6, 8, 45 / 8) = 5;
    # reference rows 16512 -> tm = 129 > 128 with nk < 72 does not pay -> the hinted launch must not split either
    ("rev_own", f"{CONV8} M=11008 N=160 C0=320 flags=2", dict(family="mfma128", nf=5, splits=5, tiles=86, grid=430)),
    ("rev_hinted", f"{CONV8} M=11008 N=160 C0=320 hint=16512 flags=2", dict(family="mfma128", nf=5, splits=1, tiles=86, grid=86)),
    # ---- GroupNorm records: the decline rules and every clause of gn_shape_ok ----
    # 320 / 32 = 10 channels per group divides 40, M and rows per group multiples of 16
    ("gn_ok_big", f"{CONV64} M=196608 N=320 C0=320 {GN} flags=2", dict(tiles=1024, grid=256, family="big", splits=1, gn_records=True, gn_decline="")),
    # SiLU keeps the launch off the persistent kernel (big_ok: act 0); with gn_stats set the 128-row kernel uses the 160-column tile
    ("gn_ok_silu", f"{CONV64} M=196608 N=320 C0=320 act=1 {GN} gn=1 flags=2", dict(tilesN=2, tiles=3072, grid=3072, family="mfma128", nf=5, splits=1, gn_records=True)),
    # nf_default's shape prefers NF 4; the query (no gn_stats) plans that launch, the launch with records takes NF 5 (N / 160 tiles)
    ("gn_query_nf4", f"mode=0 M=4096 N=640 C0=320 {GN} flags=2", dict(tiles=160, grid=160, family="mfma128", nf=4, tilesN=5, gn_records=True)),
    ("gn_launch_nf5", f"mode=0 M=4096 N=640 C0=320 {GN} gn=1 flags=2", dict(family="mfma128", nf=5, tilesN=4, tiles=128, grid=128, gn_records=True)),
    ("gn_split", f"{CONV8} M=3072 N=1280 C0=1280 gn_groups=32 gn_rpg=64 flags=2", dict(family="big", splits=4, grid=256, gn_records=False, gn_decline="a split-K plan")),
    ("gn_geglu", f"mode=0 M=49152 N=5120 C0=640 act=3 {GN} flags=2", dict(family="big", tiles=4096, grid=256, gn_records=False, gn_decline=SHAPE)),
    ("gn_f32out", f"mode=0 M=4096 N=320 C0=640 act=4 {GN} flags=2", dict(nf=5, splits=1, tilesN=2, tiles=64, grid=64, family="mfma128", gn_records=False, gn_decline=SHAPE)),
    ("gn_no_dma", f"{CONV64} M=196608 N=320 C0=320 {GN} flags=0", dict(tiles=3072, grid=3072, family="mfma128", nf=5, gn_records=False, gn_decline=SHAPE)),
    ("gn_groups_0", f"{CONV64} M=196608 N=320 C0=320 gn_groups=0 gn_rpg=4096 flags=2", dict(gn_records=False, gn_decline=SHAPE)),
    ("gn_rpg_0", f"{CONV64} M=196608 N=320 C0=320 gn_groups=32 gn_rpg=0 flags=2", dict(gn_records=False, gn_decline=SHAPE)),
    ("gn_n_160", f"mode=0 M=4096 N=128 C0=640 {GN} flags=2", dict(gn_records=False, gn_decline=SHAPE)),
    ("gn_n_groups", f"{CONV64} M=196608 N=320 C0=320 gn_groups=3 gn_rpg=4096 flags=2", dict(gn_records=False, gn_decline=SHAPE)),
    ("gn_cg_16", f"{CONV64} M=196608 N=320 C0=320 gn_groups=20 gn_rpg=4096 flags=2", dict(gn_records=False, gn_decline=SHAPE)),   # 40 % 16
    ("gn_m_16", "mode=0 M=4104 N=320 C0=640 gn_groups=32 gn_rpg=4104 flags=2", dict(gn_records=False, gn_decline=SHAPE)),
    ("gn_rpg_16", f"{CONV64} M=196608 N=320 C0=320 gn_groups=32 gn_rpg=8 flags=2", dict(gn_records=False, gn_decline=SHAPE)),
    ("gn_m_rpg", f"{CONV64} M=196608 N=320 C0=320 gn_groups=32 gn_rpg=20480 flags=2", dict(gn_records=False, gn_decline=SHAPE)),
    ("gn_naive", f"{CONV64} M=196608 N=320 C0=320 {GN} flags=3", dict(grid=245760, family="naive", gn_records=False, gn_decline="the naive kernel")),
    ("gn_pp", f"{CONV64} M=196608 N=320 C0=320 {GN} flags={2 | 1 << 17}", dict(tiles=768, grid=256, family="pp", gn_records=False)),
    # ---- the launches of the all-fp16-inputs activation checks (tests/gpu_checks.py: check_silu_all_inputs, check_gelu_all_inputs) and the
    # split-K activation rows of check_gemm_splitk: a retune that moves one of them must not silently change the epilogue under test ----
    # values in rowvec, 496 x 128 x 64, SiLU / GELU: N = 128 is no multiple of 320 (no persistent kernel) nor of 160 -> NF 4; tm = 4 x 1,
    # nk = 1: no split.  The same with register staging (flags 0); bit0: the naive kernel, 496 x 128 / 256 blocks
    ("act_tile_silu", "mode=0 M=496 N=128 C0=64 rowvec=1 act=1 flags=2", dict(family="mfma128", nf=4, splits=1, tilesN=1, tiles=4, grid=4)),
    ("act_tile_silu_reg", "mode=0 M=496 N=128 C0=64 rowvec=1 act=1 flags=0", dict(family="mfma128", nf=4, splits=1, tilesN=1, tiles=4, grid=4)),
    ("act_naive_silu", "mode=0 M=496 N=128 C0=64 rowvec=1 act=1 flags=3", dict(family="naive", splits=1, grid=248)),
    ("act_naive_gelu", "mode=0 M=496 N=128 C0=64 rowvec=1 act=2 flags=3", dict(family="naive", splits=1, grid=248)),
    # GEGLU on the naive kernel: one thread per OUTPUT, 63488 x 64 / 256 blocks
    ("act_naive_geglu", "mode=0 M=63488 N=128 C0=64 bias=1 act=3 flags=3", dict(family="naive", splits=1, grid=15872)),
    # 64 x 1024 x 2048: N = 1024 is no multiple of 320 / 160 -> 128-row kernel, NF 4, tm = 1 x 8 = 8 <= 128 with nk = 32 >= 32 pays:
    # sp = min(ceil(512 / 8) = 64, 8, 32 / 8) = 4, 4 x 64 x 1024 x 4 B = 1 MiB fits -> the reduce kernel applies the activation
    ("act_splitk_silu", "mode=0 M=64 N=1024 C0=2048 rowvec=1 act=1 flags=2",
     dict(family="mfma128", nf=4, splits=4, tilesN=8, tiles=8, grid=32, gn_decline="a split-K plan")),
    ("act_splitk_gelu", "mode=0 M=64 N=1024 C0=2048 rowvec=1 act=2 flags=2", dict(family="mfma128", nf=4, splits=4, tilesN=8, tiles=8, grid=32)),
    # check_gemm_splitk's first case with an activation: SiLU / GELU keep it off the persistent kernel (big_ok: act 0); N = 320: NF 5
    # (320 % 128 != 0), tm = 24 x 2 = 48, nk = 9 x 4 = 36 >= 32: sp = min(ceil(512 / 48) = 11, 8, 36 / 8) = 4; bit4: unsplit
    ("splitk_conv_silu", f"{CONV8} M=3072 N=320 C0=256 bias=1 rowvec=1 rowvec_div=1024 R=1 act=1 flags=2",
     dict(family="mfma128", nf=5, splits=4, tilesN=2, tiles=48, grid=192)),
    ("splitk_conv_gelu", f"{CONV8} M=3072 N=320 C0=256 bias=1 rowvec=1 rowvec_div=1024 R=1 act=2 flags=2",
     dict(family="mfma128", nf=5, splits=4, tilesN=2, tiles=48, grid=192)),
    ("splitk_conv_silu_bit4", f"{CONV8} M=3072 N=320 C0=256 bias=1 rowvec=1 rowvec_div=1024 R=1 act=1 flags=18",
     dict(family="mfma128", nf=5, splits=1, tilesN=2, tiles=48, grid=48)),
    # GEGLU, 63488 x 640: bit3 (and tb = 331 x 2 = 662 on 3 rounds, 662 x 4 >= 3 x 256 x 3, fills anyway) -> persistent kernel, 2 N-tiles:
    # classic order
    ("act_big_geglu", "mode=0 M=63488 N=640 C0=64 bias=1 act=3 flags=10",
     dict(family="big", splits=1, tilesN=2, tiles=662, grid=256, raster=[0, 0, 0, 0, 0])),
    # bit21 with nk = 2 (the one-wave kernel needs >= 2 K-tiles; GEGLU Linear without residual / rowvec is eligible)
    ("act_sw_geglu", f"mode=0 M=63488 N=640 C0=128 bias=1 act=3 flags={2 | 1 << 21}",
     dict(family="sw", tilesN=2, tiles=662, grid=256, raster=[0, 0, 0, 0, 0])),
    # bit27: U = 662 x 2 = 1324 units in [1024, 2^22] -> 256 blocks (5.2 units each: whole tiles and cut tiles), 125.8 MB <= 128 MiB
    ("act_sk_geglu", f"mode=0 M=63488 N=640 C0=128 bias=1 act=3 flags={2 | 1 << 27}",
     dict(family="sw_streamk", sk_blocks=256, grid=256, tiles=662, tilesN=2)),
    # ---- descriptor validation (gemm_impl's checks, same texts) ----
    ("bad_mode", "mode=3 M=128 N=320 C0=320 flags=2", dict(status=-1, message="gemm: bad mode 3")),
    ("bad_shape", "mode=0 M=0 N=320 C0=320 flags=2", dict(status=-1, message="gemm: bad M/N/C0/C1 (0 320 320 0)")),
    ("null_w", "mode=0 M=128 N=320 C0=320 W=0 flags=2", dict(status=-1, message="gemm: null A0/W/C")),
    ("conv_geometry", "mode=1 M=128 N=320 C0=320 Hi=8 Wi=8 Ho=8 Wo=8 stride=3 flags=2", dict(status=-1, message="gemm: bad conv geometry")),
    ("geglu_n", "mode=0 M=128 N=48 C0=320 act=3 flags=2", dict(status=-1, message="gemm: GEGLU needs N % 32 == 0")),
    # temporal (3,1,1) convolution: 3 taps, nk = 15, tb = 1024 fills
    ("temporal", "mode=2 M=196608 N=320 C0=320 F=16 HW=4096 flags=2", dict(tiles=1024, status=0, family="big", splits=1, grid=256)),
    # a leading dimension that is no multiple of 8 halves: not `fast`, the naive kernel
    ("lda_644", "mode=0 M=4096 N=320 C0=640 lda0=644 flags=2", dict(grid=5120, family="naive")),
]

# ---- the launches of the exact-data check (tests/gpu_checks.py: check_gemm_exact; descriptors from exact_gemm_plan_rows, ldc = N rounded
# up to 8): a retune that moves one of them must not silently take an exact row off the family it names.  The expected plan comes from
# the family the CHECK names, worked out from the rules once per family:
#  * flags 4 | 16 (no persistent kernel -- which also keeps the weight-stationary kernel out -- and no split-K): every operand is
#    16-byte aligned with ld % 8 = 0 -> `fast`, 128-row kernel, unsplit, with LDS-DMA staging (flags 2) or without; bit0: the naive kernel;
#  * bit3: big_ok (N % 320 = 0, act 0) and forced -> persistent kernel, and bit3 switches its split-K off;
#  * bit17 + bit19 / bit20: no case splits (nk <= 9 < 32), so the ping-pong arm takes them on 192- / 256-row tiles;
#  * bit21: N % 320 = 0, act 0, nk >= 2, never residual AND rowvec -> one-wave-per-SIMD kernel;
#  * bit27: the same test, and tiles x nk >= 8 units (M197 N640 K192: 4 x 3; the 16x16 convs: 4 x 9) -> forced stream-K on units / 4 blocks;
#    the launches below 8 units are skipped by name in the check and have no row here;
#  * no bits, 48 x 8x8 256->320: tb = 16 does not fill, nk = 36 < 72 -> 128-row kernel, N = 320 -> NF 5 (320 % 128 != 0), tm = 24 x 2 = 48
#    <= 128 with nk >= 32: sp = min(ceil(512 / 48) = 11, 8, 36 / 8) = 4; 640->1280: tb = 16 x 4 = 64 <= 128, nk = 90 >= 72:
#    sp = min(256 / 64, 8, 90 / 12) = 4, 256 >= 224 work items, 4 x 3072 x 1280 x 4 B = 62.9 MB fits -> persistent kernel, 4 splits;
#  * bit28: stride 1, "same", Wi = 16 / 32 / 64, N = 320, act 0, residual without rowvec -> LDS-patch kernel;
#  * bit10: Linear, C0 = 320 with N % 160 = 0, or C0 = 512 with N = 512; no rowvec -> weight-stationary kernel below its row threshold.
EXACT_PLANS = {
    "naive kernel": dict(family="naive", splits=1), "128-row reg": dict(family="mfma128", splits=1), "128-row glds": dict(family="mfma128", splits=1),
    "persistent 192x320": dict(family="big", splits=1), "ping-pong 192": dict(family="pp", pp_mf=3, splits=1),
    "ping-pong 256": dict(family="pp", pp_mf=4, splits=1), "one-wave-per-SIMD": dict(family="sw", splits=1),
    "stream-K": dict(family="sw_streamk", splits=1), "split-K on the 128-row kernel": dict(family="mfma128", nf=5, splits=4, tiles=48, grid=192),
    "split-K on the persistent kernel": dict(family="big", splits=4, tilesN=4, tiles=64, grid=256), "LDS patch": dict(family="swh", splits=1),
    "ws": dict(family="ws", splits=1),
}


def _exact_rows():
    import gpu_checks as gc
    rows = gc.exact_gemm_plan_rows()
    assert {fam for _n, _d, fam, _c in rows} == set(EXACT_PLANS)      # every family the check names has a launch that is not skipped
    return [(name, desc, EXACT_PLANS[fam]) for name, desc, fam, _case in rows]


ROWS += _exact_rows()


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "gemm_plan_main.cpp"),
                    os.path.join(CSRC, "gemm_plan.cpp"), "-o", exe], check=True)
    names = [r[0] for r in ROWS]
    assert len(set(names)) == len(names)
    out = subprocess.run([exe], input="".join(r[1] + "\n" for r in ROWS), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(ROWS)
    return {name: json.loads(line) for name, line in zip(names, lines)}


@pytest.mark.parametrize("name,desc,want", ROWS, ids=[r[0] for r in ROWS])
def test_plan(plans, name, desc, want):
    got = plans[name]
    if "status" not in want:
        assert got["status"] == 0, got
    if want.get("status", 0) == -2:
        assert "ln_c1 (LayerNorm fold) needs mode 0" in got["message"]
    assert {k: got[k] for k in want} == want, (desc, got)


def test_workspace_above_64_mib_does_not_change_the_split(plans):
    geometry = ("family", "nf", "splits", "tilesN", "tiles", "grid")
    for a, b in (("ws_64_a", "ws_256_a"), ("ws_64_b", "ws_256_b")):
        assert [plans[a][k] for k in geometry] == [plans[b][k] for k in geometry]


def test_flag_names_mirror_the_header():
    """anyv2v_amd/_lib.py carries every ANYV2V_GEMM_* constant of include/anyv2v_hip.h, with the header's value, and no other."""
    from anyv2v_amd import _lib
    header = open(os.path.join(ROOT, "include", "anyv2v_hip.h")).read()
    defs = re.findall(r"^#define (ANYV2V_GEMM_\w+) +(\(1 << \d+\)|\d+) +/\*", header, re.M)
    assert len(defs) >= 20 and len(defs) == len(re.findall(r"^#define ANYV2V_GEMM_", header, re.M))
    want = {name: eval(value) for name, value in defs}   # "(1 << n)" or "n"
    have = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith("ANYV2V_GEMM_")}
    assert have == want
    bits = [v for n, v in want.items() if not n.endswith("_SHIFT")]
    assert len(set(bits)) == len(bits) and all(v & (v - 1) == 0 for v in bits)
