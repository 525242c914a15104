"""The attention launch planner (anyv2v_amd/csrc/attention_plan.cpp) on the CPU: which kernel instantiation, grid, block and dynamic LDS a
descriptor gets at each of the three entry points.  The planner is plain C++; this test builds it with the host compiler under the address
and undefined-behaviour sanitizers, next to tests/attention_plan_main.cpp, runs that program once as its own process and compares the
plans with

 * a table worked out BY HAND from the dispatch code the planner replaced (anyv2v_attention_f16 / _small_f16 / _bias_f16 of attention.hip
   as they were then) -- each row says how;
 * the kernel every attention launch of tests/gpu_checks.py NAMES: the exact specs, the far specs with the layouts of their far launches,
   the edge cases (plain and framed operands) and the random-data checks that carry a kernel in their row names.  The descriptors come from
   the layout code of those launches, run on the device "meta".  A retune that moves a threshold past a named shape fails here;
 * the planner's own list of instantiations: the exact check alone and the edge checks alone each reach every one of them.

No GPU.  Unless a row says otherwise: entry 0 (anyv2v_attention_f16), batch = heads = 1, inner = kv_div = 1, qk_mod = 0, dense strides
(q_outer = Sq, kv_outer = Sk, seq strides 1), every leading dimension heads * head_dim, 16-byte aligned fake pointers, flags 0.
q_tiles = ceil(Sq / 128); a flash grid is batch * heads * q_tiles blocks of 256 threads; the whole-sequence and loop kernels run
(ceil(Sq / 64), heads, batch) blocks of 256 with 2 * (16 nkb * (32 ds + 8) + 32 ds * (16 nkb + 4)) bytes of dynamic LDS; the generic
kernel ceil(batch * heads * Sq / 128) blocks of 128.
"""
import json
import os
import shutil
import subprocess

import pytest

import gpu_checks as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anyv2v_amd", "csrc")

PNP8 = "batch=96 heads=4 qk_mod=32"            # 32 source elements x 3 branches
WIDE = "K / V tile offsets beyond 32 bits"
SMALL = "entry=1 batch=2 heads=2"
BIAS = "entry=2 bias=1 batch=2 heads=2 Sq=20"

# (name, descriptor, expected fields of the plan)
ROWS = [
    # ---- anyv2v_attention_f16 ----
    # `fast`, neither <= 16 positions nor wide nor PnP; nwg8 = 2 x 2 x 1 = 4 < 1024 -> 4-wave blocks on the 2-stage ring; q_tiles = ceil(130 / 128)
    ("flash", "batch=2 heads=2 Sq=130 Sk=145", dict(name="flash<2,1,4>", q_tiles=2, grid=[8, 1, 1], block=256, lds=0, causal=0, wide="")),
    # bit0 -> !fast -> launch_naive: 2 x 2 x 130 = 520 threads, 5 blocks of 128
    ("d64_bit0", "batch=2 heads=2 Sq=130 Sk=145 flags=1", dict(name="naive", grid=[5, 1, 1], block=128, lds=0)),
    # fast needs ldq, ldk, ldv % 8 == 0 and ldo % 4 == 0 and all four pointers 16-byte aligned
    ("d64_ldq", "batch=2 heads=2 Sq=130 Sk=145 ldq=132", dict(name="naive")),
    ("d64_ldk", "batch=2 heads=2 Sq=130 Sk=145 ldk=132", dict(name="naive")),
    ("d64_ldv", "batch=2 heads=2 Sq=130 Sk=145 ldv=132", dict(name="naive")),
    ("d64_ldo_4", "batch=2 heads=2 Sq=130 Sk=145 ldo=132", dict(name="flash<2,1,4>")),     # 132 % 4 == 0 is enough for the flash kernels
    ("d64_ldo_2", "batch=2 heads=2 Sq=130 Sk=145 ldo=130", dict(name="naive")),
    ("d64_q_8", "batch=2 heads=2 Sq=130 Sk=145 Q=8", dict(name="naive")),
    ("d64_k_8", "batch=2 heads=2 Sq=130 Sk=145 K=8", dict(name="naive")),
    ("d64_v_8", "batch=2 heads=2 Sq=130 Sk=145 V=8", dict(name="naive")),
    ("d64_o_8", "batch=2 heads=2 Sq=130 Sk=145 O=8", dict(name="naive")),                   # this entry point wants O 16-byte aligned
    # bit7 (8-byte epilogue stores) and bit4 (causal: the small entry's) do not move the plan; causal stays 0
    ("d64_bit7", "batch=2 heads=2 Sq=130 Sk=145 flags=128", dict(name="flash<2,1,4>", grid=[8, 1, 1])),
    ("d64_bit4", "batch=2 heads=2 Sq=130 Sk=145 flags=16", dict(name="flash<2,1,4>", causal=0)),
    # the short path: Sq <= 16 && Sk <= 16 && ldo % 8 == 0 && !bit1; one wave per (element, head): ceil(6 x 2 / 4) blocks of 256
    ("short", "batch=6 heads=2 Sq=16 Sk=16", dict(name="short<1>", grid=[3, 1, 1], block=256, lds=0)),
    ("short_sq17", "batch=6 heads=2 Sq=17 Sk=16", dict(name="flash<2,1,4>", grid=[12, 1, 1])),
    ("short_sk17", "batch=6 heads=2 Sq=16 Sk=17", dict(name="flash<2,1,4>", grid=[12, 1, 1])),
    ("short_ldo", "batch=6 heads=2 Sq=16 Sk=16 ldo=132", dict(name="flash<2,1,4>")),        # ldo % 8 != 0 (but % 4 == 0: still fast)
    ("short_bit1", "batch=6 heads=2 Sq=16 Sk=16 flags=2", dict(name="flash<2,1,4>")),
    # av_attn_pnp3: qk_mod > 0 && batch == 3 qk_mod && kv_div == 1 && !bit3 -> one wave per (source element, head): ceil(2 x 2 / 4)
    ("short_pnp", "batch=6 heads=2 Sq=16 Sk=16 qk_mod=2", dict(name="short<3>", grid=[1, 1, 1], block=256)),
    ("short_pnp_bit3", "batch=6 heads=2 Sq=16 Sk=16 qk_mod=2 flags=8", dict(name="short<1>", grid=[3, 1, 1])),
    ("short_pnp_kv_div", "batch=6 heads=2 Sq=16 Sk=16 qk_mod=2 kv_div=2", dict(name="short<1>", grid=[3, 1, 1])),
    ("short_pnp_batch", "batch=6 heads=2 Sq=16 Sk=16 qk_mod=3", dict(name="short<1>", grid=[3, 1, 1])),      # 6 != 3 x 3: plain aliasing
    # the same predicate on the flash path: qk_mod x heads x q_tiles = 1 x 1 x 2 blocks; n8 = 1 < 1024 and Sk < 2048 -> 4 waves
    ("flash_pnp", "batch=3 qk_mod=1 Sq=130 Sk=130", dict(name="flash<2,3,4>", grid=[2, 1, 1], block=256, q_tiles=2)),
    ("flash_pnp_bit3", "batch=3 qk_mod=1 Sq=130 Sk=130 flags=8", dict(name="flash<2,1,4>", grid=[6, 1, 1])),
    ("flash_pnp_kv_div", "batch=3 qk_mod=1 kv_div=3 Sq=130 Sk=130", dict(name="flash<2,1,4>", grid=[6, 1, 1])),
    ("flash_pnp_batch", "batch=4 qk_mod=1 Sq=130 Sk=130", dict(name="flash<2,1,4>", grid=[8, 1, 1])),
    # 8-wave blocks, plain: !bit2 && Sk >= 2048 && Sq >= 1024 && nwg8 = batch x heads x ceil(Sq / 256) >= 1024.  64 x 4 x 4 = 1024 exactly
    ("w8", "batch=64 heads=4 Sq=1024 Sk=2048", dict(name="flash<3,1,8>", q_tiles=4, grid=[1024, 1, 1], block=512, lds=0)),
    ("w8_sk2047", "batch=64 heads=4 Sq=1024 Sk=2047", dict(name="flash<2,1,4>", q_tiles=8, grid=[2048, 1, 1], block=256)),
    ("w8_sq1023", "batch=64 heads=4 Sq=1023 Sk=2048", dict(name="flash<2,1,4>", q_tiles=8, grid=[2048, 1, 1])),   # nwg8 is still 1024: Sq decides
    ("w8_bit2", "batch=64 heads=4 Sq=1024 Sk=2048 flags=4", dict(name="flash<2,1,4>", grid=[2048, 1, 1])),
    # block count: Sq = 2816 = 11 x 256; 31 x 3 x 11 = 1023 -> 4 waves (93 x 22 blocks); 32 x 3 x 11 = 1056 -> 8 waves
    ("w8_1023_blocks", "batch=31 heads=3 Sq=2816 Sk=2048", dict(name="flash<2,1,4>", q_tiles=22, grid=[2046, 1, 1])),
    ("w8_1056_blocks", "batch=32 heads=3 Sq=2816 Sk=2048", dict(name="flash<3,1,8>", q_tiles=11, grid=[1056, 1, 1])),
    # 8-wave blocks, PnP: !bit2 && Sk >= 2048 && Sq >= 2048 && n8 = qk_mod x heads x ceil(Sq / 256) >= 1024.  32 x 4 x 8 = 1024 exactly
    ("w8_pnp", f"{PNP8} Sq=2048 Sk=2048", dict(name="flash<3,3,8>", q_tiles=8, grid=[1024, 1, 1], block=512)),
    ("w8_pnp_sq2047", f"{PNP8} Sq=2047 Sk=2048", dict(name="flash<2,3,4>", q_tiles=16, grid=[2048, 1, 1], block=256)),
    ("w8_pnp_sk2047", f"{PNP8} Sq=2048 Sk=2047", dict(name="flash<2,3,4>", q_tiles=16, grid=[2048, 1, 1])),
    ("w8_pnp_bit2", f"{PNP8} Sq=2048 Sk=2048 flags=4", dict(name="flash<2,3,4>", grid=[2048, 1, 1])),
    # the plain launch's Sq >= 1024 is not enough for a PnP one: 64 x 4 x 4 = 1024 blocks, Sq = 1024 < 2048
    ("w8_pnp_sq1024", "batch=192 heads=4 qk_mod=64 Sq=1024 Sk=2048", dict(name="flash<2,3,4>", q_tiles=8, grid=[2048, 1, 1])),
    ("w8_pnp_1023_blocks", "batch=93 heads=3 qk_mod=31 Sq=2816 Sk=2048", dict(name="flash<2,3,4>", q_tiles=22, grid=[2046, 1, 1])),   # 31 x 3 x 11
    ("w8_pnp_1056_blocks", "batch=96 heads=3 qk_mod=32 Sq=2816 Sk=2048", dict(name="flash<3,3,8>", q_tiles=11, grid=[1056, 1, 1])),
    # bit3 on a PnP launch at 8-wave size: the plain rule on all 96 elements, 96 x 4 x 8 blocks
    ("w8_pnp_bit3", f"{PNP8} Sq=2048 Sk=2048 flags=8", dict(name="flash<3,1,8>", grid=[3072, 1, 1])),
    # wide: kv_seq < 0 || kv_seq > ((2^32 - 1) / 2 - 64) / 63 / max(ldk, ldv) = 34087041 / ld (integer divisions).  ld = 34087040 -> 1,
    # kv_seq = 1 is not above it; ld = 34087048 -> 0.  The loop kernel on head_dim 64: DS 2, (3, 1, 1) blocks, 2 x (96 x 72 + 64 x 100) bytes
    ("wide_at_limit_k", "Sq=130 Sk=70 ldk=34087040", dict(name="flash<2,1,4>", wide="")),
    ("wide_at_limit_v", "Sq=130 Sk=70 ldv=34087040", dict(name="flash<2,1,4>", wide="")),
    ("wide_past_limit_k", "Sq=130 Sk=70 ldk=34087048", dict(name="loop<2>", grid=[3, 1, 1], block=256, lds=26624, wide=WIDE, causal=0)),
    ("wide_past_limit_v", "Sq=130 Sk=70 ldv=34087048", dict(name="loop<2>", lds=26624, wide=WIDE)),
    # the product decides: kv_seq = 2 with half the leading dimension (34087041 / 17043520 = 2, / 17043528 = 1)
    ("wide_at_limit_seq2", "Sq=130 Sk=70 kv_seq=2 ldk=17043520", dict(name="flash<2,1,4>", wide="")),
    ("wide_past_limit_seq2", "Sq=130 Sk=70 kv_seq=2 ldk=17043528", dict(name="loop<2>", wide=WIDE)),
    ("wide_negative", "batch=2 heads=2 Sq=130 Sk=70 kv_seq=-1", dict(name="loop<2>", grid=[3, 2, 2], wide="negative kv_seq")),
    # heads or batch above the loop kernel's grid (65535) -> the generic kernel: 65536 x 130 / 128 blocks
    ("wide_batch", "batch=65536 Sq=130 Sk=70 kv_seq=-1", dict(name="naive", grid=[66560, 1, 1], block=128, wide="negative kv_seq")),
    ("wide_heads", "heads=65536 Sq=130 Sk=70 kv_seq=-1", dict(name="naive", grid=[66560, 1, 1], wide="negative kv_seq")),
    ("wide_batch_65535", "batch=65535 Sq=130 Sk=70 kv_seq=-1", dict(name="loop<2>", grid=[3, 1, 65535])),
    # the short path comes before the wide test: two positions run on the one-wave kernel unless bit1 forbids it
    ("wide_short_first", "batch=65536 Sq=2 Sk=2 kv_seq=-1", dict(name="short<1>", grid=[16384, 1, 1], wide="")),
    ("wide_short_bit1", "batch=65536 Sq=2 Sk=2 kv_seq=-1 flags=2", dict(name="naive", grid=[1024, 1, 1], wide="negative kv_seq")),
    # nwg = 65536 x 32768 x 2 = 2^32 >= 2^31
    ("grid_too_large", "batch=65536 heads=32768 Sq=130 Sk=70", dict(status=-1, message="attention: grid too large")),
    # ---- every check of fill ----
    ("null_desc", "null_desc=1 Sq=130 Sk=70", dict(status=-1, message="attention: null descriptor")),
    ("null_q", "Sq=130 Sk=70 Q=-1", dict(status=-1, message="attention: null pointer")),
    ("null_o", "Sq=130 Sk=70 O=-1", dict(status=-1, message="attention: null pointer")),
    ("bad_batch", "batch=0 Sq=130 Sk=70", dict(status=-1, message="attention: bad sizes")),
    ("bad_sk", "Sq=130 Sk=0", dict(status=-1, message="attention: bad sizes")),
    ("bad_inner", "Sq=130 Sk=70 inner=0", dict(status=-1, message="attention: bad inner/kv_div/qk_mod")),
    ("bad_kv_div", "Sq=130 Sk=70 kv_div=0", dict(status=-1, message="attention: bad inner/kv_div/qk_mod")),
    ("bad_qk_mod", "Sq=130 Sk=70 qk_mod=-1", dict(status=-1, message="attention: bad inner/kv_div/qk_mod")),
    ("bad_ldk", "Sq=130 Sk=70 ldk=-64", dict(status=-1, message="attention: leading dimensions must be positive")),
    ("bad_ldo", "Sq=130 Sk=70 ldo=0", dict(status=-1, message="attention: leading dimensions must be positive")),
    # ---- anyv2v_attention_small_f16 (the head_dim x Sk table follows below) ----
    ("small_head_dim_0", f"{SMALL} Sq=50 Sk=50 head_dim=0", dict(status=-1, message="attention_small: head_dim must be in 1..160")),
    ("small_head_dim_161", f"{SMALL} Sq=50 Sk=50 head_dim=161", dict(status=-1, message="attention_small: head_dim must be in 1..160")),
    ("small_null_desc", "entry=1 null_desc=1 head_dim=40", dict(status=-1, message="attention: null descriptor")),
    ("small_null_desc_head_dim", "entry=1 null_desc=1 head_dim=0", dict(status=-1, message="attention_small: head_dim must be in 1..160")),   # checked first
    ("small_bad_sizes", f"{SMALL} Sq=0 Sk=50 head_dim=40", dict(status=-1, message="attention: bad sizes")),
    # DS 2, NKB 6: (1, 2, 2) blocks, 2 x (96 x 72 + 64 x 100) bytes
    ("small_d40", f"{SMALL} Sq=50 Sk=50 head_dim=40", dict(name="small<2,6>", grid=[1, 2, 2], block=256, lds=26624, causal=0, q_tiles=1)),
    ("small_d44", f"{SMALL} Sq=50 Sk=50 head_dim=44", dict(name="naive", grid=[2, 1, 1], block=128)),       # head_dim % 8: 200 threads
    ("small_d44_long", f"{SMALL} Sq=300 Sk=300 head_dim=44", dict(name="naive")),                              # ... for the loop kernel too
    ("small_o_8", f"{SMALL} Sq=50 Sk=50 head_dim=40 O=8", dict(name="small<2,6>")),                           # O: 8-byte stores
    ("small_o_4", f"{SMALL} Sq=50 Sk=50 head_dim=40 O=4", dict(name="naive")),
    ("small_o_8_long", f"{SMALL} Sq=300 Sk=300 head_dim=40 O=8", dict(name="loop<2>")),
    ("small_o_4_long", f"{SMALL} Sq=300 Sk=300 head_dim=40 O=4", dict(name="naive")),
    ("small_q_8", f"{SMALL} Sq=50 Sk=50 head_dim=40 Q=8", dict(name="naive")),
    ("small_k_8", f"{SMALL} Sq=300 Sk=300 head_dim=40 K=8", dict(name="naive")),
    ("small_ldv", f"{SMALL} Sq=50 Sk=50 head_dim=40 ldv=84", dict(name="naive")),
    ("small_ldo_4", f"{SMALL} Sq=50 Sk=50 head_dim=40 ldo=84", dict(name="small<2,6>")),
    ("small_ldo_2", f"{SMALL} Sq=50 Sk=50 head_dim=40 ldo=82", dict(name="naive")),
    ("small_bit0", f"{SMALL} Sq=50 Sk=50 head_dim=40 flags=1", dict(name="naive")),
    ("small_bit0_long", f"{SMALL} Sq=300 Sk=300 head_dim=40 flags=1", dict(name="naive")),
    # bit4 = causal, on each kernel of this entry point
    ("small_causal", f"{SMALL} Sq=77 Sk=77 head_dim=64 flags=16", dict(name="small<2,6>", causal=1)),
    ("small_causal_loop", f"{SMALL} Sq=300 Sk=300 head_dim=64 flags=16", dict(name="loop<2>", causal=1)),
    ("small_causal_naive", f"{SMALL} Sq=77 Sk=77 head_dim=64 flags=17", dict(name="naive", causal=1)),
    # more heads / batch elements than a grid's y / z take: 65536 x 20 threads on the generic kernel
    ("small_heads", "entry=1 heads=65536 Sq=20 Sk=20 head_dim=40", dict(name="naive", grid=[10240, 1, 1])),
    ("small_batch", "entry=1 batch=65536 Sq=20 Sk=20 head_dim=40", dict(name="naive", grid=[10240, 1, 1])),
    ("small_batch_long", "entry=1 batch=65536 Sq=20 Sk=300 head_dim=40", dict(name="naive")),
    ("small_batch_65535", "entry=1 batch=65535 Sq=20 Sk=20 head_dim=40", dict(name="small<2,6>", grid=[1, 1, 65535])),
    # dynamic LDS of the largest instantiations: 2 x (288 x 136 + 128 x 292); 2 x (96 x 168 + 160 x 100), which the loop kernel shares
    ("small_lds_4_18", f"{SMALL} Sq=288 Sk=288 head_dim=128", dict(name="small<4,18>", grid=[5, 2, 2], lds=153088)),
    ("small_lds_2_18", f"{SMALL} Sq=97 Sk=97 head_dim=40", dict(name="small<2,18>", grid=[2, 2, 2], lds=78848)),
    ("small_lds_5_6", f"{SMALL} Sq=96 Sk=96 head_dim=160", dict(name="small<5,6>", lds=64256)),
    ("small_lds_loop5", f"{SMALL} Sq=97 Sk=97 head_dim=160", dict(name="loop<5>", grid=[2, 2, 2], block=256, lds=64256)),
    # ---- anyv2v_attention_bias_f16 ----
    # the MFMA form: the small entry's conditions with Sk <= 96 and without the causal flag; always NKB 6
    ("bias_96", f"{BIAS} Sk=96 head_dim=40", dict(name="small<2,6,bias>", grid=[1, 2, 2], block=256, lds=26624, causal=0)),
    ("bias_97", f"{BIAS} Sk=97 head_dim=40", dict(name="naive+bias", grid=[1, 1, 1], block=128, causal=0)),     # 2 x 2 x 20 = 80 threads
    ("bias_causal", f"{BIAS} Sk=96 head_dim=40 flags=16", dict(name="naive+bias", causal=1)),
    ("bias_bit0", f"{BIAS} Sk=96 head_dim=40 flags=1", dict(name="naive+bias")),
    ("bias_d20", f"{BIAS} Sk=96 head_dim=20", dict(name="naive+bias")),                                          # % 8, and one 32-column group
    ("bias_d24", f"{BIAS} Sk=96 head_dim=24", dict(name="naive+bias")),                                          # ds = 1
    ("bias_d80", f"{BIAS} Sk=96 head_dim=80", dict(name="small<3,6,bias>")),
    ("bias_d128", f"{BIAS} Sk=96 head_dim=128", dict(name="small<4,6,bias>")),
    ("bias_d160", f"{BIAS} Sk=96 head_dim=160", dict(name="small<5,6,bias>", lds=64256)),
    ("bias_o_4", f"{BIAS} Sk=96 head_dim=40 O=4", dict(name="naive+bias")),
    ("bias_scale_0", f"{BIAS} Sk=96 head_dim=40 scale_milli=0", dict(status=-1, message="attention_bias: scale must be positive")),
    ("bias_scale_neg", f"{BIAS} Sk=96 head_dim=40 scale_milli=-125", dict(status=-1, message="attention_bias: scale must be positive")),
    ("bias_null", "entry=2 bias=0 Sq=20 Sk=96 head_dim=40", dict(status=-1, message="attention_bias: null bias")),
    ("bias_head_dim", f"{BIAS} Sk=96 head_dim=161", dict(status=-1, message="attention_bias: head_dim must be in 1..160")),
    ("bias_null_desc", "entry=2 bias=1 null_desc=1 head_dim=40", dict(status=-1, message="attention_bias: scale must be positive")),   # `d && d->scale > 0`
    ("bias_bad_sizes", f"{BIAS} Sk=0 head_dim=40", dict(status=-1, message="attention: bad sizes")),
]

# anyv2v_attention_small_f16 at Sq = Sk = 96 / 97 / 288 / 289: ds = ceil(head_dim / 32); nkb = 6 up to 96 keys, 18 up to 288 keys while
# ds <= 4, else 0.  nkb == 0 -> the loop kernel at max(ds, 2); nkb > 0 and ds >= 2 -> the whole-sequence kernel; ds = 1 with nkb > 0 ->
# neither (`fast` wants ds >= 2, `loop_ok` nkb == 0): the generic kernel.  So head_dim 8..32 changes kernels at 289 keys, 136..160 at 97.
SMALL_TABLE = {
    24: ("naive", "naive", "naive", "loop<2>"), 32: ("naive", "naive", "naive", "loop<2>"),
    40: ("small<2,6>", "small<2,18>", "small<2,18>", "loop<2>"), 64: ("small<2,6>", "small<2,18>", "small<2,18>", "loop<2>"),
    96: ("small<3,6>", "small<3,18>", "small<3,18>", "loop<3>"),
    104: ("small<4,6>", "small<4,18>", "small<4,18>", "loop<4>"), 128: ("small<4,6>", "small<4,18>", "small<4,18>", "loop<4>"),
    136: ("small<5,6>", "loop<5>", "loop<5>", "loop<5>"), 160: ("small<5,6>", "loop<5>", "loop<5>", "loop<5>"),
}
ROWS += [(f"small_d{d}_sk{sk}", f"{SMALL} Sq={sk} Sk={sk} head_dim={d}", dict(name=name, grid=[(sk + 63) // 64, 2, 2] if name != "naive" else
                                                                          [(4 * sk + 127) // 128, 1, 1]))
         for d, names in SMALL_TABLE.items() for sk, name in zip((96, 97, 288, 289), names)]

HAND = len(ROWS)
EXACT, EDGE, NAMED, FAR = gc.exact_attention_plan_rows(), gc.attention_edge_plan_rows(), gc.named_attention_plan_rows(), gc.far_attention_plan_rows()
CHECK_ROWS = [r[:4] for r in EXACT + EDGE + NAMED + FAR]
ROWS += [(name, words, None) for name, words, _kernel, _inst in CHECK_ROWS]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("attention_plan") / "attention_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "attention_plan_main.cpp"),
                    os.path.join(CSRC, "attention_plan.cpp"), "-o", exe], check=True)
    names = [r[0] for r in ROWS]
    assert len(set(names)) == len(names)
    out = subprocess.run([exe], input="".join(r[1] + "\n" for r in ROWS) + "instantiations\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(ROWS) + 1
    got = {name: json.loads(line) for name, line in zip(names, lines)}
    got["instantiations"] = json.loads(lines[-1])["instantiations"]
    return got


@pytest.mark.parametrize("name,desc,want", ROWS[:HAND], ids=[r[0] for r in ROWS[:HAND]])
def test_plan(plans, name, desc, want):
    got = plans[name]
    if "status" not in want:
        assert got["status"] == 0, got
    assert {k: got[k] for k in want} == want, (desc, got)


@pytest.mark.parametrize("name,desc,kernel,inst", CHECK_ROWS, ids=[r[0] for r in CHECK_ROWS])
def test_named_launch_plans_to_the_kernel_it_names(plans, name, desc, kernel, inst):
    got = plans[name]
    assert got["status"] == 0, (desc, got)
    assert got["name"] in gc.ATTN_KERNEL_INSTANTIATIONS[kernel], (kernel, desc, got)
    if inst is not None:
        assert got["name"] == inst, (desc, got)


def test_far_launches_keep_the_near_plan_unless_the_layout_is_beyond_the_flash_limit(plans):
    near = None
    for name, _words, kernel, _inst, fallback in FAR:
        got = plans[name]
        if name.endswith("| near"):
            near = got
            assert not fallback
        elif fallback:
            assert got["name"] == "loop<2>" and got["wide"] == WIDE and near["kernel"] == "flash", (name, got)
        else:
            assert got["wide"] == "" and [got[k] for k in ("name", "grid", "block", "lds", "q_tiles")] == \
                [near[k] for k in ("name", "grid", "block", "lds", "q_tiles")], (name, got, near)
    assert sum(r[4] for r in FAR) >= 4


def test_framed_operands_get_the_plan_of_the_plain_ones(plans):
    rows = {r[0]: plans[r[0]] for r in EDGE}
    pairs = [(n, n.replace("| plain", "| framed")) for n in rows if n.endswith("| plain")]
    assert pairs
    for a, b in pairs:
        assert rows[a] == rows[b], (a, rows[a], rows[b])


def test_exact_specs_alone_and_edge_cases_alone_reach_every_instantiation(plans):
    every = plans["instantiations"]
    assert len(every) == len(set(every)) >= 23
    assert set(every) == {i for names in gc.ATTN_KERNEL_INSTANTIATIONS.values() for i in names}     # the names the checks may use are the planner's
    for what, rows in (("exact", EXACT), ("edge", EDGE)):
        reached = {plans[r[0]]["name"] for r in rows}
        assert not set(every) - reached, (what, sorted(set(every) - reached))


def test_entry_point_choice():
    from anyv2v_amd import ops
    assert [ops.attention_entry(64, False, False), ops.attention_entry(64, True, False), ops.attention_entry(80, False, False),
            ops.attention_entry(64, False, True), ops.attention_entry(40, True, True)] == [0, 1, 1, 2, 2]
