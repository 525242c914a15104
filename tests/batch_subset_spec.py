"""The cases of the branch-subset tests, as plain data (no torch, no GPU): tests/test_batch_subset_host.py plans every one on the CPU,
tests/gpu_checks.py (check_subset_*) runs them through tests/test_batch_subset_gpu.py.

The invariant (ops.batch_hint, csrc/errors.hip, csrc/gemm_plan.cpp): a launch on the last B - 1 of a step's B branches, planned under
``anyv2v_set_batch_hint(B, B - 1)``, computes for its rows the bits the launch on all B branches computes for them.  A case is ``T`` rows
of ``B`` branches (``r`` = T / B rows each); the subset is the contiguous copy of rows [r, T).

``sharp`` names the plan word in which the subset planned WITHOUT the hint differs from the full launch -- the reason the GPU row has
to fail when the hint is ignored -- or None where only the tile / chunk origin of the rows moves.  The shapes are the smallest the
planner programs (tests/gemm_plan_main.cpp, tests/norm_plan_main.cpp) gave in a scan over N, K and r at the default flags; the comment
of each case holds the words the scan found as (family, nf, splits, tiles) of the full launch / the hinted subset / the un-hinted subset.
"""

LDS_DMA = 2    # ANYV2V_GEMM_LDS_DMA: what ops.gemm always sets (ops.USE_GLDS)
CONV8 = dict(mode=1, geo=(8, 8))     # 3x3 stride 1 on 8 x 8 images: r a multiple of 64
CONV16 = dict(mode=1, geo=(16, 16))


def _g(name, line, sharp, *, B=3, r, N, C0, C1=0, mode=0, geo=None, act=0, flags=0, epi=("bias",), ln=False, gpu_skip=None):
    return dict(name=name, line=line, sharp=sharp, B=B, r=r, N=N, C0=C0, C1=C1, mode=mode, geo=geo, act=act, flags=flags, epi=tuple(epi), ln=ln,
                gpu_skip=gpu_skip)


# activations as include/anyv2v_hip.h numbers them
ACT_NONE, ACT_SILU, ACT_GELU, ACT_GEGLU = 0, 1, 2, 3

# flag bits of the forced families, as tests/gpu_checks.py: PERSISTENT_FAMILIES / check_edges_conv_lds_patch set them
FORCED = (("persistent 192x320", 8, "big"), ("ping-pong 192", (1 << 17) | (1 << 19), "pp"), ("ping-pong 256", (1 << 17) | (1 << 20), "pp"),
          ("one-wave-per-SIMD", 1 << 21, "sw"), ("stream-K", 1 << 27, "sw_streamk"))
STREAMK_SKIP = ("the planner refuses stream-K for a hinted launch (its K ranges depend on the launch's own tile count), so the subset "
                "runs another family than the forced full launch: no bit equality is claimed; the host test asserts the refusal")

GEMM_SPECS = [
    # ---- 128-row kernel, split-K: the factor is inherited from the full launch ----
    # (mfma128, 4, 7, 80) / (mfma128, 4, 7, 56) / (mfma128, 4, 8, 56); GELU in the reduce pass
    _g("linear 128-row split-K +GELU", "128-row split-K", "splits", r=400, N=1024, C0=4096, act=ACT_GELU),
    # (mfma128, 4, 4, 128) / (mfma128, 4, 4, 84) / (mfma128, 4, 5, 84); the subset takes rowvec[1:]
    _g("conv 3x3 128-row split-K +rowvec", "128-row split-K", "splits", r=1344, N=512, C0=320, epi=("bias", "rowvec"), **CONV8),
    # (mfma128, 4, 5, 104) / (mfma128, 4, 5, 68) / (mfma128, 4, 6, 68)
    _g("temporal 128-row split-K +res", "128-row split-K", "splits", r=1080, N=512, C0=1024, mode=2, geo=(5, 36), epi=("bias", "res")),
    # ---- reverse: the full launch does not split, the subset on its own rows would (gemm_plan_host: rev_hinted) ----
    # (mfma128, 4, 1, 130) / (mfma128, 4, 1, 86) / (mfma128, 4, 4, 86)
    _g("conv 3x3 128-row reverse split", "128-row reverse split", "splits", r=2752, N=256, C0=256, **CONV8),
    # ---- persistent 192 x 320 kernel, split-K ----
    # (big, 4, 6, 38) / (big, 4, 6, 26) / (mfma128, 5, 7, 76): the un-hinted subset leaves the family as well
    _g("conv 3x3 persistent split-K +res", "persistent split-K", "splits", r=1216, N=640, C0=512, epi=("bias", "res"), **CONV8),
    # ---- big vs 128-row family, both unsplit ----
    # (big, 4, 1, 232) / (mfma128, 5, 1, 464) / (mfma128, 5, 1, 464): the family is planned on the launch's own rows, hint or not
    _g("linear persistent vs 128-row", "family", "family", r=1800, N=2560, C0=64),
    # ---- tile width 160 vs 128 columns ----
    # (mfma128, 5, 1, 208) / (mfma128, 4, 1, 180) / (mfma128, 4, 1, 180); two sources
    _g("linear nf 5 vs 4, two sources", "nf", "nf", r=1100, N=1280, C0=64, C1=64),
    # ---- weight-stationary K = 320: T = 32775 >= 32768 > 21850 ----
    # (ws) / (ws) / (mfma128, 5, 1, 171)
    _g("linear weight-stationary on hinted rows +res", "weight-stationary", "family", r=10925, N=160, C0=320, epi=("bias", "res")),
    # ---- LayerNorm fold: the weight-stationary kernel at any row count ----
    _g("linear LayerNorm fold", "ln / ff", None, r=100, N=160, C0=320, ln=True),
    # ---- GEGLU on the 128-row kernel ----
    _g("linear GEGLU", "epilogues", None, r=300, N=256, C0=128, act=ACT_GEGLU),
    # ---- the (2, 1) stem hint ----
    # (mfma128, 4, 5, 104) / (mfma128, 4, 5, 56) / (mfma128, 4, 6, 56)
    _g("stem linear 128-row split-K", "stem hint", "splits", B=2, r=800, N=1024, C0=3072),
]
# ---- forced families at row counts that are no multiple of their tiles: the same family must be planned under the hint ----
for _fam, _bits, _word in FORCED:
    GEMM_SPECS.append(_g(f"forced {_fam} linear +res", "forced families", None, r=197, N=320, C0=128, flags=_bits, epi=("bias", "res"),
                         gpu_skip=STREAMK_SKIP if _word == "sw_streamk" else None))
GEMM_SPECS.append(_g("forced LDS-patch conv 3x3 +res", "forced families", None, r=256, N=320, C0=64, flags=1 << 28, epi=("bias", "res"), **CONV16))
FORCED_FAMILY_OF = {f"forced {fam} linear +res": word for fam, _bits, word in FORCED}
FORCED_FAMILY_OF["forced LDS-patch conv 3x3 +res"] = "swh"

GEMM_LINES = ("128-row split-K", "128-row reverse split", "persistent split-K", "family", "nf", "weight-stationary", "ln / ff", "forced families",
              "epilogues", "stem hint")
# lines whose specs are `origin` only by design (the table of the issue says so)
GEMM_ORIGIN_LINES = ("ln / ff", "forced families", "epilogues")

# the fused feed-forward kernel (ops.ff_geglu, C = 320, H = 1280; 32-row strips): rows per branch
FF_SPEC = dict(name="ff_geglu +res", B=3, r=167)


def gemm_plan_line(spec, rows, hint=None):
    """The descriptor ``ops.gemm`` builds for ``rows`` rows of the case, as a line for tests/gemm_plan_main.cpp."""
    w = [f"mode={spec['mode']}", f"M={rows}", f"N={spec['N']}", f"C0={spec['C0']}", f"C1={spec['C1']}", f"act={spec['act']}",
         f"flags={LDS_DMA | spec['flags']}", f"bias={int('bias' in spec['epi'])}", f"R={int('res' in spec['epi'])}", f"ln={int(spec['ln'])}"]
    if "rowvec" in spec["epi"]:
        w += ["rowvec=1", f"rowvec_div={spec['r']}"]
    if spec["mode"] == 1:
        H, W = spec["geo"]
        w += [f"Hi={H}", f"Wi={W}", f"Ho={H}", f"Wo={W}", "stride=1"]
    elif spec["mode"] == 2:
        w += [f"F={spec['geo'][0]}", f"HW={spec['geo'][1]}"]
    if spec["act"] == ACT_GEGLU:
        w.append(f"ldc={spec['N'] // 2}")
    if hint is not None:
        w.append(f"hint={hint}")
    return " ".join(w)


# ---- GroupNorm: (name, C0, C1, rows_per_group, statistics groups per branch, B, silu, sharp) ----
# One call.  C = 320: 6 rows per block, at most ceil(6500 / 48) = 136 chunks.  12 groups: ceil(1536 / 12) = 128 chunks of 51 rows; 8 groups
# un-hinted: min(192, 136) = 136 chunks of 48 rows; 51 does not divide 6500.  C = 640: 3 rows per block, at most ceil(3251 / 24) = 136 chunks:
# a target of 128 gives 126 chunks of 26 rows, un-hinted 136 chunks of 24 rows; 26 does not divide 3251.  The stem pair (2, 1): 12 groups
# against 6 (ceil(1536 / 6) = 256 > 136).  Plan words (nchunks, rows_chunk) full / hinted subset / un-hinted subset:
# (128, 51) / (128, 51) / (136, 48); C = 640: (126, 26) / (126, 26) / (136, 24)
NORM_SPECS = [
    dict(name="groupnorm C320 silu", C0=320, C1=0, rpg=6500, per_branch=4, B=3, silu=True, sharp="rows_chunk"),
    dict(name="groupnorm C320+320", C0=320, C1=320, rpg=3251, per_branch=4, B=3, silu=False, sharp="rows_chunk"),
    dict(name="stem groupnorm C320", C0=320, C1=0, rpg=6500, per_branch=6, B=2, silu=False, sharp="rows_chunk"),
]
NORM_OFFSET_SIGMA = 50    # gpu_checks._offset_data: group means 50 sigma off zero, so another summation order shows in the bits
# the two-phase entry points (pivot, partial about the pivot, apply) on the first case's shape
NORM_TWO_PHASE = NORM_SPECS[0]
# groupnorm_from_stats on the records of a producing GEMM: 4112 rows per group = 257 records -> folded in runs of 2 (the last run one
# record); one statistics group per branch; the producer M = 12336, N = 320, K = 64 is an unsplit 128-row launch (tb = 65 tiles do not fill)
NORM_RECORDS = dict(name="groupnorm_from_stats on GEMM records", C=320, K=64, rpg=4112, per_branch=1, B=3)


def norm_plan_line(spec, nsg, num=1, den=1):
    return f"C0={spec['C0']} C1={spec['C1']} rows={spec['rpg']} nsg={nsg} num={num} den={den}"


# ---- attention: the planner does not read the hint; the rows hold with and without it ----
# layout "rows": batch element i at rows [i Sq, (i + 1) Sq); "temporal": (HW, Fr) -- element i = (clip, pixel), frame f at row clip Fr HW + f HW + pixel.
# `sub`: how many leading batch elements (units of the outer index) the subset drops; full / subset instantiations as the planner names them.
def _a(name, *, batch, heads, Sq, Sk, sub, full, subset, d=64, layout="rows", kv_div=1, HW=0, causal=False):
    return dict(name=name, batch=batch, heads=heads, Sq=Sq, Sk=Sk, sub=sub, full=full, subset=subset, d=d, layout=layout, kv_div=kv_div, HW=HW, causal=causal)


ATTN_SPECS = [
    # Sq = 200: two query tiles of 128 rows per (element, head), the second ragged, so a branch's 200 rows are no multiple of what a block covers
    _a("flash b3 h3 S200", batch=3, heads=3, Sq=200, Sk=200, sub=1, full="flash<2,1,4>", subset="flash<2,1,4>"),
    # cross-attention: 2 frames share one K / V sequence (kv_div = 2); 6 elements, the subset drops branch 0's two
    _a("flash cross b6 h2 Sq130 Sk77 kv_div2", batch=6, heads=2, Sq=130, Sk=77, kv_div=2, sub=2, full="flash<2,1,4>", subset="flash<2,1,4>"),
    # one-wave temporal kernel: units = batch x heads packed 4 to a block; 3 x 7 pixels x 1 head: the subset starts at unit 7
    _a("short temporal 3 x 7 px h1 F8", batch=21, heads=1, Sq=8, Sk=8, sub=7, layout="temporal", HW=7, full="short<1>", subset="short<1>"),
    # from attention_edge_specs: one 96-key loop shape and one whole-sequence MFMA shape (3 branches of them)
    _a("loop b3 h2 S289 d72", batch=3, heads=2, Sq=289, Sk=289, d=72, sub=1, full="loop<3>", subset="loop<3>"),
    _a("small b3 h2 S50 d80", batch=3, heads=2, Sq=50, Sk=50, d=80, sub=1, full="small<3,6>", subset="small<3,6>"),
    # 8-wave blocks for the full launch (30 x 4 x 9 = 1080 blocks of 256 queries >= 1024), 4-wave blocks for the subset (20 x 4 x 9 = 720 < 1024);
    # the 10 elements of a branch share one K / V sequence (kv_div = 10), which keeps K / V small
    _a("flash 8-wave vs 4-wave b30 h4 S2100 kv_div10", batch=30, heads=4, Sq=2100, Sk=2100, kv_div=10, sub=10, full="flash<3,1,8>", subset="flash<2,1,4>"),
]
# PnP: the three-branch shared-softmax launch (qk_mod = batch / 3) against the launch a replayed site issues for [negative, editing]: Q, K from the
# cached source rows [Ts, 2 C], V from the two-branch matrix, qk_mod = batch / 2 (unet.py: HipAttnProcessor.run, src_io = ("replay", ...))
ATTN_PNP_SPECS = [
    dict(name="PnP flash b3x2 h2 S200", per_branch=2, heads=2, S=200, layout="rows", HW=0, full="flash<2,3,4>", subset="flash<2,1,4>"),
    dict(name="PnP short temporal 3 x 7 px h2 F16", per_branch=7, heads=2, S=16, layout="temporal", HW=7, full="short<3>", subset="short<1>"),
]

# ---- step kernels that take branch indices: Vtok of 3 branches with (b_unc, b_cond) = (1, 2) against Vtok[1:] with (0, 1) ----
STEP_SPEC = dict(C=4, F=5, H=9, W=7, ld=8, guidance=9.0)     # 315 pixels per branch: no multiple of a block's 256 threads
# ---- layernorm / softmax_rows: rows [T / 3, T) of the full launch; T / 3 no multiple of the rows a block takes ----
LAYERNORM_SPEC = dict(r=333, C=320)
SOFTMAX_SPEC = dict(r=333, cols=77)

# ---- the probe of check_subset_hint_restored: a Linear launch whose own 5472 rows split K (tm = 2 x 43 = 86 tiles <= 128, nk = 32: no GroupNorm
# records) while 3 / 2 of them do not (tm = 2 x 65 = 130 > 128 with nk < 72: records) -- the records query tells the two plans apart without a launch
HINT_PROBE = dict(M=5472, N=320, K=2048)
