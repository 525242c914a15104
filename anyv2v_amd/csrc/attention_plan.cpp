// Launch planning of the attention entry points (attention_plan.h): every rule that decides which kernel instantiation runs a
// descriptor, with the measurements behind each threshold.  Host code only.
#include "attention_plan.h"

namespace {
bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

#define PLAN_CHECK(cond, ...) do { if (!(cond)) { anyv2v_set_error(__VA_ARGS__); p.status = ANYV2V_EINVAL; return p; } } while (0)

// kernel and template arguments of every instantiation attention.hip holds, in the order of av_attn_instantiation()
struct Inst { AttnKernel kernel; int stages, streams, waves, ds, nkb; bool bias; const char* name; };
const Inst INSTS[] = {
    {ATTN_NAIVE, 0, 0, 0, 0, 0, false, "naive"},           {ATTN_NAIVE, 0, 0, 0, 0, 0, true, "naive+bias"},
    {ATTN_SHORT, 0, 1, 0, 0, 0, false, "short<1>"},        {ATTN_SHORT, 0, 3, 0, 0, 0, false, "short<3>"},
    {ATTN_FLASH, 2, 1, 4, 0, 0, false, "flash<2,1,4>"},    {ATTN_FLASH, 3, 1, 8, 0, 0, false, "flash<3,1,8>"},
    {ATTN_FLASH, 2, 3, 4, 0, 0, false, "flash<2,3,4>"},    {ATTN_FLASH, 3, 3, 8, 0, 0, false, "flash<3,3,8>"},
    {ATTN_SMALL, 0, 0, 0, 2, 6, false, "small<2,6>"},      {ATTN_SMALL, 0, 0, 0, 3, 6, false, "small<3,6>"},
    {ATTN_SMALL, 0, 0, 0, 4, 6, false, "small<4,6>"},      {ATTN_SMALL, 0, 0, 0, 5, 6, false, "small<5,6>"},
    {ATTN_SMALL, 0, 0, 0, 2, 18, false, "small<2,18>"},    {ATTN_SMALL, 0, 0, 0, 3, 18, false, "small<3,18>"},
    {ATTN_SMALL, 0, 0, 0, 4, 18, false, "small<4,18>"},
    {ATTN_SMALL, 0, 0, 0, 2, 6, true, "small<2,6,bias>"},  {ATTN_SMALL, 0, 0, 0, 3, 6, true, "small<3,6,bias>"},
    {ATTN_SMALL, 0, 0, 0, 4, 6, true, "small<4,6,bias>"},  {ATTN_SMALL, 0, 0, 0, 5, 6, true, "small<5,6,bias>"},
    {ATTN_LOOP, 0, 0, 0, 2, 6, false, "loop<2>"},          {ATTN_LOOP, 0, 0, 0, 3, 6, false, "loop<3>"},
    {ATTN_LOOP, 0, 0, 0, 4, 6, false, "loop<4>"},          {ATTN_LOOP, 0, 0, 0, 5, 6, false, "loop<5>"},
};
constexpr int N_INSTS = (int)(sizeof(INSTS) / sizeof(INSTS[0]));

const Inst* find_inst(const AttnPlan& p) {
    for (int i = 0; i < N_INSTS; ++i) {
        const Inst& t = INSTS[i];
        if (t.kernel == p.kernel && t.stages == p.stages && t.streams == p.streams && t.waves == p.waves && t.ds == p.ds && t.nkb == p.nkb &&
            t.bias == p.bias)
            return &t;
    }
    return nullptr;
}

// K [keys][32 ds + 8] and V^T [32 ds][keys + 4] of one head in fp16: the dynamic LDS of the whole-sequence and the 96-key loop kernels
size_t kv_lds_bytes(int ds, int nkb) { return (size_t)(nkb * 16) * (ds * 32 + 8) * 2 + (size_t)(ds * 32) * (nkb * 16 + 4) * 2; }

// one thread per (batch, head, query), 128 per block
void naive(AttnPlan& p, const AnyV2VAttnDesc& d, bool bias, int causal) {
    const long long total = (long long)d.batch * d.heads * d.Sq;
    p.kernel = ATTN_NAIVE;
    p.bias = bias;
    p.causal = causal;
    p.grid_x = (unsigned)((total + 127) / 128);
    p.block = 128;
}
// one block per (64 queries, head, batch element), K / V of the head in dynamic LDS
void kv_in_lds(AttnPlan& p, const AnyV2VAttnDesc& d, AttnKernel kernel, int ds, int nkb, bool bias, int causal) {
    p.kernel = kernel;
    p.ds = ds;
    p.nkb = nkb;
    p.bias = bias;
    p.causal = causal;
    p.grid_x = (unsigned)((d.Sq + 63) / 64);
    p.grid_y = (unsigned)d.heads;
    p.grid_z = (unsigned)d.batch;
    p.block = 256;
    p.lds_bytes = kv_lds_bytes(ds, nkb);
}
void flash(AttnPlan& p, int stages, int streams, int waves, long long blocks) {
    p.kernel = ATTN_FLASH;
    p.stages = stages;
    p.streams = streams;
    p.waves = waves;
    p.grid_x = (unsigned)blocks;
    p.block = 64 * waves;
}

// what the vectorised kernels need of the operands: 16-byte chunks of Q / K / V, 8-byte stores of O (o_align = 15: 16-byte)
bool vector_ok(const AnyV2VAttnDesc& d, uintptr_t o_align) {
    return !(d.flags & 1) && d.ldq % 8 == 0 && d.ldk % 8 == 0 && d.ldv % 8 == 0 && d.ldo % 4 == 0 && aligned16(d.Q) && aligned16(d.K) &&
           aligned16(d.V) && (((uintptr_t)d.O) & o_align) == 0;
}

// PnP injection launch (i2vgen-xl/pnp_utils.py:189-196, :295-302): three branches whose Q / K are the source branch's -> the shared-softmax
// kernels.  ONE predicate for the short and the flash path (flag bit3 forces the per-branch aliasing form).
bool pnp3(const AnyV2VAttnDesc& d) { return d.qk_mod > 0 && d.batch == 3 * d.qk_mod && d.kv_div == 1 && !(d.flags & 8); }

// ---- anyv2v_attention_f16: head_dim 64 ----
AttnPlan plan_d64(AttnPlan p, const AnyV2VAttnDesc& d) {
    if (!vector_ok(d, 15)) { naive(p, d, false, 0); return p; }
    if (d.Sq <= 16 && d.Sk <= 16 && d.ldo % 8 == 0 && !(d.flags & 2)) {   // temporal attention at <= 16 frames: one wave per sequence
        // PnP injection step: one wave per (source element, head), one softmax, three V / O streams (flag bit3: aliasing form)
        const bool three = pnp3(d);
        const long long units = (long long)(three ? d.qk_mod : d.batch) * d.heads;
        p.kernel = ATTN_SHORT;
        p.streams = three ? 3 : 1;
        p.grid_x = (unsigned)((units + 3) / 4);
        p.block = 256;
        return p;
    }
    // The flash kernels keep the per-lane K / V source offsets of one 64-key tile in 32 bits (koff / voff_g: byte offsets of key rows
    // 0 .. 63 from the tile pointer, 16-byte chunk included).  A layout whose largest in-tile byte offset does not fit -- or a negative
    // sequence stride, which those unsigned offsets cannot hold -- runs on kernels that address every row in 64 bits: the 96-key loop
    // kernel (same addressing contract: strides, kv_div, qk_mod as per-branch aliasing), or the generic kernel when the grid does not
    // fit the loop kernel's.  Every shape the models issue stays far below the limit (4096 x 960 elements per key step against 34.1 M).
    {
        const long long ldkv = d.ldk > d.ldv ? d.ldk : d.ldv;
        const bool wide = d.kv_seq < 0 || d.kv_seq > ((long long)0xFFFFFFFFll / 2 - 64) / 63 / ldkv;   // (63 kv_seq ld + 64) * 2 > 2^32 - 1
        if (wide) {
            p.wide_reason = d.kv_seq < 0 ? "negative kv_seq" : "K / V tile offsets beyond 32 bits";
            if (d.heads <= 65535 && d.batch <= 65535) kv_in_lds(p, d, ATTN_LOOP, 2, 6, false, 0);   // 26 KiB: below the default dynamic-LDS limit
            else naive(p, d, false, 0);
            return p;
        }
    }
    const long long nwg = (long long)d.batch * d.heads * p.q_tiles;
    PLAN_CHECK(nwg < (1ll << 31), "attention: grid too large");
    const int q_tiles8 = (d.Sq + 255) / 256;
    if (pnp3(d)) {
        // PnP injection step: one softmax per source element, three V / O streams (flag bit3 forces the aliasing form)
        // long KV loops with enough 256-query blocks to fill the chip (the 64x64 level: 16 x 5 x 16 = 1280): 8-wave blocks around a
        // 3-stage ring -- two K / V tile sets in flight instead of one, half the LDS-DMA per query, one 96-KiB block per CU (the same
        // two waves per SIMD as two 4-wave blocks).  0.6845 -> 0.6479 ms at (48, 5, 4096); 7 % slower at (48, 10, 1024), which stays
        // on the 4-wave form (profiles/r05_attn_pnp_8wave_ab.txt); bit-equal.  Flag bit2: never (as for the plain kernel).
        const long long n8 = (long long)d.qk_mod * d.heads * q_tiles8;
        if (!(d.flags & 4) && d.Sk >= 2048 && d.Sq >= 2048 && n8 >= 1024) {
            p.q_tiles = q_tiles8;
            flash(p, 3, 3, 8, n8);
            return p;
        }
        flash(p, 2, 3, 4, (long long)d.qk_mod * d.heads * p.q_tiles);
        return p;
    }
    // 8-wave blocks (256 query rows per K / V ring) for launches that still fill the chip with them and whose KV loop is long
    // enough to amortise the bigger block (measured: 1.19 -> 1.09 ms at 48 x 5 x 4096^2, equal at 1024^2, slower at Sk = 145)
    const long long nwg8 = (long long)d.batch * d.heads * q_tiles8;
    // (round 5: from Sk = 2048 on -- at 48 x 10 x 1024^2 the 4-wave kernel on its 2-stage ring is 4 % faster, 146.4 vs 152.0 us)
    if (!(d.flags & 4) && d.Sk >= 2048 && d.Sq >= 1024 && nwg8 >= 1024) {
        p.q_tiles = q_tiles8;
        flash(p, 3, 1, 8, nwg8);
        return p;
    }
    // 4-wave blocks on a 2-stage ring: 32 KiB of LDS per block = four blocks per CU (three with 3 stages; the kernel's launch bounds ask
    // for four waves per SIMD, it allocates 126 VGPRs -- profiles/r06_attention_resource_usage.txt); the short-KV launches
    // (cross-attention, Sk = 145: three tiles per block, 7680 blocks) are bound by how many blocks are in flight -- 95.8 -> 82.6 us at
    // (48, 5, 4096, 145), never slower up to Sk = 1024 (profiles/r05_attn_cross_2stage_ab.txt); bit-equal
    flash(p, 2, 1, 4, nwg);
    return p;
}

// ---- anyv2v_attention_small_f16: any head_dim <= 160 ----
AttnPlan plan_small(AttnPlan p, const AnyV2VAttnDesc& d, int head_dim) {
    const int causal = (d.flags & 16) ? 1 : 0;
    // short sequences, head_dim a multiple of 8 (16-byte chunks of a head are loaded whole): whole-sequence MFMA kernel (K and V^T of
    // a head in LDS, zero-padded to 32 DS columns); flag bit0 = naive kernel.  DS = 5 (head_dim 136..160, ConsistI2V's temporal
    // attention at C = 1280 / 8 heads) fits the LDS with up to 96 keys only.
    const int ds = (head_dim + 31) / 32;
    const int nkb = d.Sk <= 96 ? 6 : (d.Sk <= 288 && ds <= 4 ? 18 : 0);
    const bool operands_ok = vector_ok(d, 7) && head_dim % 8 == 0 && d.heads <= 65535 && d.batch <= 65535;
    // a longer key sequence: the 96-key loop kernel (online softmax), head_dim 8..24 on its DS = 2 form
    if (operands_ok && ds >= 1 && ds <= 5 && nkb == 0) {
        kv_in_lds(p, d, ATTN_LOOP, ds < 2 ? 2 : ds, 6, false, causal);
        return p;
    }
    if (!(operands_ok && ds >= 2 && ds <= 5 && nkb > 0)) { naive(p, d, false, causal); return p; }
    kv_in_lds(p, d, ATTN_SMALL, ds, nkb, false, causal);
    return p;
}

// ---- anyv2v_attention_bias_f16: additive score bias ----
AttnPlan plan_bias(AttnPlan p, const AnyV2VAttnDesc& d, int head_dim) {
    // short sequences at head_dim % 8 == 0: the whole-sequence MFMA kernel with the bias added to the score fragments
    const int ds = (head_dim + 31) / 32;
    if (vector_ok(d, 7) && head_dim % 8 == 0 && ds >= 2 && ds <= 5 && d.Sk <= 96 && d.heads <= 65535 && d.batch <= 65535 && !(d.flags & 16)) {
        kv_in_lds(p, d, ATTN_SMALL, ds, 6, true, 0);
        return p;
    }
    naive(p, d, true, (d.flags & 16) ? 1 : 0);
    return p;
}
}   // namespace

AttnPlan av_attn_plan(const AnyV2VAttnDesc* d, AttnEntry entry, int head_dim, bool has_bias) {
    AttnPlan p = {};
    p.status = ANYV2V_OK;
    p.kernel = ATTN_NAIVE;
    p.grid_y = p.grid_z = 1;
    if (entry == ATTN_ENTRY_SMALL) PLAN_CHECK(head_dim > 0 && head_dim <= 160, "attention_small: head_dim must be in 1..160");
    if (entry == ATTN_ENTRY_BIAS) {
        PLAN_CHECK(head_dim > 0 && head_dim <= 160, "attention_bias: head_dim must be in 1..160");
        PLAN_CHECK(has_bias, "attention_bias: null bias");
        PLAN_CHECK(d && d->scale > 0.f, "attention_bias: scale must be positive");
    }
    PLAN_CHECK(d != nullptr, "attention: null descriptor");
    PLAN_CHECK(d->Q && d->K && d->V && d->O, "attention: null pointer");
    PLAN_CHECK(d->batch > 0 && d->heads > 0 && d->Sq > 0 && d->Sk > 0, "attention: bad sizes");
    PLAN_CHECK(d->inner > 0 && d->kv_div > 0 && d->qk_mod >= 0, "attention: bad inner/kv_div/qk_mod");
    PLAN_CHECK(d->ldq > 0 && d->ldk > 0 && d->ldv > 0 && d->ldo > 0, "attention: leading dimensions must be positive");
    p.q_tiles = (d->Sq + 127) / 128;
    p = entry == ATTN_ENTRY_D64 ? plan_d64(p, *d) : entry == ATTN_ENTRY_SMALL ? plan_small(p, *d, head_dim) : plan_bias(p, *d, head_dim);
    // a plan outside the table names a kernel attention.hip does not hold (and av_attn_instantiation() would not list): an error, never another kernel
    PLAN_CHECK(p.status != ANYV2V_OK || find_inst(p) != nullptr, "attention: the plan names no instantiation");
    return p;
}

const char* av_attn_kernel_name(const AttnPlan& p) {
    const Inst* t = find_inst(p);
    return t != nullptr ? t->name : "?";
}

int av_attn_instantiation_count() { return N_INSTS; }

AttnPlan av_attn_instantiation(int i) {
    AttnPlan p = {};
    const Inst& t = INSTS[i];
    p.kernel = t.kernel;
    p.stages = t.stages; p.streams = t.streams; p.waves = t.waves;
    p.ds = t.ds; p.nkb = t.nkb; p.bias = t.bias;
    return p;
}
