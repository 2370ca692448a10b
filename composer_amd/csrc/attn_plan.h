// attn_plan.h -- what an attention launch is (AttnDesc) and the ONE decision of how it runs (attn_plan_fwd / attn_plan_bwd): which
// kernel form, which grids, LDS bytes and opt-in, the block plan, bias sums fused or a column-sum pass, the timing classes with
// their figures, or a refusal.  Pure host code: no HIP header, no HIP call, no allocation, no environment variable; pointers are
// looked at for null-ness only.  attention.hip: attn_fwd_run / attn_bwd_run build the plan and launch it; cmp_attn_plan shows it
// to the CPU tests (tests/test_attn_plan_host.py).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/composer_hip.h"

// Round 6 (backward pass of the fused block path): the attention backward kernels store rstd o [dQ | dK | dV], rstd being that of the
// token's row in the LayerNorm whose output fed c_attn (ln_stats_merge_kernel) -- the c_attn weight gradient then
// runs on the raw rows (elementwise.hip: wgrad_ln_fix_kernel).  The bias gradient stays the column sums of the unscaled gradient.
struct AttnLnRows {
    const float* rstd = nullptr;      // [tokens]; null: nothing of this
};

// One launch by name: causal attention on qkv [B, T, 3 H D] (head-merged), forward (o, lse out) or backward (o, lse, d_o in;
// delta, dqkv out).
struct AttnDesc {
    int dtype = CMP_BF16;
    int B = 0, T = 0, H = 0, D = 0;
    float scale = 1.f;                // the factor on q.k (the model passes 1/sqrt(E/H) of the reference's head size, which may be
                                      // smaller than D: zero-padded heads)
    float p_drop = 0.f;
    uint64_t seed = 0;
    uint32_t rng_stream = 0;
    const void* qkv = nullptr;
    void* o = nullptr;                // [B, T, H D]: written by the forward pass, read by the backward pass
    float* lse = nullptr;             // [B, H, T] row log-sum-exp
    const void* d_o = nullptr;
    float* delta = nullptr;           // [B, H, T] workspace: rowsum(dO o O)
    void* dqkv = nullptr;
    const float* amask = nullptr;     // forward: device float [B, T] added to the scaled scores of every query of a batch row
    float* bias_grad = nullptr;       // backward: also add the column sums of [dQ | dK | dV] to bias_grad[0..3 H D)
    AttnLnRows ln;                    // backward: rows stored times their token's rstd
};

// Process facts the decision depends on (attention.hip: attn_env reads them once)
struct AttnEnv {
    int ks_mode = -1;                 // COMPOSER_ATTN_KS: 0 never the key-split kernels, 1 wherever they exist (tests), else by grid size
    int bias_pass_mib = 16;           // COMPOSER_ATTN_BIAS_PASS: largest [tokens, 3E] bf16 gradient whose bias sums are a pass (0: never)
};
// Device facts about the kernels of this (type, head size), asked by the launcher once each (attention.hip: *_caps)
struct AttnCaps {
    bool ks_ok = false;               // the key-split set got its LDS opt-in (attn_ks_available)
    int wgs_per_cu = 0;               // resident workgroups per CU of the forward / dQ kernel the block plan is for; < 1: no plan
};

struct AttnLaunch {
    unsigned grid_x = 0, grid_y = 1;
    size_t smem = 0;                  // dynamic LDS bytes
    int cls = -1;                     // cmp_prof_* timing class (3 forward, 4 dQ, 5 dK/dV; -1: not timed)
    double work = 0., bytes = 0.;     // its flops and algorithmic HBM bytes
};
// Everything that is decided before the first launch.
struct AttnPlan {
    int status = CMP_OK;              // != CMP_OK: a refusal, msg says why; nothing may be enqueued
    char msg[160] = {0};
    bool empty = false;               // B * T == 0: nothing to launch
    int form = CMP_ATTN_FWD_ROWS;     // CMP_ATTN_* (composer_hip.h)
    bool drop = false;                // the DROP instantiations
    int nlaunch = 1;
    AttnLaunch l[2];                  // backward, two launches: dQ, then dK/dV
    unsigned block = 256;
    bool optin = false;               // an image above 64 KiB: the kernels need hipFuncAttributeMaxDynamicSharedMemorySize = l[i].smem
                                      // (the 128-row kernels per launch, the key-split set once per process)
    int plan_u = -1;                  // block plan of the forward / dQ launch (attn_plan_u); -1: the plain 2-D grid
    bool bias_fused = false;          // the kernels add the bias sums (float atomics)
    bool bias_pass = false;           // ... or a column-sum pass over the stored gradient follows
};

static inline int ap_cdiv(int a, int b) { return (a + b - 1) / b; }

// LDS row stride of the kernels (attention.hip: Geo<T, D>::S, tied by a static_assert there) and the images built from it
constexpr int attn_lds_stride(bool bf16, int D) { return (D < 32 ? 32 : D) + (bf16 ? 8 : 1); }
constexpr size_t attn_rows_smem(bool bf16, int D) { return (size_t)4 * 64 * attn_lds_stride(bf16, D) * (bf16 ? 2 : 4); }   // 4 images of 64 rows
constexpr size_t attn_ks_smem(bool bf16, int D) { return (size_t)4 * 256 * attn_lds_stride(bf16, D) * (bf16 ? 2 : 4); }   // 4 x 256 staged rows
constexpr size_t attn_ks_kv_smem(bool bf16, int D) { return attn_ks_smem(bf16, D) / 2 + 3 * 256 * sizeof(float); }
constexpr size_t ATTN_DKV_EXTRA = 384 * sizeof(float);        // dK/dV: lse | delta | row hash of a 128-query tile beside the images
constexpr bool attn_fwd_optin(size_t smem) { return smem > 65536; }
constexpr bool attn_bwd_optin(size_t smem) { return smem + ATTN_DKV_EXTRA > 65536; }
// the key-split kernels exist for bf16 heads up to 32 wide (at D = 64 the 256-row staging registers spill: not built)
constexpr bool attn_ks_built(bool bf16, int D) { return bf16 && D <= 32; }

// grid.x: block pairs, or single blocks when the paired grid would leave most of the 256 CUs x 2-3 workgroups without work
static inline int attn_grid_x(int Tn, int BH) {
    const int nb = ap_cdiv(Tn, 128), pairs = (nb + 1) / 2;
    return (nb > 1 && (int64_t)pairs * BH < 512) ? nb : pairs;
}
// The block plan of a forward / dQ launch (attn_job): how many (batch, head) rows per XCD run as single blocks behind the paired
// ones.  An XCD's workgroups start in order on 32 CUs x wgs_per_cu slots; the paired rows fill whole rounds of those slots and
// the rows of the last, partial round go unpaired (with less than one round of pairs: three quarters of the rows).  Measured
// (tools/ubench/attn_plan_probe.py, outputs bit-identical): B*H = 256: forward 73.6 -> 68.7 us, dQ 87.8 -> 82.0; 512: 140 -> 131,
// 171 -> 154; 1024: 286 -> 281, 321 -> 314; 128: 42 -> 38, 50 -> 46.  (A list-scheduling model of the launch predicted three times
// these gains: workgroups of a partly filled round run faster, the slots are not independent machines.)
// -1 = the plain 2-D grid (B*H not a multiple of 8, a single block, few rows, or the pairs already fill whole rounds).
static inline int attn_plan_u(int Tn, int BH, int wgs_per_cu) {
    const int nb = ap_cdiv(Tn, 128), pairs = (nb + 1) / 2;
    if (nb < 2 || (BH & 7) || (int64_t)pairs * BH < 512 || wgs_per_cu < 1) return -1;
    const int rows_x = BH / 8, slots = 32 * wgs_per_cu;
    const int rounds = rows_x * pairs / slots;
    const int paired_rows = rounds > 0 ? rounds * slots / pairs : rows_x / 4;
    const int u = rows_x - paired_rows;
    return u > 0 ? u : -1;
}
static inline void attn_plan_grid(AttnLaunch& l, int Tn, int BH, int u) {
    const int nb = ap_cdiv(Tn, 128), pairs = (nb + 1) / 2, rows_x = BH / 8;
    if (u < 0) { l.grid_x = attn_grid_x(Tn, BH); l.grid_y = BH; }
    else { l.grid_x = 8 * ((rows_x - u) * pairs + u * nb); l.grid_y = 1; }
}
// Small grids (the reference's default configuration at batch 1: 16 (batch, head) rows of 1024 tokens = 128 workgroups of the
// 128-row kind, every one a serial walk over up to 16 key tiles at ~1 us each): the key-split forms of the three kernels (KS).
static inline bool attn_key_split(int Tn, int BH, int D, bool bf16, const AttnEnv& env, bool ks_ok) {
    if (!attn_ks_built(bf16, D) || !ks_ok || Tn < 64) return false;
    if (env.ks_mode == 0) return false;
    if (env.ks_mode == 1) return true;
    // one round of 512 key-split workgroups (two per CU); with twice the rows the split already loses (default model at batch 2:
    // 2.17 vs 2.01 ms/step, tools/ks_threshold_probe.py)
    return (int64_t)ap_cdiv(Tn, 128) * BH <= 128;
}

// what no device fact changes: the refusals and the empty launch (the launcher asks this before it asks the device anything)
static inline AttnPlan attn_plan_check(const AttnDesc& d, bool backward) {
    AttnPlan p;
    p.empty = d.B * d.T == 0;
    if (p.empty) return p;
    if (d.D != 16 && d.D != 32 && d.D != 64 && d.D != 128) {
        p.status = CMP_ERR_INVALID;
        snprintf(p.msg, sizeof(p.msg), "attention: head size %d unsupported (16/32/64/128)", d.D);
    } else if (backward && d.dtype != CMP_BF16 && d.ln.rstd) {
        p.status = CMP_ERR_INVALID;
        snprintf(p.msg, sizeof(p.msg), "attention backward: LayerNorm row scaling exists in bf16 only");
    }
    return p;
}
// products: matrix products over the unmasked half, B H T^2 D flops each; rows_moved: head rows read or written per (token, head),
// beside one float (forward: lse) or two (backward: lse, delta)
static inline void attn_plan_timing(AttnLaunch& l, const AttnDesc& d, int cls, double products, double rows_moved) {
    l.cls = cls;
    l.work = products * ((double)d.B * d.H * (double)d.T * d.T * d.D);
    l.bytes = (double)d.B * d.T * d.H * (rows_moved * d.D * (d.dtype == CMP_BF16 ? 2 : 4) + (cls == 3 ? 4.0 : 8.0));
}
static inline bool attn_plan_drop(float p) { return p > 0.f && (double)p * 4294967296.0 >= 1.0; }      // common.h: make_drop(...).thr != 0

static inline AttnPlan attn_plan_fwd(const AttnDesc& d, const AttnEnv& env, const AttnCaps& caps) {
    AttnPlan p = attn_plan_check(d, false);
    if (p.status != CMP_OK || p.empty) return p;
    const bool bf16 = d.dtype == CMP_BF16;
    const int BH = d.B * d.H;
    p.drop = attn_plan_drop(d.p_drop);
    AttnLaunch& l = p.l[0];
    if (!d.amask) attn_plan_timing(l, d, 3, 2.0, 4.0);       // QK^T + PV; q, k, v in; o, lse out  (the masked forward is not timed)
    if (!d.amask && attn_key_split(d.T, BH, d.D, bf16, env, caps.ks_ok)) {
        p.form = CMP_ATTN_FWD_KS;
        l.grid_x = ap_cdiv(d.T, 32); l.grid_y = BH;
        l.smem = attn_ks_smem(bf16, d.D);
        p.optin = attn_fwd_optin(l.smem);
        return p;
    }
    p.form = d.amask ? CMP_ATTN_FWD_MASK : CMP_ATTN_FWD_ROWS;        // Transformer.call(attention_mask=...): the instances with the mask term
    l.smem = attn_rows_smem(bf16, d.D);
    p.optin = attn_fwd_optin(l.smem);
    p.plan_u = attn_plan_u(d.T, BH, caps.wgs_per_cu);
    attn_plan_grid(l, d.T, BH, p.plan_u);
    return p;
}

static inline AttnPlan attn_plan_bwd(const AttnDesc& d, const AttnEnv& env, const AttnCaps& caps) {
    AttnPlan p = attn_plan_check(d, true);
    if (p.status != CMP_OK || p.empty) return p;
    const bool bf16 = d.dtype == CMP_BF16, want_bias = d.bias_grad != nullptr;
    const int BH = d.B * d.H;
    p.drop = attn_plan_drop(d.p_drop);
    AttnLaunch &q = p.l[0], &kv = p.l[1];
    if (!d.ln.rstd && attn_key_split(d.T, BH, d.D, bf16, env, caps.ks_ok)) {
        // The c_attn bias gradient (column sums of [dQ | dK | dV]) is NOT fused here: a fused sum ends a workgroup on a transpose-reduce
        // and a device-scope float atomic whose round trip the launch has to wait out -- 16.5 of the 29.4 us of the dK/dV launch (two
        // sums) and ~8 of dQ's 19 at the default configuration (measurement builds, profiles/r5_06); only a launch of several rounds
        // hides that tail behind other workgroups.  A column-sum pass over the [tokens, 3E] gradient costs ~5 us at these sizes (63 us
        // at the benchmark's, where the fused sums stay).
        p.bias_pass = want_bias;
        p.optin = attn_fwd_optin(attn_ks_smem(bf16, d.D));
        if ((int64_t)2 * ap_cdiv(d.T, 32) * BH > 512) {      // not resident at once: two launches
            p.form = CMP_ATTN_BWD_KS2;
            p.nlaunch = 2;
            q.grid_x = kv.grid_x = ap_cdiv(d.T, 32); q.grid_y = kv.grid_y = BH;
            q.smem = attn_ks_smem(bf16, d.D);
            kv.smem = attn_ks_kv_smem(bf16, d.D);
            attn_plan_timing(q, d, 4, 3.0, 6.0);
            attn_plan_timing(kv, d, 5, 4.0, 6.0);
            return p;
        }
        // one launch, both roles: LDS = the larger of the two (dQ double-buffers its 256-key tiles)
        p.form = CMP_ATTN_BWD_KS1;
        q.grid_x = 2 * ap_cdiv(d.T, 32); q.grid_y = BH;
        q.smem = attn_ks_smem(bf16, d.D);
        attn_plan_timing(q, d, 5, 7.0, 9.0);                 // (counted with the dK/dV class: one launch carries the seven products)
        return p;
    }
    // the 128-row kernels; with ln.rstd the backward pass of the fused block path (bf16, chip-filling launches): rstd-scaled stores
    p.form = d.ln.rstd ? CMP_ATTN_BWD_LN : CMP_ATTN_BWD_ROWS;
    p.nlaunch = 2;
    // Short launches take the c_attn bias sums out of the kernels too (see the key-split branch): the fused float atomics leave a ~16 us
    // tail that only a launch of several rounds hides.  Same box, [tokens, 3E] gradient of 1.6 ... 12.6 MB (the default model at batch
    // 1 ... 8): 2.99 -> 2.67 ms/step at batch 8, 1.95 -> 1.76 at batch 2; 25 MB (6L/8H/d512 at batch 8): 3.03 vs 3.04; 100 MB (batch 32):
    // 7.39 vs 7.43 -- the pass re-reads the gradient, so it stops at 16 MiB (COMPOSER_ATTN_BIAS_PASS=<MiB> overrides, 0 = never).
    p.bias_pass = want_bias && !d.ln.rstd && bf16 && (int64_t)d.B * d.T * 3 * d.H * d.D * 2 <= (int64_t)env.bias_pass_mib << 20;
    p.bias_fused = want_bias && !p.bias_pass;
    q.smem = attn_rows_smem(bf16, d.D);
    kv.smem = q.smem + ATTN_DKV_EXTRA;
    p.optin = attn_bwd_optin(q.smem);
    p.plan_u = attn_plan_u(d.T, BH, caps.wgs_per_cu);
    attn_plan_grid(q, d.T, BH, p.plan_u);
    kv.grid_x = attn_grid_x(d.T, BH); kv.grid_y = BH;
    attn_plan_timing(q, d, 4, 3.0, 6.0);                     // q, k, v, o, dO, lse in; dQ, delta out
    attn_plan_timing(kv, d, 5, 4.0, 6.0);                    // q, k, v, dO, lse, delta in; dK, dV out
    return p;
}
