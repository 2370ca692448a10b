// gemm_plan.h -- what a GEMM launch is (GemmDesc, GemmExtra) and the ONE decision of how it runs (gemm_plan): which kernel, which
// grid, which epilogue kind, column sums fused or not, slabs or atomics, LayerNorm kind or refusal.  Pure host code: no HIP
// header, no HIP call, no allocation, no environment variable; pointers are looked at for null-ness and 16-byte alignment only.
// gemm.hip: gemm_run builds the plan and launches it; cmp_gemm_plan shows it to the CPU tests (tests/test_gemm_plan_host.py).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/composer_hip.h"

// tile shapes of the kernel families (gemm.hip)
#define F_BM 64                // fp32 (parity mode): 64x64x16
#define F_BN 64
#define F_BK 16
#define G_BM 128               // bf16 generic and 128x128 direct-to-LDS: 128x128x64
#define G_BN 128
#define G_BK 64
#define G_IMG (128 * 64 * 2)   // bytes per operand image
#define H_BM 256               // persistent 256x256 two-stage: 256x256x64
#define H_BN 256
#define H_IMG (256 * 64 * 2)
#define P_BK 32                // deep pipeline: k-steps of 32

// compile-time epilogue kinds (gemm.hip: "compile-time epilogue kinds for the persistent kernels")
enum { EPI_GENERIC = 0, EPI_PLAIN = 1, EPI_GELU_AUX = 2, EPI_RESID = 3, EPI_GELUGRAD = 4, EPI_PLAIN32 = 5 };

// LayerNorm folded into the epilogues of the forward GEMMs (gemm.hip: epi_tile<.., LNM, NP>; full 256x256 tiles, bf16).  The
// statistics of a row travel as PARTIALS: (mean, M2 = sum of squared deviations from that mean) of every 256-column segment of
// the row, written by the epilogue of the GEMM (or the embedding kernel) that produced the row and merged by whoever consumes
// it (Chan's parallel update -- never a sum of squares).
//   consumer, fold (c_attn / c_fc: transformer.py:583-584,591 followed by Conv1D :205-209):
//       LN(x).W + b = rstd * (x.(gamma o W)) - rstd*mean * colsum(gamma o W) + (beta.W + b)
//     the GEMM runs on the RAW rows x and the gamma-scaled weight shadow; `cs` = colsum of that shadow, bias = beta.W + b.
//   consumer, residual (attention c_proj, :587 r = LN1(x) + dropout(proj)): the residual operand is rebuilt from the raw
//     row, its statistics and gamma / beta.
//   producer (both c_proj): the epilogue owns a 256-column tile of every output row and emits that segment's partial.
struct LnEpi {
    const float* in_part = nullptr;   // [rows][np][2] partial statistics of the LayerNorm input's rows (null: no LayerNorm on the way in)
    int np = 0;                       // segments per row = E / 256
    float eps = 0.f;
    const float* cs = nullptr;        // fold: [N] column sums of the gamma-scaled bf16 weight
    const float* gamma = nullptr;     // residual rebuild: [N] gamma, beta of the LayerNorm whose output is the residual operand
    const float* beta = nullptr;
    float* out_part = nullptr;        // [rows][N / 256][2] partial statistics of the OUTPUT rows (null: not wanted)
    // Round 6, the backward pass of the fused block path ("scale" mode, with in_part): nothing is normalised, the row's rstd is a
    // FACTOR -- EPI_GELUGRAD writes rstd o (acc * gelu'(aux)) (the column sums of the unscaled product still go to the launch's colsum);
    // EPI_RESID adds rstd o resid instead of resid (model.hip: backward).
    int scale = 0;
};

// The problem of one launch: C[M,N] = epilogue(A . B), the arguments of the C ABI's cmp_k_gemm by name.
struct GemmDesc {
    int dtype = CMP_BF16;
    int ta = 0, tb = 0;               // ta: A stored [K,M]; tb: B stored [N,K]
    int M = 0, N = 0, K = 0;
    const void* A = nullptr;
    int lda = 0;
    const void* B = nullptr;
    int ldb = 0;
    void* C = nullptr;
    int ldc = 0;
    const float* bias = nullptr;      // [N] or null
    int act = 0;                      // 0 none, 1 gelu (pre-activation -> aux), 2 multiply by gelu'(aux)
    void* aux = nullptr;
    int ldaux = 0;
    const void* resid = nullptr;
    int ldr = 0;
    int out_fp32 = 0;
    int splitk = 1;
    float p_drop = 0.f;
    uint64_t seed = 0;
    uint32_t rng_stream = 0;
    int flags = 0;                    // CMP_GEMM_*
};

// Per-launch context of the GEMM launcher (gemm.hip: gemm_run) that the C ABI's cmp_k_gemm does not carry.  The model driver
// fills one per call, so nothing about a launch lives in process-wide state.
struct SchedWs;
struct WgradWs;
struct GemmExtra {
    LnEpi ln;                    // LayerNorm fused into this launch's epilogue (forward GEMMs of the fused block path, model.hip)
    float* colsum = nullptr;     // also add the column sums of the output to colsum[0..N) (the bias gradient that goes with an
                                 // input-gradient GEMM); fused into the epilogue where possible, else a colsum pass after it
    float* slab_ws = nullptr;    // split-K: per-split fp32 partial tiles + fixed-order reduce instead of float atomics
    size_t slab_bytes = 0;
    int role = -1;               // cmp_prof_* timing class: 0 forward, 1 dgrad, 2 wgrad, -1 = by operand layout
    int max_wgs = 0;             // cap on the persistent kernels' grid (CUs left to a concurrent RCCL kernel); 0 = all 256
    bool rev = false;            // persistent 256x256 kernel: walk every XCD group's run of tiles from its end (gemm.hip: item_coords)
    bool dp = false;             // the launch belongs to a data-parallel job: persistent kernels hand their items out dynamically
    SchedWs* sched = nullptr;    // the calling context's item-counter workspace (a cmp_ctx is single-threaded by contract: no lock)
    WgradWs* wws = nullptr;      // grouped weight gradients: the caller's partial-tile workspace selects the last-arriver form
                                 // (no float atomics: deterministic mode); null: the float-atomic form (default, faster)
};

// Process facts the decision depends on (gemm.hip: gemm_env reads them)
struct GemmEnv {
    bool fast_kinds = true;      // COMPOSER_GEMM_FAST_KINDS != 0: compile-time epilogue kinds on the 128x128 kernel
    int ring_min = 2;            // COMPOSER_GEMM_RING: fewest k-steps that take the four-stage ring (0: off)
    bool stamps = false;         // a timeline stamp buffer is set (cmp_gemm_set_stamps): the diagnostic builds of the deep pipeline
};


// 256x256 persistent tiles once they give most of the chip a tile (or a split-K launch sizes its own item count); the 128x128
// kernel (2 workgroups per CU) below that: at the default config (E=256, B=1: M=1024) the 256-tile kernels ran 4-16
// workgroups on 256 CUs (27 us for a 4-tile launch)
constexpr int64_t GEMM_BIG_MIN_MN = 512ll * 512;
constexpr int64_t GEMM_BIG_MIN_TILES = 192;

// Everything that is decided before the first HIP call of a launch.
struct GemmPlan {
    int status = CMP_OK;         // != CMP_OK: a refusal, msg says why; nothing may be enqueued
    char msg[320] = {0};
    bool empty = false;          // M == 0 or N == 0: nothing to launch
    int family = CMP_GEMM_FAM_F32;
    bool a_km = false, b_km = false;      // A / B stored K-contiguous (!ta / tb): the kernels' layout parameters
    bool swap = false;           // bf16 kernels: the non-atomic epilogue (transposed accumulator tiles, vector stores)
    int kind = EPI_GENERIC;      // compile-time epilogue kind; EPI_GENERIC: the run-time epilogue
    int lnm = 0, np = 1;         // LayerNorm mode and segment count of the persistent 256x256 kernel (LNM, NP)
    bool diag = false;           // the timeline-stamp build of the deep pipeline
    unsigned grid_x = 0, grid_y = 1, grid_z = 1, block = 0;
    size_t smem = 0;             // dynamic LDS bytes
    int nk = 0;                  // k-steps of the family's depth (16 / 64 / 32)
    int per = 0, nsplit = 1;     // k-steps per split, splits
    int tiles_n = 0, ntiles = 0;
    bool slabs = false;          // split-K through per-split slabs in the workspace + gemm_slab_reduce_kernel (else f32 atomics)
    int reduce_grid = 0;
    bool colsum_fused = false;   // the epilogue adds the column sums
    bool colsum_pass = false;    // ... or cmp_k_colsum runs after the launch
    int cls = -1;                // cmp_prof_* timing class (-1: the fp32 kernel is not timed)
    bool sched = false;          // the launch draws an item-counter set (sched_next)
};

static inline int gp_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int gp_min(int a, int b) { return a < b ? a : b; }
static inline int gp_max(int a, int b) { return a > b ? a : b; }

// the kind a launch may use (full tiles only; everything else takes the generic run-time epilogue).  `atomic`: the epilogue
// accumulates with f32 atomics (split-K without slabs); slab launches store fp32, so out_fp32 already rules them out.
static inline int gemm_epi_kind(const GemmDesc& d, bool drop, bool atomic, int tile) {
    if (atomic || d.out_fp32 || (d.flags & CMP_GEMM_NOSTORE) || d.M % tile || d.N % tile) return EPI_GENERIC;
    if (d.act == 1) return (!d.resid && !drop) ? EPI_GELU_AUX : EPI_GENERIC;
    if (d.act == 2) return (!d.resid && !drop && !d.bias) ? EPI_GELUGRAD : EPI_GENERIC;
    if (d.resid) return EPI_RESID;
    return drop ? EPI_GENERIC : EPI_PLAIN;
}

#define GP_REQUIRE(cond, ...)                                   \
    do {                                                        \
        if (!(cond)) {                                          \
            p.status = CMP_ERR_INVALID;                         \
            snprintf(p.msg, sizeof(p.msg), __VA_ARGS__);        \
            return p;                                           \
        }                                                       \
    } while (0)

static inline GemmPlan gemm_plan(const GemmDesc& d, const GemmExtra& ex, const GemmEnv& env) {
    GemmPlan p;
    const int M = d.M, N = d.N, K = d.K, flags = d.flags;
    const bool ta = d.ta != 0, tb = d.tb != 0;
    p.empty = M == 0 || N == 0;
    if (p.empty) return p;
    GP_REQUIRE(K > 0, "gemm: K must be positive");
    const int lnm = (ex.ln.in_part ? 1 : 0) | (ex.ln.out_part ? 2 : 0);
    const int np = ex.ln.np;
    if (ex.colsum) GP_REQUIRE(!d.out_fp32 && d.splitk <= 1, "gemm: column sums need a plain (non split-K) output in the compute dtype");
    if (d.splitk > 1)
        GP_REQUIRE(d.out_fp32 && !d.bias && d.act == 0 && !d.resid && d.p_drop == 0.f, "gemm: split-K needs a plain fp32 accumulate epilogue");
    GP_REQUIRE(d.act == 0 || d.aux != nullptr || d.act == 1, "gemm: act=2 needs aux");
    const bool atomic = d.splitk > 1;                                             // (as asked for, before the clamp to the k-steps)
    const bool drop = d.p_drop > 0.f && (double)d.p_drop * 4294967296.0 >= 1.0;   // common.h: make_drop(...).thr != 0
    const int max_wgs = ex.max_wgs > 0 ? gp_min(ex.max_wgs, 256) : 256;
    p.a_km = !ta;
    p.b_km = tb;
    p.swap = !atomic;
    p.block = 256;
    p.colsum_pass = ex.colsum != nullptr;
    // a launch that asks for a LayerNorm epilogue must reach a kernel that has one: the persistent 256x256 kernel only
#define GP_NO_LN() GP_REQUIRE(lnm == 0, "gemm: a LayerNorm epilogue was asked of a launch that went to a kernel without one (M=%d N=%d K=%d dtype=%d flags=%d)", M, N, K, d.dtype, flags)
    if (d.dtype == CMP_FP32) {
        p.family = CMP_GEMM_FAM_F32;
        p.nk = gp_cdiv(K, F_BK);
        p.per = gp_cdiv(p.nk, gp_max(1, gp_min(d.splitk, p.nk)));
        p.nsplit = gp_cdiv(p.nk, p.per);
        p.tiles_n = gp_cdiv(N, F_BN);
        p.ntiles = p.tiles_n * gp_cdiv(M, F_BM);
        p.grid_x = p.tiles_n; p.grid_y = gp_cdiv(M, F_BM); p.grid_z = p.nsplit;
        GP_NO_LN();
        return p;
    }
    GP_REQUIRE(d.lda % 8 == 0 && d.ldb % 8 == 0, "gemm(bf16): leading dimensions must be multiples of 8 (lda=%d ldb=%d)", d.lda, d.ldb);
    GP_REQUIRE(((uintptr_t)d.A & 15) == 0 && ((uintptr_t)d.B & 15) == 0, "gemm(bf16): operands must be 16-byte aligned");
    // timing class of cmp_prof_*: by role when the caller announced one (the model: 0 forward, 1 dgrad, 2 wgrad),
    // otherwise by layout (the forward GEMMs read a transposed weight copy, i.e. the dgrad layout)
    p.cls = ex.role >= 0 ? ex.role : (ta ? 2 : (tb ? 1 : 0));
    p.nk = gp_cdiv(K, G_BK);
    p.per = gp_cdiv(p.nk, gp_max(1, gp_min(d.splitk, p.nk)));
    p.nsplit = gp_cdiv(p.nk, p.per);
    // fast path: direct-to-LDS staging needs every 64-deep k-step of a K-contiguous operand inside its row
    // (K % 64 == 0, or the caller vouches for zero padding up to a multiple of 64 with CMP_GEMM_KPAD_ZERO) and
    // 32-bit byte offsets.
    const int k64 = (K + 63) / 64 * 64;
    const bool kpad = (K % 64 == 0) || ((flags & CMP_GEMM_KPAD_ZERO) && (ta || d.lda >= k64) && (!tb || d.ldb >= k64));
    const bool km_ok = (ta && !tb) || kpad;
    const int64_t a_span = (int64_t)(ta ? K : M) * d.lda * 2, b_span = (int64_t)(tb ? N : K) * d.ldb * 2;
    const bool fast = km_ok && a_span < 0x7FFFFFF0ll && b_span < 0x7FFFFFF0ll && d.ldc % 8 == 0 && (d.out_fp32 || N % 8 == 0) &&
                      (!d.aux || (d.ldaux % 8 == 0 && N % 8 == 0)) && (!d.resid || (d.ldr % 8 == 0 && N % 8 == 0)) && !(flags & CMP_GEMM_GENERIC);
    const int64_t t256 = (int64_t)gp_cdiv(M, 256) * gp_cdiv(N, 256);
    const bool big = fast && !(flags & CMP_GEMM_TILE128) &&
                     ((flags & (CMP_GEMM_TILE256 | CMP_GEMM_P4)) || ((int64_t)M * N >= GEMM_BIG_MIN_MN && (t256 >= GEMM_BIG_MIN_TILES || d.splitk > 1)));
    // measured at the C2 shapes (tools/kbench.py): both-K-contiguous (dgrad) is fastest on the 2-stage BK=64 kernel
    // (its DMA pieces are whole 128-byte lines); forward and wgrad on the 4-stage BK=32 deep pipeline.
    const bool prefer_p4 = !(!ta && tb);
    if (big && ((flags & CMP_GEMM_P4) || (!(flags & CMP_GEMM_TILE256) && K % 32 == 0 && prefer_p4))) {
        // deep-pipeline kernels: split granularity is a 32-deep k-step.  128x256 tiles, 2 workgroups per CU (one's epilogue /
        // store drain overlaps the other's main loop), or 256x256, 1 per CU.
        const int nwm = (flags & CMP_GEMM_P4_128) ? 1 : 2, nst = nwm == 1 ? 3 : 4, bm = 128 * nwm;
        p.family = nwm == 1 ? CMP_GEMM_FAM_P4_128 : CMP_GEMM_FAM_P4_256;
        p.nk = gp_cdiv(K, P_BK);
        p.per = gp_cdiv(p.nk, gp_max(1, gp_min(d.splitk, p.nk)));
        p.nsplit = gp_cdiv(p.nk, p.per);
        // split-K: partial slabs + reduce when the registered workspace is large enough, else f32 atomics
        p.slabs = atomic && p.nsplit > 1 && d.ldc == N && (N % 4 == 0) && ex.slab_ws && (size_t)p.nsplit * M * N * 4 <= ex.slab_bytes &&
                  !(flags & CMP_GEMM_ATOMICS);
        p.swap = !atomic || p.slabs;
        const int64_t reduce_wgs = ((int64_t)M * N / 4 + 255) / 256;               // gemm_slab_reduce_kernel: 16 bytes per lane
        if (p.slabs) p.reduce_grid = (int)(reduce_wgs < 2048 ? reduce_wgs : 2048);
        p.tiles_n = gp_cdiv(N, H_BN);
        p.ntiles = p.tiles_n * gp_cdiv(M, bm);
        p.grid_x = gp_min(p.ntiles * p.nsplit, nwm == 1 ? 2 * max_wgs : max_wgs);   // persistent: one (two) workgroups per CU in use
        p.block = 256 * nwm;
        p.smem = (size_t)nst * (bm * P_BK * 2 + 256 * P_BK * 2) + 16;               // + the item slot
        p.sched = true;
        if (!ta && !tb) {
            // the forward layout carries the compile-time kinds (whole 256x256 tiles in both configurations) and the timeline build
            const int kind = gemm_epi_kind(d, drop, atomic, 256);
            if (kind == EPI_PLAIN || kind == EPI_GELU_AUX || kind == EPI_RESID) p.kind = kind;
            p.diag = env.stamps && p.swap && nwm == 2;
        } else if (ta && !tb) {
            p.diag = env.stamps && !p.swap && nwm == 2;                             // timeline of the wgrad layout (split-K atomics epilogue)
        }
        GP_NO_LN();
    } else if (big) {
        p.family = CMP_GEMM_FAM_TILE256;
        p.tiles_n = gp_cdiv(N, H_BN);
        p.ntiles = p.tiles_n * gp_cdiv(M, H_BM);
        p.grid_x = gp_min(p.ntiles * p.nsplit, max_wgs);
        p.block = 512;
        p.smem = 4 * H_IMG + 32;                                                    // + the scheduler words
        p.sched = true;
        if (!ta && tb) p.kind = gemm_epi_kind(d, drop, atomic, 256);                // the dgrad layout carries the compile-time kinds
        if (lnm) {
            // LayerNorm-fused kinds: fold into c_attn / c_fc, statistics out of (and the rebuilt residual into) both c_proj
            const bool np_ok = np == 2 || np == 3;
            bool ok;
            if (lnm == 1 && d.out_fp32) {
                // ln_f into the tied-logits GEMM: fp32 output, the last tile column may be ragged (EPI_PLAIN32)
                ok = !ta && tb && p.swap && d.act == 0 && !d.resid && !drop && M % 256 == 0 && p.nsplit == 1 && !ex.colsum && d.bias && ex.ln.cs &&
                     np_ok && K == 256 * np;
                p.kind = EPI_PLAIN32; p.lnm = 1; p.np = np;
            } else if (lnm == 1 && ex.ln.scale) {
                // the backward pass's scale kinds: rows of 256 * np columns own the statistics, whatever N and K are
                ok = np_ok && p.nsplit == 1 && (p.kind == EPI_GELUGRAD || (p.kind == EPI_RESID && !ex.colsum));
                p.lnm = 5; p.np = np;
            } else {
                const bool in_ok = !(lnm & 1) || (np_ok && (p.kind == EPI_RESID ? (ex.ln.gamma && ex.ln.beta && N == 256 * np)
                                                                                : (ex.ln.cs && d.bias && K == 256 * np)));
                const bool kind_ok = (lnm == 1 && (p.kind == EPI_PLAIN || p.kind == EPI_GELU_AUX)) || ((lnm & 2) && p.kind == EPI_RESID);
                ok = kind_ok && in_ok && p.nsplit == 1 && !ex.colsum;
                p.lnm = lnm; p.np = lnm == 2 ? 1 : np;
            }
            GP_REQUIRE(ok, "gemm: this launch cannot carry the LayerNorm epilogue that was asked for (M=%d N=%d K=%d ta=%d tb=%d act=%d): "
                           "bf16, A[M,K] . W^T[N,K], whole 256x256 tiles, 2 or 3 segments of 256 columns", M, N, K, d.ta, d.tb, d.act);
        }
    } else if (fast) {
        p.family = CMP_GEMM_FAM_TILE128;
        p.tiles_n = gp_cdiv(N, G_BN);
        p.ntiles = p.tiles_n * gp_cdiv(M, G_BM);
        p.grid_x = p.ntiles; p.grid_y = p.nsplit;
        p.smem = 4 * G_IMG;
        // forward (transposed weight shadow) and dgrad layout: compile-time kinds on whole 128x128 tiles
        if (!ta && tb && env.fast_kinds && p.nsplit == 1) p.kind = gemm_epi_kind(d, drop, atomic, 128);
        // at most one workgroup per CU and whole k-steps: the four-stage ring (COMPOSER_GEMM_RING=0 off, =<n> from n k-steps on)
        if (p.kind != EPI_GENERIC && env.ring_min > 0 && p.ntiles <= 256 && K % G_BK == 0 && K >= gp_max(2, env.ring_min) * G_BK) {
            p.family = CMP_GEMM_FAM_RING;
            p.smem = 4 * 2 * G_IMG;
        }
        GP_NO_LN();
    } else {
        p.family = CMP_GEMM_FAM_GENERIC;
        p.tiles_n = gp_cdiv(N, G_BN);
        p.ntiles = p.tiles_n * gp_cdiv(M, G_BM);
        p.grid_x = p.tiles_n; p.grid_y = gp_cdiv(M, G_BM); p.grid_z = p.nsplit;
        p.smem = 4 * G_IMG;
        GP_NO_LN();
    }
    p.colsum_fused = ex.colsum && p.kind != EPI_GENERIC;
    p.colsum_pass = ex.colsum && !p.colsum_fused;
    return p;
#undef GP_NO_LN
}
#undef GP_REQUIRE
