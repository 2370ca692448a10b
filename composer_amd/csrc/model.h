// model.h -- shared definitions of the device-resident model state (see model.hip for the layout notes)
#pragma once
#include "common.h"
#include <rccl/rccl.h>
#include <vector>
#include <string>
#include <map>

struct DecodeState;
struct DecodeBatchState;

// what cmp_decode_grammar keeps for one decode chain until it is replaced (decode_common.h: the begin functions read it)
struct DecGrammarCfg {
    bool has_layout = false;
    cmp_event_grammar g = {};
    std::vector<uint32_t> words;       // static bans, ceil(V / 32) words; empty: none
};

// ... and cmp_decode_budget (both 0: off)
struct DecBudgetCfg {
    int64_t time_steps = 0;
    int32_t max_polyphony = 0;
};

// ... and cmp_decode_copy_guard (ids null: off).  Plain values: the dataset's pointers as they were when the guard was attached.
// epoch: bumped by every accepted cmp_decode_copy_guard call of the chain -- a captured per-token chain holds these values in its
// nodes, so a begin that finds another epoch than the one its graphs were captured under drops them
struct DecGuardCfg {
    const uint16_t* ids = nullptr;
    int64_t n = 0;
    const uint32_t* start_bits = nullptr;
    cmp_event_grammar layout = {};
    cmp_copy_guard_opts opts = {};
    int64_t epoch = 0;
    bool on() const { return ids != nullptr; }
};

struct GradClipStats { double norm; float scale; float factor; };     // elementwise.hip: grad_clip_finish_kernel

struct Metrics {
    double loss_sum;
    long long correct;
    float loss_mean;
    float acc;
    int bad_ids;        // ids outside [0, V) seen (and clamped) by the device-pointer entry points
    int pad;
};

#define NCCL_CHECK(expr)                                                                         \
    do {                                                                                         \
        ncclResult_t _r = (expr);                                                                \
        if (_r != ncclSuccess) {                                                                 \
            cmp_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, ncclGetErrorString(_r)); \
            return CMP_ERR_RCCL;                                                                 \
        }                                                                                        \
    } while (0)

#define CHECK_RC(expr)            \
    do {                          \
        int _rc = (expr);         \
        if (_rc != CMP_OK) return _rc; \
    } while (0)

struct cmp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;       // compute
    hipStream_t comm_stream = nullptr;  // RCCL
    ncclComm_t comm = nullptr;
    // cmp_dp_init_exchange: the sum over ranks is delegated to the caller (another transport; two ranks sharing one device in tests)
    int (*xfn)(void*, void*, int64_t, void*) = nullptr;
    void* xuser = nullptr;
    bool dp_on() const { return comm != nullptr || xfn != nullptr; }
    int rank = 0, nranks = 1;
    uint32_t seed_mix = 0;              // mix32(rank), xor-ed into every dropout seed: replicas draw independent masks
    int mask_rank = 0;                  // the rank seed_mix was made from (micro-step j of k accumulated ones draws mask rank r * k + j)
    int gemm_max_wgs = 0;               // cap on the persistent GEMM grids while a communicator exists (0 = all CUs)
    hipStream_t copy_stream = nullptr;  // host -> device id uploads of the pipelined train loop
    SchedWs gemm_sched;                 // item counters of the persistent GEMMs launched on `stream` (gemm.hip: sched_next)
};
void sched_ws_free(SchedWs* w);

struct ParamInfo {
    std::string name;
    int rank;
    int64_t shape[4];          // the reference's (logical) shape
    int64_t numel;             // logical element count
    int64_t offset;
    // head-size padding (cmp_model::Dl < D): 0 stored as is; 1 the last dimension is [3][H][Dl] stored as [3][H][D] (c_attn weight
    // and bias); 2 the first dimension is [H][Dl] stored as [H][D] (attention c_proj weight).  Padding entries are zero, stay zero.
    int pad = 0;
    int64_t store = 0;         // stored element count
};

struct LayerOff {   // element offsets into the flat buffers
    int64_t ln1_g, ln1_b, attn_w, attn_b, proj_w, proj_b, ln2_g, ln2_b, fc_w, fc_b, pr_w, pr_b;
    int64_t begin, end;
};

struct WDesc {      // one Conv1D weight in the flat buffers: [rows = in][cols = out]
    int64_t off;
    int rows, cols;
};

struct FoldDesc {   // one LayerNorm -> Conv1D pair of the fused block path (elementwise.hip: ln_fold_prep_kernel); offsets into the flat buffers
    int64_t w_off, b_off, g_off, be_off;   // weight [rows][cols], bias [cols], gamma [rows], beta [rows]
    int64_t out_off;                       // in the fold buffer: cs [cols], then bias' [cols]
    int rows, cols;
};

struct LayerAct {
    void *u, *qkv, *att, *r, *n, *fc, *g;
    float *ln1_mean, *ln1_rstd, *ln2_mean, *ln2_rstd, *lse;
    float *ln1_part = nullptr, *ln2_part = nullptr;    // fused block path: partial row statistics [tokens][E/256][2] of xs[i] and of r
};

struct cmp_model {
    cmp_ctx* ctx = nullptr;
    cmp_model_cfg cfg;
    int V, E, W, L, H, D, ldz;
    // Head sizes other than 16 / 32 / 64 / 128 (E / H = Dl) run on the next supported size D with zero-filled columns: the c_attn
    // output is [.., 3 * Ea], Ea = H * D, head h of q / k / v at h * D with Dl live columns; the attention kernels see (H, D) and
    // the scale 1/sqrt(Dl); zero columns of q, k, v leave every score and every output value unchanged and their gradients are
    // exactly zero.  Parameters, presents and `past` keep the reference's shapes at the ABI.  Dl == D: Ea == E, nothing changes.
    int Dl = 0, Ea = 0;
    int dtype;
    size_t es;                 // activation element size
    std::vector<ParamInfo> params;
    std::map<std::string, int> index;
    int64_t total = 0;         // elements in the flat buffers
    int64_t off_wte = 0, off_wpe = 0, off_lnf_g = 0, off_lnf_b = 0;
    std::vector<LayerOff> lo;
    float *P = nullptr, *G = nullptr, *Am = nullptr, *Av = nullptr;
    bf16_t* S = nullptr;       // bf16 shadow (bf16 mode)
    // Transposed bf16 copies of the four Conv1D weights of every block ([in,out] -> [out,in], same flat offsets), refreshed
    // at the top of every forward pass: with the weight K-contiguous the forward GEMMs run on the kernel whose both
    // operands are read with ds_read_b128 (c_attn 275 -> 209 us, c_fc 393 -> 350, c_proj 104 -> 93, mlp c_proj 298 -> 272
    // at B=128); the refresh moves 38 MB (~12 us).
    bf16_t* ST = nullptr;
    void* wdesc = nullptr;     // device table of (offset, rows, cols) for the 4L matrices
    // LayerNorm-fused block path (model.hip: ln_fused_ok): c_attn and c_fc run on the RAW residual rows and a gamma-scaled
    // transposed shadow (in ST, at the weight's own offset), with the fold vectors cs / bias' of common.h's LnEpi in `lnfold`
    // ([L] x {c_attn: cs[3E], bias'[3E]; c_fc: cs[4E], bias'[4E]}); refreshed with the transposed copies when a parameter moved.
    void* wdesc_plain = nullptr;       // the 2L matrices that stay unscaled in that mode (both c_proj)
    void* fdesc = nullptr;             // 2L FoldDesc
    void* ln_sites = nullptr;          // 2L {partials, mean, rstd} pointer triples of the blocks' LayerNorm sites (ln_stats_merge_kernel); rebuilt with the workspace
    float* lnfold = nullptr;
    int64_t fold_stride = 0;           // floats per block in lnfold; c_attn vectors at 0, c_fc vectors at 6E
    int st_state = 0;                  // what ST holds: 0 nothing, 1 plain transposes, 2 the fused path's set
    int64_t st_version = -1;           // ... of which param_version
    bool fused_last = false;           // the forward pass whose activations are held took the fused path (its backward must too)
    // ln_f folded into the tied-logits GEMM (inference passes on the fused path): the gamma-scaled copy of wte, its fold vectors
    // (cs then bias', `lnf_npad` entries each) and the partial statistics of the last block's output rows
    bf16_t* wte_lnf = nullptr;
    float* lnf_fold = nullptr;
    int lnf_npad = 0;
    float* lnf_part = nullptr;
    bool hf_valid = false;             // hf = ln_f(xs[L]) of the pass held has been written (cmp_hidden_get_at computes it on demand)
    int64_t iterations = 0;
    int64_t param_version = 0;         // bumped whenever a parameter value changes (cmp_param_set, Adam): the decode state's
                                       // transposed weight copies are refreshed when it has moved
    // workspace
    int capB = 0, capT = 0;
    std::vector<void*> allocs;
    std::vector<void*> xs;     // L+1 residual-stream tensors
    const int32_t* fwd_pos_ids = nullptr;      // cmp_forward_ex only: per-token position / token-type ids of the pass being run
    const int32_t* fwd_type_ids = nullptr;
    const float* fwd_amask = nullptr;          // ... and its additive attention mask term, float [B, past + T]
    float* const* fwd_probs_out = nullptr;     // ... and, when asked for, L host tensors [B, H, T, past + T] for the attention weights
    float* fwd_probs_dev = nullptr;            //     (one layer's worth of device staging)
    void* io_buf[3] = {nullptr, nullptr, nullptr};     // device staging of the inspection entry points (model.hip: io_scratch)
    size_t io_buf_bytes[3] = {0, 0, 0};
    std::vector<LayerAct> act;
    void *hf = nullptr, *dlogits = nullptr;
    float* logits_pack = nullptr;      // [tokens, V] contiguous copy of the logits for cmp_forward's host transfer (allocated on first use)
    float *logits = nullptr, *lnf_mean = nullptr, *lnf_rstd = nullptr, *row_loss = nullptr, *delta = nullptr;
    int32_t *row_correct = nullptr, *x_dev = nullptr, *y_dev = nullptr;
    void *dx = nullptr, *dr = nullptr, *tmpE = nullptr, *dmask = nullptr, *dfc = nullptr, *dqkv = nullptr;
    int* embed_ws = nullptr;           // workspace of the sorted embedding backward (elementwise.hip: embed_bwd_sort_ws_words)
    int64_t embed_ws_words = 0;
    void* dmask2 = nullptr;            // the attention branch's masked gradient: both masked copies of a block stay live until its grouped wgrad launch
    std::vector<WgradGroup> wgrad_groups;      // per decoder block: item table + problem descriptors of that launch
    WgradWs wgrad_ws;                          // ... and the partial-tile workspace they share (one launch at a time on the stream)
    void* ln_ws = nullptr;
    void* slab = nullptr;              // split-K slab workspace (deterministic mode only)
    int64_t slab_bytes = 0;
    Metrics* metrics = nullptr;        // device
    Metrics* metrics_host = nullptr;   // pinned
    float* dp_metrics = nullptr;       // device [4]: {loss mean, accuracy, 1, 0} summed over ranks (3-float all-reduce)
    // pipelined train loop (cmp_train_step_async): STAGES pinned id buffers + device copies, one metrics slot and two
    // events per in-flight step
    static constexpr int STAGES = 3;
    int32_t* stage_host[STAGES] = {nullptr, nullptr, nullptr};     // pinned [2][cap tokens]: x then y
    int32_t* stage_dev[STAGES] = {nullptr, nullptr, nullptr};
    Metrics* stage_metrics = nullptr;                              // pinned [STAGES]
    hipEvent_t stage_uploaded[STAGES] = {nullptr, nullptr, nullptr};
    hipEvent_t stage_done[STAGES] = {nullptr, nullptr, nullptr};
    int64_t stage_ticket[STAGES] = {-1, -1, -1};
    int64_t next_ticket = 0;
    int64_t stage_cap = 0;             // tokens per staging buffer
    // cmp_train_step_dataset: the slot's plan on the device (uploaded from stage_host) and the status the kernel writes beside x / y
    cmp_batch_row* stage_plan[STAGES] = {nullptr, nullptr, nullptr};
    int32_t* stage_status[STAGES] = {nullptr, nullptr, nullptr};
    int stage_plan_cap = 0;            // rows
    int lastB = 0, lastT = 0, last_past = 0;   // shape of the forward pass whose activations are held (cmp_present_get)
    int64_t fwd_gen = 0;               // bumped by every forward pass (train steps and decode prefill included): a Presents
                                       // object remembers the pass it came from and cmp_present_get_at refuses any other
    std::vector<hipEvent_t> bucket_ev; // L+2 events
    hipEvent_t comm_done = nullptr, metrics_ev = nullptr;
    // data-parallel telemetry (cmp_dp_stats): a ring of timed event pairs around the compute stream's wait for the
    // communication stream at the end of a step = the communication time the backward pass did NOT hide
    static constexpr int DP_RING = 32;
    hipEvent_t dp_wait_a[DP_RING] = {}, dp_wait_b[DP_RING] = {};
    bool dp_wait_used[DP_RING] = {};
    int64_t dp_steps = 0;              // steps recorded since the last reset
    int64_t dp_folded = 0;             // ... of which already summed into dp_exposed_ms
    double dp_exposed_ms = 0.0;
    int64_t dp_bytes_step = 0;         // bytes handed to ncclAllReduce by the last step (gradients + the 3-float metrics message)
    int dp_msgs_step = 0;              // all-reduce calls of the last step
    int dp_buckets_updated = 0;        // buckets of the step being enqueued whose Adam update is already on the communication stream
    bool poisoned = false;             // a data-parallel step failed after some of them: parameters partially stepped (train steps refuse)
    // train options (cmp_train_options): global-norm clipping and gradient accumulation
    float clip_norm = 0.f;             // 0 off, > 0 on, +inf measure only
    int accum_steps = 1;               // k: micro-steps per optimiser step
    int accum_pending = 0;             // micro-steps of the current group already enqueued (their gradients are summed in G)
    int accumB = 0, accumT = 0;        // ... and their shape
    double* clip_slots = nullptr;      // device: one float64 partial sum of squares per CLIP_CHUNK elements (grad_sumsq_kernel)
    int64_t clip_slots_cap = 0;
    int64_t clip_slots_used = 0;       // data-parallel step being enqueued: slots handed to the buckets so far
    GradClipStats* clip_out = nullptr;     // device: what grad_clip_finish_kernel wrote for the last clipped step
    GradClipStats* clip_host = nullptr;    // pinned [1 + STAGES]: the last step's, then one per staging slot
    bool last_has_norm = false;        // the last enqueued step computed a norm
    bool stage_has_norm[3] = {false, false, false};
    std::vector<char> reload_seen;     // while poisoned: which parameters cmp_param_set has replaced since (all of them clears the flag)
    int ln_fused_mode = -1;            // COMPOSER_LN_FUSED as read when the model was created (-1 unset, 1 the same, 0 off, 3 training passes too)
    int bias_wgrad = 10;               // COMPOSER_BIAS_WGRAD as read when the model was created: which bias gradients of a block ride on its grouped
                                       // weight-gradient launch where backward() can carry them -- bits 1 pr_b, 2 fc_b, 4 proj_b, 8 attn_b; 0: none.
                                       // Default fc_b + attn_b: their producers (GELU' dgrad epilogue, attention backward) lose 39 / 31 us per block
                                       // without the sums; the LayerNorm backward kernel loses nothing (profiles/bias_from_wgrad.txt), so pr_b /
                                       // proj_b stay with it and spare the grouped launch four of its eighteen summing tiles
    bool bias_carried_last = false;    // the last backward pass did so (cmp_model_bias_path)
    DecodeState* dec = nullptr;
    DecodeBatchState* decb = nullptr;  // batched decode (decode_batch.hip): its own buffers, KV caches and captured chains
    DecGrammarCfg gram[2];             // event grammar of the batch-1 chain [0] and of the batched chain [1] (cmp_decode_grammar)
    DecBudgetCfg budget[2];            // time budget and polyphony cap of the two chains, likewise (cmp_decode_budget)
    DecGuardCfg guard[2];              // copy guard of the two chains, likewise (cmp_decode_copy_guard)
    void* eval_buf = nullptr;          // evalpass.hip (cmp_eval_dataset): the pass's table, then its partial tables
    int gemm_role = -1;                // profiler class of the GEMMs being enqueued (0 while the forward pass is)

    // dropout seed of this replica: the model seed with the data-parallel rank folded in (rank 0: the seed itself)
    uint64_t drop_seed() const { return (uint64_t)((uint32_t)cfg.seed ^ ctx->seed_mix); }
    const void* w(int64_t off) const { return dtype == CMP_BF16 ? (const void*)(S + off) : (const void*)(P + off); }
};


template <typename Tp> static int dev_alloc(cmp_model* m, Tp** p, size_t bytes) {
    void* q = nullptr;
    HIP_CHECK(hipMalloc(&q, bytes ? bytes : 16));
    m->allocs.push_back(q);
    *p = (Tp*)q;
    return CMP_OK;
}

// the id stream of a training set in HBM (batch.hip; composer_hip.h, "device dataset")
struct cmp_dataset {
    cmp_ctx* ctx = nullptr;
    uint16_t* ids_dev = nullptr;
    int64_t n = 0;
    int max_id = 0;
    bool has_layout = false;
    cmp_event_grammar layout = {};
    uint32_t* start_bits_dev = nullptr;        // novelty.hip (cmp_dataset_set_pieces): bit p % 32 of word p / 32 = p is a piece start; null: one piece
    int64_t n_pieces = 1;
};
// novelty.hip: the refusals of the novelty options that the copy guard shares (layout and velocity ranges, n)
int nov_check(const char* who, int64_t n, const cmp_event_grammar* g, int B, int ld, const cmp_novelty_opts* o);
// copyguard.hip: the scan in front of a draw -- words_out [B][nw] = static words | copy bans, count_out [B] (accumulate: added to, not
// zeroed: the per-row counter of a chain)
int copy_guard_check(const char* who, int64_t n, const cmp_event_grammar* layout, const cmp_copy_guard_opts* o);
int copy_guard_run(hipStream_t s, const DecGuardCfg& g, const int32_t* hist, const int32_t* lens, int B, int ld, int V,
                   const uint32_t* static_words, uint32_t* words_out, unsigned long long* count_out, bool accumulate);
// batch.hip: every refusal of the contract for a HOST plan (V = 0: no model to check the ids and the layout against), and the launch
int batch_plan_check(const char* who, const cmp_dataset* ds, const cmp_batch_row* plan, int B, int W, int V);
int batch_rows_run(hipStream_t s, const cmp_dataset* ds, const cmp_batch_row* plan_dev, int B, int W, int32_t* x, int32_t* y,
                   int32_t* status);

// elementwise.hip
int embed_fwd_run(void* stream, const int32_t* ids, const float* wte, const float* wpe, void* out, int B, int T, int E, int pos0,
                  int dtype, float p_drop, uint64_t seed, uint32_t rng_stream, const int32_t* pos_ids, const int32_t* type_ids);
int embed_bwd_run(void* stream, const int32_t* ids, const void* dh, float* dwte, float* dwpe, int B, int T, int E, int pos0,
                  int dtype, float p_drop, uint64_t seed, uint32_t rng_stream, int V, float* det_ws, size_t det_ws_bytes,
                  int sort_V = 0, int* sort_ws = nullptr, int64_t sort_ws_words = 0);
int64_t embed_bwd_sort_ws_words(int64_t ntok, int V);
// G[k, j] = gamma[k] * (G[k, j] - mean_k' G[k', j]) + beta[k] * colsum[j] over one or two [rows, cols] weight gradients that were
// accumulated as (raw rows)^T . (rstd o D): turns them into LN(raw rows)^T . D (elementwise.hip: wgrad_ln_fix_kernel)
int wgrad_ln_fix_run(void* stream, float* G0, int rows0, int cols0, const float* gamma0, const float* beta0, const float* colsum0,
                     float* G1, int rows1, int cols1, const float* gamma1, const float* beta1, const float* colsum1);
int layernorm_bwd_run(void* stream, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                      const void* resid, void* dx, float* dgamma, float* dbeta, void* ws, int rows, int E, int dtype, void* dmask,
                      float* colsum, float p_drop, uint64_t seed, uint32_t rng_stream, bool deterministic, bool keep_dmask = false,
                      bool prescaled = false);     // prescaled (bf16): dy holds rstd o gradient, what a dgrad GEMM yields from an rstd-scaled A operand
int ln_stats_merge_run(void* stream, const void* sites_dev, int nsites, int np, float eps, int rows);      // sites: {part, mean, rstd} triples of pointers
int embed_fwd_stats_run(void* stream, const int32_t* ids, const float* wte, const float* wpe, void* out, float* part, int B, int T,
                        int E, int pos0, float p_drop, uint64_t seed, uint32_t rng_stream);
int ln_fold_prep_run(void* stream, const float* P, void* ST, float* fold, const void* desc_dev, int ndesc, int max_cols);
int lnf_fold_prep_run(void* stream, const float* wte, const float* gamma, const float* beta, void* out, float* cs, float* bias, int V, int E,
                      int npad);
int colsum_run(void* stream, const void* X, int ldx, float* out, int rows, int cols, int dtype, float* det_ws, size_t det_ws_bytes);
int launch_metrics_reduce(hipStream_t s, const float* row_loss, const int32_t* row_correct, int rows, void* metrics);
int launch_cast_bf16(hipStream_t s, const float* in, void* out, int64_t n);
int64_t grad_sumsq_slots(int64_t n);
int grad_sumsq_run(void* stream, const float* g, int64_t n, double* slots);
int grad_clip_finish_run(void* stream, const double* slots, int nslots, float gscale, float clip_norm, void* out);
// model.hip
int ensure_workspace(cmp_model* m, int B, int T);
int model_forward(cmp_model* m, const int32_t* x_dev, int B, int T, bool training, int64_t step, int past_len = 0);
// decode.hip, decode_batch.hip (what the two chains share: decode_common.h)
void decode_state_free(DecodeState* d);
void decode_batch_state_free(DecodeBatchState* d);
