/*
 * composer_hip.h -- C ABI of libcomposer_hip.so: the MI355X (gfx950) implementation of
 * galacticglum/composer's Transformer hot path (teacher-forced train step, evaluation step,
 * autoregressive decode).
 *
 * The reference has no FFI: its seam is the Python class `composer.models.Transformer`
 * (reference composer/models/transformer.py:599-960) called from composer/cli.py:95-141,516-680.
 * Each entry point below names the reference interface it replaces.  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success, a negative cmp_status otherwise;
 * cmp_last_error() returns a thread-local, library-owned message for the last failure.
 * Plain pointers and sizes only.  "host" pointers are ordinary CPU memory owned by the caller for
 * the duration of the call; "dev" pointers are HIP device pointers (the cmp_k_* kernel-level entry
 * points, used by the parity tests and micro-benchmarks, take dev pointers and a hipStream_t passed
 * as void*).  A cmp_ctx is bound to one device and is not thread-safe.
 */
#ifndef COMPOSER_HIP_H
#define COMPOSER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cmp_ctx cmp_ctx;
typedef struct cmp_model cmp_model;

enum cmp_status {
    CMP_OK = 0,
    CMP_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
    CMP_ERR_HIP = -2,       /* a HIP runtime call failed */
    CMP_ERR_RCCL = -3,      /* an RCCL call failed */
    CMP_ERR_STATE = -4      /* call sequence error (e.g. decode_steps before decode_begin) */
};

enum cmp_dtype {
    CMP_FP32 = 0,           /* fp32 storage + f32-input MFMA: the parity mode */
    CMP_BF16 = 1            /* bf16 activations / weight shadow, fp32 accumulate + master: throughput */
};

enum cmp_decode_mode {
    CMP_DECODE_LITERAL = 0, /* composer/cli.py:663-676 as written: `past` never fed back */
    CMP_DECODE_KV = 1       /* model(x, past=presents), transformer.py:735-765,423-426 */
};

/* Constructor arguments of Transformer.__init__ (transformer.py:610-614) plus device-side sizing. */
typedef struct cmp_model_cfg {
    int32_t vocab_size;        /* V  */
    int32_t embedding_size;    /* E, multiple of 8 */
    int32_t window_size;       /* W = rows of wpe */
    int32_t layers;            /* L  */
    int32_t heads;             /* H, E % H == 0 (transformer.py:255), head size E/H <= 128 (see cmp_model_create) */
    float   ln_eps;            /* layer_normalization_epsilon */
    int32_t scale_attention;   /* `scale` */
    int32_t use_layer_norm;    /* `use_layer_normalization` */
    float   attn_dropout;      /* attention_dropout_rate */
    float   resid_dropout;     /* residual_dropout_rate */
    int32_t dtype;             /* cmp_dtype */
    int32_t max_batch;         /* largest B of any later call */
    int32_t max_seq;           /* largest T of any later call (<= window_size) */
    uint64_t seed;             /* dropout / sampling seed */
} cmp_model_cfg;

const char* cmp_last_error(void);
int cmp_version(void);
/* key (SHA-256 over sources, headers, flags, compiler) this library was linked from: composer_amd/build.py verify() */
const char* cmp_build_key(void);
/* number of visible HIP devices (0 when none); never initialises a device context beyond the count */
int cmp_device_count(void);

/* ---- context: one per (process, device) ------------------------------------------------------ */
int cmp_ctx_create(int device, cmp_ctx** out);
int cmp_ctx_destroy(cmp_ctx* ctx);
int cmp_sync(cmp_ctx* ctx);
/* hipStream_t of the compute stream (for HIP-event timing by the caller) */
void* cmp_ctx_stream(cmp_ctx* ctx);

/* ---- data parallel: RCCL communicator, one rank per process (new; the reference is single-device) */
int cmp_dp_unique_id(void* id128);                                   /* rank 0: fills 128 bytes */
int cmp_dp_init(cmp_ctx* ctx, int rank, int nranks, const void* id128);
int cmp_dp_allreduce_test(cmp_ctx* ctx, float* host_inout, int n);    /* sum over ranks, for tests */
/* The same data-parallel step over a transport of the caller's instead of RCCL (a fabric RCCL does not drive; in tests/ two ranks
 * that share the one GPU of a box and sum over gloo -- this image's RCCL refuses two ranks on one device).  Everything else is the
 * path cmp_dp_init selects: the same gradient buckets in the same order, the bucket's event on the compute stream, Adam on the
 * bucket right behind its sum on the communication stream, 1/nranks folded into the update, seed ^ mix32(rank) dropout masks,
 * the 3-float metrics message, dynamic GEMM item scheduling.  `fn` is called on the enqueuing thread once per message, every rank
 * in the same order: it must leave the element-wise sum over all ranks of the `count` floats at `dev_f32` (device memory) in place,
 * ORDERED ON `hip_stream` (the communication stream, which already waits for the producers of the buffer; the function may
 * synchronise it), and return 0; any other value fails the step (CMP_ERR_INVALID, cmp_last_error names the message size). */
typedef int (*cmp_exchange_fn)(void* user, void* dev_f32, int64_t count, void* hip_stream);
int cmp_dp_init_exchange(cmp_ctx* ctx, int rank, int nranks, cmp_exchange_fn fn, void* user);
/* measurement aid: `wgs` workgroups that no persistent GEMM workgroup can share a CU with spin for `usec` microseconds on the
 * communication stream -- a stand-in for a concurrent RCCL kernel on a 1-GPU box (tools/ab_sched.sh) */
int cmp_dp_test_hog(cmp_ctx* ctx, int wgs, int usec);
/* While a communicator exists the persistent GEMM kernels launch at most `cus` workgroups (0 = all 256 CUs), leaving the
 * rest of the chip to the RCCL kernels of the overlapped gradient all-reduce.  Also settable with COMPOSER_DP_GEMM_CUS. */
int cmp_dp_set_gemm_cus(cmp_ctx* ctx, int cus);
/* Dropout masks are drawn from seed ^ mix32(rank) so that the replicas of a data-parallel job draw independent masks (the
 * reference is single-device).  cmp_dp_init sets the rank of the communicator; this call overrides it (tests, or a
 * launcher that shards without RCCL).  Parameter initialisation does NOT depend on it: replicas start identical. */
int cmp_dp_set_mask_rank(cmp_ctx* ctx, int rank);
/* Telemetry of the overlapped gradient exchange ("report exposed (non-overlapped) comm time per step").  Inside a
 * train step every gradient bucket is all-reduced and Adam-updated on the communication stream while the backward pass goes
 * on; at the end of the step the compute stream waits for that stream between two timed HIP events.  This call returns, over
 * the steps since the last reset: their count, the SUM of those waits in milliseconds (0 per step = everything was hidden
 * behind the backward pass), and the last step's bytes and number of ncclAllReduce calls (L+2 gradient buckets + the 3-float
 * metrics message).  All zeros without a communicator.  Synchronises with the steps it reports. */
int cmp_dp_stats(cmp_model* m, int reset, int64_t* steps, double* exposed_ms, int64_t* bytes_per_step, int* msgs_per_step);
/* ncclGetVersion of the RCCL this process is bound to (major * 10000 + minor * 100 + patch); needs no communicator. */
int cmp_dp_rccl_version(int* version);
/* The gradient exchange of one train step ALONE: the step's message pattern (3-float metrics message, then the L + 2 gradient buckets
 * in backward order, each its own range of the gradient buffer) issued back to back on the communication stream, `reps` times between
 * two HIP events after one untimed repetition; nothing runs on the compute stream.  ms = the reps' total; bytes / messages per
 * repetition.  The gradient buffer is left zeroed.  Every rank must call it with the same reps (bench.py --allreduce-only). */
int cmp_dp_allreduce_pattern(cmp_model* m, int reps, double* ms, int64_t* bytes_per_rep, int* msgs_per_rep);

/* ---- model: replaces models.Transformer(...) construction (cli.py:123-132) --------------------- */
/* Accepted configurations (anything else: CMP_ERR_INVALID with the reason in cmp_last_error): any vocabulary size; embedding_size
 * a multiple of 8, at most 2048 (LayerNorm keeps a row in registers); embedding_size divisible by heads
 * (transformer.py:255) with a head size of at most 128 -- 16 / 32 / 64 / 128 run natively, every other size runs zero-padded on
 * the next of those with the reference's shapes kept at this ABI (parameters, presents, past); at most 63 blocks; fp32 or bf16. */
int cmp_model_create(cmp_ctx* ctx, const cmp_model_cfg* cfg, cmp_model** out);
int cmp_model_destroy(cmp_model* m);

/* parameter / optimizer-state surface == checkpoint surface (transformer.py:890, models/__init__.py:75-80).
 * Names: "wte/weight" [V,E], "wpe/embeddings" [W,E], "decoder_blocks/<i>/{ln_1,ln_2}/{gamma,beta}" [E],
 * ".../attn/{c_attn,c_proj}/{weight,bias}", ".../mlp/{c_fc,c_proj}/{weight,bias}" (bias is [1,N],
 * transformer.py:190), "ln_f/{gamma,beta}".  kind: 0 value, 1 Adam m, 2 Adam v, 3 last gradient. */
int cmp_param_count(cmp_model* m, int* n);
int cmp_param_info(cmp_model* m, int i, const char** name, int* rank, int64_t shape[4], int64_t* numel);
int cmp_param_get(cmp_model* m, const char* name, int kind, float* host, int64_t numel);
int cmp_param_set(cmp_model* m, const char* name, int kind, const float* host, int64_t numel);
int cmp_adam_iter_get(cmp_model* m, int64_t* iterations);            /* Keras optimizer.iterations */
int cmp_adam_iter_set(cmp_model* m, int64_t iterations);

/* ---- training: one iteration of the loop body at transformer.py:914-930 ------------------------
 * x, y: host int32 [B,T].  Forward (training=True) + sparse-CE + backward + (DP all-reduce) + Adam.
 * Ids outside [0, V) fail the call before anything is enqueued; in a data-parallel job that is fatal for the whole job (the
 * peer ranks are already waiting in the all-reduce): validate the dataset up front, abort every rank on an error.
 * loss/acc (host, may be NULL) are the batch mean loss and accuracy -- of this rank's shard, or, once cmp_dp_init has
 * run, the mean over all ranks (one 3-float all-reduce per step; the reference logs one loss per step, :929-939). */
int cmp_train_step(cmp_model* m, const int32_t* x, const int32_t* y, int B, int T, float lr,
                   float* loss, float* acc);
/* Device-resident variant: x_dev/y_dev int32 [B,T] already in HBM; loss/acc are fetched later with
 * cmp_train_metrics (no host sync in the step itself). */
int cmp_train_step_dev(cmp_model* m, const void* x_dev, const void* y_dev, int B, int T, float lr);
int cmp_train_metrics(cmp_model* m, float* loss, float* acc);        /* syncs; last step's values */
/* Diagnostic (bench.py `default_cfg.launches`): the kernel launches (and memset / copy nodes) ONE train step of this shape enqueues,
 * counted on a stream capture of the step that is then dropped -- nothing executes, no state changes.  Single-process models only.
 * Under cmp_train_options it is the FINAL micro-step of a group that is counted / replayed (accum_steps 1: the whole step). */
int cmp_train_step_launches(cmp_model* m, const void* x_dev, const void* y_dev, int B, int T, int* kernels, int* others);
/* The same capture, instantiated and replayed `replay_reps` times back to back: milliseconds per replay (measurement only -- every
 * replay repeats the captured step's dropout masks and Adam iteration, the model is not a training run afterwards).  What a hipGraph of
 * the whole step would cost against stream launches (tools/default_config_graph_probe.py). */
int cmp_train_step_graph_probe(cmp_model* m, const void* x_dev, const void* y_dev, int B, int T, int* kernels, int* others,
                               int replay_reps, float* replay_ms);
/* Pipelined host-buffer step for the train loop (transformer.py:914-946): x/y are copied to pinned staging and uploaded on a
 * copy stream while earlier steps compute; returns at once with a ticket.  cmp_train_metrics_wait blocks until THAT step has
 * finished and returns its loss/accuracy.  At most 3 steps are in flight (a 4th submit waits for the oldest). */
int cmp_train_step_async(cmp_model* m, const int32_t* x, const int32_t* y, int B, int T, float lr, int64_t* ticket);
int cmp_train_metrics_wait(cmp_model* m, int64_t ticket, float* loss, float* acc);
/* ---- train options: global-norm gradient clipping and gradient accumulation -------------------
 * N ranks, k = accum_steps; G = the flat fp32 gradient buffer after the last micro-batch of an optimiser step and after the
 * all-reduce: the SUM over micro-batches and ranks (the tied wte gradient once, as stored; padding words zero).  gscale = 1/(k*N);
 * the gradient Adam applies is gscale * G.
 * Accumulation (k > 1): cmp_train_step / _dev / _async become micro-steps.  Calls 1 .. k-1 of a group run forward, loss and backward
 * and add into G: no gradient all-reduce, no Adam; iterations, parameters, m and v do not change.  Call k adds its gradient,
 * all-reduces the buckets, updates with gscale and increments iterations once.  Every call returns its own micro-batch's loss and
 * accuracy (the 3-float metrics all-reduce stays per call).  G is zeroed only by the first micro-step of a group.  All micro-steps of
 * a group have the shape (B, T) of the first: another shape is CMP_ERR_INVALID before anything is enqueued, the pending group is
 * kept.  Dropout: micro-step j (0-based) draws the masks cmp_dp_set_mask_rank(r * k + j) would select, r the mask rank in force; the
 * optimiser iteration is the same for the whole group (k = 1: today's masks; k micro-batches on one GPU: the masks of a k-rank job).
 * cmp_loss_and_grads never takes part in a group (it zeroes G: a pending group ends there).  After a group's final step
 * cmp_param_get(kind = 3) returns G, the SUM.  Every mode accumulates except COMPOSER_LN_FUSED=3 (refused here, by name).
 * Clipping: clip_norm 0 off, > 0 on, +inf measure only.  norm = gscale * sqrt(sum G^2), squares and sum in FLOAT64 on the device in a
 * fixed order (no float atomic, no arrival order: the same bits in G and the same bucket layout give the same double; between no
 * communicator and a 1-rank communicator the norm may differ by float64 summation order only).  scale = 1 if norm <= clip_norm, else
 * clip_norm / norm (tf.clip_by_global_norm).  Adam multiplies every gradient element by ONE fp32 number, factor = gscale * scale,
 * read from device memory, exactly where it multiplies by 1/N today: a clip that does not bind changes no bit of the update.  A
 * non-finite norm gets no special case (factor and parameters become non-finite, as in TensorFlow; the reported norm shows it).
 * With a communicator and clipping on, no bucket is updated before the last all-reduce has been enqueued: each bucket's sum of
 * squares follows its all-reduce on the communication stream, then the norm and ONE Adam launch over the whole buffer.
 * clip_norm: 0 off, > 0 on, +inf measure only; accum_steps >= 1.
 * CMP_ERR_INVALID: negative or NaN clip, accum_steps < 1, a mode that cannot accumulate.  Discards a pending partial group. */
int cmp_train_options(cmp_model* m, float clip_norm, int accum_steps);
int cmp_train_options_get(cmp_model* m, float* clip_norm, int* accum_steps, int* pending_micro_steps);
/* Last enqueued step: norm (NaN when no norm was computed: clipping off, or a non-final micro-step), scale (1 then).
 * Syncs like cmp_train_metrics. */
int cmp_train_grad_stats(cmp_model* m, float* norm, float* scale);
/* The same for the step a ticket was issued for. */
int cmp_train_metrics_wait_ex(cmp_model* m, int64_t ticket, float* loss, float* acc, float* norm, float* scale);
/* forward+backward only (no all-reduce, no Adam): gradients readable with cmp_param_get(kind=3) */
int cmp_loss_and_grads(cmp_model* m, const int32_t* x, const int32_t* y, int B, int T,
                       float* loss, float* acc);

/* ---- evaluation: model.evaluate (cli.py:613) --------------------------------------------------- */
int cmp_eval_step(cmp_model* m, const int32_t* x, const int32_t* y, int B, int T,
                  double* loss_sum, int64_t* correct, int64_t* count);

/* ---- scoring: per-event log-likelihood, rank and entropy of given sequences, reduced on the device ---------------------------
 * The contract (composer_amd.transformer.score_windows / Transformer.score restate it on the host):
 *   For a sequence s of N ids, W = window_size and 1 <= keep <= W - 1 (default W / 2), every position n in 1 .. N-1 is scored
 *   against the context s[n - c(n) : n] at positions 0 .. c(n) - 1, c the context length of cmp_decode_begin_slide below:
 *       c(n) = n                                          if n <= W
 *       c(n) = keep + ((n - W - 1) mod (W - keep + 1))    otherwise.
 *   For n <= W that is the plain causal pass; past W it is exactly the conditioning kv-slide generation draws s[n] under: scoring
 *   and generation share one definition.  Position 0 has no context and is not scored.
 *   Each scored position gets three numbers from its fp32 logits row z over the columns [0, V), at temperature 1, no filter, no
 *   grammar (the model's distribution, not the one a truncated or constrained draw was taken from), y = s[n]:
 *     logp    = z[y] - logsumexp(z), in nats;
 *     rank    = #{c : z[c] > z[y] or (z[c] == z[y] and c < y)}: 0-based, exact on the fp32 values, the order of the truncated
 *               sampler (below) and of the greedy argmax -- rank == 0 is cmp_k_softmax_xent's row_correct;
 *     entropy = logsumexp(z) - sum_c p_c z[c], p = softmax(z); a column at -inf contributes 0.
 *   A target outside [0, V) (negative values are the padding convention) marks a row as not scored: logp = 0, rank = -1, entropy
 *   as computed.
 * cmp_score: x, y host int32 [B,T]; row (b, t) is scored against x[b, 0..t] with target y[b, t] -- one window of the contract per
 * batch row, right-padded by the caller (causal attention keeps padding from touching earlier rows).  Uploads the inputs, runs the
 * inference forward pass (training = false), scores its logits with cmp_k_score_rows, synchronises once and copies back only the
 * requested host [B,T] arrays (any of the three may be null).  Ids of x outside [0, V) fail the call before anything is enqueued.
 * Read-only for everything that lasts: parameters, gradients, Adam state and iterations, a pending accumulation group, the
 * metrics of the last train step and both decode chains are what they were.  The workspace is sized as for cmp_eval_step. */
int cmp_score(cmp_model* m, const int32_t* x, const int32_t* y, int B, int T, float* logp, int32_t* rank, float* entropy);
/* The kernel alone (dev pointers): logits fp32 [rows, ldz], columns [V, ldz) are padding of any content; y int32 [rows]; outputs
 * [rows], any of them null.  One pass over the logits; writes nothing else. */
int cmp_k_score_rows(void* stream, const float* logits, int ldz, const int32_t* y, float* logp, int32_t* rank, float* entropy,
                     int rows, int V);

/* ---- inference forward: Transformer.call(inputs, training=False) (transformer.py:696-833) -------
 * logits_out: host fp32 [B,T,V]. */
int cmp_forward_logits(cmp_model* m, const int32_t* x, int B, int T, float* logits_out);
/* The general form, Transformer.call(inputs, past=presents, training=...) (transformer.py:696-833):
 *   past_len > 0: `past` points to L host tensors fp32 [2, B, H, past_len, D] (an earlier call's presents, :735-765); the T
 *   ids of x are the tokens at positions past_len .. past_len+T-1 (the reference passes the last one, :735-737), their keys
 *   and values are appended to `past` (:423-426) and logits_out is [B,T,V]; cmp_present_get then takes T' = past_len + T.
 *   training != 0: dropout active (transformer.py:916-917 calls self(x, training=True)), masks from the model's seed and
 *   optimizer iteration like a train step's; with past, the attention-probability mask of a new token is its row of the
 *   mask over all past_len + T positions. */
int cmp_forward(cmp_model* m, const int32_t* x, int B, int T, int past_len, const float* const* past, int training,
                float* logits_out);
/* ... with Transformer.call's position_ids, token_type_ids (transformer.py:770-773, 786-793: host int32 [B*T] each, or null) and
 * attention_mask (:774-779, 356-358: host int32 [B*(past_len+T)], 1 = attend, 0 = masked; or null).
 *   position_ids: the wpe row of every token (default past_len + t); token_type_ids: a second wte row added to every token's
 *   embedding; attention_mask: (1 - mask) * -1e4 is added to the scaled, causally masked scores of every query of the batch
 *   row, in every layer and head.  Forward passes only (the reference's train loop passes none of them, :916-917).
 *   attention_weights_out (Transformer(..., output_attention_weights=True), :360-369, 808-809, 827-831): null, or L host
 *   tensors fp32 [B, H, T, past_len + T] that receive every layer's attention probabilities after their dropout. */
int cmp_forward_ex(cmp_model* m, const int32_t* x, int B, int T, int past_len, const float* const* past, int training,
                   const int32_t* position_ids, const int32_t* token_type_ids, const int32_t* attention_mask,
                   float* const* attention_weights_out, float* logits_out);
/* presents[layer] of the LAST forward pass (Transformer.call's second result, transformer.py:797-806, 820-821):
 * host fp32 [2, B, H, T, D] = stack([key, value]) after split_heads.  B, T must be that pass's shape (T = past + new). */
int cmp_present_get(cmp_model* m, int layer, int B, int T, float* host_out);
/* The activations a `presents` is read from live until the NEXT forward pass of the model (any of: cmp_forward*, a train or
 * eval step, cmp_decode_begin's prefill, a slide's re-encode inside cmp_decode_steps / cmp_decode_batch_steps in the
 * sliding-window mode).  cmp_forward_generation returns the id of the pass just run; cmp_present_get_at
 * refuses (CMP_ERR_INVALID) when a later pass has replaced it -- the reference returns real tensors (transformer.py:820-821),
 * so a stale read must be an error, never another pass's keys/values. */
int cmp_forward_generation(cmp_model* m, int64_t* generation);
int cmp_present_get_at(cmp_model* m, int layer, int B, int T, int64_t generation, float* host_out);
/* all_hidden_states[index] of the forward pass `generation` (Transformer(..., output_hidden_states=True), transformer.py:610-614,
 * 800-816, 824-825): host fp32 [B, T, E] -- the input of decoder block `index` for index < L (index 0 = token + position
 * embedding after the embedding dropout), the ln_f output for index = L.  T = the pass's NEW positions (1 with `past`). */
int cmp_hidden_get_at(cmp_model* m, int index, int B, int T, int64_t generation, float* host_out);

/* ---- decode: the loop of cli.py:659-676 -------------------------------------------------------
 * temperature <= 0 => argmax with lowest-index tie-break (the tau->0 limit; cli.py:671 divides). */
int cmp_decode_begin(cmp_model* m, const int32_t* prompt, int P, int mode, float temperature, uint64_t seed);
int cmp_decode_steps(cmp_model* m, int n, int32_t* ids_out);
/* The logits the most recent per-token step drew its id from: host fp32 [V], copied after a stream synchronise; read-only, not
 * part of the per-token chain.  A steps(n) call leaves the last step's logits, so step one id at a time between reads.
 * CMP_ERR_STATE before begin and before the first per-token step (the first id is drawn from the prefill's logits, which
 * cmp_forward_logits shows). */
int cmp_decode_logits_get(cmp_model* m, float* host_out);
/* Sliding-window decode: kv mode that goes on past window_size.  W = window_size, 1 <= keep <= W - 1 (else CMP_ERR_INVALID).
 * With s = prompt ++ ids so far and n = len(s), the next id is drawn from the last position of a plain forward pass over
 * s[n - c(n) : n] at positions 0 .. c(n) - 1,
 *     c(n) = n                                          if n <= W
 *     c(n) = keep + ((n - W - 1) mod (W - keep + 1))    otherwise:
 * the context grows to W; the next draw re-encodes the last `keep` tokens (the newest included) from position 0 -- the position
 * table is absolute, cached keys cannot be shifted -- and draws from that pass's last row as cmp_decode_begin draws its first id
 * from the prompt; then the context grows again.  The i-th id uses draw counter i, slides or not.  While n <= W the mode is
 * CMP_DECODE_KV itself (same kernels, same bits).  cmp_decode_steps enqueues slides like steps (one synchronise at its end);
 * cmp_decode_logits_get shows the logits the latest id was drawn from, slide steps included.  The re-encode runs through the
 * model's workspace, which never grows: begin sizes it for max(P, keep) tokens, or refuses before any id is produced when an
 * earlier call sized it smaller (create the model with max_batch / max_seq covering it). */
int cmp_decode_begin_slide(cmp_model* m, const int32_t* prompt, int P, int keep, float temperature, uint64_t seed);
/* Since the chain's last begin (batched != 0: the batched chain's): rows re-encoded by slides, and forward passes run for them
 * (the batched chain packs the rows that slide at the same step into as few passes as the workspace allows). */
int cmp_decode_slide_stats(cmp_model* m, int batched, int64_t* row_slides, int64_t* forward_calls);
/* The sampler of the decode chain on its own (dev pointers): n independent draws from ONE logits row [V] with draw counters
 * counter0 .. counter0+n-1 -> ids_out[n].  tf.random.categorical(logits / temperature), cli.py:671-673. */
int cmp_k_sample(void* stream, const float* logits, int V, float temperature, uint64_t seed, uint32_t counter0, int n,
                 int32_t* ids_out);

/* ---- truncated sampling: top-k and nucleus (top-p), drawn on the device inside the per-token chain ------------------------
 * The contract, for one row of fp32 logits z[0..V), fp32 temperature, int top_k, fp32 top_p
 * (composer_amd.transformer.sampling_keep_set restates it on the host in numpy):
 *   1. Order: columns are ranked by (z descending, index ascending) -- exact on the fp32 values (-0 == +0), ties at a boundary
 *      go to the lower index, the rule of the greedy argmax.
 *   2. top_k = 0 or top_k >= V: off.  Otherwise the candidates are the first top_k columns of the order.
 *   3. top_p = 1: off.  Otherwise, with q_c = exp((z_c - z_max) / temperature) over the candidates of step 2, the kept set is the
 *      shortest prefix of the order whose mass reaches top_p: the smallest n >= 1 with sum(q[:n]) >= top_p * sum(q).  The
 *      masses are FLOAT64 on the device (logits, temperature and top_p widened to double; a fixed summation order), so against
 *      a float64 host restatement the cumulative masses differ by summation order only (~1e-13 relative).
 *   4. The id is the plain sampler's Gumbel-max restricted to the kept set: the same per-column hash of (seed, draw counter,
 *      column) and the same fp32 arithmetic, so it equals, bit for bit, cmp_k_sample on a copy of the row with every dropped
 *      column set to -inf (same seed and counter), and is one draw from softmax(z / temperature) renormalised over the kept set.
 *   5. temperature <= 0 stays the greedy argmax: the filters are accepted and change nothing.
 *   6. CMP_ERR_INVALID before any device work: top_k < 0, top_p outside (0, 1] or NaN.  The truncating sampler ranks the row in
 *      LDS and takes V <= 4096; a wider vocabulary is refused, naming the limit, only when a filter is on.
 *   7. Both filters off is the plain sampler itself: every id of every entry point without `_ex` is what it was, bit for bit,
 *      and those entry points mean "filters off".
 * The filters live in the device-side decode state beside the temperature: changing them re-captures nothing.
 * cmp_k_sample with the filters: */
int cmp_k_sample_ex(void* stream, const float* logits, int V, float temperature, int top_k, float top_p, uint64_t seed,
                    uint32_t counter0, int n, int32_t* ids_out);
/* cmp_decode_begin (keep = 0) and cmp_decode_begin_slide (keep >= 1, mode CMP_DECODE_KV) with the filters; cmp_decode_steps and
 * cmp_decode_logits_get as before. */
int cmp_decode_begin_ex(cmp_model* m, const int32_t* prompt, int P, int mode, int keep, float temperature, int top_k, float top_p,
                        uint64_t seed);

/* ---- event-grammar decoding: on-device note / pedal state masks the sampler -------------------------------------------------
 * The vocabulary is a grammar: NoteSequence.from_events (the reference's EventSequence.to_note_sequence) silently drops a NOTE_OFF
 * of a silent pitch, a NOTE_ON of a sounding one, a SUSTAIN_ON while the pedal is down and a SUSTAIN_OFF while it is up.  With a
 * grammar configured, both decode chains draw only events that mean something in the row's current state.  The contract
 * (composer_amd.grammar.EventGrammar restates it on the host):
 *   Layout: given by the caller, never hard-coded.  note_on0 / note_off0: the first of 128 consecutive ids each, id - base = the
 *     pitch; time_shift0 / time_shift_n: the TIME_SHIFT ids; sustain_on / sustain_off: single ids, or -1 for BOTH when the
 *     vocabulary has none.  (composer_amd.dataset.event_ranges; the default dataset config: 0 / 128 / 288, 100 / 388 / 389, V = 390.)
 *   State: of a sequence s = prompt ++ ids so far, a 128-bit sounding set and a pedal bit: the left fold over s of from_events'
 *     transition -- NOTE_ON p sets bit p if clear, else is ignored; NOTE_OFF p clears bit p if set, else is ignored; SUSTAIN_ON /
 *     SUSTAIN_OFF set / clear the pedal likewise; every other id leaves the state alone.  The prompt is folded the same way (its
 *     ignored events are allowed and change nothing).  The state is a function of the whole sequence: a kv-slide re-encode does
 *     not reset it, and the literal mode carries it too.
 *   Rules: a bit mask selects what is banned in the current state -- CMP_GRAMMAR_NOTE_OFF_SOUNDING: NOTE_OFF p while p is silent;
 *     CMP_GRAMMAR_NOTE_ON_SILENT: NOTE_ON p while p sounds; CMP_GRAMMAR_PEDAL: SUSTAIN_ON while the pedal is down, SUSTAIN_OFF while
 *     it is up.
 *   Static bans: an optional bit vector of ceil(V / 32) words (bit c % 32 of word c / 32 set: column c is never drawn), shared by
 *     all rows of the chain and ORed with the dynamic bans.
 *   The draw: with the ban set N of that step, the id equals, bit for bit, cmp_k_sample_ex on a copy of the logits row with the
 *     columns of N at -inf (same temperature, top_k, top_p, seed and draw counter).  So the bans apply before the ranking: top_k
 *     counts allowed columns first, a banned column carries mass 0 in top_p, and the greedy draw (temperature <= 0) is the argmax
 *     over the allowed columns, lowest index on ties -- unlike the filters, the grammar is NOT a no-op for greedy.
 *   Always a drawable column: no dynamic rule ever bans a TIME_SHIFT; with a layout, a static vector must leave at least one
 *     TIME_SHIFT id clear; without one, at least one id.
 *   Off: rules 0 and no static bit set is today's sampler itself (the kernels that draw branch, uniformly, to the banning
 *     samplers only when a rule or a static bit is active): every id of every entry point is what it was, bit for bit.
 *   Refusals (CMP_ERR_INVALID before any device work, the reason in cmp_last_error): a range outside [0, V); overlapping ranges;
 *     one sustain id without the other; time_shift_n < 1; unknown rule bits; a static vector that bans every id it must not.
 *   No vocabulary limit of its own: the predicate is evaluated per column from a few uniform words at any V (the 4096-column limit
 *     of the truncating sampler keeps applying only when a filter is on). */
#define CMP_GRAMMAR_NOTE_OFF_SOUNDING 1
#define CMP_GRAMMAR_NOTE_ON_SILENT 2
#define CMP_GRAMMAR_PEDAL 4
#define CMP_GRAMMAR_ALL 7
typedef struct cmp_event_grammar {
    int32_t note_on0;
    int32_t note_off0;
    int32_t time_shift0;
    int32_t time_shift_n;
    int32_t sustain_on;
    int32_t sustain_off;
    int32_t rules;             /* CMP_GRAMMAR_* bits */
} cmp_event_grammar;
/* Configures the batch-1 chain (batched = 0) or the batched chain (batched != 0).  Validated against the model's V here; takes
 * effect at that chain's next begin call (any of them: the begin argument lists do not grow) and stays until replaced.  g: the
 * layout and the rules, or null (no layout: no dynamic rule, the state stays empty); banned_words: HOST array of ceil(V / 32)
 * words (bits at or above V are ignored), or null.  Both null: off.  The configuration lives in the device-side decode state and
 * in a device buffer of fixed address: changing it re-captures nothing. */
int cmp_decode_grammar(cmp_model* m, int batched, const cmp_event_grammar* g, const uint32_t* banned_words);
/* The state of row `row` of the chain (batch-1: row 0) after its latest id; synchronises.  sounding: bit p % 32 of word p / 32 =
 * pitch p sounds; time_steps: the sum over all TIME_SHIFT events of s, id time_shift0 + j counting j + 1 (what a duration-based
 * stop would read).  All zero while the chain has no layout.  CMP_ERR_STATE before begin, CMP_ERR_INVALID for a bad row. */
int cmp_decode_grammar_state(cmp_model* m, int batched, int row, uint32_t sounding[4], int32_t* pedal, int64_t* time_steps);
/* The sampler alone with a DEVICE bit vector of ceil(V / 32) words (the kernel-level test of the draw): cmp_k_sample_ex reading
 * every banned column as -inf. */
int cmp_k_sample_banned(void* stream, const float* logits, int V, float temperature, int top_k, float top_p,
                        const uint32_t* banned_dev, uint64_t seed, uint32_t counter0, int n, int32_t* ids_out);

/* ---- timed generation: a time budget and a polyphony cap in the sampler ------------------------------------------------------
 * The vocabulary has no end-of-piece event, so a decode that stops after a number of ids stops wherever that id falls: the length
 * in seconds is an accident of the draws, and NoteSequence.from_events drops every note (and the pedal period) still open at the
 * end.  With a budget configured, both decode chains draw a generated part that lasts exactly `time_steps` steps, then release
 * what sounds, and never stack more than `max_polyphony` pitches.  Enforced per draw on the device, like the grammar; the
 * contract (composer_amd.grammar.TimedRules restates it on the host):
 *   Configuration: per chain, read by that chain's next begin call (any of them), as cmp_decode_grammar is.  time_steps >= 0 in
 *     the units of cmp_decode_grammar_state's time_steps (id time_shift0 + j counts j + 1), 0: no time budget; max_polyphony >= 0,
 *     0: no cap; both 0: off.  At begin every row gets t_end = time_steps(its prompt) + time_steps (0 without a time budget): the
 *     budget covers the generated part, the prompt's own duration is not charged to it.
 *   Phases, a pure function of the row's state: PLAY: t_end == 0 or time_steps < t_end.  ENDING: time_steps == t_end and a pitch
 *     sounds or the pedal is down.  DONE: time_steps == t_end, nothing sounds, the pedal is up.
 *   Ban set of a draw.  PLAY: the grammar's (rules and static vector), plus TIME_SHIFT j while time_steps + j + 1 > t_end -- time
 *     never passes t_end and can always reach it -- plus, with a cap, every NOTE_ON while popcount(sounding) >= max_polyphony.
 *     ENDING: everything but NOTE_OFF p of a sounding p, and SUSTAIN_OFF while the pedal is down; the static vector and the rule
 *     bits are ignored here (the ending must always be able to finish), the model still chooses the order of the releases.
 *     DONE: everything but time_shift0.  That id is a filler: it does not move the grammar state (time_steps stays at t_end);
 *     the produced count, the draw counter and the position go on as for any id, so the chain is otherwise unchanged.
 *   The draw is the grammar's: the id equals, bit for bit, cmp_k_sample_ex on a copy of the logits row with the ban set's columns
 *     at -inf (same temperature, top_k, top_p, seed and draw counter), before the ranking and for greedy too.
 *   done_at, per row on the device: -1 until the state first becomes DONE, then the number of ids the row had produced at that
 *     moment.  Ids from done_at on are filler and not part of the result.
 *   The state is a function of the whole sequence: a kv-slide re-encode does not reset it, the literal mode carries it too, and a
 *     held row of the batched chain stays untouched by the replay.  A row's ids depend on its own prompt, seed, parameters and the
 *     chain's budget only.
 *   Off (both 0) is the code path without this section: every id of every entry point is what it was, bit for bit.
 *   Refusals (CMP_ERR_INVALID before any device work, the reason in cmp_last_error): a negative value, at the call; at a begin
 *     call, a budget on a chain without a grammar layout (which ids are TIME_SHIFT, NOTE_ON, NOTE_OFF and pedal events is the
 *     layout's to say; rules = 0 is enough) and a time budget whose static vector bans time_shift0 (a row one step short of t_end
 *     could never land on it).  A refused call leaves the configuration and a decode in progress as they were. */
#define CMP_BUDGET_PLAY 0
#define CMP_BUDGET_ENDING 1
#define CMP_BUDGET_DONE 2
int cmp_decode_budget(cmp_model* m, int batched, int64_t time_steps, int32_t max_polyphony);
/* Row `row` of the chain (batch-1: row 0) after its latest id; synchronises, like cmp_decode_grammar_state.  steps_left:
 * t_end - time_steps; phase: CMP_BUDGET_*.  Without a budget: steps_left 0, phase PLAY, done_at -1.  CMP_ERR_STATE before begin,
 * CMP_ERR_INVALID for a bad row. */
int cmp_decode_budget_state(cmp_model* m, int batched, int row, int64_t* steps_left, int32_t* phase, int32_t* done_at);

/* ---- batched decode: B independent sequences per step (1 <= B <= 256), state apart from cmp_decode_begin's ----------------
 * prompts: host int32 [B][ld], row b holds lens[b] ids (1 <= lens[b] <= window_size).  Row b samples with seed (uint32)(seed + b);
 * its i-th generated id uses draw counter i, as cmp_decode_begin does, so its first id equals cmp_decode_begin's on that prompt
 * with seed + b.  A row's ids depend on (weights, its prompt, seed + b, mode, temperature) only, never on B or the other rows.
 * Steps before begin: CMP_ERR_STATE.  kv mode: a call that would take a row past window_size is refused, naming the row,
 * before any step runs. */
int cmp_decode_batch_begin(cmp_model* m, const int32_t* prompts, const int32_t* lens, int B, int ld, int mode,
                           float temperature, uint64_t seed);
/* cmp_decode_begin_slide for B rows: every row slides on its own length (rows that reach the window at the same step are
 * re-encoded together); a row's ids and logits depend on (weights, its prompt, seed + b, temperature, keep) only. */
int cmp_decode_batch_begin_slide(cmp_model* m, const int32_t* prompts, const int32_t* lens, int B, int ld, int keep,
                                 float temperature, uint64_t seed);
int cmp_decode_batch_steps(cmp_model* m, int n, int32_t* ids_out);      /* host int32 [B][n], row-major */
/* cmp_decode_logits_get for the batched chain: host fp32 [B][V], row b = the logits row b's latest id was drawn from. */
int cmp_decode_batch_logits_get(cmp_model* m, float* host_out);
/* The batched sampler on its own (dev pointers): row b of logits [B][ldz] -> ids_out[b], seed + b, draw counter `counter`. */
int cmp_k_sample_rows(void* stream, const float* logits, int ldz, int B, int V, float temperature, uint64_t seed,
                      uint32_t counter, int32_t* ids_out);
/* Truncated sampling (the contract above) in the batched chain, PER ROW: temperature / top_k / top_p are HOST arrays of B entries;
 * a null array is the default for every row (temperature 1, top_k 0, top_p 1).  keep = 0: cmp_decode_batch_begin; keep >= 1
 * (mode CMP_DECODE_KV): cmp_decode_batch_begin_slide.  Row b's ids depend on (weights, its prompt, seed + b, mode, keep, and its
 * own temperature, top_k, top_p) only -- never on B, the graph switch or another row's parameters. */
int cmp_decode_batch_begin_ex(cmp_model* m, const int32_t* prompts, const int32_t* lens, int B, int ld, int mode, int keep,
                              const float* temperature, const int32_t* top_k, const float* top_p, uint64_t seed);
/* cmp_k_sample_rows with the rows' own parameters (host arrays as above, B <= 256); row b equals cmp_k_sample_ex on that row
 * with seed + b. */
int cmp_k_sample_rows_ex(void* stream, const float* logits, int ldz, int B, int V, const float* temperature, const int32_t* top_k,
                         const float* top_p, uint64_t seed, uint32_t counter, int32_t* ids_out);

/* ---- device dataset: train-time augmentation (transpose, time stretch, random crop) in front of the train step --------------
 * The reference augments offline (composer/dataset/preprocess.py:84-100 writes transposed and stretched copies of every piece).
 * Here the id stream of the training set lives in HBM as uint16 and one kernel cuts, transposes and re-times the rows of a batch
 * straight into the buffers the train step reads; the host sends 16 bytes per row.  Integers only: every result is bitwise what
 * the host restatement composer_amd.augment computes, and no tolerance appears anywhere.  The contract:
 *   Layout: given by the caller, never hard-coded -- the cmp_event_grammar fields note_on0, note_off0 (128 consecutive ids each,
 *     id - base = the pitch), time_shift0 and time_shift_n = M (id time_shift0 + j counts j + 1 steps); the other fields are checked
 *     as a grammar's and not used.
 *   Row plan: (offset, transpose k, stretch f), f in 1/1024ths, 512 <= f <= 1536; f = 1024 is the identity.  |k| <= 127.
 *   Source span: src = ids[offset : offset + S], S = min(2 (W + 1), n - offset); 0 <= offset <= n - (W + 1).
 *   Transpose: a NOTE_ON / NOTE_OFF id of pitch p becomes pitch clip(p + k, 0, 127) (the reference's rule, sequence.py:379, per
 *     token); every other id is untouched.
 *   Stretch: R(t) = (t f + 512) >> 10 on 64-bit integers.  Walking src with the running unstretched time t, every maximal run of
 *     consecutive TIME_SHIFT ids, r steps in all, is replaced by d = R(t + r) - R(t) steps, emitted as d / M ids of M steps and
 *     then one id of d % M steps if that is not zero (notes.py:116-120); a run with d = 0 vanishes; then t += r.  The rounding is
 *     cumulative: the emitted steps of a span sum to R(its total), nothing drifts.  A run cut by either end of the span is the
 *     part inside it.
 *   Output: out = the first W + 1 emitted ids; x = out[:W], y = out[1:].
 *   Identity: f = 1024 does not walk at all: out = src[:W + 1], transposed (re-chunking would merge a non-canonical run such as
 *     30 + 50 steps into one id of 80).
 *   Fallback: a span that emits fewer than W + 1 ids gives the f = 1024 row, still transposed, with CMP_BATCH_FALLBACK set.
 *   Status, int32 [B, 2]: (emitted ids clipped to W + 1 -- W + 1 for an identity row --, flag bits).
 * Refusals (CMP_ERR_INVALID before any device work, the reason in cmp_last_error): an offset outside [0, n - (W + 1)]; f outside
 *   [512, 1536]; |k| > 127; a plan that is not all identity on a dataset without a layout; W > 2^20; with a model, a dataset
 *   whose largest id is >= V or whose layout is not a grammar layout inside [0, V) (the rules of cmp_decode_grammar). */
#define CMP_BATCH_FALLBACK 1
#define CMP_BATCH_REFUSED 2        /* cmp_k_batch_rows only: a row of the DEVICE plan the host entry points refuse; nothing read, x / y not written */
typedef struct cmp_dataset cmp_dataset;
typedef struct cmp_batch_row { int64_t offset; int32_t transpose; int32_t stretch_q10; } cmp_batch_row;
/* Uploads the n ids once (host uint16) and records the largest.  layout: null only if every later plan is the identity. */
int cmp_dataset_create(cmp_ctx* ctx, const uint16_t* ids, int64_t n, const cmp_event_grammar* layout, cmp_dataset** out);
int cmp_dataset_destroy(cmp_dataset* ds);
/* The kernel alone (dev pointers): ids_dev uint16 [n], plan_dev [B], x / y int32 [B, W], status int32 [B, 2]; layout (host) may be
 * null for identity plans.  Reads ids_dev[offset : offset + S] of every row and nothing else of the stream. */
int cmp_k_batch_rows(void* stream, const uint16_t* ids_dev, int64_t n, const cmp_event_grammar* layout, const cmp_batch_row* plan_dev,
                     int B, int W, int32_t* x, int32_t* y, int32_t* status);
/* Builds a batch from a HOST plan and reads it back (host int32 [B, W] twice, [B, 2]; status_host may be null): tests, debugging. */
int cmp_dataset_batch(cmp_dataset* ds, const cmp_batch_row* plan, int B, int W, int32_t* x_host, int32_t* y_host, int32_t* status_host);
/* cmp_train_step_async fed by a plan: the same step, the same kind of ticket (cmp_train_metrics_wait[_ex], train options and data
 * parallelism unchanged).  The plan travels through the pinned stage of the ticket's slot -- B * 16 bytes in place of B * T * 8 --,
 * the kernel writes x and y into that slot's device stage on the compute stream and the step reads them there.  ds and m must
 * share a context. */
int cmp_train_step_dataset(cmp_model* m, cmp_dataset* ds, const cmp_batch_row* plan, int B, int T, float lr, int64_t* ticket);

/* ---- novelty check: the longest training-set match of every event of a sample ------------------------------------------------
 * Is a sample new, or a passage of the training set played back?  A high cmp_score cannot tell: a memorised passage scores best.
 * For every event of a query this section finds the longest run that occurs verbatim in the id stream of a cmp_dataset, optionally
 * transposed (the reference's preprocess and the train-time augmentation both put transposed copies in front of the model).
 * Integers only: every result is bitwise what the host restatement composer_amd.novelty.match_table computes, and no tolerance
 * appears anywhere.  The contract:
 *   Corpus: c[0..n), the uint16 id stream; n < 2^40.  Piece starts: a sorted (non-decreasing) list of offsets in [0, n), one per
 *     file, the first of them 0; a dataset without a list is one piece.  A match never continues across a start.
 *   Queries: B ragged rows x[b][0..lens[b]), int32 [B][ld]; 1 <= B <= 256, 1 <= lens[b] <= ld <= 32768, every id in [0, 65535).
 *   Options: min_match >= 1; transpose N, 0 <= N <= 24; velocity0 / velocity_n: the VELOCITY id range folded into one class
 *     (velocity_n = 0: velocities must match exactly; passed explicitly because cmp_event_grammar does not name the range).  The
 *     layout (note_on0, note_off0: 128 consecutive ids each, id - base = the pitch) is required as soon as N > 0.
 *   Token equality under a transposition k in [-N, N]: a NOTE_ON / NOTE_OFF of pitch p in the QUERY stands for pitch p + k if
 *     0 <= p + k <= 127 and otherwise equals nothing -- never clipped: the augmentation's clip rule merges pitches and would invent
 *     matches.  With velocity folding every id of the range equals every other, in query and corpus alike.  Every other id equals
 *     itself.  Corpus tokens are never transposed.
 *   Match length: m(s, p, k) = 0 if x[s] under k differs from c[p], else 1 + m(s + 1, p + 1, k), where the continuation counts as 0
 *     when s + 1 == len, when p + 1 == n, or when p + 1 is a piece start.
 *   Result per query position s: (len, pos, k) = the maximum of m(s, p, k) over all p and k under the total order: larger m; then
 *     smaller |k|; then negative k before positive k; then smaller p.  A maximum below min_match gives (0, -1, 0), and so does every
 *     position s >= lens[b] of a padded row.  The order is total, so the result does not depend on the order in which workgroups
 *     finish: the device takes an atomic maximum of the 64-bit key (len << 48 | (255 - rank(k)) << 40 | (2^40 - 1 - p)), rank
 *     0, -1, +1, -2, +2 ... -> 0, 1, 2, 3, 4 ...
 *   Refusals (CMP_ERR_INVALID before any device work, the reason in cmp_last_error): B, ld, lens, min_match or N outside the ranges
 *     above; a query id outside [0, 65535); N > 0 without a layout; a velocity range outside [0, 65536) or overlapping the note
 *     ranges; note ranges outside [0, 65536) or overlapping each other; starts that are unsorted, outside [0, n) or do not begin
 *     with 0; n >= 2^40.
 *   Known limit: a time-stretched copy re-chunks its TIME_SHIFT runs and is not found. */
typedef struct cmp_novelty_opts {
    int32_t min_match;
    int32_t transpose;         /* N: every k in [-N, N] is tried */
    int32_t velocity0;
    int32_t velocity_n;        /* 0: no folding */
} cmp_novelty_opts;
/* Records the piece starts of the dataset's stream (HOST array of n_pieces offsets) as a device bit vector of ceil(n / 32) words, bit
 * p % 32 of word p / 32 set: p is a start.  Replaces an earlier list; cmp_dataset_destroy frees it. */
int cmp_dataset_set_pieces(cmp_dataset* ds, const int64_t* starts, int n_pieces);
/* HOST arrays: x int32 [B][ld], lens [B]; len_out / k_out int32 [B][ld], pos_out int64 [B][ld].  The layout is the dataset's.
 * Synchronises. */
int cmp_novelty(cmp_dataset* ds, const int32_t* x, const int32_t* lens, int B, int ld, const cmp_novelty_opts* opts, int32_t* len_out,
                int64_t* pos_out, int32_t* k_out);
/* The kernels alone (dev pointers; layout and opts on the host): ids_dev uint16 [n], n >= 1; start_bits_dev ceil(n / 32) words or
 * null (one piece).  Writes every element of the three outputs.  No workspace is allocated: pos_out holds the packed keys
 * between the matching kernel and the small kernel that unpacks them in place.  The host cannot see lens_dev and x_dev: a length is
 * clamped to [0, ld] and a query id outside [0, 65535) equals nothing.  Reads ids_dev[0 .. n), the start bits of those positions,
 * x_dev[b][0 .. lens[b]) and lens_dev[0 .. B), and nothing else. */
int cmp_k_novelty(void* stream, const uint16_t* ids_dev, int64_t n, const uint32_t* start_bits_dev, const cmp_event_grammar* layout,
                  const int32_t* x_dev, const int32_t* lens_dev, int B, int ld, const cmp_novelty_opts* opts, int32_t* len_out,
                  int64_t* pos_out, int32_t* k_out);

/* ---- copy guard: decode never extends a training-set match past max_copy ----------------------------------------------------
 * The novelty check diagnoses a copy; this section prevents one.  With a guard attached, at every draw of a decode chain the id
 * that would complete a verbatim run of more than max_copy events somewhere in the corpus cannot be drawn: n-gram blocking
 * against the training set, decided exactly (the corpus itself is scanned at every step: no Bloom filter, no false positive),
 * inside the per-token chain, with no host round trip.  Integers only: the ban set is bitwise what the host restatement
 * composer_amd.novelty.copy_bans computes.  The contract:
 *   Configuration, per chain: a cmp_dataset with its stream c[0..n), n < 2^40, and its piece starts (none: one piece); the dataset
 *     must have a layout (the rule has to know the TIME_SHIFT and the note ids).  max_copy M, 1 <= M <= 64; transpose N,
 *     0 <= N <= 24; velocity0 / velocity_n as in cmp_novelty_opts (velocity_n = 0: no folding).
 *   Token equality under a transposition k is cmp_novelty's, word for word: a history NOTE_ON / NOTE_OFF of pitch p stands for
 *     p + k if that stays in 0..127 and otherwise equals nothing (never clipped); folded velocities all equal each other; every other
 *     id equals itself; an id outside [0, 65535) equals nothing.  Corpus tokens are never transposed.
 *   History of a row: h = prompt ++ ids so far, t = len(h).  The prompt counts: a prompt taken from a training piece must not simply
 *     be continued.  The history is a function of the whole sequence: a kv-slide re-encode does not shorten it, the literal mode
 *     carries it, and a held row of the batched chain is left alone.
 *   Copy bans of a draw: column v is banned iff v is not a TIME_SHIFT id, t >= M, and there are a corpus position p, M <= p < n, and
 *     a k in [-N, N] such that h[t - M + j] under k equals c[p - M + j] for j = 0 .. M - 1, v under k equals c[p], and none of
 *     p - M + 1 .. p is a piece start (p - M may be one).  So with c[p] a note of pitch q the banned column is the note of pitch q - k
 *     when that is in 0..127; with c[p] in a folded velocity range the whole range is banned; otherwise it is c[p] itself.
 *   TIME_SHIFT is exempt because the grammar section promises that no dynamic rule ever bans a TIME_SHIFT, and the time budget
 *     relies on that to reach t_end.
 *   Consequence: in prompt ++ ids, every DRAWN event that is the (M + 1)-th or a later event of a match (cmp_novelty's, same N and
 *     folding) is a TIME_SHIFT; with a prompt of at most M events, every match of more than M events consists of TIME_SHIFT events
 *     only from its (M + 1)-th event on.  (A prompt that is itself a passage of the corpus stays the match it is.)
 *   Composition: the copy bans are ORed with the chain's static vector and, in PLAY, with the grammar's and the budget's bans.  In
 *     ENDING and DONE they are ignored exactly as the static vector is: the ending must always be able to finish.  The draw equals,
 *     bit for bit, cmp_k_sample_ex on the logits row with the whole ban set at -inf (same temperature, top_k, top_p, seed and draw
 *     counter).  The samplers are the grammar's: a guarded row reads its own ban words, which the scan fills in front of every draw
 *     (the first draw after the prefill, the draws of a slide and the literal mode included).
 *   Counter, per row on the device: banned_columns = the sum over the row's draws in PLAY of the number of columns the copy rule
 *     banned that the static vector had not.
 *   Off (no guard attached) is the code path without this section: every id of every entry point is what it was, bit for bit, and
 *     the captured per-token chain has the nodes it had.  Attaching or detaching invalidates that chain's captured graphs: the next
 *     begin captures the chain with or without the scan.
 *   Refusals (CMP_ERR_INVALID before any device work, the reason in cmp_last_error): M or N out of range; a dataset without a
 *     layout; a velocity range outside [0, 65536) or overlapping the note ranges (cmp_novelty's checks); a dataset on another device
 *     than the model's.  A refused call leaves the configuration and a decode in progress as they were. */
typedef struct cmp_copy_guard_opts {
    int32_t max_copy;          /* M */
    int32_t transpose;         /* N: every k in [-N, N] counts */
    int32_t velocity0;
    int32_t velocity_n;        /* 0: no folding */
} cmp_copy_guard_opts;
/* Configures the batch-1 chain (batched = 0) or the batched chain (batched != 0); takes effect at that chain's next begin call (any of
 * them) and stays until replaced.  ds null: off (opts is not read).  The caller keeps ds alive, with its piece starts unchanged,
 * while it is attached and while a decode begun under it goes on. */
int cmp_decode_copy_guard(cmp_model* m, int batched, cmp_dataset* ds, const cmp_copy_guard_opts* opts);
/* Row `row` of the chain (batch-1: row 0) after its latest id; synchronises.  0 on a chain begun without a guard.  CMP_ERR_STATE
 * before begin, CMP_ERR_INVALID for a bad row. */
int cmp_decode_copy_guard_state(cmp_model* m, int batched, int row, int64_t* banned_columns);
/* The scan alone (dev pointers; layout and opts on the host): ids_dev uint16 [n], n >= 1; start_bits_dev ceil(n / 32) words or null
 * (one piece); hist_dev int32 [B][ld], row b holds lens_dev[b] ids (clamped to [0, ld]; its last M are the window; an id outside
 * [0, 65535) equals nothing); 1 <= B <= 256, ld >= 1; static_words_dev ceil(V / 32) words shared by all rows, or null (none);
 * words_out uint32 [B][ceil(V / 32)] = the static words OR the copy bans of the row (bits at or above V: the static vector's);
 * count_out int64 [B] = the bits the copy rule set that the static words had not.  Every element of both outputs is written.  Reads
 * ids_dev[0 .. n), the start bits of those positions, hist_dev[b][lens[b] - M .. lens[b]) of the rows with lens[b] >= M,
 * lens_dev[0 .. B) and the static words, and nothing else. */
int cmp_k_copy_bans(void* stream, const uint16_t* ids_dev, int64_t n, const uint32_t* start_bits_dev, const cmp_event_grammar* layout,
                    const cmp_copy_guard_opts* opts, const int32_t* hist_dev, const int32_t* lens_dev, int B, int ld, int V,
                    const uint32_t* static_words_dev, uint32_t* words_out, int64_t* count_out);

/* ---- validation pass: held-out loss of a split in HBM, summed per event class on the device ---------------------------------
 * When does the model start memorising?  One call evaluates a whole held-out split that a cmp_dataset keeps in HBM and returns one
 * small table; Transformer.train runs it every eval_freq optimiser steps (Transformer.evaluate_dataset restates the arithmetic).
 *   Windows: window i of the stream ids[0..n) is ids[i (T + 1) .. (i + 1)(T + 1)), x its first T ids and y its last T -- the fixed
 *   grid of WindowDataset / DeviceDataset.  The windows first_window .. first_window + n_windows - 1 are evaluated, ALL of them, in
 *   batches of `batch` rows; the last batch holds the n_windows % batch windows that remain (ragged, not dropped).
 *   Per row with y inside [0, V), from the fp32 logits row z of the inference forward pass (training = false, the model's dtype):
 *     nll     = -(z[y] - logsumexp(z)): the fp32 value cmp_k_score_rows yields as -logp (one device function computes both);
 *     correct = (rank == 0): the greedy argmax, lowest index on ties -- cmp_k_softmax_xent's row_correct.
 *   A row whose target lies outside [0, V) is counted nowhere.
 *   Classes: n <= 8 disjoint, non-empty half-open id ranges [lo[c], hi[c]) inside [0, V).  A row belongs to the class whose range
 *   holds y; slot n collects every other id; slots above n are zero.  The grand total is the sum over the slots.  Null: n = 0.
 *   Sums: nll in float64, count and correct in int64, in a fixed order -- a wave adds its rows in ascending order, a workgroup its
 *   four waves in order, one workgroup the per-workgroup partial tables by index (cmp_k_grad_clip's scheme), batches ascending.  No
 *   float atomics, nothing depends on arrival order: two calls on the same inputs return the same bits.
 * cmp_eval_dataset: waits for the compute stream's earlier work (a train step may be in flight), enqueues every batch -- the window
 * cut, the forward pass, the row reduction -- with the table kept on the device, synchronises once and copies back only
 * sizeof(cmp_eval_table); nothing goes up.  The stream is idle when it returns.  1 <= batch <= max_batch, 1 <= T <= min(window_size,
 * max_seq), (first_window + n_windows)(T + 1) <= n, n_windows >= 1.  CMP_ERR_INVALID before any device work (reason in
 * cmp_last_error): ds and m in different contexts, a dataset whose largest id is >= V, windows outside the stream, batch or T out of
 * range, a class range outside [0, V), empty, or overlapping another, n > 8.
 * Read-only for everything that lasts: parameters, gradients, Adam state and iterations, a pending accumulation group, the dropout
 * counters, the metrics and stage slots of train steps in flight or just retired and both decode chains are what they were. */
typedef struct cmp_eval_classes { int32_t n; int32_t lo[8]; int32_t hi[8]; } cmp_eval_classes;
typedef struct cmp_eval_table { double nll[9]; int64_t count[9]; int64_t correct[9]; } cmp_eval_table;
int cmp_eval_dataset(cmp_model* m, cmp_dataset* ds, int64_t first_window, int64_t n_windows, int T, int batch,
                     const cmp_eval_classes* classes, cmp_eval_table* out);
/* The kernels alone (dev pointers; classes on the host): logits fp32 [rows, ldz], columns [V, ldz) are padding of any content; y
 * int32 [rows]; table_dev a cmp_eval_table the sums of these rows are ADDED INTO (all nine slots of the three arrays are rewritten);
 * ws_dev cmp_k_eval_rows_ws(rows) bytes of workspace; both 8-byte aligned.  One pass over the logits, two launches. */
int64_t cmp_k_eval_rows_ws(int rows);
int cmp_k_eval_rows(void* stream, const float* logits, int ldz, const int32_t* y, int rows, int V, const cmp_eval_classes* classes,
                    void* table_dev, void* ws_dev);

/* ---- live kernel timing (bench.py roofline): HIP events around every launch of ONE kernel class on the
 * stream it is launched on.  cls: 0 gemm forward (A[M,K].B[K,N]), 1 gemm dgrad (B stored [N,K]), 2 gemm wgrad
 * (A stored [K,M]), 3 attention forward, 4 attention dQ, 5 attention dK/dV, 6 layernorm fwd, 7 adam.
 * cmp_prof_end syncs the device and returns summed milliseconds, launch count and summed algorithmic work
 * (flops for 0-5, bytes for 6-7). */
int cmp_prof_begin(int cls);
int cmp_prof_end(double* total_ms, int64_t* launches, double* work);
/* the same, and the summed ALGORITHMIC HBM bytes of those launches (every operand read once, every result written once):
 * what bench.py's per-class `algorithmic_bytes` is, next to the PMC-measured `traffic`.  Class 8 = layernorm backward.
 * Class 9 = the decoder-block stack of a forward pass as ONE span (work = L * (24 E^2 + 2 E T) flops per token). */
int cmp_prof_end2(double* total_ms, int64_t* launches, double* work, double* bytes);
/* between begin and end: stop / continue recording (what has been recorded stays); bench.py times a subset of its timed steps */
int cmp_prof_pause(void);
int cmp_prof_resume(void);

/* ---- kernel-level entry points (dev pointers; dtype = cmp_dtype of activations) ----------------
 * Used by tests/ and bench.py to check and time single kernels against the oracle/roofline. */
int cmp_k_embed_fwd(void* stream, const int32_t* ids, const float* wte, const float* wpe, void* out,
                    int B, int T, int E, int pos0, int dtype, float p_drop, uint64_t seed, uint32_t rng_stream);
int cmp_k_embed_bwd(void* stream, const int32_t* ids, const void* dh, float* dwte, float* dwpe,
                    int B, int T, int E, int pos0, int dtype, float p_drop, uint64_t seed, uint32_t rng_stream);
/* cmp_k_embed_fwd with the two optional per-token arrays of a forward pass (int32 [B*T], either may be NULL): pos_ids replaces
 * pos0 + t as the row of wpe; type_ids names a second row of wte that is added LAST: out = ((wte[id] + wpe[pos]) + wte[type]) in
 * fp32, then dropout, then one rounding to the output dtype.  Both NULL: exactly cmp_k_embed_fwd. */
int cmp_k_embed_fwd_ex(void* stream, const int32_t* ids, const float* wte, const float* wpe, void* out,
                       int B, int T, int E, int pos0, int dtype, float p_drop, uint64_t seed, uint32_t rng_stream,
                       const int32_t* pos_ids, const int32_t* type_ids);
/* the same through the sorted form the model uses for batches of 4096 tokens or more (tokens counting-sorted by id, up to 128 rows of
 * one id summed by a workgroup before they are added: E f32 atomics per 128 rows instead of one per element); V = vocabulary size
 * (<= 8192).  Below 4096 tokens, above 8192 ids or with E no multiple of 8 (bf16) / 4 (fp32) this is cmp_k_embed_bwd: see
 * cmp_embed_bwd_form. */
int cmp_k_embed_bwd_v(void* stream, const int32_t* ids, const void* dh, float* dwte, float* dwpe,
                      int B, int T, int E, int pos0, int dtype, float p_drop, uint64_t seed, uint32_t rng_stream, int V);
/* the same through the atomic-free form of the deterministic mode: 64 token segments summed in order per id into ws, folded in
 * segment order, then dwte += ; dwpe += the batch sum in batch order.  Bitwise reproducible.  ws: cmp_k_embed_bwd_det_ws(V, E) bytes
 * (= V * 64 * E * 4), contents of no meaning before or after; fewer bytes, a NULL ws or V <= 0: CMP_ERR_INVALID and nothing is
 * written. */
int64_t cmp_k_embed_bwd_det_ws(int V, int E);
int cmp_k_embed_bwd_det(void* stream, const int32_t* ids, const void* dh, float* dwte, float* dwpe,
                        int B, int T, int E, int pos0, int dtype, float p_drop, uint64_t seed, uint32_t rng_stream, int V,
                        float* ws, int64_t ws_bytes);
/* Host only, no device work: the form the embedding backward takes for these arguments -- 0: one f32 atomic per gradient element,
 * 1: sorted, 2: atomic-free.  det != 0: the deterministic mode with a workspace for V ids; otherwise V ids and a sort workspace of
 * sort_ws_words int32 words (0: none; cmp_embed_bwd_sort_ws_words(B * T, V) is what the sorted form needs, 0 when V is outside
 * 1..8192).  The launcher itself decides through the same function. */
int cmp_embed_bwd_form(int B, int T, int E, int dtype, int V, int64_t sort_ws_words, int det);
int64_t cmp_embed_bwd_sort_ws_words(int64_t ntok, int V);
int cmp_k_layernorm_fwd(void* stream, const void* x, const float* gamma, const float* beta, void* y,
                        float* mean, float* rstd, int rows, int E, float eps, int dtype);
/* dx = resid(optional) + LN_bwd(dy); dgamma/dbeta fp32 [E] are ACCUMULATED into; ws >= cmp_k_layernorm_bwd_ws bytes */
int cmp_k_layernorm_bwd(void* stream, const void* dy, const void* x, const float* gamma, const float* mean,
                        const float* rstd, const void* resid, void* dx, float* dgamma, float* dbeta,
                        void* ws, int rows, int E, int dtype);
int64_t cmp_k_layernorm_bwd_ws(int rows, int E);
/* same, plus the prologue of the projection that consumes dx as the gradient of `x + dropout(proj)`: colsum[E] +=
 * column sums of dropout_grad(dx) (that projection's bias gradient) and, when p_drop > 0, dmask = dx * mask/(1-p). */
int cmp_k_layernorm_bwd_fused(void* stream, const void* dy, const void* x, const float* gamma, const float* mean,
                              const float* rstd, const void* resid, void* dx, float* dgamma, float* dbeta,
                              void* ws, int rows, int E, int dtype, void* dmask, float* colsum, float p_drop,
                              uint64_t seed, uint32_t rng_stream);
/* C[M,N] = epilogue(A.B): ta=0: A is [M,K] (lda); ta=1: A stored [K,M].  tb=0: B stored [K,N]; tb=1: B stored [N,K].
 * epilogue: +bias[N] (fp32, may be NULL); act: 0 none, 1 gelu (pre-activation stored to aux if aux!=NULL),
 * 2 multiply by gelu'(aux[m,n]); dropout (p>0) then +resid[m,n] (may be NULL).  out_fp32: C is fp32 regardless of
 * dtype.  splitk>1: fp32 atomic accumulation into C (C must be pre-zeroed or hold the value to add to).
 * The dropout mask of element (m, n) is a function of (seed, rng_stream, m, n) only -- the oracle's dropout_keep_rows over [M, N] --
 * independent of ldc. */
int cmp_k_gemm(void* stream, int dtype, int ta, int tb, int M, int N, int K,
               const void* A, int lda, const void* Bm, int ldb, void* C, int ldc,
               const float* bias, int act, void* aux, int ldaux, const void* resid, int ldr,
               int out_fp32, int splitk, float p_drop, uint64_t seed, uint32_t rng_stream, int flags);
/* flags: CMP_GEMM_KPAD_ZERO -- K-contiguous bf16 operands are stored with their rows zero-padded to a multiple of
 * 64 elements (lets a ragged K, e.g. the vocabulary, use the direct-to-LDS path); CMP_GEMM_GENERIC forces the
 * register-staged generic kernel (tests). */
#define CMP_GEMM_KPAD_ZERO 1
#define CMP_GEMM_GENERIC 2
#define CMP_GEMM_TILE128 4      /* tests/bench: force the 128x128 direct-to-LDS kernel */
#define CMP_GEMM_TILE256 8      /* tests/bench: force the persistent 256x256 2-stage kernel */
#define CMP_GEMM_P4 16          /* tests/bench: force the persistent deep-pipeline (BK=32) kernel */
#define CMP_GEMM_P4_128 32      /* with CMP_GEMM_P4: 128x256 tile / 4 waves / 3 stages / 2 workgroups per CU instead of 256x256 / 8 waves / 4 stages */
#define CMP_GEMM_NOSTORE 64     /* timing experiment only: run the whole epilogue but skip the global stores */
#define CMP_GEMM_ATOMICS 128    /* split-K: f32 atomics even where the registered slab workspace would do (cmp_gemm_set_workspace) */
/* ONE launch for up to 8 split-K weight gradients that contract over the same K rows -- the four Conv1D weight gradients of a
 * decoder block (tf.GradientTape through transformer.py:205-209) contract over the tokens: C_i[M_i, N_i] (fp32, ACCUMULATED into
 * with f32 atomics) += A_i^T . B_i, A_i bf16 stored [K, M_i] (lda_i), B_i bf16 stored [K, N_i] (ldb_i).  Requirements
 * (CMP_ERR_INVALID otherwise): K a multiple of 32, leading dimensions multiples of 8, 16-byte aligned operands, every operand
 * below 2 GiB.  The model's backward pass uses this launch in bf16 mode. */
int cmp_k_wgrad_group(void* stream, int nprob, const void* const* A, const int* lda, const void* const* B, const int* ldb,
                      float* const* C, const int* ldc, const int* M, const int* N, int K);
/* The same launch with the bias gradients riding on it: bias (NULL: as cmp_k_wgrad_group) holds per problem NULL or a vector of N_i
 * floats that receives, ACCUMULATED with f32 atomics, the column sums of B_i over the K rows -- the bias gradient of the Conv1D whose
 * weight gradient problem i is (tf.GradientTape through transformer.py:205-209: dy is that B operand).  One more MFMA per B fragment
 * in the items of a problem's first tile row, no pass of its own.  The last-arriver form (COMPOSER_WGRAD_TAIL=la) refuses a bias. */
int cmp_k_wgrad_group_bias(void* stream, int nprob, const void* const* A, const int* lda, const void* const* B, const int* ldb,
                           float* const* C, const int* ldc, const int* M, const int* N, int K, float* const* bias);
/* Host-only window on the grouped launch's plan (CPU tests; no HIP call, works without a device): whether the problems fit the
 * kernel, whether the cost model takes the grouped launch, and the item table.  A / B (NULL: aligned) are looked at for 16-byte
 * alignment only.  flags: 1 = slab split-K asked for (refused), 2 = take the launch whatever the cost model says (as
 * cmp_k_wgrad_group does).  items (NULL: not wanted): up to max_items rows of 8 int32 {problem, m0, n0, first k-step, end k-step,
 * index of this K range among the tile's, K ranges of the tile, tile}, in item-table order. */
typedef struct cmp_wgrad_plan_info {
    int32_t fits;                /* the problems are in the grouped kernel's domain */
    int32_t taken;               /* ... and the grouped launch is chosen */
    int32_t refusal;             /* 0 fits, 1 problem count, 2 K, 3 workgroups, 4 slab workspace, 5 shape, 6 leading dimension,
                                    7 alignment, 8 operand span, 9 table fields */
    int32_t wgs, tiles, nk;      /* workgroups the launch may use, output tiles of all problems, k-steps of 32 */
    int32_t nitems, grid;
    int32_t max_split, longest;  /* most K ranges of a tile, longest item in k-steps */
    int32_t nslots;              /* last-arriver form: partial-tile workspace slots */
} cmp_wgrad_plan_info;
int cmp_wgrad_group_plan(int nprob, const void* const* A, const int* lda, const void* const* B, const int* ldb, const int* M,
                         const int* N, int K, int max_wgs, int flags, cmp_wgrad_plan_info* out, int32_t* items, int max_items);
/* ---- LayerNorm folded into the block's GEMM epilogues (the fused block path of the bf16 train / inference forward) -----------
 * Replaces the stand-alone tf.keras LayerNormalization calls of DecoderBlock.call (transformer.py:583-584 ln_1, :591 ln_2; layers
 * built at :551,563) for large batches: no LayerNorm kernel runs in the forward pass.  Row statistics travel as PARTIALS, fp32
 * [rows][E/256][2] = (mean, M2 = sum of squared deviations from that mean) of every 256-column segment of a row, merged with
 * Chan's update by the consumer (never a sum of squares).
 *   cmp_k_embed_fwd_stats: cmp_k_embed_fwd (bf16) that also leaves the partials of the rows it wrote (SharedTokenEmbedding +
 *     position embedding, transformer.py:786-794, feeding block 0's ln_1).  E a multiple of 256.
 *   cmp_k_ln_fold_prep: weight side of  LN(x).W + b = rstd*(x.(gamma o W)) - rstd*mean*colsum(gamma o W) + (beta.W + b):
 *     W fp32 [E,N] (Conv1D weight, transformer.py:184-189), bias [N], gamma / beta [E] -> WT bf16 [N,E] = (gamma o W)^T,
 *     cs[N] = column sums of the ROUNDED WT, bias_out[N] = bias + beta.W.  E, N multiples of 32.
 *   cmp_gemm_ln_next: one-shot, the NEXT cmp_k_gemm of this thread carries a LayerNorm epilogue -- in_part (+ np = E/256 in
 *     2..3, eps): statistics of the rows of A (fold: cs given; the GEMM's B operand is WT and its bias is bias_out) or of the
 *     rows of `resid` (gamma, beta given: the residual operand becomes LN(resid), transformer.py:587); out_part: the partials of
 *     the OUTPUT rows are written (residual epilogues).  bf16, ta=0, tb=1, M and N multiples of 256, and a shape that reaches the
 *     persistent 256x256 kernel (CMP_GEMM_TILE256 forces it); anything else fails with CMP_ERR_INVALID.  With out_fp32 the fold also
 *     takes a ragged N (ln_f folded into the tied-logits matmul, transformer.py:811, 818: N = vocabulary size; cs and bias must then
 *     hold N rounded up to 256 entries, zero beyond N). */
int cmp_k_embed_fwd_stats(void* stream, const int32_t* ids, const float* wte, const float* wpe, void* out, float* part,
                          int B, int T, int E, int pos0, float p_drop, uint64_t seed, uint32_t rng_stream);
int cmp_k_ln_fold_prep(void* stream, const float* W, const float* bias, const float* gamma, const float* beta, void* WT,
                       float* cs, float* bias_out, int E, int N);
int cmp_gemm_ln_next(const float* in_part, int np, float eps, const float* cs, const float* gamma, const float* beta,
                     float* out_part);
/* Round 6, the backward pass of the LayerNorm-fused block path (weight gradients on the RAW LayerNorm input rows, no LayerNorm output
 * ever written).  One-shot arming calls like cmp_gemm_ln_next, consumed by this thread's next cmp_k_gemm / cmp_k_attn_bwd:
 *   cmp_gemm_ln_scale_next: the rows' rstd (merged from in_part) is a FACTOR -- with act = 2 (gelu' epilogue) the launch stores
 *     C = rstd o (acc * gelu'(aux)) and still sends the column sums of the UNSCALED product to cmp_gemm_colsum_next's vector; with
 *     a residual operand it stores C = acc + rstd o resid.
 *   cmp_k_ln_stats_merge: (mean, rstd) per row from the rows' partial statistics [rows][np][2] (the model merges all its sites in one launch).
 *   cmp_attn_bwd_ln_next: cmp_k_attn_bwd stores rstd[token] o [dQ | dK | dV].
 *   cmp_k_layernorm_bwd_prescaled: the LayerNorm backward (mean / rstd arrays) on a dy that holds rstd o (the gradient); bf16;
 *     dmask (when given) is written whatever p_drop is.
 *   cmp_k_wgrad_ln_fix: G[k, j] = gamma[k] * (G[k, j] - mean over k' of G[k', j]) + beta[k] * colsum[j] -- turns R = (raw rows)^T .
 *     (rstd o D) into LN(raw rows)^T . D: the mean term mean^T . (rstd o D) IS the column mean of R, a row's mean being the mean of
 *     that row as stored. */
int cmp_gemm_ln_scale_next(const float* in_part, int np, float eps);
int cmp_k_ln_stats_merge(void* stream, const float* part, int np, float eps, float* mean, float* rstd, int rows);
int cmp_attn_bwd_ln_next(const float* rstd);
int cmp_k_layernorm_bwd_prescaled(void* stream, const void* dy_scaled, const void* x, const float* gamma, const float* mean,
                                  const float* rstd, const void* resid, void* dx, float* dgamma, float* dbeta, void* ws,
                                  int rows, int E, void* dmask, float* colsum, float p_drop, uint64_t seed, uint32_t rng_stream);
int cmp_k_wgrad_ln_fix(void* stream, float* G, int rows, int cols, const float* gamma, const float* beta, const float* colsum);
/* Diagnostics of the model's last passes: fused = 1 when the last forward pass took the LayerNorm-fused block path;
 * wgrad_table_builds = item tables of the grouped weight-gradient launches built so far (a steady train loop builds one per
 * decoder block, once). */
int cmp_model_path_info(cmp_model* m, int* fused, int64_t* wgrad_table_builds);
/* carried = 1 when the last backward pass took the bias gradients of its decoder blocks from the blocks' grouped weight-gradient
 * launches (cmp_k_wgrad_group_bias) instead of the producers' own column sums; 0 otherwise (no backward pass yet, fp32, no
 * LayerNorm, COMPOSER_LN_FUSED=3, COMPOSER_DETERMINISTIC=1, COMPOSER_BIAS_WGRAD=0, or shapes at which the grouped launch is not
 * taken).  COMPOSER_BIAS_WGRAD is read once per model at cmp_model_create: a mask of the carried bias gradients, 1 mlp c_proj, 2 c_fc,
 * 4 attention c_proj, 8 c_attn; unset = 10 (c_fc + c_attn: the two whose producers are faster without their sums), 15 = all four. */
int cmp_model_bias_path(cmp_model* m, int* carried);
/* Registers a device workspace for split-K reductions: with it, split-K launches write per-split fp32 partial tiles and
 * fold them in a fixed order (reproducible, no float atomics); without it (or if too small: splitk*M*N*4 bytes) they
 * accumulate with f32 atomics.  CMP_GEMM_ATOMICS forces the atomic path. */
int cmp_gemm_set_workspace(void* ws_dev, int64_t bytes);
/* One-shot: the next cmp_k_gemm (plain output in the compute dtype) also adds the column sums of its output to
 * out[0..N) -- the bias gradient that goes with an input-gradient GEMM (transformer.py:916-920 via tf.GradientTape).
 * Fused into the GEMM epilogue where possible, otherwise a cmp_k_colsum pass after it. */
int cmp_gemm_colsum_next(float* out);
/* One-shot: the next cmp_k_gemm (or cmp_gemm_plan) of this thread launches its persistent kernel on at most max_wgs CUs
 * (0 = no cap, up to 256; the 128x256 deep pipeline runs two workgroups per capped CU) and, with rev != 0, the 256x256
 * two-stage kernel walks every XCD group's tiles from the end -- the model's grid cap under a communicator and its alternating
 * walk direction, for the kernel-level tests that give a workgroup several items.  Values outside 0..256: CMP_ERR_INVALID.
 * cmp_k_wgrad_group / cmp_k_wgrad_group_bias consume the same state: the cap becomes the workgroup count of the grouped launch's
 * plan (cmp_wgrad_group_plan's max_wgs; rounded down to a multiple of 8, so a cap of 1..7 is refused by that call with
 * CMP_ERR_INVALID and a message that names the cap), `rev` is ignored there, and both are cleared -- by a refused call too -- so
 * that neither reaches a later cmp_k_gemm. */
int cmp_gemm_grid_next(int max_wgs, int rev);
/* diagnostic only: a device buffer of 500 uint64 receives (id, s_memtime) pairs from one workgroup of the next
 * deep-pipeline GEMM launches (tools/gemm_timeline.py); pass NULL to switch it off. */
int cmp_gemm_set_stamps(void* dev_buf);
/* Host-only window on the launcher's decision (CPU tests): the plan of the launch that cmp_k_gemm would make of the same
 * arguments.  Consumes the calling thread's armed one-shot state (cmp_gemm_colsum_next, cmp_gemm_grid_next, cmp_gemm_ln_next,
 * cmp_gemm_ln_scale_next; reads cmp_gemm_set_workspace) exactly as the next cmp_k_gemm would, dereferences nothing and calls
 * no HIP function: it works without a device, operand pointers may be any non-null 16-byte-aligned value.  A launch cmp_k_gemm
 * would refuse returns the same status and sets the same cmp_last_error() text. */
enum {
    CMP_GEMM_FAM_F32 = 0,        /* fp32 parity kernel, 64x64x16 */
    CMP_GEMM_FAM_GENERIC = 1,    /* bf16, register-staged: any shape */
    CMP_GEMM_FAM_TILE128 = 2,    /* bf16 128x128 direct-to-LDS, two stages */
    CMP_GEMM_FAM_RING = 3,       /* ... its four-stage ring (at most 256 tiles, whole k-steps, a compile-time epilogue kind) */
    CMP_GEMM_FAM_TILE256 = 4,    /* bf16 persistent 256x256, two stages of 64 */
    CMP_GEMM_FAM_P4_256 = 5,     /* bf16 persistent deep pipeline (k-steps of 32), 256x256 */
    CMP_GEMM_FAM_P4_128 = 6      /* ... 128x256, two workgroups per CU */
};
typedef struct cmp_gemm_plan_info {
    int32_t family;              /* CMP_GEMM_FAM_* */
    int32_t a_km, b_km;          /* A / B stored K-contiguous (ta == 0 / tb == 1) */
    int32_t swap;                /* non-atomic epilogue */
    int32_t kind;                /* epilogue: 0 run-time, 1 plain, 2 gelu + aux, 3 residual, 4 gelu', 5 plain fp32 (LayerNorm fold) */
    int32_t lnm, np;             /* LayerNorm mode and segments of the persistent 256x256 kernel (0, 1: none) */
    int32_t diag;                /* timeline-stamp build (cmp_gemm_set_stamps) */
    int32_t grid_x, grid_y, grid_z, block;
    int64_t smem;                /* dynamic LDS bytes */
    int32_t nk, per, nsplit;     /* k-steps of the family's depth, k-steps per split, splits */
    int32_t tiles_n, ntiles;
    int32_t slabs, reduce_grid;  /* split-K through workspace slabs + fixed-order reduce (else f32 atomics) */
    int32_t colsum_fused, colsum_pass;   /* armed column sums: in the epilogue, or a cmp_k_colsum pass after the launch */
    int32_t cls;                 /* cmp_prof_* timing class, -1: not timed */
    int32_t sched;               /* the launch draws an item-counter set */
    int32_t empty;               /* M == 0 or N == 0: nothing is launched */
} cmp_gemm_plan_info;
int cmp_gemm_plan(int dtype, int ta, int tb, int M, int N, int K, const void* A, int lda, const void* Bm, int ldb, void* C,
                  int ldc, const float* bias, int act, void* aux, int ldaux, const void* resid, int ldr, int out_fp32, int splitk,
                  float p_drop, uint64_t seed, uint32_t rng_stream, int flags, cmp_gemm_plan_info* out);
int cmp_k_colsum(void* stream, const void* X, int ldx, float* out, int rows, int cols, int dtype);
/* the same without float atomics, as the deterministic mode runs it: every row split writes its partial sums to ws, one fold adds
 * them in split order, then out += .  Bitwise reproducible.  ws: cmp_k_colsum_det_ws(rows, cols, dtype) bytes (splits * cols * 4);
 * fewer bytes or a NULL ws: CMP_ERR_INVALID and nothing is written. */
int64_t cmp_k_colsum_det_ws(int rows, int cols, int dtype);
int cmp_k_colsum_det(void* stream, const void* X, int ldx, float* out, int rows, int cols, int dtype, float* ws, int64_t ws_bytes);
/* causal attention on qkv [B,T,3E] (head-merged, transformer.py:417): o [B,T,E], lse fp32 [B,H,T] */
int cmp_k_attn_fwd(void* stream, const void* qkv, void* o, float* lse, int B, int T, int H, int D,
                   int scale, int dtype, float p_drop, uint64_t seed, uint32_t rng_stream);
/* One-shot: the next cmp_k_attn_bwd also adds the column sums of [dQ | dK | dV] to out[0..3E): the c_attn bias gradient
 * (Conv1D bias under tf.GradientTape, transformer.py:205-209, 916-920), taken from the f32 accumulators. */
int cmp_attn_bwd_bias_next(float* out);
int cmp_k_attn_bwd(void* stream, const void* qkv, const void* o, const void* d_o, const float* lse,
                   float* delta_ws, void* dqkv, int B, int T, int H, int D, int scale, int dtype,
                   float p_drop, uint64_t seed, uint32_t rng_stream);
/* Host-only window on the attention launcher's decision (CPU tests): the plan of the launch that cmp_k_attn_fwd (backward = 0) or
 * cmp_k_attn_bwd (backward = 1) would make of such arguments -- has_amask: a per-key mask term (the model's forward only);
 * want_bias: cmp_attn_bwd_bias_next armed; has_ln_rows: cmp_attn_bwd_ln_next armed -- on a device that answers wgs_per_cu and
 * ks_ok (cmp_attn_caps).  Reads COMPOSER_ATTN_KS / COMPOSER_ATTN_BIAS_PASS as the launcher does, calls no HIP function and
 * works without a device.  A launch that would be refused returns the same status and sets the same cmp_last_error() text. */
enum {
    CMP_ATTN_FWD_KS = 0,         /* key-split forward (bf16, head size <= 32, small grids) */
    CMP_ATTN_FWD_MASK = 1,       /* 128-row forward with the mask term */
    CMP_ATTN_FWD_ROWS = 2,       /* 128-row forward */
    CMP_ATTN_BWD_LN = 3,         /* 128-row dQ, dK/dV with rstd-scaled stores */
    CMP_ATTN_BWD_KS1 = 4,        /* key-split backward in one launch */
    CMP_ATTN_BWD_KS2 = 5,        /* key-split dQ, then key-split dK/dV */
    CMP_ATTN_BWD_ROWS = 6        /* 128-row dQ, dK/dV */
};
enum { CMP_ATTN_K_FWD = 0, CMP_ATTN_K_DQ = 1, CMP_ATTN_K_DQ_LN = 2 };   /* the kernel a block plan is for (cmp_attn_caps) */
typedef struct cmp_attn_plan_info {
    int32_t form;                /* CMP_ATTN_* */
    int32_t drop;                /* the dropout instantiations */
    int32_t nlaunch;             /* 1, or 2: [0] dQ, [1] dK/dV */
    int32_t grid_x[2], grid_y[2], block;
    int64_t smem[2];             /* dynamic LDS bytes per launch */
    int32_t optin;               /* an image above 64 KiB: the kernels need the dynamic-LDS opt-in with smem[i] */
    int32_t plan_u;              /* forward / dQ block plan: (batch, head) rows per XCD that run as single blocks; -1: the 2-D grid */
    int32_t bias_fused, bias_pass;   /* wanted bias sums: in the kernels (float atomics), or a cmp_k_colsum pass after them */
    int32_t cls[2];              /* cmp_prof_* timing class per launch, -1: not timed */
    double work[2], bytes[2];    /* ... its flops and algorithmic HBM bytes */
    int32_t empty;               /* B * T == 0: nothing is launched */
} cmp_attn_plan_info;
int cmp_attn_plan(int dtype, int B, int T, int H, int D, float p_drop, int has_amask, int want_bias, int has_ln_rows,
                  int backward, int wgs_per_cu, int ks_ok, cmp_attn_plan_info* out);
/* What the attention launcher asks the current device about the kernels of (dtype, D): resident workgroups per CU of `kernel`
 * (CMP_ATTN_K_*; the block plan's slots) and whether the key-split set got its LDS opt-in (0 where none is built).  Needs a GPU. */
int cmp_attn_caps(int dtype, int D, int kernel, int* wgs_per_cu, int* ks_ok);
/* fused softmax cross-entropy forward+backward: logits fp32 [rows, ldz]; dlogits (dtype) [rows, ldz] with
 * zeroed padding; row_loss fp32 [rows]; row_correct int32 [rows]; inv_n = 1/(B*T) */
int cmp_k_softmax_xent(void* stream, const float* logits, int ldz, const int32_t* y, void* dlogits,
                       float* row_loss, int32_t* row_correct, int rows, int V, float inv_n, int dtype);
/* Keras Adam (transformer.py:887,921): eps outside the bias correction; step = optimizer.iterations+1 */
int cmp_k_adam(void* stream, float* p, const float* g, float* m, float* v, void* shadow_bf16,
               int64_t n, float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale);
/* cmp_k_adam with the factor read from device memory (the float cmp_k_grad_clip leaves in out.factor): the same multiply at the
 * same place, bitwise equal to cmp_k_adam with grad_scale = *factor_dev. */
int cmp_k_adam_dev(void* stream, float* p, const float* g, float* m, float* v, void* shadow_bf16,
                   int64_t n, float lr, float beta1, float beta2, float eps, int64_t step, const float* factor_dev);
/* Global-norm clipping at kernel level: sum of squares + finish on n floats (n % 4 == 0, g 16-byte aligned); ws >=
 * cmp_k_grad_clip_ws(n) bytes; out = {double norm; float scale; float factor}: norm = gscale * sqrt(sum g^2) with the squares and
 * their sum in float64 in a fixed order (no atomics: the same bits give the same double), scale = 1 if norm <= clip_norm else
 * clip_norm / norm, factor = gscale * scale.  clip_norm > 0 (+inf: measure only). */
int64_t cmp_k_grad_clip_ws(int64_t n);
int cmp_k_grad_clip(void* stream, const float* g, int64_t n, float gscale, float clip_norm, void* ws, void* out);

#ifdef __cplusplus
}
#endif
#endif /* COMPOSER_HIP_H */
