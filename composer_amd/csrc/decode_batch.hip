// decode_batch.hip -- B independent sequences decoded together (cmp_decode_batch_begin / cmp_decode_batch_steps).
//
// The per-token chain has the structure of the batch-1 chain of decode.hip -- per layer LN1+c_attn, attention,
// combine+c_proj+residual, LN2+c_fc+GELU, c_proj+residual, then LN_f+logits and the sampler -- with ONE launch per stage
// for all B rows, so one replay reads the fp32 weights once for every row and the launch chain is shared by all of them.
// Prefill runs each row on its own through the same model_forward(m, x, 1, lens[b]) call as cmp_decode_begin, so a row's
// first id is the batch-1 first id for seed + b.
//
// Per-row reproducibility: no arithmetic of a row depends on B or on the other rows.  The projections run on the exact-f32
// MFMA (an output element is a fixed sum of k-ordered fma chains, the split fixed by K alone); padding rows of a 16-row tile are zero
// and never stored; the attention key split is a function of the row's own position; the LayerNorm statistics are per row.
// A row's ids are therefore a function of (weights, prompt, seed + b, mode, and the row's own temperature, top_k, top_p) only.
//
// Sliding-window mode (cmp_decode_batch_begin_slide): a row whose cache is full sits out the replay (DecRow::hold) and draws
// that step's id from a re-encode of its last `keep` tokens; rows that slide at the same step share forward calls.
//
// State lives apart from the batch-1 DecodeState (m->dec): own transposed weights, buffers, KV caches and captured chains.
#include "model.h"
#include "decode_common.h"

#include <map>

#define DECB_MAX_ROWS 256

struct DecRow {          // device-resident per-row loop state (the captured chain does not depend on it)
    int pos;             // position id of the token about to be consumed
    int token;           // that token
    int produced;        // ids written to this row's slot of ids[]
    int advance;         // 1: kv mode (pos += 1 per step), 0: literal (pos stays 0)
    unsigned rng;        // sampling counter
    unsigned seed;       // (uint32)(seed + b)
    float temperature;   // <= 0: greedy
    int hold;            // sliding-window mode: 1 while the row sits out a replay (its cache is full, pos == W): attention neither
                         // appends nor reads, the sampler leaves the row alone; the row's slide, run after the replay, clears it
    int top_k;           // truncated sampling (decode_common.h), per row: 0 or >= V: off
    float top_p;         // 1: off
    DecGrammar gr;       // event grammar (decode_common.h): layout, rules and the fold of the row's prompt ++ ids so far
};

struct DecRowList {      // rows of one slide, by value in the kernel arguments: no host buffer has to outlive an enqueued step
    unsigned char row[DECB_MAX_ROWS];
};

struct DecBatchLayerW {
    float *attn_wT, *proj_wT, *fc_wT, *pr_wT;
    float *kc, *vc;      // [capB] x the batch-1 layouts: K [H][D/4][W][4], V [H][W][D]
};

struct DecodeBatchState {
    int capB = 0;                       // rows the row buffers and caches hold
    int cap = 0;                        // ids per row
    DecRow* st = nullptr;
    int32_t* ids = nullptr;             // [capB][cap]
    float *x = nullptr, *u = nullptr, *qkv = nullptr, *att = nullptr, *r = nullptr, *g = nullptr, *logits = nullptr;
    std::vector<DecBatchLayerW> lw;
    std::vector<void*> row_allocs;      // sized by capB (replaced when a larger B is asked for)
    std::vector<void*> w_allocs;        // transposed weights (independent of B)
    unsigned* banw = nullptr;           // static bans of the event grammar, ceil(V / 32) words shared by all rows (in w_allocs: its
                                        // address outlives every captured chain)
    std::map<int, std::pair<hipGraph_t, hipGraphExec_t>> graphs;     // captured chain per B
    bool graph_on = true;
    int64_t weights_version = -1;
    int B = 0, mode = 0;
    int produced = 0, returned = 0;
    std::vector<int> pos;               // host mirror of each row's position (kv-mode window check; which rows slide at which step)
    bool begun = false;
    // sliding-window mode (cmp_decode_batch_begin_slide): every row's prompt and its length stay on the device beside its ids
    int32_t* prompts = nullptr;         // [capB][W]
    int32_t* plen = nullptr;            // [capB]
    int keep = 0;                       // 0: plain kv / literal decode
    int64_t row_slides = 0, fwd_calls = 0;
};

static void decb_drop_graphs(DecodeBatchState* d) {
    for (auto& kv : d->graphs) {
        if (kv.second.second) hipGraphExecDestroy(kv.second.second);
        if (kv.second.first) hipGraphDestroy(kv.second.first);
    }
    d->graphs.clear();
}

static void decb_free_rows(DecodeBatchState* d) {
    decb_drop_graphs(d);
    for (void* p : d->row_allocs) hipFree(p);
    d->row_allocs.clear();
    for (auto& w : d->lw) w.kc = w.vc = nullptr;
    d->capB = 0;
}

void decode_batch_state_free(DecodeBatchState* d) {
    if (!d) return;
    decb_free_rows(d);
    for (void* p : d->w_allocs) hipFree(p);
    delete d;
}

template <typename Tp> static int balloc(std::vector<void*>& list, Tp** p, size_t bytes) {
    void* q = nullptr;
    HIP_CHECK(hipMalloc(&q, bytes ? bytes : 16));
    list.push_back(q);
    *p = (Tp*)q;
    return CMP_OK;
}

// out[n][k] = in[k][n] (the batch-1 transpose, here for the batch state's own copies)
__global__ void decb_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int K, int N) {
    __shared__ float tile[32][33];
    int n0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int j = ty; j < 32; j += 8) {
        int k = k0 + j, n = n0 + tx;
        tile[j][tx] = (k < K && n < N) ? in[(int64_t)k * N + n] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        int n = n0 + j, k = k0 + tx;
        if (n < N && k < K) out[(int64_t)n * K + k] = tile[tx][j];
    }
}

// Y[b][n] = act( IN(X)[b,:] . Wt[n,:] + bias[n] ) + resid[b][n] for b < B, on v_mfma_f32_16x16x4_f32.
// Workgroup = one 16-column x 16-row output tile (blockIdx.x, blockIdx.y); its 4 waves split K: wave w takes the 64-wide k blocks
// w, w + 4, w + 8, ... and the four partial tiles are added in wave order through LDS.  Lane l holds A[row l&15][k] (the input row)
// and B[k][col l&15] (the weight row) for the k of its quarter q = l>>4: in each k block lane q reads the 16 contiguous floats
// kb + 16q .. kb + 16q + 15 of its row (four 16-B loads), and MFMA (u, j) sums over q the products at k = kb + 16q + 4u + j into
// accumulator u>>1.  That order depends on K only: an output element is the same sequence of fma chains whatever B is.
// IN: 0 the rows as they are, 1 LayerNorm (per-row statistics computed by each workgroup for its 16 rows), 2 the combine of the
// split-key attention partials [B][H][ATT_SPLITS][PSTRIDE(D)] (K = H*D).  u_out (IN 0/1): the workgroups of column tile 0 also
// write the normalised rows (the residual of the attention branch).
template <int ACT, int IN>
__global__ __launch_bounds__(256) void decb_proj_kernel(const float* __restrict__ x, const float* __restrict__ ln_g,
                                                        const float* __restrict__ ln_b, float eps,
                                                        const float* __restrict__ Wt, const float* __restrict__ bias,
                                                        const float* __restrict__ resid, float* __restrict__ y, int ldy,
                                                        float* __restrict__ u_out, int K, int N, int D, int B) {
    extern __shared__ float cw[];                     // IN == 2: [16][H][ATT_SPLITS] combine weights
    __shared__ float smu[16], srs[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, c16 = lane & 15;
    const int r0 = blockIdx.y * 16;
    const int row = r0 + c16;
    const bool rv = row < B;
    const int H = K / D;
    const int ps_row = H * ATT_SPLITS * PSTRIDE(D);   // IN == 2: floats per row of partials
    if (IN == 1) {
#pragma unroll 1
        for (int i = 0; i < 4; i++) {
            const int t = wave * 4 + i, rr = r0 + t;
            if (rr >= B) break;                       // wave-uniform
            const float* xr = x + (int64_t)rr * K;
            float s = 0.f;
            for (int k = lane * 4; k < K; k += 256) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(xr + k);
                s += (v[0] + v[1]) + (v[2] + v[3]);
            }
            const float mu = wave_sum2(s) / (float)K;
            float qs = 0.f;
            for (int k = lane * 4; k < K; k += 256) {
                const f32x4 dv = *reinterpret_cast<const f32x4*>(xr + k) - mu;
                qs += (dv[0] * dv[0] + dv[1] * dv[1]) + (dv[2] * dv[2] + dv[3] * dv[3]);
            }
            const float var = wave_sum2(qs) / (float)K;
            if (lane == 0) { smu[t] = mu; srs[t] = 1.0f / sqrtf(var + eps); }
        }
    } else if (IN == 2) {
        for (int t = threadIdx.x; t < 16 * H; t += 256) {
            const int rr = r0 + t / H, h = t % H;
            if (rr >= B) continue;
            const float* p = x + (int64_t)rr * ps_row + (size_t)h * ATT_SPLITS * PSTRIDE(D);
            float mv[ATT_SPLITS], sv[ATT_SPLITS];
            float mx = -INFINITY;
#pragma unroll
            for (int sI = 0; sI < ATT_SPLITS; sI++) {
                mv[sI] = p[sI * PSTRIDE(D) + D];
                sv[sI] = p[sI * PSTRIDE(D) + D + 1];
                mx = fmaxf(mx, mv[sI]);
            }
            float den = 0.f;
#pragma unroll
            for (int sI = 0; sI < ATT_SPLITS; sI++) { mv[sI] = expf(mv[sI] - mx); den += mv[sI] * sv[sI]; }   // empty splits: 0
            const float inv = 1.0f / den;
#pragma unroll
            for (int sI = 0; sI < ATT_SPLITS; sI++) cw[t * ATT_SPLITS + sI] = mv[sI] * inv;
        }
    }
    __syncthreads();
    const int n0 = blockIdx.x * 16;
    const float* wr = Wt + (int64_t)min(n0 + c16, N - 1) * K;
    const float* xr = x + (int64_t)min(row, B - 1) * (IN == 2 ? ps_row : K);
    const float mu = (IN == 1) ? smu[c16] : 0.f, rs = (IN == 1) ? srs[c16] : 0.f;
    const bool write_u = (IN != 2) && u_out && blockIdx.x == 0 && rv;
    f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll 2
    for (int kb = wave * 64; kb < K; kb += 256) {
        f32x4 wv[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int k = kb + 16 * q + 4 * u;
            // streamed once per step: non-temporal, as the batch-1 GEMV
            wv[u] = (k < K) ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(wr + k)) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int k = kb + 16 * q + 4 * u;
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (k < K && rv) {
                if (IN == 2) {
                    const int h = k / D, dd = k % D;
                    const float* p = xr + (size_t)h * ATT_SPLITS * PSTRIDE(D) + dd;
                    const float* w = cw + (c16 * H + h) * ATT_SPLITS;
#pragma unroll
                    for (int sI = 0; sI < ATT_SPLITS; sI++) v += *reinterpret_cast<const f32x4*>(p + sI * PSTRIDE(D)) * w[sI];
                } else {
                    v = *reinterpret_cast<const f32x4*>(xr + k);
                    if (IN == 1) {
                        const f32x4 gv = *reinterpret_cast<const f32x4*>(ln_g + k);
                        const f32x4 bv = *reinterpret_cast<const f32x4*>(ln_b + k);
                        v = (v - mu) * rs * gv + bv;
                    }
                    if (write_u) *reinterpret_cast<f32x4*>(u_out + (int64_t)row * K + k) = v;
                }
            }
            xv[u] = v;
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[u >> 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[u][j], wv[u][j], acc[u >> 1], 0, 0, 0);
    }
    __shared__ __attribute__((aligned(16))) f32x4 red[4][64];
    red[wave][lane] = acc[0] + acc[1];
    __syncthreads();
    if (wave != 0) return;
    const f32x4 t = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    const int n = n0 + c16;
    if (n >= N) return;
    const float bn = bias ? bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {                     // accumulator i: row r0 + 4q + i, column n
        const int rr = r0 + 4 * q + i;
        if (rr < B) {
            float v = t[i];
            if (bias) v += bn;
            if (ACT == 1) v = gelu_f<true>(v);
            if (resid) v += resid[(int64_t)rr * N + n];
            y[(int64_t)rr * ldy + n] = v;
        }
    }
}

// Split-key single-query attention for B rows, grid (H, ATT_SPLITS, B): dec_attn2_kernel of decode.hip with the row's own
// position, qkv row, KV caches and partial records.  The key split depends on the row's position only.
template <int D>
__global__ __launch_bounds__(256) void decb_attn_kernel(const float* __restrict__ qkv, float* __restrict__ kcT,
                                                        float* __restrict__ vc, float* __restrict__ part,
                                                        const DecRow* __restrict__ st, int E, int W, float scale) {
    constexpr int CH = D / 4;                       // 16-byte chunks per row
    constexpr int CPL = CH / 2;                     // K chunks per lane of a key pair
    constexpr int KPI = 64 / CH;                    // V rows per wave-instruction
    constexpr int VL = 32 / KPI;                    // V loads per lane per 32-key pass
    __shared__ __attribute__((aligned(16))) float opart[4][KPI][D];
    __shared__ float pw[4][32];
    __shared__ float mw[4], lw[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = blockIdx.x, sp = blockIdx.y, b = blockIdx.z;
    const int H = gridDim.x;
    const int pos = st[b].pos;
    const int chunk = ((pos + 1 + ATT_SPLITS - 1) / ATT_SPLITS + 3) & ~3;
    const int j0 = sp * chunk, j1 = min(pos + 1, j0 + chunk);
    const int nk = j1 - j0;
    float* out = part + (((size_t)b * H + h) * ATT_SPLITS + sp) * PSTRIDE(D);
    if (nk <= 0 || st[b].hold || pos >= W) {        // a held row (pos == W) has no cache slot left: it must not append
        if (tid < D) out[tid] = 0.f;
        if (tid == 0) { out[D] = -INFINITY; out[D + 1] = 0.f; }
        return;
    }
    const float* qr = qkv + (size_t)b * 3 * E;
    const float* qh = qr + h * D;
    const float* kcur = qr + E + h * D;
    const float* vcur = qr + 2 * E + h * D;
    float* kh = kcT + (int64_t)b * W * E + (int64_t)h * CH * W * 4;
    float* vh = vc + (int64_t)b * W * E + (int64_t)h * W * D;
    if (pos >= j0 && pos < j1 && tid < D) {        // append (read by later tokens only)
        kh[((int64_t)(tid >> 2) * W + pos) * 4 + (tid & 3)] = kcur[tid];
        vh[(int64_t)pos * D + tid] = vcur[tid];
    }
    const int pairI = lane >> 1, half = lane & 1;
    const int kg = lane / CH, vcI = lane % CH;
    f32x4 qv[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) qv[c] = *reinterpret_cast<const f32x4*>(qh + (half * CPL + c) * 4);
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int jb = wave * 32; jb < nk; jb += 128) {       // wave-uniform: this wave's 32 keys of the pass
        const int j = jb + pairI;
        const int key = j0 + j;
        const bool valid = j < nk;
        f32x4 kv[CPL], vv[VL];
#pragma unroll
        for (int c = 0; c < CPL; c++) {
            const int cc = half * CPL + c;
            const float* src = (key == pos) ? kcur + cc * 4 : kh + ((int64_t)cc * W + key) * 4;
            kv[c] = valid ? *reinterpret_cast<const f32x4*>(src) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < VL; u++) {
            const int jv = jb + u * KPI + kg;
            const int keyv = j0 + jv;
            const float* src = (keyv == pos) ? vcur + vcI * 4 : vh + (int64_t)keyv * D + vcI * 4;
            vv[u] = (jv < nk) ? *reinterpret_cast<const f32x4*>(src) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < CPL; c++) a += (qv[c][0] * kv[c][0] + qv[c][1] * kv[c][1]) + (qv[c][2] * kv[c][2] + qv[c][3] * kv[c][3]);
        a += DPP_F(a, DPP_XOR1);
        a = valid ? a * scale : -INFINITY;
        const float m_new = fmaxf(m_run, wave_max2(a));          // finite: key jb of this wave is valid
        const float p = valid ? expf(a - m_new) : 0.f;
        const float alpha = expf(m_run - m_new);                 // exp(-inf) = 0 on the first pass
        l_run = l_run * alpha + wave_sum2(half == 0 ? p : 0.f);
        m_run = m_new;
        if (half == 0) pw[wave][pairI] = p;
        o *= alpha;
#pragma unroll
        for (int u = 0; u < VL; u++) o += vv[u] * pw[wave][u * KPI + kg];
    }
    *reinterpret_cast<f32x4*>(&opart[wave][kg][vcI * 4]) = o;
    if (lane == 0) { mw[wave] = m_run; lw[wave] = l_run; }
    __syncthreads();
    if (tid < D) {
        const float M = fmaxf(fmaxf(mw[0], mw[1]), fmaxf(mw[2], mw[3]));
        float t = 0.f, l = 0.f;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const float f = expf(mw[w] - M);                     // a wave without keys: exp(-inf) = 0
            float ow = 0.f;
#pragma unroll
            for (int r = 0; r < KPI; r++) ow += opart[w][r][tid];
            t += f * ow;
            l += f * lw[w];
        }
        out[tid] = t;
        if (tid == 0) { out[D] = M; out[D + 1] = l; }
    }
}

// the prompt's K / V rows of one row's prefill into that row's caches
template <typename T>
__global__ void decb_cache_fill_kernel(const T* __restrict__ qkv, float* __restrict__ kcT, float* __restrict__ vc, int P, int E,
                                       int D, int W) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * E) return;
    int t = i / E, e = i % E, h = e / D, d = e % D;
    kcT[(((int64_t)h * (D / 4) + (d >> 2)) * W + t) * 4 + (d & 3)] = to_f32<T>(qkv[(int64_t)t * 3 * E + E + e]);
    vc[((int64_t)h * W + t) * D + d] = to_f32<T>(qkv[(int64_t)t * 3 * E + 2 * E + e]);
}

// Row b = row0 + blockIdx.x: next id from logits row blockIdx.x (stride ldz), then the row's next input embedding.  first: the
// draw from the prefill's last row (the position stays where cmp_decode_batch_begin put it).
__global__ __launch_bounds__(256) void decb_sample_kernel(const float* __restrict__ logits, int ldz, int V, DecRow* __restrict__ st,
                                                          int row0, int32_t* __restrict__ ids, int cap,
                                                          const float* __restrict__ wte, const float* __restrict__ wpe,
                                                          float* __restrict__ x, int E, int W, int first,
                                                          const unsigned* __restrict__ banw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char trunc_lds[];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int tid = threadIdx.x, b = row0 + blockIdx.x;
    const float* z = logits + (int64_t)blockIdx.x * ldz;
    DecRow* rs = st + b;
    if (rs->hold) return;                  // the row's slide draws this step's id (workgroup-uniform); its grammar state stays
    const GramRegs g0 = grammar_read(&rs->gr);          // the grammar state the draw sees: in registers before thread 0 moves it on
    const unsigned ctr = rs->rng;
    const float temperature = rs->temperature;
    const unsigned seed = rs->seed;
    const int pos0 = rs->pos, adv = rs->advance, nprod = rs->produced;
    const int pos = first ? pos0 : (adv ? pos0 + 1 : 0);
    const int posc = min(pos, W - 1);      // host refuses to step past the table; never index outside it
    float* xr = x + (int64_t)b * E;
    const int id = sample_block_grammar(z, V, temperature, rs->top_k, rs->top_p, seed, ctr, bv, bi, trunc_lds, g0, banw);
    if (tid == 0) {
        if (nprod < cap) ids[(int64_t)b * cap + nprod] = id;
        rs->produced = nprod + 1;
        rs->rng = ctr + 1;
        rs->token = id;
        rs->pos = pos;
        grammar_advance(&rs->gr, g0, id);
    }
    for (int e = tid; e < E; e += 256) xr[e] = wte[(int64_t)id * E + e] + wpe[(int64_t)posc * E + e];
}

// ---- sliding window (cmp_decode_batch_begin_slide) ----
// rows rl.row[0 .. nb) sit out the next replay
__global__ void decb_hold_kernel(DecRow* __restrict__ st, DecRowList rl, int nb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb) st[rl.row[i]].hold = 1;
}

// The re-encode input [nb][keep] of the rows rl.row[r0 + blockIdx.y]: the last `keep` tokens of the row's prompt ++ ids, of which
// `produced` ids exist (the same count for every row of the batch).
__global__ void decb_slide_gather_kernel(const int32_t* __restrict__ prompts, const int32_t* __restrict__ plen,
                                         const int32_t* __restrict__ ids, int cap, int W, int produced, int keep, DecRowList rl,
                                         int r0, int32_t* __restrict__ out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= keep) return;
    const int b = rl.row[r0 + blockIdx.y];
    const int P = plen[b];
    const int j = P + produced - keep + g;
    out[(int64_t)blockIdx.y * keep + g] = j < P ? prompts[(int64_t)b * W + j] : ids[(int64_t)b * cap + (j - P)];
}

// decb_cache_fill_kernel for the nb rows of one re-encode: qkv [nb][keep][3E], row blockIdx.y into the caches of rl.row[r0 + blockIdx.y]
template <typename T>
__global__ void decb_slide_fill_kernel(const T* __restrict__ qkv, float* __restrict__ kcT, float* __restrict__ vc, int keep, int E,
                                       int D, int W, DecRowList rl, int r0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= keep * E) return;
    const int b = rl.row[r0 + blockIdx.y];
    const T* q = qkv + (int64_t)blockIdx.y * keep * 3 * E;
    float* kr = kcT + (int64_t)b * W * E;
    float* vr = vc + (int64_t)b * W * E;
    const int t = i / E, e = i % E, h = e / D, d = e % D;
    kr[(((int64_t)h * (D / 4) + (d >> 2)) * W + t) * 4 + (d & 3)] = to_f32<T>(q[(int64_t)t * 3 * E + E + e]);
    vr[((int64_t)h * W + t) * D + d] = to_f32<T>(q[(int64_t)t * 3 * E + 2 * E + e]);
}

// The draw of a slide for row b = rl.row[r0 + blockIdx.x], from the last row of its re-encode (logits [nb][keep][ldz]): as the
// first id of a begin, but the row's draw counter, produced count and seed carry on.  The token is consumed next at position
// `keep`; the logits row goes to where cmp_decode_batch_logits_get reads; the hold is over.
__global__ __launch_bounds__(256) void decb_slide_sample_kernel(const float* __restrict__ logits, int ldz, int V, DecRow* __restrict__ st,
                                                                DecRowList rl, int r0, int32_t* __restrict__ ids, int cap,
                                                                const float* __restrict__ wte, const float* __restrict__ wpe,
                                                                float* __restrict__ x, int E, int keep, float* __restrict__ zout,
                                                                const unsigned* __restrict__ banw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char trunc_lds[];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int tid = threadIdx.x, b = rl.row[r0 + blockIdx.x];
    const float* z = logits + ((int64_t)blockIdx.x * keep + keep - 1) * ldz;
    DecRow* rs = st + b;
    const unsigned ctr = rs->rng;
    const int nprod = rs->produced;
    const GramRegs g0 = grammar_read(&rs->gr);
    const int id = sample_block_grammar(z, V, rs->temperature, rs->top_k, rs->top_p, rs->seed, ctr, bv, bi, trunc_lds, g0, banw);
    __syncthreads();                       // every thread has read the state before thread 0 moves it on
    if (tid == 0) {
        if (nprod < cap) ids[(int64_t)b * cap + nprod] = id;
        rs->produced = nprod + 1;
        rs->rng = ctr + 1;
        rs->token = id;
        rs->pos = keep;
        rs->hold = 0;
        grammar_advance(&rs->gr, g0, id);
    }
    float* xr = x + (int64_t)b * E;
    for (int e = tid; e < E; e += 256) xr[e] = wte[(int64_t)id * E + e] + wpe[(int64_t)keep * E + e];
    float* zo = zout + (int64_t)b * ldz;
    for (int c = tid; c < V; c += 256) zo[c] = z[c];
}

// row b of logits [B][ldz] -> ids_out[b], seed (uint32)(seed + b), draw counter `counter`
__global__ __launch_bounds__(256) void sample_rows_kernel(const float* __restrict__ z, int ldz, int V, float temperature,
                                                          uint64_t seed, unsigned counter, int32_t* __restrict__ ids) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int b = blockIdx.x;
    const int id = sample_block(z + (int64_t)b * ldz, V, temperature, (unsigned)(seed + (uint64_t)b), counter, bv, bi);
    if (threadIdx.x == 0) ids[b] = id;
}
extern "C" int cmp_k_sample_rows(void* stream, const float* logits, int ldz, int B, int V, float temperature, uint64_t seed,
                                 uint32_t counter, int32_t* ids_out) {
    CMP_REQUIRE(logits && ids_out && V > 0 && ldz >= V && B >= 0, "k_sample_rows: bad arguments");
    if (B == 0) return CMP_OK;
    sample_rows_kernel<<<B, 256, 0, (hipStream_t)stream>>>(logits, ldz, V, temperature, seed, counter, ids_out);
    KERNEL_CHECK();
    return CMP_OK;
}

// the same with every row's own (temperature, top_k, top_p), by value in the kernel arguments like DecRowList
struct SampleRowParams {
    float temperature[DECB_MAX_ROWS];
    int top_k[DECB_MAX_ROWS];
    float top_p[DECB_MAX_ROWS];
};
__global__ __launch_bounds__(256) void sample_rows_ex_kernel(const float* __restrict__ z, int ldz, int V, SampleRowParams sp,
                                                             uint64_t seed, unsigned counter, int32_t* __restrict__ ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char trunc_lds[];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int b = blockIdx.x;
    const int id = sample_block_any(z + (int64_t)b * ldz, V, sp.temperature[b], sp.top_k[b], sp.top_p[b],
                                    (unsigned)(seed + (uint64_t)b), counter, bv, bi, trunc_lds);
    if (threadIdx.x == 0) ids[b] = id;
}
extern "C" int cmp_k_sample_rows_ex(void* stream, const float* logits, int ldz, int B, int V, const float* temperature,
                                    const int32_t* top_k, const float* top_p, uint64_t seed, uint32_t counter, int32_t* ids_out) {
    CMP_REQUIRE(logits && ids_out && V > 0 && ldz >= V && B >= 0, "k_sample_rows_ex: bad arguments");
    CMP_REQUIRE(B <= DECB_MAX_ROWS, "k_sample_rows_ex: B=%d rows; at most %d", B, DECB_MAX_ROWS);
    SampleRowParams sp = {};
    for (int b = 0; b < B; b++) {
        sp.temperature[b] = temperature ? temperature[b] : 1.0f;
        sp.top_k[b] = top_k ? top_k[b] : 0;
        sp.top_p[b] = top_p ? top_p[b] : 1.0f;
        CHECK_RC(sampling_check("k_sample_rows_ex", V, sp.temperature[b], sp.top_k[b], sp.top_p[b]));
    }
    if (B == 0) return CMP_OK;
    sample_rows_ex_kernel<<<B, 256, trunc_lds_bytes(V), (hipStream_t)stream>>>(logits, ldz, V, sp, seed, counter, ids_out);
    KERNEL_CHECK();
    return CMP_OK;
}

// -------------------------------------------------------------------------------------------------
static int launch_proj(hipStream_t s, int act, int in_mode, const float* x, const float* g, const float* b, float eps,
                       const float* Wt, const float* bias, const float* resid, float* y, int ldy, float* u_out, int K, int N,
                       int D, int B) {
    CMP_REQUIRE(K % 4 == 0 && D % 4 == 0, "decode_batch: K=%d / D=%d must be multiples of 4", K, D);
    const dim3 grid(cdiv(N, 16), cdiv(B, 16));
    const size_t smem = in_mode == 2 ? (size_t)16 * (K / D) * ATT_SPLITS * 4 : 0;
#define PJ(A, I) decb_proj_kernel<A, I><<<grid, 256, smem, s>>>(x, g, b, eps, Wt, bias, resid, y, ldy, u_out, K, N, D, B)
    if (act == 1) { if (in_mode == 1) PJ(1, 1); else if (in_mode == 2) PJ(1, 2); else PJ(1, 0); }
    else { if (in_mode == 1) PJ(0, 1); else if (in_mode == 2) PJ(0, 2); else PJ(0, 0); }
#undef PJ
    KERNEL_CHECK();
    return CMP_OK;
}

static int launch_attn(hipStream_t s, cmp_model* m, DecodeBatchState* d, const DecBatchLayerW& w, float scale, int B) {
    dim3 grid(m->H, ATT_SPLITS, B);
    switch (m->D) {
        case 16: decb_attn_kernel<16><<<grid, 256, 0, s>>>(d->qkv, w.kc, w.vc, d->att, d->st, m->Ea, m->W, scale); break;
        case 32: decb_attn_kernel<32><<<grid, 256, 0, s>>>(d->qkv, w.kc, w.vc, d->att, d->st, m->Ea, m->W, scale); break;
        case 64: decb_attn_kernel<64><<<grid, 256, 0, s>>>(d->qkv, w.kc, w.vc, d->att, d->st, m->Ea, m->W, scale); break;
        case 128: decb_attn_kernel<128><<<grid, 256, 0, s>>>(d->qkv, w.kc, w.vc, d->att, d->st, m->Ea, m->W, scale); break;
        default: CMP_REQUIRE(false, "decode_batch attention: head size %d has no kernel (16, 32, 64, 128)", m->D);
    }
    KERNEL_CHECK();
    return CMP_OK;
}

// one token for every row: consumes d->x (row b: embedding of its token at its position), produces the next ids and d->x
static int enqueue_batch_step(cmp_model* m, DecodeBatchState* d, int B) {
    hipStream_t s = m->ctx->stream;
    const int E = m->E, Ea = m->Ea, L = m->L;
    const bool ln = m->cfg.use_layer_norm != 0;
    const float eps = m->cfg.ln_eps;
    const float scale = m->cfg.scale_attention ? 1.0f / sqrtf((float)m->Dl) : 1.0f;
    for (int i = 0; i < L; i++) {
        const LayerOff& o = m->lo[i];
        const DecBatchLayerW& w = d->lw[i];
        CHECK_RC(launch_proj(s, 0, ln ? 1 : 0, d->x, m->P + o.ln1_g, m->P + o.ln1_b, eps, w.attn_wT, m->P + o.attn_b, nullptr,
                             d->qkv, 3 * Ea, d->u, E, 3 * Ea, m->D, B));
        CHECK_RC(launch_attn(s, m, d, w, scale, B));
        CHECK_RC(launch_proj(s, 0, 2, d->att, nullptr, nullptr, eps, w.proj_wT, m->P + o.proj_b, d->u, d->r, E, nullptr, Ea, E,
                             m->D, B));
        CHECK_RC(launch_proj(s, 1, ln ? 1 : 0, d->r, m->P + o.ln2_g, m->P + o.ln2_b, eps, w.fc_wT, m->P + o.fc_b, nullptr, d->g,
                             4 * E, nullptr, E, 4 * E, m->D, B));
        CHECK_RC(launch_proj(s, 0, 0, d->g, nullptr, nullptr, eps, w.pr_wT, m->P + o.pr_b, d->r, d->x, E, nullptr, 4 * E, E, m->D,
                             B));
    }
    CHECK_RC(launch_proj(s, 0, 1, d->x, m->P + m->off_lnf_g, m->P + m->off_lnf_b, eps, m->P + m->off_wte, nullptr, nullptr,
                         d->logits, m->ldz, nullptr, E, m->V, m->D, B));
    decb_sample_kernel<<<B, 256, trunc_lds_bytes(m->V), s>>>(d->logits, m->ldz, m->V, d->st, 0, d->ids, d->cap, m->P + m->off_wte, m->P + m->off_wpe,
                                         d->x, E, m->W, 0, d->banw);
    KERNEL_CHECK();
    return CMP_OK;
}

static int decb_alloc_rows(cmp_model* m, DecodeBatchState* d, int B) {
    decb_free_rows(d);
    const int E = m->E, Ea = m->Ea, W = m->W;
    const size_t Bz = (size_t)B;
    std::vector<void*>& al = d->row_allocs;
    CHECK_RC(balloc(al, &d->st, Bz * sizeof(DecRow)));
    CHECK_RC(balloc(al, &d->ids, Bz * d->cap * 4));
    CHECK_RC(balloc(al, &d->x, Bz * E * 4));
    CHECK_RC(balloc(al, &d->u, Bz * E * 4));
    CHECK_RC(balloc(al, &d->qkv, Bz * 3 * Ea * 4));
    CHECK_RC(balloc(al, &d->att, Bz * m->H * ATT_SPLITS * PSTRIDE(m->D) * 4));
    CHECK_RC(balloc(al, &d->r, Bz * E * 4));
    CHECK_RC(balloc(al, &d->g, Bz * 4 * E * 4));
    CHECK_RC(balloc(al, &d->logits, Bz * m->ldz * 4));
    CHECK_RC(balloc(al, &d->prompts, Bz * W * 4));
    CHECK_RC(balloc(al, &d->plen, Bz * 4));
    for (auto& w : d->lw) {
        CHECK_RC(balloc(al, &w.kc, Bz * W * Ea * 4));
        CHECK_RC(balloc(al, &w.vc, Bz * W * Ea * 4));
    }
    d->capB = B;
    return CMP_OK;
}

// keep > 0: sliding-window mode (cmp_decode_batch_begin_slide), kv mode otherwise unchanged
// temperature / top_k / top_p: host arrays of B entries, or null for `temperature0` / off in every row
static int decode_batch_begin_impl(cmp_model* m, const int32_t* prompts, const int32_t* lens, int B, int ld, int mode,
                                   float temperature0, const float* temperature, const int32_t* top_k, const float* top_p,
                                   uint64_t seed, int keep) {
    CMP_REQUIRE(m && prompts && lens, "decode_batch_begin: null argument");
    CMP_REQUIRE(B >= 1 && B <= DECB_MAX_ROWS, "decode_batch_begin: B=%d rows; 1 <= B <= %d", B, DECB_MAX_ROWS);
    for (int b = 0; b < B; b++)
        CHECK_RC(sampling_check("decode_batch_begin", m->V, temperature ? temperature[b] : temperature0, top_k ? top_k[b] : 0,
                                top_p ? top_p[b] : 1.0f));
    CMP_REQUIRE(mode == CMP_DECODE_LITERAL || mode == CMP_DECODE_KV, "decode_batch_begin: bad mode %d", mode);
    CMP_REQUIRE(ld >= 1, "decode_batch_begin: leading dimension %d", ld);
    for (int b = 0; b < B; b++) {
        CMP_REQUIRE(lens[b] >= 1, "decode_batch_begin: row %d is empty", b);
        CMP_REQUIRE(lens[b] <= ld, "decode_batch_begin: row %d: length %d exceeds the leading dimension %d", b, lens[b], ld);
        CMP_REQUIRE(lens[b] <= m->W, "decode_batch_begin: row %d: prompt length %d exceeds window_size %d", b, lens[b], m->W);
        for (int i = 0; i < lens[b]; i++) {
            const int v = prompts[(int64_t)b * ld + i];
            CMP_REQUIRE(v >= 0 && v < m->V, "decode_batch_begin: row %d: prompt id %d out of range [0,%d)", b, v, m->V);
        }
    }
    HIP_CHECK(hipSetDevice(m->ctx->device));
    hipStream_t s = m->ctx->stream;
    if (keep > 0) {
        // the workspace never grows after its first sizing: a slide re-encodes `keep` tokens per row through it, so it is sized
        // (or found too small) here, before any id is produced
        int maxP = 1;
        for (int b = 0; b < B; b++) maxP = std::max(maxP, lens[b]);
        CHECK_RC(ensure_workspace(m, 1, std::max(maxP, keep)));
    }
    const bool graph_on = [] { const char* e = getenv("COMPOSER_NO_GRAPH"); return !(e && e[0] == '1'); }();
    DecodeBatchState* d = m->decb;
    if (!d) {
        d = new DecodeBatchState();
        m->decb = d;
        d->cap = 1 << 16;
    }
    d->begun = false;
    const int E = m->E, Ea = m->Ea, L = m->L, W = m->W;
    if (d->lw.empty()) {
        d->lw.resize(L);
        for (auto& w : d->lw) {
            CHECK_RC(balloc(d->w_allocs, &w.attn_wT, (size_t)3 * Ea * E * 4));
            CHECK_RC(balloc(d->w_allocs, &w.proj_wT, (size_t)Ea * E * 4));
            CHECK_RC(balloc(d->w_allocs, &w.fc_wT, (size_t)4 * E * E * 4));
            CHECK_RC(balloc(d->w_allocs, &w.pr_wT, (size_t)4 * E * E * 4));
            w.kc = w.vc = nullptr;
        }
    }
    if (!d->banw) CHECK_RC(balloc(d->w_allocs, &d->banw, (size_t)grammar_words(m->V) * 4));
    if (d->graph_on != graph_on) {
        HIP_CHECK(hipStreamSynchronize(s));
        decb_drop_graphs(d);
        d->graph_on = graph_on;
    }
    if (B > d->capB) {                          // the captured chains hold the old buffers: they go with them
        HIP_CHECK(hipStreamSynchronize(s));
        const int rc = decb_alloc_rows(m, d, B);
        if (rc != CMP_OK) { decb_free_rows(d); return rc; }
    }
    if (d->weights_version != m->param_version) {
        for (int i = 0; i < L; i++) {
            const LayerOff& o = m->lo[i];
            DecBatchLayerW& w = d->lw[i];
            auto tr = [&](const float* in, float* out, int K, int N) {
                dim3 grid(cdiv(N, 32), cdiv(K, 32));
                decb_transpose_kernel<<<grid, 256, 0, s>>>(in, out, K, N);
            };
            tr(m->P + o.attn_w, w.attn_wT, E, 3 * Ea);
            tr(m->P + o.proj_w, w.proj_wT, Ea, E);
            tr(m->P + o.fc_w, w.fc_wT, E, 4 * E);
            tr(m->P + o.pr_w, w.pr_wT, 4 * E, E);
            KERNEL_CHECK();
        }
        d->weights_version = m->param_version;
    }
    std::vector<DecRow> h(B, DecRow{});
    d->pos.assign(B, 0);
    for (int b = 0; b < B; b++) {
        h[b].pos = (mode == CMP_DECODE_KV) ? lens[b] : 0;     // position of the row's first generated token when it is fed back
        h[b].token = 0;
        h[b].produced = 0;
        h[b].advance = (mode == CMP_DECODE_KV) ? 1 : 0;
        h[b].rng = 0;
        h[b].seed = (unsigned)(seed + (uint64_t)b);
        h[b].temperature = temperature ? temperature[b] : temperature0;
        h[b].hold = 0;
        h[b].top_k = top_k ? top_k[b] : 0;
        h[b].top_p = top_p ? top_p[b] : 1.0f;
        h[b].gr = grammar_begin(m->gram[1], prompts + (int64_t)b * ld, lens[b]);
        d->pos[b] = h[b].pos;
    }
    d->keep = keep;
    d->row_slides = d->fwd_calls = 0;
    HIP_CHECK(grammar_upload(m->gram[1], m->V, d->banw, s));
    HIP_CHECK(hipMemcpyAsync(d->st, h.data(), (size_t)B * sizeof(DecRow), hipMemcpyHostToDevice, s));
    if (keep > 0) HIP_CHECK(hipMemcpyAsync(d->plen, lens, (size_t)B * 4, hipMemcpyHostToDevice, s));
    // prefill, one row at a time through the batch-1 path's forward call; the host prompt upload is stream-ordered, so the
    // stream is drained before the next row's ids overwrite the staging buffer
    for (int b = 0; b < B; b++) {
        const int P = lens[b];
        CHECK_RC(ensure_workspace(m, 1, P));
        HIP_CHECK(hipMemcpyAsync(m->x_dev, prompts + (int64_t)b * ld, (size_t)P * 4, hipMemcpyHostToDevice, s));
        if (keep > 0) HIP_CHECK(hipMemcpyAsync(d->prompts + (int64_t)b * W, m->x_dev, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
        CHECK_RC(model_forward(m, m->x_dev, 1, P, false, 0));
        if (mode == CMP_DECODE_KV) {
            for (int i = 0; i < L; i++) {
                float* kc = d->lw[i].kc + (int64_t)b * W * Ea;
                float* vc = d->lw[i].vc + (int64_t)b * W * Ea;
                const int grid = cdiv(P * Ea, 256);
                if (m->dtype == CMP_BF16)
                    decb_cache_fill_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)m->act[i].qkv, kc, vc, P, Ea, m->D, W);
                else
                    decb_cache_fill_kernel<float><<<grid, 256, 0, s>>>((const float*)m->act[i].qkv, kc, vc, P, Ea, m->D, W);
                KERNEL_CHECK();
            }
        }
        // first id from the row's last prompt position (cli.py:673 `[-1, 0]`), seed + b, draw counter 0
        decb_sample_kernel<<<1, 256, trunc_lds_bytes(m->V), s>>>(m->logits + (int64_t)(P - 1) * m->ldz, m->ldz, m->V, d->st, b, d->ids, d->cap,
                                             m->P + m->off_wte, m->P + m->off_wpe, d->x, E, W, 1, d->banw);
        KERNEL_CHECK();
        HIP_CHECK(hipStreamSynchronize(s));
    }
    d->B = B;
    d->mode = mode;
    d->produced = 1;
    d->returned = 0;
    if (graph_on && !d->graphs.count(B)) {      // the per-token chain, captured once per B on one linear stream
        HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue_batch_step(m, d, B);
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(s, &g);
        if (rc != CMP_OK) { if (g) hipGraphDestroy(g); return rc; }
        HIP_CHECK(e);
        hipGraphExec_t ex = nullptr;
        hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        if (ei != hipSuccess) hipGraphDestroy(g);
        HIP_CHECK(ei);
        d->graphs[B] = {g, ex};
    }
    d->begun = true;
    return CMP_OK;
}

extern "C" int cmp_decode_batch_begin(cmp_model* m, const int32_t* prompts, const int32_t* lens, int B, int ld, int mode,
                                      float temperature, uint64_t seed) {
    return decode_batch_begin_impl(m, prompts, lens, B, ld, mode, temperature, nullptr, nullptr, nullptr, seed, 0);
}

// every begin of the batched chain with per-row sampling parameters: keep = 0 is cmp_decode_batch_begin, keep > 0 (kv mode only)
// cmp_decode_batch_begin_slide; a null array is the default for every row (temperature 1, top_k 0, top_p 1)
extern "C" int cmp_decode_batch_begin_ex(cmp_model* m, const int32_t* prompts, const int32_t* lens, int B, int ld, int mode,
                                         int keep, const float* temperature, const int32_t* top_k, const float* top_p,
                                         uint64_t seed) {
    CMP_REQUIRE(m, "decode_batch_begin_ex: null model");
    if (keep != 0) {
        CMP_REQUIRE(mode == CMP_DECODE_KV, "decode_batch_begin_ex: keep=%d goes with CMP_DECODE_KV", keep);
        CMP_REQUIRE(keep >= 1 && keep <= m->W - 1, "decode_batch_begin_ex: keep=%d outside [1, window_size - 1 = %d]", keep, m->W - 1);
    }
    return decode_batch_begin_impl(m, prompts, lens, B, ld, mode, 1.0f, temperature, top_k, top_p, seed, keep);
}

extern "C" int cmp_decode_batch_begin_slide(cmp_model* m, const int32_t* prompts, const int32_t* lens, int B, int ld, int keep,
                                            float temperature, uint64_t seed) {
    CMP_REQUIRE(m, "decode_batch_begin_slide: null model");
    CMP_REQUIRE(keep >= 1 && keep <= m->W - 1, "decode_batch_begin_slide: keep=%d outside [1, window_size - 1 = %d]", keep, m->W - 1);
    return decode_batch_begin_impl(m, prompts, lens, B, ld, CMP_DECODE_KV, temperature, nullptr, nullptr, nullptr, seed, keep);
}

// The slide of the nb rows of rl (all at pos == W, held during the replay just enqueued): their tails go through the forward pass
// together, as many rows per call as the workspace holds.  An fp32 forward is the same arithmetic per row whatever rows share the
// call (one GEMM kernel, no split-K, per-row attention and LayerNorm); the bf16 forward picks its GEMM kernels by the token
// count, so a bf16 model re-encodes one row per call, as its prefill does, and a row stays independent of its neighbours.
static int enqueue_batch_slide(cmp_model* m, DecodeBatchState* d, const DecRowList& rl, int nb) {
    hipStream_t s = m->ctx->stream;
    const int keep = d->keep, Ea = m->Ea, W = m->W;
    const int64_t ws_rows = ((int64_t)m->capB * m->capT) / keep;
    const int per = m->dtype == CMP_BF16 ? 1 : (int)std::max<int64_t>(1, std::min<int64_t>(ws_rows, nb));
    for (int r0 = 0; r0 < nb; r0 += per) {
        const int nc = std::min(per, nb - r0);
        decb_slide_gather_kernel<<<dim3(cdiv(keep, 256), nc), 256, 0, s>>>(d->prompts, d->plen, d->ids, d->cap, W, d->produced, keep, rl,
                                                                          r0, m->x_dev);
        KERNEL_CHECK();
        CHECK_RC(model_forward(m, m->x_dev, nc, keep, false, 0));
        for (int i = 0; i < m->L; i++) {
            const dim3 grid(cdiv(keep * Ea, 256), nc);
            if (m->dtype == CMP_BF16)
                decb_slide_fill_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)m->act[i].qkv, d->lw[i].kc, d->lw[i].vc, keep, Ea, m->D, W, rl, r0);
            else
                decb_slide_fill_kernel<float><<<grid, 256, 0, s>>>((const float*)m->act[i].qkv, d->lw[i].kc, d->lw[i].vc, keep, Ea, m->D, W, rl, r0);
            KERNEL_CHECK();
        }
        decb_slide_sample_kernel<<<nc, 256, trunc_lds_bytes(m->V), s>>>(m->logits, m->ldz, m->V, d->st, rl, r0, d->ids, d->cap, m->P + m->off_wte,
                                                    m->P + m->off_wpe, d->x, m->E, keep, d->logits, d->banw);
        KERNEL_CHECK();
        d->fwd_calls++;
    }
    d->row_slides += nb;
    return CMP_OK;
}

int decode_batch_slide_stats(DecodeBatchState* d, int64_t* row_slides, int64_t* forward_calls) {
    if (!d || !d->begun) {
        cmp_set_error("decode_slide_stats: call cmp_decode_batch_begin first");
        return CMP_ERR_STATE;
    }
    *row_slides = d->row_slides;
    *forward_calls = d->fwd_calls;
    return CMP_OK;
}

int decode_batch_grammar_state(cmp_model* m, int row, uint32_t sounding[4], int32_t* pedal, int64_t* time_steps) {
    DecodeBatchState* d = m->decb;
    if (!d || !d->begun) {
        cmp_set_error("decode_grammar_state: call cmp_decode_batch_begin first");
        return CMP_ERR_STATE;
    }
    CMP_REQUIRE(row >= 0 && row < d->B, "decode_grammar_state: row %d outside the batch of %d rows", row, d->B);
    HIP_CHECK(hipSetDevice(m->ctx->device));
    HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
    DecRow h;
    HIP_CHECK(hipMemcpy(&h, d->st + row, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; i++) sounding[i] = h.gr.sounding[i];
    *pedal = h.gr.pedal;
    *time_steps = h.gr.time_steps;
    return CMP_OK;
}

extern "C" int cmp_decode_batch_steps(cmp_model* m, int n, int32_t* ids_out) {
    CMP_REQUIRE(m && n >= 0 && (ids_out || n == 0), "decode_batch_steps: bad arguments");
    DecodeBatchState* d = m->decb;
    if (!d || !d->begun) {
        cmp_set_error("decode_batch_steps: call cmp_decode_batch_begin first");
        return CMP_ERR_STATE;
    }
    HIP_CHECK(hipSetDevice(m->ctx->device));
    hipStream_t s = m->ctx->stream;
    const int B = d->B;
    const int need = d->returned + n;
    CMP_REQUIRE(need <= d->cap, "decode_batch_steps: more than %d ids per row per decode_batch_begin", d->cap);
    auto it = d->graphs.find(B);
    hipGraphExec_t ex = (d->graph_on && it != d->graphs.end()) ? it->second.second : nullptr;
    // kv mode: refused before any step runs, so a refused call consumes nothing (the last step consumes position pos + todo - 1)
    const int todo = std::max(0, need - d->produced);
    if (d->mode == CMP_DECODE_KV && d->keep == 0 && todo > 0)
        for (int b = 0; b < B; b++)
            CMP_REQUIRE(d->pos[b] + todo - 1 < m->W, "decode_batch_steps: row %d: position %d outside the wpe table (window_size %d): "
                        "prompt_len + length - 1 must be <= window_size in kv-cache mode", b, d->pos[b] + todo - 1, m->W);
    while (d->produced < need) {
        if (d->keep > 0) {
            // rows whose cache is full draw this step's id from a re-encode of their tail; they sit out the replay, which
            // still runs all B rows (one capture per B).  When every row slides there is nothing to replay.
            DecRowList rl = {};
            int nb = 0;
            for (int b = 0; b < B; b++)
                if (d->pos[b] >= m->W) rl.row[nb++] = (unsigned char)b;
            if (nb > 0) {
                if (nb < B) {
                    decb_hold_kernel<<<1, DECB_MAX_ROWS, 0, s>>>(d->st, rl, nb);
                    KERNEL_CHECK();
                    if (ex) HIP_CHECK(hipGraphLaunch(ex, s));
                    else CHECK_RC(enqueue_batch_step(m, d, B));
                }
                CHECK_RC(enqueue_batch_slide(m, d, rl, nb));
                for (int b = 0; b < B; b++) d->pos[b]++;
                for (int i = 0; i < nb; i++) d->pos[rl.row[i]] = d->keep;
                d->produced++;
                continue;
            }
        }
        if (ex) HIP_CHECK(hipGraphLaunch(ex, s));
        else CHECK_RC(enqueue_batch_step(m, d, B));
        d->produced++;
        if (d->mode == CMP_DECODE_KV)
            for (int b = 0; b < B; b++) d->pos[b]++;
    }
    if (n > 0)
        HIP_CHECK(hipMemcpy2DAsync(ids_out, (size_t)n * 4, d->ids + d->returned, (size_t)d->cap * 4, (size_t)n * 4, B,
                                   hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    d->returned = need;
    return CMP_OK;
}

// The logits the most recent per-token step drew every row's id from (d->logits [B][ldz], padding stripped): host fp32 [B][V].
// Read-only, outside the per-token chain; nothing to read before the first step has run (the first ids come from the prefills).
extern "C" int cmp_decode_batch_logits_get(cmp_model* m, float* host_out) {
    CMP_REQUIRE(m && host_out, "decode_batch_logits_get: null argument");
    DecodeBatchState* d = m->decb;
    if (!d || !d->begun) {
        cmp_set_error("decode_batch_logits_get: call cmp_decode_batch_begin first");
        return CMP_ERR_STATE;
    }
    if (d->produced < 2) {
        cmp_set_error("decode_batch_logits_get: no per-token step has run yet (the first ids are drawn from the prefills' logits)");
        return CMP_ERR_STATE;
    }
    HIP_CHECK(hipSetDevice(m->ctx->device));
    HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
    HIP_CHECK(hipMemcpy2D(host_out, (size_t)m->V * 4, d->logits, (size_t)m->ldz * 4, (size_t)m->V * 4, d->B, hipMemcpyDeviceToHost));
    return CMP_OK;
}
