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
// State lives apart from the batch-1 DecodeState (m->dec): own transposed weights, buffers, KV caches and captured chains.  What
// surrounds the chain -- row state, prefill of a row, slide, checks, capture -- is decode.hip's, shared through decode_common.h.
#include "model.h"
#include "decode_common.h"

static void decb_drop_graphs(DecodeBatchState* d) {
    for (auto& kv : d->graphs) {
        if (kv.second.second) hipGraphExecDestroy(kv.second.second);
        if (kv.second.first) hipGraphDestroy(kv.second.first);
    }
    d->graphs.clear();
}

void decode_batch_state_free(DecodeBatchState* d) {
    if (!d) return;
    decb_drop_graphs(d);
    dec_rows_free(d->rows);
    for (void* p : d->w.allocs) hipFree(p);
    delete d;
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

// Row b = row0 + blockIdx.x: next id from logits row blockIdx.x (stride ldz), then the row's next input embedding.  first: the
// draw from the prefill's last row (the position stays where cmp_decode_batch_begin put it).
__global__ __launch_bounds__(256) void decb_sample_kernel(const float* __restrict__ logits, int ldz, int V, DecRow* __restrict__ st,
                                                          int row0, int32_t* __restrict__ ids, int cap,
                                                          const float* __restrict__ wte, const float* __restrict__ wpe,
                                                          float* __restrict__ x, int E, int W, int first,
                                                          const unsigned* __restrict__ banw, int ban_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char trunc_lds[];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int tid = threadIdx.x, b = row0 + blockIdx.x;
    banw += (int64_t)b * ban_stride;       // a guarded chain: the row's own words (stride 0: the chain's static words)
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
    const int id = sample_block_grammar(z, V, temperature, rs->top_k, rs->top_p, seed, ctr, bv, bi, trunc_lds, g0, &rs->bd, banw);
    if (tid == 0) {
        if (nprod < cap) ids[(int64_t)b * cap + nprod] = id;
        rs->produced = nprod + 1;
        rs->rng = ctr + 1;
        rs->token = id;
        rs->pos = pos;
        grammar_advance(&rs->gr, &rs->bd, g0, id, nprod + 1);
    }
    for (int e = tid; e < E; e += 256) xr[e] = wte[(int64_t)id * E + e] + wpe[(int64_t)posc * E + e];
}

// sliding window (cmp_decode_batch_begin_slide): rows rl.row[0 .. nb) sit out the next replay
__global__ void decb_hold_kernel(DecRow* __restrict__ st, DecRowList rl, int nb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb) st[rl.row[i]].hold = 1;
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

static int launch_attn(hipStream_t s, cmp_model* m, const DecRows& R, int layer, float scale, int B) {
    dim3 grid(m->H, ATT_SPLITS, B);
    float *kc = R.kc[layer], *vc = R.vc[layer];
    switch (m->D) {
        case 16: decb_attn_kernel<16><<<grid, 256, 0, s>>>(R.qkv, kc, vc, R.att, R.st, m->Ea, m->W, scale); break;
        case 32: decb_attn_kernel<32><<<grid, 256, 0, s>>>(R.qkv, kc, vc, R.att, R.st, m->Ea, m->W, scale); break;
        case 64: decb_attn_kernel<64><<<grid, 256, 0, s>>>(R.qkv, kc, vc, R.att, R.st, m->Ea, m->W, scale); break;
        case 128: decb_attn_kernel<128><<<grid, 256, 0, s>>>(R.qkv, kc, vc, R.att, R.st, m->Ea, m->W, scale); break;
        default: CMP_REQUIRE(false, "decode_batch attention: head size %d has no kernel (16, 32, 64, 128)", m->D);
    }
    KERNEL_CHECK();
    return CMP_OK;
}

int decb_launch_sample(cmp_model* m, DecRows& R, const DecWeights& w, const float* logits, int nrows, int row0, int first) {
    decb_sample_kernel<<<nrows, 256, trunc_lds_bytes(m->V), m->ctx->stream>>>(logits, m->ldz, m->V, R.st, row0, R.ids, R.cap, m->P + m->off_wte,
                                                                            m->P + m->off_wpe, R.x, m->E, m->W, first, dec_ban_words(R, w),
                                                                            dec_ban_stride(m, R));
    KERNEL_CHECK();
    return CMP_OK;
}

// one token for every row: consumes R.x (row b: embedding of its token at its position), produces the next ids and R.x
static int enqueue_batch_step(cmp_model* m, DecodeBatchState* d, int B) {
    hipStream_t s = m->ctx->stream;
    DecRows& R = d->rows;
    const int E = m->E, Ea = m->Ea, L = m->L;
    const bool ln = m->cfg.use_layer_norm != 0;
    const float eps = m->cfg.ln_eps;
    const float scale = m->cfg.scale_attention ? 1.0f / sqrtf((float)m->Dl) : 1.0f;
    for (int i = 0; i < L; i++) {
        const LayerOff& o = m->lo[i];
        const DecLayerW& w = d->w.lw[i];
        CHECK_RC(launch_proj(s, 0, ln ? 1 : 0, R.x, m->P + o.ln1_g, m->P + o.ln1_b, eps, w.attn_wT, m->P + o.attn_b, nullptr,
                             R.qkv, 3 * Ea, R.u, E, 3 * Ea, m->D, B));
        CHECK_RC(launch_attn(s, m, R, i, scale, B));
        CHECK_RC(launch_proj(s, 0, 2, R.att, nullptr, nullptr, eps, w.proj_wT, m->P + o.proj_b, R.u, R.r, E, nullptr, Ea, E,
                             m->D, B));
        CHECK_RC(launch_proj(s, 1, ln ? 1 : 0, R.r, m->P + o.ln2_g, m->P + o.ln2_b, eps, w.fc_wT, m->P + o.fc_b, nullptr, R.g,
                             4 * E, nullptr, E, 4 * E, m->D, B));
        CHECK_RC(launch_proj(s, 0, 0, R.g, nullptr, nullptr, eps, w.pr_wT, m->P + o.pr_b, R.r, R.x, E, nullptr, 4 * E, E, m->D,
                             B));
    }
    CHECK_RC(launch_proj(s, 0, 1, R.x, m->P + m->off_lnf_g, m->P + m->off_lnf_b, eps, m->P + m->off_wte, nullptr, nullptr,
                         R.logits, m->ldz, nullptr, E, m->V, m->D, B));
    CHECK_RC(dec_enqueue_guard(m, R, d->w, DecRowList{}, -1, 0, B));
    return decb_launch_sample(m, R, d->w, R.logits, B, 0, 0);
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
        CHECK_RC(dec_check_prompt("decode_batch_begin", b, prompts + (int64_t)b * ld, lens[b], m->V, m->W));
    }
    CHECK_RC(dec_check_budget("decode_batch_begin", m->gram[1], m->budget[1]));
    HIP_CHECK(hipSetDevice(m->ctx->device));
    hipStream_t s = m->ctx->stream;
    if (keep > 0) {
        // the workspace never grows after its first sizing: a slide re-encodes `keep` tokens per row through it, so it is sized
        // (or found too small) here, before any id is produced
        int maxP = 1;
        for (int b = 0; b < B; b++) maxP = std::max(maxP, lens[b]);
        CHECK_RC(ensure_workspace(m, 1, std::max(maxP, keep)));
    }
    const bool graph_on = dec_graph_enabled();
    DecodeBatchState* d = m->decb;
    if (!d) m->decb = d = new DecodeBatchState();
    DecRows& R = d->rows;
    R.begun = false;
    if (d->graph_on != graph_on) {
        HIP_CHECK(hipStreamSynchronize(s));
        decb_drop_graphs(d);
        d->graph_on = graph_on;
    }
    if (d->guard_epoch != m->guard[1].epoch) {  // a guard attached or detached since: the chains are captured again, with or without the scan
        HIP_CHECK(hipStreamSynchronize(s));
        decb_drop_graphs(d);
        d->guard_epoch = m->guard[1].epoch;
    }
    if (B > R.capB) {                           // the captured chains hold the old buffers: they go with them
        HIP_CHECK(hipStreamSynchronize(s));
        decb_drop_graphs(d);
        const int rc = dec_rows_alloc(m, R, B);
        if (rc != CMP_OK) { dec_rows_free(R); return rc; }
    }
    CHECK_RC(dec_weights_refresh(m, d->w));
    R.mode = mode;
    R.keep = keep;
    R.row_slides = R.fwd_calls = 0;
    R.guard = m->guard[1];
    std::vector<DecRow> h(B);
    d->pos.assign(B, 0);
    for (int b = 0; b < B; b++) {
        h[b] = dec_row_init(mode, lens[b], (unsigned)(seed + (uint64_t)b), temperature ? temperature[b] : temperature0,
                            top_k ? top_k[b] : 0, top_p ? top_p[b] : 1.0f, m->gram[1], m->budget[1], prompts + (int64_t)b * ld,
                            R.guard.on());
        d->pos[b] = h[b].pos;
    }
    HIP_CHECK(grammar_upload(m->gram[1], m->V, d->w.banw, s));
    HIP_CHECK(hipMemcpyAsync(R.st, h.data(), (size_t)B * sizeof(DecRow), hipMemcpyHostToDevice, s));
    if (keep > 0 || R.guard.on()) HIP_CHECK(hipMemcpyAsync(R.plen, lens, (size_t)B * 4, hipMemcpyHostToDevice, s));
    if (R.guard.on()) HIP_CHECK(hipMemsetAsync(R.cgcount, 0, (size_t)B * 8, s));
    // prefill, one row at a time through the batch-1 chain's own call: a row's first id is the batch-1 first id for seed + b
    for (int b = 0; b < B; b++) CHECK_RC(dec_prefill_row(m, R, d->w, b, prompts + (int64_t)b * ld, lens[b]));
    R.B = B;
    R.produced = 1;
    R.returned = 0;
    if (graph_on && !d->graphs.count(B)) {      // the per-token chain, captured once per B on one linear stream
        hipGraph_t g = nullptr;
        hipGraphExec_t ex = nullptr;
        CHECK_RC(dec_capture(s, [&] { return enqueue_batch_step(m, d, B); }, &g, &ex));
        d->graphs[B] = {g, ex};
    }
    R.begun = true;
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
        CHECK_RC(dec_check_keep("decode_batch_begin_ex", keep, m->W));
    }
    return decode_batch_begin_impl(m, prompts, lens, B, ld, mode, 1.0f, temperature, top_k, top_p, seed, keep);
}

extern "C" int cmp_decode_batch_begin_slide(cmp_model* m, const int32_t* prompts, const int32_t* lens, int B, int ld, int keep,
                                            float temperature, uint64_t seed) {
    CMP_REQUIRE(m, "decode_batch_begin_slide: null model");
    CHECK_RC(dec_check_keep("decode_batch_begin_slide", keep, m->W));
    return decode_batch_begin_impl(m, prompts, lens, B, ld, CMP_DECODE_KV, temperature, nullptr, nullptr, nullptr, seed, keep);
}

extern "C" int cmp_decode_batch_steps(cmp_model* m, int n, int32_t* ids_out) {
    CMP_REQUIRE(m && n >= 0 && (ids_out || n == 0), "decode_batch_steps: bad arguments");
    DecodeBatchState* d = m->decb;
    CHECK_RC(dec_require_begun("decode_batch_steps", d && d->rows.begun, "cmp_decode_batch_begin"));
    DecRows& R = d->rows;
    HIP_CHECK(hipSetDevice(m->ctx->device));
    hipStream_t s = m->ctx->stream;
    const int B = R.B;
    const int need = R.returned + n;
    CMP_REQUIRE(need <= R.cap, "decode_batch_steps: more than %d ids per row per decode_batch_begin", R.cap);
    auto it = d->graphs.find(B);
    hipGraphExec_t ex = (d->graph_on && it != d->graphs.end()) ? it->second.second : nullptr;
    // kv mode: refused before any step runs, so a refused call consumes nothing (the last step consumes position pos + todo - 1)
    const int todo = std::max(0, need - R.produced);
    if (R.mode == CMP_DECODE_KV && R.keep == 0 && todo > 0)
        for (int b = 0; b < B; b++)
            CMP_REQUIRE(d->pos[b] + todo - 1 < m->W, "decode_batch_steps: row %d: position %d outside the wpe table (window_size %d): "
                        "prompt_len + length - 1 must be <= window_size in kv-cache mode", b, d->pos[b] + todo - 1, m->W);
    while (R.produced < need) {
        if (R.keep > 0) {
            // rows whose cache is full draw this step's id from a re-encode of their tail; they sit out the replay, which
            // still runs all B rows (one capture per B).  When every row slides there is nothing to replay.
            DecRowList rl = {};
            int nb = 0;
            for (int b = 0; b < B; b++)
                if (d->pos[b] >= m->W) rl.row[nb++] = (unsigned char)b;
            if (nb > 0) {
                if (nb < B) {
                    decb_hold_kernel<<<1, DECB_MAX_ROWS, 0, s>>>(R.st, rl, nb);
                    KERNEL_CHECK();
                    if (ex) HIP_CHECK(hipGraphLaunch(ex, s));
                    else CHECK_RC(enqueue_batch_step(m, d, B));
                }
                CHECK_RC(dec_enqueue_slide(m, R, d->w, rl, nb));
                for (int b = 0; b < B; b++) d->pos[b]++;
                for (int i = 0; i < nb; i++) d->pos[rl.row[i]] = R.keep;
                R.produced++;
                continue;
            }
        }
        if (ex) HIP_CHECK(hipGraphLaunch(ex, s));
        else CHECK_RC(enqueue_batch_step(m, d, B));
        R.produced++;
        if (R.mode == CMP_DECODE_KV)
            for (int b = 0; b < B; b++) d->pos[b]++;
    }
    if (n > 0)
        HIP_CHECK(hipMemcpy2DAsync(ids_out, (size_t)n * 4, R.ids + R.returned, (size_t)R.cap * 4, (size_t)n * 4, B,
                                   hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    R.returned = need;
    return CMP_OK;
}

// The logits the most recent per-token step drew every row's id from (R.logits [B][ldz], padding stripped): host fp32 [B][V].
// Read-only, outside the per-token chain; nothing to read before the first step has run (the first ids come from the prefills).
extern "C" int cmp_decode_batch_logits_get(cmp_model* m, float* host_out) {
    CMP_REQUIRE(m && host_out, "decode_batch_logits_get: null argument");
    DecodeBatchState* d = m->decb;
    CHECK_RC(dec_require_begun("decode_batch_logits_get", d && d->rows.begun, "cmp_decode_batch_begin"));
    const DecRows& R = d->rows;
    if (R.produced < 2) {
        cmp_set_error("decode_batch_logits_get: no per-token step has run yet (the first ids are drawn from the prefills' logits)");
        return CMP_ERR_STATE;
    }
    HIP_CHECK(hipSetDevice(m->ctx->device));
    HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
    HIP_CHECK(hipMemcpy2D(host_out, (size_t)m->V * 4, R.logits, (size_t)m->ldz * 4, (size_t)m->V * 4, R.B, hipMemcpyDeviceToHost));
    return CMP_OK;
}
