// decode.hip -- autoregressive decode: the loop of `composer generate` (cli.py:659-676) on one GPU.
//
// Two modes behind one per-token step:
//   CMP_DECODE_LITERAL : cli.py as written -- `past` is never passed back, so every step after the first
//                        feeds ONE token at position 0 with no context.
//   CMP_DECODE_KV      : model(x, past=presents) (transformer.py:735-765, 423-426): one new token per step at
//                        position P+i attending to a preallocated KV cache (the reference's tf.concat
//                        re-allocates the cache every step).
// cmp_decode_begin_slide is CMP_DECODE_KV that goes on past the window: when the cache is full, the step is a SLIDE instead of a
// graph launch -- the last `keep` tokens (prompt and ids both live on the device) are re-encoded at positions 0 .. keep - 1
// through the same prefill path and the id is drawn from that pass's last row (composer_hip.h: c(n)).
// The prompt goes through the batched forward of model.hip (prefill); each later token is a fixed chain of
// 5L+2 small kernels whose only varying inputs (position, current token, RNG counter, output slot) live in
// device memory, so the chain is captured ONCE into a hipGraph and replayed per token.
//
// Arithmetic is fp32 in both model dtypes (weights fp32 master, transposed once per decode_begin to
// [N][K] so that a wave reads one output column as a contiguous, 16-B-per-lane stream).
// Sampling: temperature <= 0 -> argmax, lowest index on ties (tf.argmax); otherwise Gumbel-max over
// logits/temperature == a draw from softmax(logits/temperature) (tf.random.categorical, cli.py:671-673).
//
// This file also holds what the batched chain (decode_batch.hip) shares with this one (declared in decode_common.h): the weight
// transposes, the row buffers, the prefill of one row, the slide, the begin-time checks and the read-backs of both chains.
#include "model.h"
#include "decode_common.h"

void decode_state_free(DecodeState* d) {
    if (!d) return;
    if (d->exec) hipGraphExecDestroy(d->exec);
    if (d->graph) hipGraphDestroy(d->graph);
    dec_rows_free(d->rows);
    for (void* p : d->w.allocs) hipFree(p);
    delete d;
}

// out[n][k] = in[k][n]: the transposed weights of both chains
__global__ void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int K, int N) {
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


__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) s += red[w];
    return s;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = -INFINITY;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) s = fmaxf(s, red[w]);
    return s;
}

// y[n] = act( IN(x) . Wt[n,:] + bias[n] ) + resid[n].  One WAVE per output column (4 columns per workgroup): the
// column's K weights are one contiguous row of the transposed matrix, read 16 bytes per lane with every load of the row
// in flight at once (K <= 64*4*GV_MAXI).  IN: 0 plain copy, 1 LayerNorm (every workgroup recomputes the row statistics of
// the 2-8 KiB input: cheaper than another launch), 2 combine of the split-key attention partials.
#define GV_MAXI 12
template <int ACT, int IN>
__global__ __launch_bounds__(256) void dec_gemv_kernel(const float* __restrict__ x, const float* __restrict__ ln_g,
                                                       const float* __restrict__ ln_b, float eps,
                                                       const float* __restrict__ Wt, const float* __restrict__ bias,
                                                       const float* __restrict__ resid, float* __restrict__ y,
                                                       float* __restrict__ u_out, int K, int N, int D, int PS) {
    // PS: floats per attention-partial record (IN == 2): D + 2 from dec_attn_kernel, PSTRIDE(D) from dec_attn2_kernel
    extern __shared__ __attribute__((aligned(16))) float xs[];   // [K] + 8
    float* red = xs + K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // this wave's weight row is requested FIRST: it does not depend on the input, and the LayerNorm / combine prologue
    // below (two block reductions) then runs under the HBM/L2 latency instead of in front of it
    const int n = blockIdx.x * 4 + wave;
    const float* wr = Wt + (int64_t)min(n, N - 1) * K;
    f32x4 wv[GV_MAXI];
#pragma unroll
    for (int i = 0; i < GV_MAXI; i++) {
        const int k = (lane + 64 * i) * 4;
        wv[i] = (k < K) ? *reinterpret_cast<const f32x4*>(wr + k) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if (IN == 1) {
        float s = 0.f;
        for (int k = tid; k < K; k += 256) s += x[k];
        float mu = block_sum(s, red) / (float)K;
        float q = 0.f;
        for (int k = tid; k < K; k += 256) { float dd = x[k] - mu; q += dd * dd; }
        float var = block_sum(q, red) / (float)K;
        float rs = 1.0f / sqrtf(var + eps);
        for (int k = tid; k < K; k += 256) {
            float v = (x[k] - mu) * rs * ln_g[k] + ln_b[k];
            xs[k] = v;
            if (u_out && blockIdx.x == 0) u_out[k] = v;
        }
    } else if (IN == 2) {
        // x: attention partials [H][ATT_SPLITS][D+2] = {o[D] (unnormalised), running max, sum}; K = H*D.
        // First the H*ATT_SPLITS combine weights exp(m_s - m) / sum (one exponential each), then the weighted sums.
        float* cw = red + 8;                              // [H * ATT_SPLITS] (the launcher sizes the LDS for it)
        const int H = K / D;
        for (int t = tid; t < H * ATT_SPLITS; t += 256) {
            const int h = t / ATT_SPLITS;
            const float* p = x + (size_t)h * ATT_SPLITS * PS;
            float mx = -INFINITY;
#pragma unroll
            for (int s = 0; s < ATT_SPLITS; s++) mx = fmaxf(mx, p[s * PS + D]);
            float den = 0.f;
#pragma unroll
            for (int s = 0; s < ATT_SPLITS; s++) den += expf(p[s * PS + D] - mx) * p[s * PS + D + 1];
            cw[t] = expf(p[(t % ATT_SPLITS) * PS + D] - mx) / den;      // exp(-inf) = 0 for empty splits
        }
        __syncthreads();
        for (int k = tid; k < K; k += 256) {
            const int h = k / D, dd = k % D;
            const float* p = x + (size_t)h * ATT_SPLITS * PS;
            float num = 0.f;
#pragma unroll
            for (int s = 0; s < ATT_SPLITS; s++) num += cw[h * ATT_SPLITS + s] * p[s * PS + dd];
            xs[k] = num;
        }
    } else {
        for (int k = tid; k < K; k += 256) {
            float v = x[k];
            xs[k] = v;
            if (u_out && blockIdx.x == 0) u_out[k] = v;
        }
    }
    __syncthreads();
    if (n >= N) return;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < GV_MAXI; i++) {
        const int k = (lane + 64 * i) * 4;
        if (k < K) {
            f32x4 xv = *reinterpret_cast<const f32x4*>(xs + k);
            acc += xv[0] * wv[i][0] + xv[1] * wv[i][1] + xv[2] * wv[i][2] + xv[3] * wv[i][3];
        }
    }
    // rows longer than one register-resident pass (K > 3072: the mlp c_proj of a model wider than 768): further passes
    for (int k0 = 256 * GV_MAXI; k0 < K; k0 += 256 * GV_MAXI) {
#pragma unroll
        for (int i = 0; i < GV_MAXI; i++) {
            const int k = k0 + (lane + 64 * i) * 4;
            wv[i] = (k < K) ? *reinterpret_cast<const f32x4*>(wr + k) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < GV_MAXI; i++) {
            const int k = k0 + (lane + 64 * i) * 4;
            if (k < K) {
                f32x4 xv = *reinterpret_cast<const f32x4*>(xs + k);
                acc += xv[0] * wv[i][0] + xv[1] * wv[i][1] + xv[2] * wv[i][2] + xv[3] * wv[i][3];
            }
        }
    }
    float v = wave_sum(acc);
    if (lane == 0) {
        if (bias) v += bias[n];
        if (ACT == 1) v = gelu_f<true>(v);
        if (resid) v += resid[n];
        y[n] = v;
    }
}



// =================================================================================================
// The per-token kernels (second generation; the first one is in history, see below).  Same arithmetic; every kernel's dependent chain is as short as the
// data flow allows, because a batch-1 token is 5L+2 dependent launches of ~1.8 us boundary each (tools/ubench/graph_chain.hip)
// and what is left to win is inside the kernels:
//   * GEMV: a workgroup is 1-4 INDEPENDENT waves, one output column per wave: no LDS, no barrier.  Each lane loads the
//     slices of the input vector that face its weight slices straight from global memory (L2), so the LayerNorm statistics
//     / the split-key attention combine are wave-local (DPP row operations + v_readlane) and recomputed by every wave.
//   * attention: the K cache is stored [H][D/4][W][4] so that TWO lanes own a key (one DPP add per score instead of a
//     16-lane shuffle tree); each wave runs its own online softmax over its keys and the four waves meet at ONE barrier;
//     the current token's k/v come from the c_attn output instead of a write -> barrier -> read through the cache.
// (The first-generation kernels are in history: git show a635116:composer_amd/csrc/experiments/decode_lab.hip)
// =================================================================================================

// y[n] = act( IN(x) . Wt[n,:] + bias[n] ) + resid[n]; a wave owns CW adjacent output columns, blockDim.x / 64 waves per workgroup.
// KI = 16-byte chunks of a row per lane (K <= 256 * KI): the loads are unrolled KI times, so the narrow model widths do not carry
// twelve predicated slots.  CW = 2 halves the number of waves to dispatch for the wide outputs and shares the input prologue.
template <int ACT, int IN, int KI, int CW>
__global__ __launch_bounds__(256) void dec_gemv2_kernel(const float* __restrict__ x, const float* __restrict__ ln_g,
                                                        const float* __restrict__ ln_b, float eps,
                                                        const float* __restrict__ Wt, const float* __restrict__ bias,
                                                        const float* __restrict__ resid, float* __restrict__ y,
                                                        float* __restrict__ u_out, int K, int N, int D) {
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * CW;
    if (n0 >= N) return;                                           // whole wave; nothing below synchronises waves
    f32x4 wv[CW][KI], xv[KI];
#pragma unroll
    for (int c = 0; c < CW; c++) {
        const float* wr = Wt + (int64_t)min(n0 + c, N - 1) * K;
#pragma unroll
        for (int i = 0; i < KI; i++) {
            const int k = (lane + 64 * i) * 4;
            // streamed once per token by one wave: non-temporal (MI355X_MICROARCH "nt-weights": shorter issue-to-landed time)
            wv[c][i] = (k < K) ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(wr + k)) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    if (IN == 2) {
        // x: attention partials [H][ATT_SPLITS][PSTRIDE]; K = H*D.  Chunk k..k+3 lies in head k/D.
#pragma unroll
        for (int i = 0; i < KI; i++) {
            const int k = (lane + 64 * i) * 4;
            f32x4 num = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (k < K) {
                const int h = k / D, dd = k % D;
                const float* p = x + (size_t)h * ATT_SPLITS * PSTRIDE(D);
                f32x4 ov[ATT_SPLITS];
                float mv[ATT_SPLITS], sv[ATT_SPLITS];
                float mx = -INFINITY;
#pragma unroll
                for (int sI = 0; sI < ATT_SPLITS; sI++) {
                    ov[sI] = *reinterpret_cast<const f32x4*>(p + sI * PSTRIDE(D) + dd);
                    const f32x2 ms = *reinterpret_cast<const f32x2*>(p + sI * PSTRIDE(D) + D);
                    mv[sI] = ms[0]; sv[sI] = ms[1];
                    mx = fmaxf(mx, mv[sI]);
                }
                float den = 0.f;
#pragma unroll
                for (int sI = 0; sI < ATT_SPLITS; sI++) { mv[sI] = expf(mv[sI] - mx); den += mv[sI] * sv[sI]; }   // exp(-inf) = 0: empty splits
                const float inv = 1.0f / den;
#pragma unroll
                for (int sI = 0; sI < ATT_SPLITS; sI++) num += ov[sI] * (mv[sI] * inv);
            }
            xv[i] = num;
        }
    } else {
#pragma unroll
        for (int i = 0; i < KI; i++) {
            const int k = (lane + 64 * i) * 4;
            xv[i] = (k < K) ? *reinterpret_cast<const f32x4*>(x + k) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        if (IN == 1) {
            f32x4 gv[KI], bv[KI];
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < KI; i++) {
                const int k = (lane + 64 * i) * 4;
                gv[i] = (k < K) ? *reinterpret_cast<const f32x4*>(ln_g + k) : (f32x4){0.f, 0.f, 0.f, 0.f};
                bv[i] = (k < K) ? *reinterpret_cast<const f32x4*>(ln_b + k) : (f32x4){0.f, 0.f, 0.f, 0.f};
                s += (xv[i][0] + xv[i][1]) + (xv[i][2] + xv[i][3]);
            }
            const float mu = wave_sum2(s) / (float)K;
            float q = 0.f;
#pragma unroll
            for (int i = 0; i < KI; i++) {
                const int k = (lane + 64 * i) * 4;
                if (k < K) {
                    const f32x4 dv = xv[i] - mu;
                    q += (dv[0] * dv[0] + dv[1] * dv[1]) + (dv[2] * dv[2] + dv[3] * dv[3]);
                }
            }
            const float var = wave_sum2(q) / (float)K;
            const float rs = 1.0f / sqrtf(var + eps);
#pragma unroll
            for (int i = 0; i < KI; i++) xv[i] = (xv[i] - mu) * rs * gv[i] + bv[i];      // padding lanes: gamma = beta = 0
        }
        if (u_out && n0 == 0) {
#pragma unroll
            for (int i = 0; i < KI; i++) {
                const int k = (lane + 64 * i) * 4;
                if (k < K) *reinterpret_cast<f32x4*>(u_out + k) = xv[i];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CW; c++) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < KI; i++) acc += (xv[i][0] * wv[c][i][0] + xv[i][1] * wv[c][i][1]) + (xv[i][2] * wv[c][i][2] + xv[i][3] * wv[c][i][3]);
        float v = wave_sum2(acc);
        const int n = n0 + c;
        if (lane == 0 && n < N) {
            if (bias) v += bias[n];
            if (ACT == 1) v = gelu_f<true>(v);
            if (resid) v += resid[n];
            y[n] = v;
        }
    }
}

// Split-key single-query attention, grid (H, ATT_SPLITS), 4 waves.  K cache [H][D/4][W][4] (chunk-major): the two lanes
// that own key j read chunk c of it at ((h*D/4 + c)*W + j)*4 -- 32 consecutive keys are one contiguous 512 bytes per chunk.
// V cache [H][W][D].  Wave w takes keys w*32 .. w*32+31 of every 128-key pass and keeps its own running max / sum / output;
// the four waves' partials meet in LDS behind one barrier.  The current token (key == pos) is read from the c_attn output
// and appended to both caches by the workgroup whose key range holds it.
template <int D>
__global__ __launch_bounds__(256) void dec_attn2_kernel(const float* __restrict__ qkv, float* __restrict__ kcT,
                                                        float* __restrict__ vc, float* __restrict__ part,
                                                        const DecRow* __restrict__ st, int E, int W, float scale) {
    constexpr int CH = D / 4;                       // 16-byte chunks per row
    constexpr int CPL = CH / 2;                     // K chunks per lane of a key pair
    constexpr int KPI = 64 / CH;                    // V rows per wave-instruction
    constexpr int VL = 32 / KPI;                    // V loads per lane per 32-key pass
    __shared__ __attribute__((aligned(16))) float opart[4][KPI][D];
    __shared__ float pw[4][32];
    __shared__ float mw[4], lw[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = blockIdx.x, sp = blockIdx.y;
    const int pos = st->pos;
    const int chunk = ((pos + 1 + ATT_SPLITS - 1) / ATT_SPLITS + 3) & ~3;
    const int j0 = sp * chunk, j1 = min(pos + 1, j0 + chunk);
    const int nk = j1 - j0;
    float* out = part + ((size_t)h * ATT_SPLITS + sp) * PSTRIDE(D);
    if (nk <= 0) {
        if (tid < D) out[tid] = 0.f;
        if (tid == 0) { out[D] = -INFINITY; out[D + 1] = 0.f; }
        return;
    }
    const float* qh = qkv + h * D;
    const float* kcur = qkv + E + h * D;
    const float* vcur = qkv + 2 * E + h * D;
    float* kh = kcT + (int64_t)h * CH * W * 4;
    float* vh = vc + (int64_t)h * W * D;
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
        // (LDS operations of one wave execute in order: the reads below see the writes above without a barrier)
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

// K / V rows of a prefill or a re-encode into the caches of both chains' attention kernels (K chunk-major): qkv [nb][T][3E], row
// blockIdx.y of it into the caches of row rl.row[r0 + blockIdx.y]
template <typename T>
__global__ void decb_cache_fill_kernel(const T* __restrict__ qkv, float* __restrict__ kcT, float* __restrict__ vc, int Tn, int E,
                                      int D, int W, DecRowList rl, int r0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Tn * E) return;
    const int b = rl.row[r0 + blockIdx.y];
    const T* q = qkv + (int64_t)blockIdx.y * Tn * 3 * E;
    float* kr = kcT + (int64_t)b * W * E;
    float* vr = vc + (int64_t)b * W * E;
    const int t = i / E, e = i % E, h = e / D, d = e % D;
    kr[(((int64_t)h * (D / 4) + (d >> 2)) * W + t) * 4 + (d & 3)] = to_f32<T>(q[(int64_t)t * 3 * E + E + e]);
    vr[((int64_t)h * W + t) * D + d] = to_f32<T>(q[(int64_t)t * 3 * E + 2 * E + e]);
}

// next id from logits[V], then the next input embedding (first: the position stays; the begin's own first draw goes through
// decb_sample_kernel, as every row of the batched chain's does)
__global__ __launch_bounds__(256) void dec_sample2_kernel(const float* __restrict__ logits, int ldz_row_off, int V,
                                                          DecRow* __restrict__ st,
                                                          int32_t* __restrict__ ids, int capI, const float* __restrict__ wte,
                                                          const float* __restrict__ wpe, float* __restrict__ x, int E, int Wn,
                                                          int first, const unsigned* __restrict__ banw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char trunc_lds[];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int tid = threadIdx.x;
    const float* z = logits + ldz_row_off;
    const GramRegs g0 = grammar_read(&st->gr);          // the grammar state the draw sees: in registers before thread 0 moves it on
    const unsigned ctr = st->rng;
    const float temperature = st->temperature;
    const int top_k = st->top_k;
    const float top_p = st->top_p;
    const unsigned seed = st->seed;
    const int pos0 = st->pos, adv = st->advance, nprod = st->produced;
    int pos = first ? pos0 : (adv ? pos0 + 1 : 0);
    const int posc = min(pos, Wn - 1);     // host refuses to step past the table; never index outside it
    // the position row does not depend on the sampled id: requested now, consumed after the argmax
    float pe[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { const int e = tid + 256 * i; pe[i] = e < E ? wpe[(int64_t)posc * E + e] : 0.f; }
    const int id = sample_block_grammar(z, V, temperature, top_k, top_p, seed, ctr, bv, bi, trunc_lds, g0, &st->bd, banw);
    if (tid == 0) {
        if (nprod < capI) ids[nprod] = id;
        st->produced = nprod + 1;
        st->rng = ctr + 1;
        st->token = id;
        st->pos = pos;
        grammar_advance(&st->gr, &st->bd, g0, id, nprod + 1);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) { const int e = tid + 256 * i; if (e < E) x[e] = wte[(int64_t)id * E + e] + pe[i]; }
    for (int e = tid + 1024; e < E; e += 256) x[e] = wte[(int64_t)id * E + e] + wpe[(int64_t)posc * E + e];
}

// n independent draws from ONE logits row with counters counter0 .. counter0+n-1: the sampler of the decode chain exposed for
// the distribution test against the oracle's softmax(z / temperature)
__global__ __launch_bounds__(256) void sample_many_kernel(const float* __restrict__ z, int V, float temperature, int top_k,
                                                          float top_p, unsigned seed, unsigned counter0,
                                                          int32_t* __restrict__ ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char trunc_lds[];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int id = sample_block_any(z, V, temperature, top_k, top_p, seed, counter0 + blockIdx.x, bv, bi, trunc_lds);
    if (threadIdx.x == 0) ids[blockIdx.x] = id;
}

extern "C" int cmp_k_sample_ex(void* stream, const float* logits, int V, float temperature, int top_k, float top_p, uint64_t seed,
                               uint32_t counter0, int n, int32_t* ids_out) {
    CMP_REQUIRE(logits && ids_out && V > 0 && n >= 0, "k_sample: bad arguments");
    CHECK_RC(sampling_check("k_sample", V, temperature, top_k, top_p));
    if (n == 0) return CMP_OK;
    sample_many_kernel<<<n, 256, trunc_lds_bytes(V), (hipStream_t)stream>>>(logits, V, temperature, top_k, top_p, (unsigned)seed,
                                                                            counter0, ids_out);
    KERNEL_CHECK();
    return CMP_OK;
}
extern "C" int cmp_k_sample(void* stream, const float* logits, int V, float temperature, uint64_t seed, uint32_t counter0, int n,
                            int32_t* ids_out) {
    return cmp_k_sample_ex(stream, logits, V, temperature, 0, 1.0f, seed, counter0, n, ids_out);
}

// cmp_k_sample_ex with a device bit vector of banned columns: the banning samplers of the event grammar on their own
__global__ __launch_bounds__(256) void sample_many_banned_kernel(const float* __restrict__ z, int V, float temperature, int top_k,
                                                                 float top_p, const unsigned* __restrict__ banw, unsigned seed,
                                                                 unsigned counter0, int32_t* __restrict__ ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char trunc_lds[];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int id = sample_block_banned(z, V, temperature, top_k, top_p, seed, counter0 + blockIdx.x, bv, bi, trunc_lds,
                                       ban_static(banw));
    if (threadIdx.x == 0) ids[blockIdx.x] = id;
}

extern "C" int cmp_k_sample_banned(void* stream, const float* logits, int V, float temperature, int top_k, float top_p,
                                   const uint32_t* banned_dev, uint64_t seed, uint32_t counter0, int n, int32_t* ids_out) {
    CMP_REQUIRE(logits && ids_out && banned_dev && V > 0 && n >= 0, "k_sample_banned: bad arguments");
    CHECK_RC(sampling_check("k_sample_banned", V, temperature, top_k, top_p));
    if (n == 0) return CMP_OK;
    sample_many_banned_kernel<<<n, 256, trunc_lds_bytes(V), (hipStream_t)stream>>>(logits, V, temperature, top_k, top_p, banned_dev,
                                                                                   (unsigned)seed, counter0, ids_out);
    KERNEL_CHECK();
    return CMP_OK;
}

// ---- event grammar: configuration and state read-back of both chains (composer_hip.h) ----
extern "C" int cmp_decode_grammar(cmp_model* m, int batched, const cmp_event_grammar* g, const uint32_t* banned_words) {
    CMP_REQUIRE(m, "decode_grammar: null model");
    const int V = m->V, nw = grammar_words(V);
    DecGrammarCfg c;
    if (g) {
        CMP_REQUIRE((g->rules & ~CMP_GRAMMAR_ALL) == 0, "decode_grammar: unknown rule bits 0x%x (known: 0x%x)", g->rules, CMP_GRAMMAR_ALL);
        CMP_REQUIRE(g->time_shift_n >= 1, "decode_grammar: time_shift_n=%d must be >= 1", g->time_shift_n);
        CMP_REQUIRE((g->sustain_on < 0) == (g->sustain_off < 0), "decode_grammar: sustain_on=%d without sustain_off=%d (or the reverse): "
                    "both ids, or -1 for both", g->sustain_on, g->sustain_off);
        CMP_REQUIRE(g->sustain_on >= -1 && g->sustain_off >= -1, "decode_grammar: sustain ids %d / %d: an id, or -1 for both",
                    g->sustain_on, g->sustain_off);
        struct R { const char* name; int64_t lo, n; };
        const R rg[5] = {{"note_on", g->note_on0, 128}, {"note_off", g->note_off0, 128}, {"time_shift", g->time_shift0, g->time_shift_n},
                         {"sustain_on", g->sustain_on, 1}, {"sustain_off", g->sustain_off, 1}};
        const int nr = g->sustain_on < 0 ? 3 : 5;
        for (int i = 0; i < nr; i++)
            CMP_REQUIRE(rg[i].lo >= 0 && rg[i].lo + rg[i].n <= V, "decode_grammar: %s ids [%lld, %lld) outside the vocabulary [0, %d)",
                        rg[i].name, (long long)rg[i].lo, (long long)(rg[i].lo + rg[i].n), V);
        for (int i = 0; i < nr; i++)
            for (int j = i + 1; j < nr; j++)
                CMP_REQUIRE(rg[i].lo + rg[i].n <= rg[j].lo || rg[j].lo + rg[j].n <= rg[i].lo,
                            "decode_grammar: the %s ids [%lld, %lld) overlap the %s ids [%lld, %lld)", rg[i].name, (long long)rg[i].lo,
                            (long long)(rg[i].lo + rg[i].n), rg[j].name, (long long)rg[j].lo, (long long)(rg[j].lo + rg[j].n));
        c.has_layout = true;
        c.g = *g;
    }
    if (banned_words) {
        c.words.assign(banned_words, banned_words + nw);
        if (V & 31) c.words[nw - 1] &= (1u << (V & 31)) - 1u;       // bits at or above V name no column
        auto clear_in = [&](int lo, int n) {
            for (int id = lo; id < lo + n; id++)
                if (!((c.words[id >> 5] >> (id & 31)) & 1u)) return true;
            return false;
        };
        if (g) CMP_REQUIRE(clear_in(g->time_shift0, g->time_shift_n), "decode_grammar: the static vector bans every TIME_SHIFT id "
                           "[%d, %d): at least one must stay drawable", g->time_shift0, g->time_shift0 + g->time_shift_n);
        else CMP_REQUIRE(clear_in(0, V), "decode_grammar: the static vector bans all %d ids: at least one must stay drawable", V);
    }
    m->gram[batched ? 1 : 0] = c;          // read by the chain's next begin
    return CMP_OK;
}

static const DecRows* dec_rows_of(const cmp_model* m, int batched) {
    if (batched) return m->decb ? &m->decb->rows : nullptr;
    return m->dec ? &m->dec->rows : nullptr;
}
static const char* dec_begin_name(int batched) { return batched ? "cmp_decode_batch_begin" : "cmp_decode_begin"; }

extern "C" int cmp_decode_grammar_state(cmp_model* m, int batched, int row, uint32_t sounding[4], int32_t* pedal, int64_t* time_steps) {
    CMP_REQUIRE(m && sounding && pedal && time_steps, "decode_grammar_state: null argument");
    const DecRows* R = dec_rows_of(m, batched);
    CHECK_RC(dec_require_begun("decode_grammar_state", R && R->begun, dec_begin_name(batched)));
    if (batched) CMP_REQUIRE(row >= 0 && row < R->B, "decode_grammar_state: row %d outside the batch of %d rows", row, R->B);
    else CMP_REQUIRE(row == 0, "decode_grammar_state: row %d of the batch-1 chain (row 0 only)", row);
    HIP_CHECK(hipSetDevice(m->ctx->device));
    HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
    DecRow h;
    HIP_CHECK(hipMemcpy(&h, R->st + row, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; i++) sounding[i] = h.gr.sounding[i];
    *pedal = h.gr.pedal;
    *time_steps = h.gr.time_steps;
    return CMP_OK;
}

// ---- timed generation: configuration and state read-back of both chains (composer_hip.h) ----
extern "C" int cmp_decode_budget(cmp_model* m, int batched, int64_t time_steps, int32_t max_polyphony) {
    CMP_REQUIRE(m, "decode_budget: null model");
    CMP_REQUIRE(time_steps >= 0, "decode_budget: time_steps=%lld must be >= 0 (0: no time budget)", (long long)time_steps);
    CMP_REQUIRE(max_polyphony >= 0, "decode_budget: max_polyphony=%d must be >= 0 (0: no cap)", max_polyphony);
    DecBudgetCfg& bc = m->budget[batched ? 1 : 0];      // read by the chain's next begin
    bc.time_steps = time_steps;
    bc.max_polyphony = max_polyphony;
    return CMP_OK;
}

extern "C" int cmp_decode_budget_state(cmp_model* m, int batched, int row, int64_t* steps_left, int32_t* phase, int32_t* done_at) {
    CMP_REQUIRE(m && steps_left && phase && done_at, "decode_budget_state: null argument");
    const DecRows* R = dec_rows_of(m, batched);
    CHECK_RC(dec_require_begun("decode_budget_state", R && R->begun, dec_begin_name(batched)));
    if (batched) CMP_REQUIRE(row >= 0 && row < R->B, "decode_budget_state: row %d outside the batch of %d rows", row, R->B);
    else CMP_REQUIRE(row == 0, "decode_budget_state: row %d of the batch-1 chain (row 0 only)", row);
    HIP_CHECK(hipSetDevice(m->ctx->device));
    HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
    DecRow h;
    HIP_CHECK(hipMemcpy(&h, R->st + row, sizeof(h), hipMemcpyDeviceToHost));
    const bool any = (h.gr.sounding[0] | h.gr.sounding[1] | h.gr.sounding[2] | h.gr.sounding[3]) != 0u || h.gr.pedal != 0;
    *steps_left = h.bd.t_end ? h.bd.t_end - h.gr.time_steps : 0;
    *phase = budget_phase(h.bd.t_end, h.gr.time_steps, any);
    *done_at = h.bd.done_at;
    return CMP_OK;
}

extern "C" int cmp_decode_slide_stats(cmp_model* m, int batched, int64_t* row_slides, int64_t* forward_calls) {
    CMP_REQUIRE(m && row_slides && forward_calls, "decode_slide_stats: null argument");
    const DecRows* R = dec_rows_of(m, batched);
    CHECK_RC(dec_require_begun("decode_slide_stats", R && R->begun, dec_begin_name(batched)));
    *row_slides = R->row_slides;
    *forward_calls = R->fwd_calls;
    return CMP_OK;
}

// ---- sliding window (cmp_decode_begin_slide / cmp_decode_batch_begin_slide) ----
// The re-encode input [nb][keep] of the rows rl.row[r0 + blockIdx.y]: the last `keep` tokens of the row's prompt ++ ids, of which
// `produced` ids exist (the same count for every row of a batch).
__global__ void dec_slide_gather_kernel(const int32_t* __restrict__ prompts, const int32_t* __restrict__ plen,
                                        const int32_t* __restrict__ ids, int cap, int W, int produced, int keep, DecRowList rl,
                                        int r0, int32_t* __restrict__ out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= keep) return;
    const int b = rl.row[r0 + blockIdx.y];
    const int P = plen[b];
    const int j = P + produced - keep + g;
    out[(int64_t)blockIdx.y * keep + g] = j < P ? prompts[(int64_t)b * W + j] : ids[(int64_t)b * cap + (j - P)];
}

// The draw of a slide for row b = rl.row[r0 + blockIdx.x], from the last row of its re-encode (logits [nb][keep][ldz]): as the
// first id of a begin, but the row's draw counter, produced count and seed carry on.  The token is consumed next at position
// `keep`; the logits row goes to where cmp_decode_logits_get / cmp_decode_batch_logits_get read; the hold is over.
__global__ __launch_bounds__(256) void dec_slide_sample_kernel(const float* __restrict__ logits, int ldz, int V, DecRow* __restrict__ st,
                                                               DecRowList rl, int r0, int32_t* __restrict__ ids, int cap,
                                                               const float* __restrict__ wte, const float* __restrict__ wpe,
                                                               float* __restrict__ x, int E, int keep, float* __restrict__ zout,
                                                               const unsigned* __restrict__ banw, int ban_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char trunc_lds[];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int tid = threadIdx.x, b = rl.row[r0 + blockIdx.x];
    banw += (int64_t)b * ban_stride;       // a guarded chain: the row's own words (stride 0: the chain's static words)
    const float* z = logits + ((int64_t)blockIdx.x * keep + keep - 1) * ldz;
    DecRow* rs = st + b;
    const unsigned ctr = rs->rng;
    const int nprod = rs->produced;
    const GramRegs g0 = grammar_read(&rs->gr);
    const int id = sample_block_grammar(z, V, rs->temperature, rs->top_k, rs->top_p, rs->seed, ctr, bv, bi, trunc_lds, g0, &rs->bd, banw);
    __syncthreads();                       // every thread has read the state before thread 0 moves it on
    if (tid == 0) {
        if (nprod < cap) ids[(int64_t)b * cap + nprod] = id;
        rs->produced = nprod + 1;
        rs->rng = ctr + 1;
        rs->token = id;
        rs->pos = keep;
        rs->hold = 0;
        grammar_advance(&rs->gr, &rs->bd, g0, id, nprod + 1);
    }
    float* xr = x + (int64_t)b * E;
    for (int e = tid; e < E; e += 256) xr[e] = wte[(int64_t)id * E + e] + wpe[(int64_t)keep * E + e];
    float* zo = zout + (int64_t)b * ldz;
    for (int c = tid; c < V; c += 256) zo[c] = z[c];
}

// -------------------------------------------------------------------------------------------------
static int launch_gemv(hipStream_t s, int act, int in_mode, const float* x, const float* g, const float* b, float eps,
                       const float* Wt, const float* bias, const float* resid, float* y, float* u_out, int K, int N, int D,
                       int PS = 0) {
    CMP_REQUIRE(K % 4 == 0 && K <= 8192, "decode gemv: K=%d unsupported (a multiple of 4, at most 8192)", K);
    if (!PS) PS = D + 2;
    int grid = cdiv(N, 4);
    size_t smem = (size_t)(K + 8 + (in_mode == 2 ? (K / D) * ATT_SPLITS : 0)) * 4;      // input | reduction scratch | combine weights
#define GV(A, I) dec_gemv_kernel<A, I><<<grid, 256, smem, s>>>(x, g, b, eps, Wt, bias, resid, y, u_out, K, N, D, PS)
    if (act == 1) { if (in_mode == 1) GV(1, 1); else if (in_mode == 2) GV(1, 2); else GV(1, 0); }
    else { if (in_mode == 1) GV(0, 1); else if (in_mode == 2) GV(0, 2); else GV(0, 0); }
#undef GV
    KERNEL_CHECK();
    return CMP_OK;
}

static int launch_gemv2(hipStream_t s, int act, int in_mode, const float* x, const float* g, const float* b, float eps,
                        const float* Wt, const float* bias, const float* resid, float* y, float* u_out, int K, int N, int D) {
    // rows longer than the register-resident kernel holds: the workgroup-staged kernel in several passes (same partial records)
    if (K > 256 * GV_MAXI) return launch_gemv(s, act, in_mode, x, g, b, eps, Wt, bias, resid, y, u_out, K, N, D, PSTRIDE(D));
    CMP_REQUIRE(K % 4 == 0, "decode gemv: K=%d must be a multiple of 4", K);
    // CW = 2 columns per wave for the wide outputs of the narrow-K launches; 4, 2 or 1 waves per workgroup so that the narrow
    // outputs still give every CU a workgroup
    const int cw = (K <= 512 && N >= 1024) ? 2 : 1;
    const int waves = cdiv(N, cw);
    int block = 256;
    while (block > 64 && cdiv(waves, block / 64) < 256) block >>= 1;
    const int grid = cdiv(waves, block / 64);
#define GV3(A, I, KI, CW) dec_gemv2_kernel<A, I, KI, CW><<<grid, block, 0, s>>>(x, g, b, eps, Wt, bias, resid, y, u_out, K, N, D)
#define GV2(A, I) do { if (K <= 512) { if (cw == 2) GV3(A, I, 2, 2); else GV3(A, I, 2, 1); } else GV3(A, I, GV_MAXI, 1); } while (0)
    if (act == 1) { if (in_mode == 1) GV2(1, 1); else if (in_mode == 2) GV2(1, 2); else GV2(1, 0); }
    else { if (in_mode == 1) GV2(0, 1); else if (in_mode == 2) GV2(0, 2); else GV2(0, 0); }
#undef GV2
#undef GV3
    KERNEL_CHECK();
    return CMP_OK;
}

static int launch_attn2(hipStream_t s, cmp_model* m, const DecRows& R, int layer, float scale) {
    dim3 grid(m->H, ATT_SPLITS);
    float *kc = R.kc[layer], *vc = R.vc[layer];
    switch (m->D) {
        case 16: dec_attn2_kernel<16><<<grid, 256, 0, s>>>(R.qkv, kc, vc, R.att, R.st, m->Ea, m->W, scale); break;
        case 32: dec_attn2_kernel<32><<<grid, 256, 0, s>>>(R.qkv, kc, vc, R.att, R.st, m->Ea, m->W, scale); break;
        case 64: dec_attn2_kernel<64><<<grid, 256, 0, s>>>(R.qkv, kc, vc, R.att, R.st, m->Ea, m->W, scale); break;
        case 128: dec_attn2_kernel<128><<<grid, 256, 0, s>>>(R.qkv, kc, vc, R.att, R.st, m->Ea, m->W, scale); break;
        default: CMP_REQUIRE(false, "decode attention: head size %d has no kernel (16, 32, 64, 128)", m->D);
    }
    KERNEL_CHECK();
    return CMP_OK;
}

// one token: consumes R.x (embedding of st->token at st->pos), produces the next id and the next R.x
static int enqueue_token_step(cmp_model* m, DecodeState* d) {
    hipStream_t s = m->ctx->stream;
    const DecRows& R = d->rows;
    const int E = m->E, Ea = m->Ea, L = m->L;
    const bool ln = m->cfg.use_layer_norm != 0;
    const float eps = m->cfg.ln_eps;
    const float scale = m->cfg.scale_attention ? 1.0f / sqrtf((float)m->Dl) : 1.0f;
    for (int i = 0; i < L; i++) {
        const LayerOff& o = m->lo[i];
        const DecLayerW& w = d->w.lw[i];
        CHECK_RC(launch_gemv2(s, 0, ln ? 1 : 0, R.x, m->P + o.ln1_g, m->P + o.ln1_b, eps, w.attn_wT, m->P + o.attn_b, nullptr,
                              R.qkv, R.u, E, 3 * Ea, m->D));
        CHECK_RC(launch_attn2(s, m, R, i, scale));
        CHECK_RC(launch_gemv2(s, 0, 2, R.att, nullptr, nullptr, eps, w.proj_wT, m->P + o.proj_b, R.u, R.r, nullptr, Ea, E, m->D));
        CHECK_RC(launch_gemv2(s, 1, ln ? 1 : 0, R.r, m->P + o.ln2_g, m->P + o.ln2_b, eps, w.fc_wT, m->P + o.fc_b, nullptr, R.g,
                              nullptr, E, 4 * E, m->D));
        CHECK_RC(launch_gemv2(s, 0, 0, R.g, nullptr, nullptr, eps, w.pr_wT, m->P + o.pr_b, R.r, R.x, nullptr, 4 * E, E, m->D));
    }
    CHECK_RC(launch_gemv2(s, 0, 1, R.x, m->P + m->off_lnf_g, m->P + m->off_lnf_b, eps, m->P + m->off_wte, nullptr, nullptr,
                          R.logits, nullptr, E, m->V, m->D));
    CHECK_RC(dec_enqueue_guard(m, d->rows, d->w, DecRowList{}, -1, 0, 1));
    dec_sample2_kernel<<<1, 256, trunc_lds_bytes(m->V), s>>>(R.logits, 0, m->V, R.st, R.ids, R.cap, m->P + m->off_wte,
                                                             m->P + m->off_wpe, R.x, E, m->W, 0, dec_ban_words(R, d->w));
    KERNEL_CHECK();
    return CMP_OK;
}

// ---- what both chains do around their per-token chains (decode_common.h) ----
bool dec_graph_enabled() {
    const char* e = getenv("COMPOSER_NO_GRAPH");
    return !(e && e[0] == '1');
}

int dec_check_prompt(const char* who, int row, const int32_t* ids, int P, int V, int W) {
    char at[96];
    if (row < 0) snprintf(at, sizeof at, "%s", who);
    else snprintf(at, sizeof at, "%s: row %d", who, row);
    CMP_REQUIRE(P <= W, "%s: prompt length %d exceeds window_size %d", at, P, W);
    for (int i = 0; i < P; i++) CMP_REQUIRE(ids[i] >= 0 && ids[i] < V, "%s: prompt id %d out of range [0,%d)", at, ids[i], V);
    return CMP_OK;
}

int dec_check_keep(const char* who, int keep, int W) {
    CMP_REQUIRE(keep >= 1 && keep <= W - 1, "%s: keep=%d outside [1, window_size - 1 = %d]", who, keep, W - 1);
    return CMP_OK;
}

int dec_require_begun(const char* who, bool begun, const char* begin_fn) {
    if (begun) return CMP_OK;
    cmp_set_error("%s: call %s first", who, begin_fn);
    return CMP_ERR_STATE;
}

int dec_weights_refresh(cmp_model* m, DecWeights& w) {
    const int E = m->E, Ea = m->Ea, L = m->L;
    if (w.lw.empty()) {
        w.lw.resize(L);
        for (DecLayerW& l : w.lw) {
            CHECK_RC(dec_alloc(w.allocs, &l.attn_wT, (size_t)3 * Ea * E * 4));
            CHECK_RC(dec_alloc(w.allocs, &l.proj_wT, (size_t)Ea * E * 4));
            CHECK_RC(dec_alloc(w.allocs, &l.fc_wT, (size_t)4 * E * E * 4));
            CHECK_RC(dec_alloc(w.allocs, &l.pr_wT, (size_t)4 * E * E * 4));
        }
    }
    if (!w.banw) CHECK_RC(dec_alloc(w.allocs, &w.banw, (size_t)grammar_words(m->V) * 4));
    if (w.version == m->param_version) return CMP_OK;
    for (int i = 0; i < L; i++) {
        const LayerOff& o = m->lo[i];
        const DecLayerW& l = w.lw[i];
        auto tr = [&](const float* in, float* out, int K, int N) {
            dim3 grid(cdiv(N, 32), cdiv(K, 32));
            transpose_kernel<<<grid, 256, 0, m->ctx->stream>>>(in, out, K, N);
        };
        tr(m->P + o.attn_w, l.attn_wT, E, 3 * Ea);
        tr(m->P + o.proj_w, l.proj_wT, Ea, E);
        tr(m->P + o.fc_w, l.fc_wT, E, 4 * E);
        tr(m->P + o.pr_w, l.pr_wT, 4 * E, E);
        KERNEL_CHECK();
    }
    w.version = m->param_version;
    return CMP_OK;
}

void dec_rows_free(DecRows& R) {
    for (void* p : R.allocs) hipFree(p);
    R.allocs.clear();
    R.kc.clear();
    R.vc.clear();
    R.capB = 0;
}

int dec_rows_alloc(cmp_model* m, DecRows& R, int B) {
    dec_rows_free(R);
    const int E = m->E, Ea = m->Ea, W = m->W;
    const size_t Bz = (size_t)B;
    std::vector<void*>& al = R.allocs;
    CHECK_RC(dec_alloc(al, &R.st, Bz * sizeof(DecRow)));
    CHECK_RC(dec_alloc(al, &R.ids, Bz * R.cap * 4));
    CHECK_RC(dec_alloc(al, &R.x, Bz * E * 4));
    CHECK_RC(dec_alloc(al, &R.u, Bz * E * 4));
    CHECK_RC(dec_alloc(al, &R.qkv, Bz * 3 * Ea * 4));
    CHECK_RC(dec_alloc(al, &R.att, Bz * m->H * ATT_SPLITS * PSTRIDE(m->D) * 4));      // split-key attention partials
    CHECK_RC(dec_alloc(al, &R.r, Bz * E * 4));
    CHECK_RC(dec_alloc(al, &R.g, Bz * 4 * E * 4));
    CHECK_RC(dec_alloc(al, &R.logits, Bz * m->ldz * 4));
    CHECK_RC(dec_alloc(al, &R.prompts, Bz * W * 4));
    CHECK_RC(dec_alloc(al, &R.plen, Bz * 4));
    CHECK_RC(dec_alloc(al, &R.cgwords, Bz * grammar_words(m->V) * 4));
    CHECK_RC(dec_alloc(al, &R.cghist, Bz * DEC_GUARD_MAX_M * 4));
    CHECK_RC(dec_alloc(al, &R.cglens, Bz * 4));
    CHECK_RC(dec_alloc(al, &R.cgcount, Bz * 8));
    R.kc.assign(m->L, nullptr);
    R.vc.assign(m->L, nullptr);
    for (int i = 0; i < m->L; i++) {
        CHECK_RC(dec_alloc(al, &R.kc[i], Bz * W * Ea * 4));
        CHECK_RC(dec_alloc(al, &R.vc[i], Bz * W * Ea * 4));
    }
    R.capB = B;
    return CMP_OK;
}

// what a begin call refuses of the chain's budget (composer_hip.h, "timed generation"), before any device work
int dec_check_budget(const char* who, const DecGrammarCfg& c, const DecBudgetCfg& bc) {
    if (bc.time_steps == 0 && bc.max_polyphony == 0) return CMP_OK;
    CMP_REQUIRE(c.has_layout, "%s: a budget (time_steps %lld, max_polyphony %d) is set but the chain has no grammar layout: "
                "cmp_decode_grammar names the TIME_SHIFT, NOTE_ON, NOTE_OFF and pedal ids (rules = 0 is enough)", who,
                (long long)bc.time_steps, bc.max_polyphony);
    if (bc.time_steps > 0 && !c.words.empty()) {
        const int id = c.g.time_shift0;
        CMP_REQUIRE(!((c.words[id >> 5] >> (id & 31)) & 1u), "%s: the static vector bans time_shift0 = %d, the one-step TIME_SHIFT: "
                    "under a time budget it must stay drawable", who, id);
    }
    return CMP_OK;
}

DecRow dec_row_init(int mode, int P, unsigned seed, float temperature, int top_k, float top_p, const DecGrammarCfg& c,
                    const DecBudgetCfg& bc, const int32_t* prompt, bool guarded) {
    DecRow h = {};
    h.pos = (mode == CMP_DECODE_KV) ? P : 0;     // position of the first generated token when it is fed back
    h.advance = (mode == CMP_DECODE_KV) ? 1 : 0;
    h.seed = seed;
    h.temperature = temperature;
    h.top_k = top_k;
    h.top_p = top_p;
    h.gr = grammar_begin(c, prompt, P);
    // the budget covers the generated part: the prompt's own duration is not charged to it
    h.bd.t_end = bc.time_steps > 0 ? h.gr.time_steps + bc.time_steps : 0;
    h.bd.max_polyphony = bc.max_polyphony;
    h.bd.done_at = -1;
    if (bc.time_steps > 0 || bc.max_polyphony > 0 || guarded) h.gr.active = 1;      // a guarded row always reads its ban words
    return h;
}

// K / V rows of the forward pass just enqueued (nc sequences of T tokens) into the caches of rows rl.row[r0 .. r0 + nc)
static int dec_cache_fill(cmp_model* m, const DecRows& R, int T, const DecRowList& rl, int r0, int nc) {
    hipStream_t s = m->ctx->stream;
    const dim3 grid(cdiv(T * m->Ea, 256), nc);
    for (int i = 0; i < m->L; i++) {
        if (m->dtype == CMP_BF16)
            decb_cache_fill_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)m->act[i].qkv, R.kc[i], R.vc[i], T, m->Ea, m->D, m->W, rl, r0);
        else
            decb_cache_fill_kernel<float><<<grid, 256, 0, s>>>((const float*)m->act[i].qkv, R.kc[i], R.vc[i], T, m->Ea, m->D, m->W, rl, r0);
        KERNEL_CHECK();
    }
    return CMP_OK;
}

// Prefill of row b, whose DecRow is already on the device: the whole prompt through the batched forward (Transformer.call with
// past=None), its K / V rows into the row's caches (kv mode), the first id from the last prompt row (cli.py:673 `[-1, 0]`).  The
// host prompt upload is stream-ordered, so the stream is drained before the next row's ids may overwrite the staging buffer.
int dec_prefill_row(cmp_model* m, DecRows& R, const DecWeights& w, int b, const int32_t* prompt, int P) {
    hipStream_t s = m->ctx->stream;
    CHECK_RC(ensure_workspace(m, 1, P));
    HIP_CHECK(hipMemcpyAsync(m->x_dev, prompt, (size_t)P * 4, hipMemcpyHostToDevice, s));
    if (R.keep > 0 || R.guard.on())
        HIP_CHECK(hipMemcpyAsync(R.prompts + (int64_t)b * m->W, m->x_dev, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
    CHECK_RC(model_forward(m, m->x_dev, 1, P, false, 0));
    if (R.mode == CMP_DECODE_KV) {
        DecRowList rl = {};
        rl.row[0] = (unsigned char)b;
        CHECK_RC(dec_cache_fill(m, R, P, rl, 0, 1));
    }
    CHECK_RC(dec_enqueue_guard(m, R, w, DecRowList{}, -1, b, 1));
    CHECK_RC(decb_launch_sample(m, R, w, m->logits + (int64_t)(P - 1) * m->ldz, 1, b, 1));
    HIP_CHECK(hipStreamSynchronize(s));
    return CMP_OK;
}

// The slide of the nb rows of rl (all at pos == W; on the batched chain held during the replay just enqueued) INSTEAD of their
// per-token step: gather the tails, re-encode them, refill the caches, draw.  The tails go through the forward pass together, as
// many rows per call as the workspace holds.  An fp32 forward is the same arithmetic per row whatever rows share the call (one
// GEMM kernel, no split-K, per-row attention and LayerNorm); the bf16 forward picks its GEMM kernels by the token count, so a
// bf16 model re-encodes one row per call, as its prefill does, and a row stays independent of its neighbours.
int dec_enqueue_slide(cmp_model* m, DecRows& R, const DecWeights& w, const DecRowList& rl, int nb) {
    hipStream_t s = m->ctx->stream;
    const int keep = R.keep;
    const int64_t ws_rows = ((int64_t)m->capB * m->capT) / keep;
    const int per = m->dtype == CMP_BF16 ? 1 : (int)std::max<int64_t>(1, std::min<int64_t>(ws_rows, nb));
    for (int r0 = 0; r0 < nb; r0 += per) {
        const int nc = std::min(per, nb - r0);
        dec_slide_gather_kernel<<<dim3(cdiv(keep, 256), nc), 256, 0, s>>>(R.prompts, R.plen, R.ids, R.cap, m->W, R.produced, keep, rl,
                                                                         r0, m->x_dev);
        KERNEL_CHECK();
        CHECK_RC(model_forward(m, m->x_dev, nc, keep, false, 0));
        CHECK_RC(dec_cache_fill(m, R, keep, rl, r0, nc));
        if (r0 == 0) CHECK_RC(dec_enqueue_guard(m, R, w, rl, nb, 0, R.B));      // one scan for all the rows of this slide
        dec_slide_sample_kernel<<<nc, 256, trunc_lds_bytes(m->V), s>>>(m->logits, m->ldz, m->V, R.st, rl, r0, R.ids, R.cap, m->P + m->off_wte,
                                                                       m->P + m->off_wpe, R.x, m->E, keep, R.logits, dec_ban_words(R, w),
                                                                       dec_ban_stride(m, R));
        KERNEL_CHECK();
        R.fwd_calls++;
    }
    R.row_slides += nb;
    return CMP_OK;
}

// ---- copy guard (composer_hip.h, "copy guard"; the scan itself: copyguard.hip) ----
// Row b = row0 + blockIdx.x: the last min(t, M) ids of its history prompt ++ ids so far, t = plen + produced, into hist[b][0 ..) and
// their count into lens[b] -- or 0 for a row that does not draw in this launch (held, or not in the list) and for a row outside PLAY,
// whose samplers do not read the ban words: such a row gets its static words alone and adds nothing to its counter.
__global__ __launch_bounds__(64) void dec_guard_gather_kernel(const DecRow* __restrict__ st, const int32_t* __restrict__ prompts,
                                                              const int32_t* __restrict__ plen, const int32_t* __restrict__ ids,
                                                              int cap, int W, int M, int row0, DecRowList rl, int nb,
                                                              int32_t* __restrict__ hist, int32_t* __restrict__ lens) {
    const int b = row0 + blockIdx.x, tid = threadIdx.x;
    const DecRow* rs = st + b;
    bool live = nb < 0 ? rs->hold == 0 : false;
    for (int i = 0; i < nb; i++) live = live || rl.row[i] == b;
    const bool any = (rs->gr.sounding[0] | rs->gr.sounding[1] | rs->gr.sounding[2] | rs->gr.sounding[3]) != 0u || rs->gr.pedal != 0;
    live = live && budget_phase(rs->bd.t_end, rs->gr.time_steps, any) == CMP_BUDGET_PLAY;
    const int P = min(max(plen[b], 0), W);
    const int t = P + min(max(rs->produced, 0), cap);
    const int n = live ? min(t, M) : 0;
    if (tid == 0) lens[b] = n;
    if (tid < n) {
        const int j = t - n + tid;                    // 0 <= j < t: j < P <= W reads the prompt, j - P < produced <= cap the ids
        hist[(int64_t)b * DEC_GUARD_MAX_M + tid] = j < P ? prompts[(int64_t)b * W + j] : ids[(int64_t)b * cap + (j - P)];
    }
}

int dec_enqueue_guard(cmp_model* m, DecRows& R, const DecWeights& w, const DecRowList& rl, int nb, int row0, int nrows) {
    if (!R.guard.on()) return CMP_OK;
    hipStream_t s = m->ctx->stream;
    const int M = R.guard.opts.max_copy, nw = grammar_words(m->V);
    dec_guard_gather_kernel<<<nrows, 64, 0, s>>>(R.st, R.prompts, R.plen, R.ids, R.cap, m->W, M, row0, rl, nb, R.cghist, R.cglens);
    KERNEL_CHECK();
    return copy_guard_run(s, R.guard, R.cghist + (int64_t)row0 * DEC_GUARD_MAX_M, R.cglens + row0, nrows, DEC_GUARD_MAX_M, m->V, w.banw,
                          R.cgwords + (int64_t)row0 * nw, R.cgcount + row0, true);
}

extern "C" int cmp_decode_copy_guard(cmp_model* m, int batched, cmp_dataset* ds, const cmp_copy_guard_opts* opts) {
    CMP_REQUIRE(m, "decode_copy_guard: null model");
    DecGuardCfg& cur = m->guard[batched ? 1 : 0];       // read by the chain's next begin
    DecGuardCfg g;
    if (ds) {
        CMP_REQUIRE(opts, "decode_copy_guard: null options");
        CHECK_RC(copy_guard_check("decode_copy_guard", ds->n, ds->has_layout ? &ds->layout : nullptr, opts));
        CMP_REQUIRE(ds->ctx->device == m->ctx->device, "decode_copy_guard: the dataset lives on device %d, the model on device %d",
                    ds->ctx->device, m->ctx->device);
        g.ids = ds->ids_dev;
        g.n = ds->n;
        g.start_bits = ds->start_bits_dev;
        g.layout = ds->layout;
        g.opts = *opts;
    }
    g.epoch = cur.epoch + 1;
    cur = g;
    return CMP_OK;
}

extern "C" int cmp_decode_copy_guard_state(cmp_model* m, int batched, int row, int64_t* banned_columns) {
    CMP_REQUIRE(m && banned_columns, "decode_copy_guard_state: null argument");
    const DecRows* R = dec_rows_of(m, batched);
    CHECK_RC(dec_require_begun("decode_copy_guard_state", R && R->begun, dec_begin_name(batched)));
    if (batched) CMP_REQUIRE(row >= 0 && row < R->B, "decode_copy_guard_state: row %d outside the batch of %d rows", row, R->B);
    else CMP_REQUIRE(row == 0, "decode_copy_guard_state: row %d of the batch-1 chain (row 0 only)", row);
    *banned_columns = 0;
    if (!R->guard.on()) return CMP_OK;
    HIP_CHECK(hipSetDevice(m->ctx->device));
    HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
    HIP_CHECK(hipMemcpy(banned_columns, R->cgcount + row, 8, hipMemcpyDeviceToHost));
    return CMP_OK;
}

// ---- the batch-1 chain's entry points ----
// keep > 0: sliding-window mode (cmp_decode_begin_slide), kv mode otherwise unchanged
static int decode_begin_impl(cmp_model* m, const int32_t* prompt, int P, int mode, float temperature, int top_k, float top_p,
                             uint64_t seed, int keep) {
    CMP_REQUIRE(m && prompt && P > 0, "decode_begin: prompt must hold at least one id");
    CMP_REQUIRE(mode == CMP_DECODE_LITERAL || mode == CMP_DECODE_KV, "decode_begin: bad mode %d", mode);
    CHECK_RC(sampling_check("decode_begin", m->V, temperature, top_k, top_p));
    CHECK_RC(dec_check_prompt("decode_begin", -1, prompt, P, m->V, m->W));
    CHECK_RC(dec_check_budget("decode_begin", m->gram[0], m->budget[0]));
    HIP_CHECK(hipSetDevice(m->ctx->device));
    hipStream_t s = m->ctx->stream;
    // the workspace never grows after its first sizing: a slide re-encodes `keep` tokens through it, so it is sized (or found too
    // small) here, before any id is produced
    if (keep > 0) CHECK_RC(ensure_workspace(m, 1, std::max(P, keep)));
    // The decode state (buffers, KV caches, transposed fp32 weights, the captured per-token chain) is built once per model
    // and reused by later calls: of the 7.6 ms a call used to spend here before the first token (45 hipMalloc / hipFree, 24
    // transposes, capture + instantiate: 6 % of a 1024-token generate) what is left is the prefill.  The transposes are
    // redone when a parameter has changed since (cmp_model::param_version); the chain is re-captured only when the graph
    // switch changes (temperature, seed and mode live in the device-side state).
    const bool graph_on = dec_graph_enabled();
    DecodeState* d = m->dec;
    // an earlier call failed part-way (an allocation, the capture), or the graph switch has changed: start over
    if (d && (!d->built || d->graph_on != graph_on)) {
        HIP_CHECK(hipStreamSynchronize(s));
        decode_state_free(d);
        m->dec = d = nullptr;
    }
    if (!d) m->dec = d = new DecodeState();
    DecRows& R = d->rows;
    R.begun = false;
    // a guard attached or detached since the capture: the chain is captured again, with or without the scan
    const bool recapture = d->built && d->guard_epoch != m->guard[0].epoch;
    if (recapture) {
        HIP_CHECK(hipStreamSynchronize(s));
        if (d->exec) hipGraphExecDestroy(d->exec);
        if (d->graph) hipGraphDestroy(d->graph);
        d->exec = nullptr;
        d->graph = nullptr;
    }
    if (!d->built) CHECK_RC(dec_rows_alloc(m, R, 1));
    CHECK_RC(dec_weights_refresh(m, d->w));
    R.B = 1;
    R.mode = mode;
    R.keep = keep;
    R.row_slides = R.fwd_calls = 0;
    R.guard = m->guard[0];
    const DecRow h = dec_row_init(mode, P, (unsigned)seed, temperature, top_k, top_p, m->gram[0], m->budget[0], prompt, R.guard.on());
    HIP_CHECK(grammar_upload(m->gram[0], m->V, d->w.banw, s));
    HIP_CHECK(hipMemcpyAsync(R.st, &h, sizeof(h), hipMemcpyHostToDevice, s));
    if (keep > 0 || R.guard.on()) HIP_CHECK(hipMemcpyAsync(R.plen, &P, 4, hipMemcpyHostToDevice, s));
    if (R.guard.on()) HIP_CHECK(hipMemsetAsync(R.cgcount, 0, 8, s));
    CHECK_RC(dec_prefill_row(m, R, d->w, 0, prompt, P));
    R.produced = 1;
    R.returned = 0;
    d->pos = h.pos;
    if (!d->built || recapture) {               // the per-token chain, captured once per decode state and guard
        d->built = false;
        if (graph_on) CHECK_RC(dec_capture(s, [&] { return enqueue_token_step(m, d); }, &d->graph, &d->exec));
        d->graph_on = graph_on;
        d->guard_epoch = m->guard[0].epoch;
        d->built = true;
    }
    R.begun = true;
    return CMP_OK;
}

extern "C" int cmp_decode_begin(cmp_model* m, const int32_t* prompt, int P, int mode, float temperature, uint64_t seed) {
    return decode_begin_impl(m, prompt, P, mode, temperature, 0, 1.0f, seed, 0);
}

// every begin of the batch-1 chain with the truncated-sampling filters: keep = 0 is cmp_decode_begin, keep > 0 (kv mode only)
// cmp_decode_begin_slide
extern "C" int cmp_decode_begin_ex(cmp_model* m, const int32_t* prompt, int P, int mode, int keep, float temperature, int top_k,
                                   float top_p, uint64_t seed) {
    CMP_REQUIRE(m, "decode_begin_ex: null model");
    if (keep != 0) {
        CMP_REQUIRE(mode == CMP_DECODE_KV, "decode_begin_ex: keep=%d goes with CMP_DECODE_KV", keep);
        CHECK_RC(dec_check_keep("decode_begin_ex", keep, m->W));
    }
    return decode_begin_impl(m, prompt, P, mode, temperature, top_k, top_p, seed, keep);
}

// kv mode that goes on past the window: when the cache is full the last `keep` tokens are re-encoded at positions 0 .. keep - 1
// and the next id is drawn from that pass (composer_hip.h: the contract c(n))
extern "C" int cmp_decode_begin_slide(cmp_model* m, const int32_t* prompt, int P, int keep, float temperature, uint64_t seed) {
    CMP_REQUIRE(m, "decode_begin_slide: null model");
    CHECK_RC(dec_check_keep("decode_begin_slide", keep, m->W));
    return decode_begin_impl(m, prompt, P, CMP_DECODE_KV, temperature, 0, 1.0f, seed, keep);
}

extern "C" int cmp_decode_steps(cmp_model* m, int n, int32_t* ids_out) {
    CMP_REQUIRE(m && ids_out && n >= 0, "decode_steps: bad arguments");
    DecodeState* d = m->dec;
    CHECK_RC(dec_require_begun("decode_steps", d && d->rows.begun, "cmp_decode_begin"));
    DecRows& R = d->rows;
    HIP_CHECK(hipSetDevice(m->ctx->device));
    hipStream_t s = m->ctx->stream;
    const int need = R.returned + n;
    CMP_REQUIRE(need <= R.cap, "decode_steps: more than %d ids per decode_begin", R.cap);
    while (R.produced < need) {
        if (R.keep > 0 && d->pos >= m->W) {         // the window is full: this id comes from a re-encode of the tail
            const DecRowList row0 = {};             // (the captured chain is not touched)
            CHECK_RC(dec_enqueue_slide(m, R, d->w, row0, 1));
            R.produced++;
            d->pos = R.keep;
            continue;
        }
        if (R.mode == CMP_DECODE_KV)
            CMP_REQUIRE(d->pos < m->W, "decode_steps: position %d outside the wpe table (window_size %d): "
                        "prompt_len + length - 1 must be <= window_size in kv-cache mode", d->pos, m->W);
        if (d->exec) HIP_CHECK(hipGraphLaunch(d->exec, s));
        else CHECK_RC(enqueue_token_step(m, d));
        R.produced++;
        if (R.mode == CMP_DECODE_KV) d->pos++;
    }
    HIP_CHECK(hipMemcpyAsync(ids_out, R.ids + R.returned, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    R.returned = need;
    return CMP_OK;
}

// The logits the most recent per-token step drew its id from (R.logits, ldz padding stripped): host fp32 [V].  Read-only, outside
// the per-token chain.  The first id of a decode comes from the prefill's logits (cmp_forward_logits shows those), so there is
// nothing to read before the first step has run.
extern "C" int cmp_decode_logits_get(cmp_model* m, float* host_out) {
    CMP_REQUIRE(m && host_out, "decode_logits_get: null argument");
    DecodeState* d = m->dec;
    CHECK_RC(dec_require_begun("decode_logits_get", d && d->rows.begun, "cmp_decode_begin"));
    if (d->rows.produced < 2) {
        cmp_set_error("decode_logits_get: no per-token step has run yet (the first id is drawn from the prefill's logits)");
        return CMP_ERR_STATE;
    }
    HIP_CHECK(hipSetDevice(m->ctx->device));
    HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
    HIP_CHECK(hipMemcpy(host_out, d->rows.logits, (size_t)m->V * 4, hipMemcpyDeviceToHost));
    return CMP_OK;
}
