// decode_common.h -- device helpers shared by the batch-1 decode chain (decode.hip) and the batched one (decode_batch.hip):
// the wave reductions, the split-key attention record layout and the sampler.  Both chains draw their ids through the same
// sample_block, so a batched row and a batch-1 decode see the same arithmetic for the same logits.
#pragma once
#include "model.h"

#ifndef ATT_SPLITS
#define ATT_SPLITS 4        // round-2 kernels, same box: 4: 124.4 us/token, 8: 128-129, 16: 128.6 (round-1 kernels: 206 / 194 / 222)
#endif

#define DPP_F(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (v)), (ctrl), 0xF, 0xF, true))
#define DPP_I(v, ctrl) __builtin_amdgcn_update_dpp(0, (v), (ctrl), 0xF, 0xF, true)
#define DPP_XOR1 0xB1          // quad_perm(1,0,3,2)
#define DPP_XOR2 0x4E          // quad_perm(2,3,0,1)
#define DPP_HALF_MIRROR 0x141
#define DPP_MIRROR 0x140
__device__ __forceinline__ float rl_f(float v, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }
// sum / max of the 64 lanes, same value (and the same summation order) in every lane
__device__ __forceinline__ float wave_sum2(float v) {
    v += DPP_F(v, DPP_XOR1);
    v += DPP_F(v, DPP_XOR2);
    v += DPP_F(v, DPP_HALF_MIRROR);
    v += DPP_F(v, DPP_MIRROR);
    return (rl_f(v, 0) + rl_f(v, 16)) + (rl_f(v, 32) + rl_f(v, 48));
}
__device__ __forceinline__ float wave_max2(float v) {
    v = fmaxf(v, DPP_F(v, DPP_XOR1));
    v = fmaxf(v, DPP_F(v, DPP_XOR2));
    v = fmaxf(v, DPP_F(v, DPP_HALF_MIRROR));
    v = fmaxf(v, DPP_F(v, DPP_MIRROR));
    return fmaxf(fmaxf(rl_f(v, 0), rl_f(v, 16)), fmaxf(rl_f(v, 32), rl_f(v, 48)));
}

#define PSTRIDE(D) ((D) + 4)          // attention partial record: o[D], running max, sum, 2 pad floats (16-byte aligned rows)

// (best, arg) of every thread -> the workgroup's maximum, lowest index on ties, in every thread.  bv/bi: 4-entry LDS scratch.
__device__ __forceinline__ int block_argmax(float best, int arg, float* bv, int* bi) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#define ARGMAX_STEP(ctrl)                                                        \
    {                                                                            \
        const float ov = DPP_F(best, ctrl);                                      \
        const int oi = DPP_I(arg, ctrl);                                         \
        if (ov > best || (ov == best && oi < arg)) { best = ov; arg = oi; }      \
    }
    ARGMAX_STEP(DPP_XOR1) ARGMAX_STEP(DPP_XOR2) ARGMAX_STEP(DPP_HALF_MIRROR) ARGMAX_STEP(DPP_MIRROR)
#undef ARGMAX_STEP
    for (int r = 16; r < 64; r += 16) {              // rows 1..3 into every lane (lane 0 ends with the wave's winner)
        const float ov = rl_f(best, r);
        const int oi = __builtin_amdgcn_readlane(arg, r);
        if (ov > best || (ov == best && oi < arg)) { best = ov; arg = oi; }
    }
    if (lane == 0) { bv[wave] = best; bi[wave] = arg; }
    __syncthreads();
    float fb = bv[0];
    int id = bi[0];
#pragma unroll
    for (int w = 1; w < 4; w++)
        if (bv[w] > fb || (bv[w] == fb && bi[w] < id)) { fb = bv[w]; id = bi[w]; }
    return id;
}

// The draw itself, shared by the per-token sampler and the kernel-level test entry (cmp_k_sample): every thread of a 256-thread
// workgroup returns the chosen id.  temperature <= 0: argmax, lowest index on ties (tf.argmax).  Otherwise Gumbel-max:
// argmax_c(z[c]/temperature + G_c), G_c = -log(-log(u_c)) with u_c a counter hash of (seed, draw counter, column) -- one
// draw from softmax(z / temperature) (tf.random.categorical, cli.py:671-673).  bv/bi: 4-entry LDS scratch.
__device__ __forceinline__ int sample_block(const float* __restrict__ z, int V, float temperature, unsigned seed, unsigned ctr,
                                            float* bv, int* bi) {
    const int tid = threadIdx.x;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    const float inv_t = temperature > 0.f ? 1.0f / temperature : 0.f;
    for (int c = tid; c < V; c += 256) {
        float v = z[c];
        if (temperature > 0.f) {
            unsigned hsh = drop_hash(seed, 0xC0FFEEu + ctr, (uint64_t)c);
            float u = ((float)(hsh >> 9) + 0.5f) * (1.0f / 8388608.0f);       // 23 bits + 0.5: exact, strictly inside (0,1)
            v = v * inv_t - __logf(-__logf(u));
        }
        if (v > best) { best = v; arg = c; }
    }
    const int id = block_argmax(best, arg, bv, bi);
    return min(max(id, 0), V - 1);       // all-NaN logits leave the sentinel index: never address outside wte
}

// ---- truncated sampling: top-k and nucleus (top-p) -------------------------------------------------------------------------
// The contract (composer_hip.h, cmp_decode_begin_ex): columns ranked by (z descending, index ascending); top_k keeps the first
// top_k of them (0 or >= V: off); top_p keeps, of those, the shortest prefix whose float64 mass reaches top_p of the candidates'
// mass (1: off); the draw is sample_block's Gumbel-max over the kept columns, the per-column arithmetic unchanged.
#define TRUNC_MAX_V 4096     // the ranking works on an LDS image of the row: 14 bytes per column
// dynamic LDS every sampler launch carries (the branch between the two samplers is taken on the device); a wider row gets none,
// and the begin functions refuse a filter on it
__host__ __device__ __forceinline__ size_t trunc_lds_bytes(int V) { return V <= TRUNC_MAX_V ? (size_t)((V + 3) & ~3) * 14 : 0; }
__host__ __device__ __forceinline__ bool trunc_filters_on(int V, float temperature, int top_k, float top_p) {
    return temperature > 0.f && ((top_k > 0 && top_k < V) || top_p < 1.0f);
}
// argument checks of every entry point that takes the filters; V: the row width the sampler will see
static inline int sampling_check(const char* who, int V, float temperature, int top_k, float top_p) {
    CMP_REQUIRE(top_k >= 0, "%s: top_k=%d must be >= 0 (0: off)", who, top_k);
    CMP_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p=%g outside (0, 1] (1: off)", who, (double)top_p);      // a NaN fails both
    CMP_REQUIRE(!trunc_filters_on(V, temperature, top_k, top_p) || V <= TRUNC_MAX_V,
                "%s: top-k / top-p sampling ranks the row in LDS: at most %d columns, this row has %d", who, TRUNC_MAX_V, V);
    return CMP_OK;
}

// The order-preserving integer image of a float: a > b as floats <=> key(a) > key(b) as unsigned, -0 and +0 the same key.  A
// NaN gets a place of its own (above +inf or below -inf by its sign), so the keys are totally ordered whatever the row holds.
__device__ __forceinline__ unsigned trunc_key(float z) {
    unsigned u = __float_as_uint(z);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// sample_block over the kept set.  Every thread of the 256-thread workgroup returns the id.  lds: trunc_lds_bytes(V) bytes,
// 8-byte aligned.  Steps, each behind one barrier, none with a float atomic or an order that depends on wave arrival:
//   1. keys of the row into LDS;
//   2. rank by counting: a thread compares each of its columns (tid, tid + 256, ...) against all V keys, four per LDS read,
//      every lane at the same address (a broadcast, no bank conflict).  Columns with equal keys get the same count; an integer
//      LDS counter per count finds them, and only they run the second pass that counts the equal keys at lower indices;
//   3. ord[rank] = column; the candidates are ranks 0 .. kc - 1;
//   4. top_p: q[r] = exp((z - z_max) / temperature) in float64 per rank; thread t sums ranks t*per .. (t+1)*per - 1 serially,
//      the chunk sums are added in chunk order by every thread (offset of its chunk, total), so cum[r] = offset + the chunk's
//      serial partial sum is non-decreasing in r and the kept count is 1 + #{r : cum[r] < top_p * total};
//   5. Gumbel-max over ranks 0 .. n - 1 with sample_block's arithmetic per column.
__device__ __forceinline__ int sample_block_trunc(const float* __restrict__ z, int V, float temperature, int top_k, float top_p,
                                                  unsigned seed, unsigned ctr, float* bv, int* bi, unsigned char* lds) {
    __shared__ double ts[256];
    __shared__ int below;
    const int tid = threadIdx.x;
    const int Vp = (V + 3) & ~3;
    double* q = reinterpret_cast<double*>(lds);                         // [Vp], step 4
    unsigned* ks = reinterpret_cast<unsigned*>(q + Vp);                 // [Vp]
    unsigned short* ord = reinterpret_cast<unsigned short*>(ks + Vp);   // [Vp]
    int* hits = reinterpret_cast<int*>(q);                              // [Vp], steps 1-3: columns per count
    unsigned short* gcnt = reinterpret_cast<unsigned short*>(hits + Vp);// [Vp], steps 2-3: a column's count
    for (int c = tid; c < Vp; c += 256) {
        ks[c] = c < V ? trunc_key(z[c]) : 0u;        // padding: key 0 at an index above every column is never counted
        hits[c] = 0;
    }
    if (tid == 0) below = 0;
    __syncthreads();
    for (int c = tid; c < V; c += 256) {
        const unsigned kc = ks[c];
        int g = 0;
        for (int j = 0; j < Vp; j += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4*>(ks + j);
            g += (k4.x > kc) + (k4.y > kc) + (k4.z > kc) + (k4.w > kc);
        }
        gcnt[c] = (unsigned short)g;
        atomicAdd(&hits[g], 1);
    }
    __syncthreads();
    for (int c = tid; c < V; c += 256) {
        int r = gcnt[c];
        if (hits[r] > 1) {                           // an exact tie: the lower index first
            const unsigned kc = ks[c];
            for (int j = 0; j < c; j++) r += (ks[j] == kc);
        }
        ord[r] = (unsigned short)c;
    }
    __syncthreads();
    const int kc = (top_k > 0 && top_k < V) ? top_k : V;
    int n = kc;
    if (top_p < 1.0f) {
        const double zmax = (double)z[min((int)ord[0], V - 1)], dt = (double)temperature;
        for (int r = tid; r < kc; r += 256) q[r] = exp(((double)z[min((int)ord[r], V - 1)] - zmax) / dt);
        __syncthreads();
        const int per = max(4, (kc + 255) >> 8), nt = (kc + per - 1) / per;
        const int r0 = tid * per, r1 = min(kc, r0 + per);
        if (tid < nt) {
            double s = 0.0;
            for (int r = r0; r < r1; r++) s += q[r];
            ts[tid] = s;
        }
        __syncthreads();
        double off = 0.0, tot = 0.0;
        for (int i = 0; i < nt; i++) {
            if (i == tid) off = tot;
            tot += ts[i];
        }
        const double thr = (double)top_p * tot;
        if (tid < nt) {
            double s = 0.0;
            int cnt = 0;
            for (int r = r0; r < r1; r++) {
                s += q[r];
                cnt += (off + s < thr);
            }
            if (cnt) atomicAdd(&below, cnt);
        }
        __syncthreads();
        n = min(below + 1, kc);                      // a NaN mass compares false everywhere: one column, never out of range
    }
    float best = -INFINITY;
    int arg = 0x7fffffff;
    const float inv_t = 1.0f / temperature;
    for (int r = tid; r < n; r += 256) {
        const int c = min((int)ord[r], V - 1);       // (the ranks are a permutation; the clamp keeps any read inside the row)
        float v = z[c];
        unsigned hsh = drop_hash(seed, 0xC0FFEEu + ctr, (uint64_t)c);
        float u = ((float)(hsh >> 9) + 0.5f) * (1.0f / 8388608.0f);
        v = v * inv_t - __logf(-__logf(u));
        if (v > best || (v == best && v > -INFINITY && c < arg)) { best = v; arg = c; }      // (a -inf column is never chosen)
    }
    const int id = block_argmax(best, arg, bv, bi);
    return min(max(id, 0), V - 1);
}

// what every kernel that draws an id calls: the existing sampler unless a filter is on (uniform per workgroup)
__device__ __forceinline__ int sample_block_any(const float* __restrict__ z, int V, float temperature, int top_k, float top_p,
                                                unsigned seed, unsigned ctr, float* bv, int* bi, unsigned char* lds) {
    if (trunc_filters_on(V, temperature, top_k, top_p) && V <= TRUNC_MAX_V)
        return sample_block_trunc(z, V, temperature, top_k, top_p, seed, ctr, bv, bi, lds);
    return sample_block(z, V, temperature, seed, ctr, bv, bi);
}
