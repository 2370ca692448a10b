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

// The draw itself, shared by the per-token sampler and the kernel-level test entry (cmp_k_sample): every thread of a 256-thread
// workgroup returns the chosen id.  temperature <= 0: argmax, lowest index on ties (tf.argmax).  Otherwise Gumbel-max:
// argmax_c(z[c]/temperature + G_c), G_c = -log(-log(u_c)) with u_c a counter hash of (seed, draw counter, column) -- one
// draw from softmax(z / temperature) (tf.random.categorical, cli.py:671-673).  bv/bi: 4-entry LDS scratch.
__device__ __forceinline__ int sample_block(const float* __restrict__ z, int V, float temperature, unsigned seed, unsigned ctr,
                                            float* bv, int* bi) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    return min(max(id, 0), V - 1);       // all-NaN logits leave the sentinel index: never address outside wte
}

