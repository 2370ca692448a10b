// score_rows.h -- the row reduction of the scoring contract (include/composer_hip.h, "scoring"), shared by score.hip (per-row outputs)
// and evalpass.hip (per-class sums): one wave walks rows of fp32 logits and hands every row's figures to a sink.  Device code only.
#pragma once
#include "common.h"

// integer wave sum, the same value in every lane (the DPP row operations of common.h's wave_sum)
__device__ __forceinline__ int wave_sum_i(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);       // quad_perm(1,0,3,2)
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);       // quad_perm(2,3,0,1)
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);      // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);      // row_mirror
    return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
           (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

// With m = max z, e_c = exp(z_c - m), s = sum e_c, t = sum e_c (z_c - m) over the columns with e_c > 0 (a column at -inf, or one
// whose e underflows, contributes 0 to both):
//   logsumexp = m + log s        logp = z_y - logsumexp        entropy = logsumexp - sum p_c z_c = log s - t / s
// log s >= 0 and -t / s >= 0: the entropy is a sum of two non-negative terms, nothing cancels.
// rank = #{c < V : z_c > z_y or (z_c == z_y and c < y)}: an integer count per lane, folded across the wave.
// e_c is v_exp_f32 of (z_c - m) log2(e), not expf: the product's rounding moves a term by at most |z_c - m| 2^-24 ln 2 of itself, and
// terms far below the maximum carry no weight, so log s moves by about 4e-8 times the mean distance to the maximum (measured against
// float64: 7e-8 .. 1.5e-7 relative on logp and entropy).  What the choice buys, and the forms that were measured and dropped (expf; the
// count on the scalar unit), are in profiles/score.txt.
__device__ __forceinline__ float score_exp(float d) { return __builtin_amdgcn_exp2f(d * 1.4426950408889634f); }

// logp of a row from its target logit, its maximum and ls = logf(s): the one statement of it (score_store; evalpass.hip's nll = -logp)
__device__ __forceinline__ float score_logp(float zy, float gmx, float ls) { return zy - (gmx + ls); }

// Every walk below calls sink(row, yy, valid, zy, gmx, s, t, cnt) once per row of this wave, in every lane with the same values:
// yy = y[row], valid = yy inside [0, V), zy = z[yy] (z[0] when not valid), gmx / s / t as above, cnt = the rank.  wpb = blockDim.x / 64,
// read by the kernel itself (read in here, hipcc fetches the block size through a dependent load at the head of the kernel).

// Register-resident rows of at most 512 columns (padding included), one wave per row, the next row requested before the current one
// is reduced (the shape of elementwise.hip's softmax_xent8_kernel / softmax_xent_kernel).
//   VEC:  a lane owns EIGHT CONSECUTIVE columns, two 16-byte loads (stride a multiple of 8, 16-byte aligned logits); the in-row
//         padding is read and replaced by -inf before any use.
//   !VEC: lane l owns columns l + 64 j, 4-byte loads of the columns below V only.
template <bool VEC, typename Sink>
__device__ __forceinline__ void score_walk_rows(const float* __restrict__ z, int ldz, const int32_t* __restrict__ y, int rows, int V,
                                                int wpb, Sink&& sink) {
    const int lane = threadIdx.x & 63;
    const int stride = gridDim.x * wpb;
    int row = blockIdx.x * wpb + (threadIdx.x >> 6);
    auto col = [&](int j) { return VEC ? 8 * lane + j : lane + 64 * j; };
    float n[8];
#pragma unroll
    for (int j = 0; j < 8; j++) n[j] = -INFINITY;
    int ny = 0;
    auto fetch = [&](int r) {
        const float* zr = z + (int64_t)r * ldz;
        if (VEC) {
            if (8 * lane < ldz) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(zr + 8 * lane);
                const f32x4 b = *reinterpret_cast<const f32x4*>(zr + 8 * lane + 4);
#pragma unroll
                for (int j = 0; j < 4; j++) { n[j] = a[j]; n[4 + j] = b[j]; }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (col(j) < V) n[j] = zr[col(j)];
        }
        ny = y[r];
    };
    if (row < rows) fetch(row);
    for (; row < rows; row += stride) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = col(j) < V ? n[j] : -INFINITY;
        const int yy = ny;
        if (row + stride < rows) fetch(row + stride);
        float mx = v[0];
#pragma unroll
        for (int j = 1; j < 8; j++) mx = fmaxf(mx, v[j]);
        const float gmx = wave_max(mx);
        float s = 0.f, t = 0.f;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            // a column at -inf (padding too) gets a finite difference whose exponential is 0 all the same: e * d is 0, not NaN
            const float d = fmaxf(v[j] - gmx, -1e30f);
            const float e = score_exp(d);
            s += e;
            t = fmaf(e, d, t);
        }
        s = wave_sum(s);
        t = wave_sum(t);
        const bool valid = (unsigned)yy < (unsigned)V;
        const int yc = valid ? yy : 0;
        // z[y]: selected with static indices, then one shuffle from the owning lane (a run-time index into v[] would go to scratch)
        float zy = 0.f;
        if (VEC) {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (j == (yc & 7)) zy = v[j];
            zy = __shfl(zy, yc >> 3);
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (j == (yc >> 6)) zy = v[j];
            zy = __shfl(zy, yc & 63);
        }
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) cnt += (v[j] > zy || (v[j] == zy && col(j) < yc)) ? 1 : 0;     // (a column >= V holds -inf and is > yc)
        cnt = wave_sum_i(cnt);
        sink(row, yy, valid, zy, gmx, s, t, cnt);
    }
}

// Any vocabulary size (ldz > 512): two passes over the row, which stays in L1 / L2 between them -- the maximum, then the sums and
// the count against z[y] (one uniform load).  Columns at or above V are never read.
template <typename Sink>
__device__ __forceinline__ void score_walk_rows_wide(const float* __restrict__ z, int ldz, const int32_t* __restrict__ y, int rows,
                                                     int V, int wpb, Sink&& sink) {
    const int lane = threadIdx.x & 63;
    for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < rows; row += gridDim.x * wpb) {
        const float* zr = z + (int64_t)row * ldz;
        const int yy = y[row];
        const bool valid = (unsigned)yy < (unsigned)V;
        const int yc = valid ? yy : 0;
        const float zy = zr[yc];
        float mx = -INFINITY;
#pragma unroll 4
        for (int c = lane; c < V; c += 64) mx = fmaxf(mx, zr[c]);
        const float gmx = wave_max(mx);
        float s = 0.f, t = 0.f;
        int cnt = 0;
#pragma unroll 4
        for (int c = lane; c < V; c += 64) {
            const float v = zr[c];
            const float d = v - gmx;
            const float e = score_exp(d);
            s += e;
            t += e > 0.f ? e * d : 0.f;
            cnt += (v > zy || (v == zy && c < yc)) ? 1 : 0;
        }
        s = wave_sum(s);
        t = wave_sum(t);
        cnt = wave_sum_i(cnt);
        sink(row, yy, valid, zy, gmx, s, t, cnt);
    }
}

// the three forms and when each runs: 0 = 16-byte loads, 1 = 4-byte loads, 2 = the two-pass form
static inline int score_rows_form(const float* logits, int ldz) {
    if (ldz > 512) return 2;
    return (ldz % 8 == 0 && ((uintptr_t)logits & 15) == 0) ? 0 : 1;
}
