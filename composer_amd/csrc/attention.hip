// attention.hip -- causal scaled-dot-product attention of Attention._multihead_attention
// (transformer.py:331-371) and its gradient, flash-style: the [B,H,T,T] score tensor the reference
// materialises ~6 times per layer is never written to HBM.
//
// Semantics kept from the reference: w = (q.k^T) * rsqrt(D) (:339-348); masked scores are EXACTLY -1e4
// (:351-354), which underflows to probability 0 in fp32, so key tiles entirely above the diagonal are
// skipped without changing a bit; softmax (:360); dropout on the probabilities (:361); w.v (:367).
// split_heads/merge_heads (:373-395) are pure addressing here: q,k,v are read straight out of the
// head-merged c_attn output [B,T,3E] and o is written head-merged [B,T,E].
//
// Matrix-core mapping (32x32 MFMA; bf16: 32x32x16, fp32 parity mode: 32x32x2 = exact fma chains):
//   forward / dQ : S^T = K.Q^T with the QUERY on the lane  -> row max/sum are lane-local (+1 cross-half
//                  exchange), and the f32 accumulator tile is directly the B operand of O^T += V^T.P^T
//                  (resp. dQ^T += K^T.dS^T) -- no LDS round trip for P.
//   dK/dV        : S = Q.K^T with the KEY on the lane -> P and dS are directly the B operands of
//                  dV^T += dO^T.P and dK^T += Q^T.dS; each wave keeps dK^T/dV^T of its 32 keys in registers.
//   "transposed" A operands (V^T, K^T, Q^T, dO^T) come from row-major LDS images through
//   ds_read_b64_tr_b16 (bf16) or plain ds_read_b32 (fp32).
#include "common.h"

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ int rho(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// combine a value with the one on lane ^ 32 (the other 32x32 half): v_permlane32_swap is a VALU instruction, the
// ds_bpermute shuffle it replaces was an LDS round trip on the softmax critical path.
__device__ __forceinline__ void both_halves(float v, float& a, float& b) {
    uint32_t u = __builtin_bit_cast(uint32_t, v), u2 = u;
    // v_permlane32_swap swaps lanes 32..63 of its first operand with lanes 0..31 of its second, in place:
    // u -> {lo, lo}, u2 -> {hi, hi}.  (Issued as asm: this hipcc lowers the builtin's SECOND result to the first
    // operand's register -- checked on hardware with tools/ubench/permlane_test.hip.)
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(u), "+v"(u2));
    const uint32_t r[2] = {u, u2};
    a = __builtin_bit_cast(float, r[0]);
    b = __builtin_bit_cast(float, r[1]);
}
__device__ __forceinline__ float half_max(float v) { float a, b; both_halves(v, a, b); return fmaxf(a, b); }
__device__ __forceinline__ float half_sum(float v) { float a, b; both_halves(v, a, b); return a + b; }

template <typename T> struct AT;
template <> struct AT<bf16_t> {
    static constexpr int KSTEP = 16;
    static constexpr int VN = 8;
    typedef bf16x8 frag;
    static constexpr bool EXACT = false;
};
template <> struct AT<float> {
    static constexpr int KSTEP = 2;
    static constexpr int VN = 4;
    typedef float frag;
    static constexpr bool EXACT = true;
};

template <typename T> using frag_t = typename AT<T>::frag;

// Requiring 2 waves/SIMD caps the kernel at 256 registers, which makes hipcc keep MFMA accumulators in VGPR form;
// with the 512-register budget of 1 wave/SIMD it parks them in AGPRs and pays a v_accvgpr_read/write pair for
// every softmax/rescale touch of an accumulator (measured: ~40% of the loop's vector instructions).
template <typename T, int D> struct Occ {
    static constexpr int MINW = (std::is_same<T, float>::value && D == 128) ? 1 : 2;
    // forward and dQ, bf16 heads up to 64 wide: 3 waves/SIMD (168 registers; dQ lands on 168-170 by itself, and 170
    // already rounds up to a 2-wave allocation).  Left at 2, hipcc's scheduler spends the spare
    // registers on a longer software pipeline (213) and the lost occupancy costs more than the schedule gains; at 4
    // (128 registers) it spills ~120 registers inside the key loop (measured: 2.2x slower).
#ifndef ATTN_MINW_Q
#define ATTN_MINW_Q 3
#endif
    static constexpr int MINW_Q = (std::is_same<T, bf16_t>::value && D <= 64) ? ATTN_MINW_Q : MINW;
};

template <typename T, int D> struct Geo {
    static constexpr int DP = D < 32 ? 32 : D;                       // padded head width (zero filled)
    static constexpr int DT = DP / 32;                               // 32-row output tiles along d
    // LDS row stride in elements. bf16: 2*S bytes, multiple of 16, odd number of 16-B chunks (b128 row reads
    // conflict-free).  fp32: odd (b32 row reads with the row on the lane conflict-free).
    static constexpr int S = std::is_same<T, float>::value ? DP + 1 : DP + 8;
    static constexpr int NS = D / AT<T>::KSTEP;                      // MFMA steps over the head dimension
};

template <typename T> __device__ __forceinline__ f32x16 mfma32(frag_t<T> a, frag_t<T> b, f32x16 c);
template <> __device__ __forceinline__ f32x16 mfma32<bf16_t>(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x16 mfma32<float>(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// stage `nrows` rows x D of a head-merged global tensor into an LDS image [nrows][S], zero filled
template <typename T, int D>
__device__ __forceinline__ void stage_rows(T* img, const T* __restrict__ g, int64_t gstride, int row0, int row_end,
                                           int nrows, int tid) {
    constexpr int VN = AT<T>::VN, DP = Geo<T, D>::DP, S = Geo<T, D>::S;
    constexpr int CPR = DP / VN;
    for (int c = tid; c < nrows * CPR; c += 256) {
        int r = c / CPR, cc = c % CPR;
        Vec16<T> v;
#pragma unroll
        for (int j = 0; j < VN; j++) v.set(j, 0.f);
        if (row0 + r < row_end && cc * VN < D) v = ld16(g + (int64_t)(row0 + r) * gstride + cc * VN);
        if (std::is_same<T, float>::value) {
#pragma unroll
            for (int j = 0; j < VN; j++) img[r * S + cc * VN + j] = from_f32<T>(v.get(j));
        } else {
            st16(img + r * S + cc * VN, v);
        }
    }
}

// Software-pipelined staging of a [64 rows][D] tile: load() issues the global loads of the NEXT tile into registers
// before the current tile's MFMA/softmax work (latency hides under it), store() writes them to the other LDS
// buffer afterwards -- one barrier per tile.
template <typename T, int D, int ROWS = 64> struct Stager {
    static constexpr int VN = AT<T>::VN, DP = Geo<T, D>::DP, S = Geo<T, D>::S;
    // 16-byte chunks per row that exist in memory.  Heads narrower than the padded width (D = 16 in bf16: DP = 32) stage only those:
    // the padding columns of the LDS image are never written and feed nothing that is stored (mma_rows reads D columns; the d >= D
    // rows of a transposed output tile, which mma_acc_b computes from them, are dropped by store_t_tile / colsum_t_tiles).
    static constexpr int CPR = (D < DP ? D : DP) / VN;
    static constexpr int NC = (ROWS * CPR + 255) / 256;
    static constexpr bool WHOLE = (ROWS * CPR) % 256 == 0;          // every thread owns NC chunks
    Vec16<T> r[NC];
    __device__ __forceinline__ void load(const T* __restrict__ g, int64_t gstride, int row0, int row_end, int tid) {
        if constexpr (!std::is_same<T, float>::value || D >= 32) {
            // Range-checked buffer loads: rows at or past row_end come back as zeros from the hardware, so the loads are
            // unconditional straight-line code.  (The guarded global loads they replace sat under divergent branches;
            // hipcc's wait-count pass then put s_waitcnt vmcnt(1)/vmcnt(0) in front of the first MFMAs of the CURRENT
            // tile, i.e. every 64-key tile waited for the NEXT tile's HBM round trip: ~3.5k cycles per 32-key
            // sub-tile instead of ~1k.)  A thread without a chunk (ROWS * CPR < 256) reads past the range: zeros, never stored.
            typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
            const int64_t span = ((int64_t)(row_end - 1) * gstride + D) * (int64_t)sizeof(T);
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g, 0, (int)span, 0x00020000);
#pragma unroll
            for (int i = 0; i < NC; i++) {
                const int c = tid + 256 * i;
                const int row = c / CPR, cc = c % CPR;
                int off = (int)(((int64_t)(row0 + row) * gstride + cc * VN) * (int64_t)sizeof(T));
                if (!WHOLE && c >= ROWS * CPR) off = 0x7FFFFFF0;
                const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
                r[i].v = __builtin_bit_cast(decltype(r[i].v), w);
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < NC; i++) {
            const int c = tid + 256 * i;
            const int row = c / CPR, cc = c % CPR;
#pragma unroll
            for (int j = 0; j < VN; j++) r[i].set(j, 0.f);
            if (c < ROWS * CPR && row0 + row < row_end && cc * VN < D) r[i] = ld16(g + (int64_t)(row0 + row) * gstride + cc * VN);
        }
    }
    __device__ __forceinline__ void store(T* img, int tid) const {
#pragma unroll
        for (int i = 0; i < NC; i++) {
            const int c = tid + 256 * i;
            const int row = c / CPR, cc = c % CPR;
            // whole chunks per thread (every D >= 32): unconditional, so the stores are straight-line code that can be scheduled
            // among the tile's last MFMAs instead of four exec-masked blocks behind them
            if (WHOLE || c < ROWS * CPR) {
                if constexpr (std::is_same<T, float>::value) {
#pragma unroll
                    for (int j = 0; j < VN; j++) img[row * S + cc * VN + j] = r[i].get(j);
                } else {
                    st16(img + row * S + cc * VN, r[i]);
                }
            }
        }
    }
};

// per-lane register fragments of a [32 rows][D] global tile used as the MFMA B operand B[k=d][col=row]
template <typename T, int D>
__device__ __forceinline__ void load_bfrags(frag_t<T>* f, const T* __restrict__ g,
                                            int64_t gstride, int row, bool valid, int h) {
    constexpr int NS = Geo<T, D>::NS;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if constexpr (std::is_same<T, float>::value) {
            f[s] = valid ? g[(int64_t)row * gstride + 2 * s + h] : 0.f;
        } else {
            bf16x8 z;
#pragma unroll
            for (int j = 0; j < 8; j++) z[j] = (bf16_t)0.f;
            f[s] = valid ? *reinterpret_cast<const bf16x8*>(g + (int64_t)row * gstride + 16 * s + 8 * h) : z;
        }
    }
}

// C(32x32) += rows(img[row0..row0+31][0..D)) . Bfrag      (A operand read row-wise from the LDS image)
template <typename T, int D>
__device__ __forceinline__ f32x16 mma_rows(const T* img, int row0, const frag_t<T>* bf,
                                           int lane, f32x16 acc) {
    constexpr int NS = Geo<T, D>::NS, S = Geo<T, D>::S;
    const int r = row0 + (lane & 31), h = lane >> 5;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        frag_t<T> a;
        if constexpr (std::is_same<T, float>::value) a = img[r * S + 2 * s + h];
        else a = *reinterpret_cast<const bf16x8*>(img + r * S + 16 * s + 8 * h);
        acc = mfma32<T>(a, bf[s], acc);
    }
    return acc;
}

// Y^T tile dt (32 d-rows x 32 cols) += img[krow0..krow0+31][32dt..32dt+31]^T . X, X = a 32x32 accumulator
// (rows = the contraction index, in registers; cols on the lanes) used directly as the B operand.
template <typename T, int D>
__device__ __forceinline__ f32x16 mma_acc_b(const T* img, int krow0, int dt, const f32x16& x, int lane, f32x16 acc) {
    constexpr int S = Geo<T, D>::S;
    const int h = lane >> 5;
    if constexpr (std::is_same<T, float>::value) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            float a = img[(krow0 + rho(r, h)) * S + 32 * dt + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x[r], acc, 0, 0, 0);
        }
    } else {
        const int G = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
        const int col = 32 * dt + 16 * (G & 1) + 4 * p;
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int kr = krow0 + 16 * s + 4 * (G >> 1) + q;
            bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + kr * S + col));
            bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + (kr + 8) * S + col));
            bf16x8 a, b;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                a[j] = lo[j];
                a[4 + j] = hi[j];
            }
#pragma unroll
            for (int j = 0; j < 8; j++) b[j] = (bf16_t)x[8 * s + j];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
        }
    }
    return acc;
}

#define LOG2E_F 1.4426950408889634f
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float max16(const f32x16& s) {
    float a = max3(s[0], s[1], s[2]), b = max3(s[3], s[4], s[5]), c = max3(s[6], s[7], s[8]);
    float d = max3(s[9], s[10], s[11]), e = max3(s[12], s[13], s[14]);
    return max3(max3(a, b, c), max3(d, e, s[15]), a);
}

// p = exp2(s * c - m) on all 16 values; returns the sum of the results as two partial sums.  Scalar fma / exp / add on purpose
// (and attention.hip is compiled without SLP vectorisation, build.py): the packed forms v_pk_fma_f32 / v_pk_add_f32 process two
// values per instruction but cost more issue time beside MFMAs than the two scalar instructions (whole-step A/B in build.py).
__device__ __forceinline__ f32x2 exp2_scaled16(f32x16& s, float c, float negm, f32x2 sum) {
    float s0 = sum[0], s1 = sum[1];
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const float p0 = fast_exp2(fmaf(s[r], c, negm)), p1 = fast_exp2(fmaf(s[r + 1], c, negm));
        s0 += p0;
        s1 += p1;
        s[r] = p0;
        s[r + 1] = p1;
    }
    return f32x2{s0, s1};
}
// Keeps hipcc from sinking a select below the bf16 conversion: it rewrites cvt(select(c, p, 0)) as
// select(c, cvt(p), 0), which turns 8 two-value v_cvt_pk_bf16_f32 into 16 single conversions plus 8 v_perm_b32.
__device__ __forceinline__ void pin16(f32x16& v) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
        float x = v[r];
        asm("" : "+v"(x));
        v[r] = x;
    }
}

// Dropout keep-test on the 16 values of one 32-key sub-tile with the QUERY on the lane (forward, dQ): the four
// registers 4*g4..4*g4+3 hold consecutive keys, so they share the xor base and use the four fixed 24-bit multipliers
// (v_mul_u32_u24 is full rate; v_mul_lo_u32 is quarter rate).  Dropped entries become 0; the 1/(1-p) scale is applied
// ONCE to the kernel's output instead of per element.
template <bool PIN = false>
__device__ __forceinline__ void mask16_qlane(f32x16& v, uint32_t rowh, int k0, int h, uint32_t thr) {
    const uint32_t gg = ((uint32_t)(k0 >> 2) + (uint32_t)h) * ATTN_G;
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {
        const uint32_t x = rowh ^ (gg + (uint32_t)(2 * g4) * ATTN_G);
        v[4 * g4 + 0] = (__umul24(x, ATTN_C0) >= thr) ? v[4 * g4 + 0] : 0.f;
        v[4 * g4 + 1] = (__umul24(x, ATTN_C1) >= thr) ? v[4 * g4 + 1] : 0.f;
        v[4 * g4 + 2] = (__umul24(x, ATTN_C2) >= thr) ? v[4 * g4 + 2] : 0.f;
        v[4 * g4 + 3] = (__umul24(x, ATTN_C3) >= thr) ? v[4 * g4 + 3] : 0.f;
    }
    if (PIN) pin16(v);
}

// store a transposed accumulator tile Y^T[d][row] (d in registers, row on the lane) to out[row][d0 + d]
template <typename T, int D>
__device__ __forceinline__ void store_t_tile(T* __restrict__ out, int64_t ostride, int row, bool valid, int dt,
                                             const f32x16& y, float mul, int h) {
    if constexpr (std::is_same<T, bf16_t>::value && D % 32 == 0) {
        // The two lanes of a row (l, l + 32) own alternating 8-byte groups of it.  One v_permlane32_swap per dword regroups them
        // so that each lane holds 16 contiguous bytes: 2 dwordx4 stores per tile and lane instead of 4 dwordx2 (the store tail of
        // a block is store-ISSUE-bound, MI355X_MICROARCH.md "attention epilogue store tail").
#pragma unroll
        for (int gp = 0; gp < 4; gp += 2) {
            uint32_t w[2][2];                  // [group gp | gp + 1][dword]: 4 bf16 each
#pragma unroll
            for (int k = 0; k < 2; k++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
                    const bf2 t = {(bf16_t)(y[4 * (gp + k) + 2 * j] * mul), (bf16_t)(y[4 * (gp + k) + 2 * j + 1] * mul)};
                    w[k][j] = __builtin_bit_cast(uint32_t, t);
                }
            // swap lanes 32..63 of the first operand with lanes 0..31 of the second: afterwards lane l < 32 holds group gp of
            // both halves (its own 4 values, then its partner's), lane l + 32 group gp + 1 of both halves
#pragma unroll
            for (int j = 0; j < 2; j++) asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(w[0][j]), "+v"(w[1][j]));
            typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
            const u32x4 v = {w[0][0], w[0][1], w[1][0], w[1][1]};
            if (valid) *reinterpret_cast<u32x4*>(out + (int64_t)row * ostride + 32 * dt + 8 * (gp + h)) = v;
        }
        return;
    }
    if (!valid) return;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        int d = 32 * dt + 8 * g + 4 * h;
        if (d < D) {
            if constexpr (std::is_same<T, float>::value) {
                f32x4 v = {y[4 * g] * mul, y[4 * g + 1] * mul, y[4 * g + 2] * mul, y[4 * g + 3] * mul};
                *reinterpret_cast<f32x4*>(out + (int64_t)row * ostride + d) = v;
            } else {
                bf16x4 v;
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = (bf16_t)(y[4 * g + j] * mul);
                *reinterpret_cast<bf16x4*>(out + (int64_t)row * ostride + d) = v;
            }
        }
    }
}

// Column sums of a wave's transposed output tiles (Y^T[d][row], 32 rows on the lanes of each half) added to
// bias_grad[d]: the c_attn bias gradient is the column sum of [dQ | dK | dV] (Conv1D bias under tf.GradientTape,
// transformer.py:205-209); taking it from the f32 accumulators saves a 63 us re-read of the [M,3E] gradient per layer.
// Transpose-reduce: 31 shuffles leave lane l (of each half) with the total of value l, then ONE atomic instruction per
// wave writes 64 distinct columns.  (A first version reduced every value to lane 0 and issued 32 two-lane atomics per
// tile set: 3 M atomic instructions per layer on 1536 addresses cost 0.8 ms.)
template <typename T, int D>
__device__ __forceinline__ void colsum_t_tiles(float* __restrict__ bias_grad, bool valid, const f32x16* y, float mul, int h,
                                               int lane) {
    constexpr int DT = Geo<T, D>::DT;
    const int l = lane & 31;
#pragma unroll
    for (int t0 = 0; t0 < DT; t0 += 2) {
        constexpr int dummy = 0;
        (void)dummy;
        const bool pair = t0 + 1 < DT;                  // two tiles = 32 values, or a single tile = 16
        float v[32];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            v[r] = valid ? y[t0][r] * mul : 0.f;
            v[16 + r] = (pair && valid) ? y[pair ? t0 + 1 : t0][r] * mul : 0.f;
        }
        if (pair) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const float keep = (l & 16) ? v[k + 16] : v[k], send = (l & 16) ? v[k] : v[k + 16];
                v[k] = keep + __shfl_xor(send, 16);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] += __shfl_xor(v[k], 16);
        }
#pragma unroll
        for (int s = 8; s >= 1; s >>= 1) {
#pragma unroll
            for (int k = 0; k < s; k++) {
                const float keep = (l & s) ? v[k + s] : v[k], send = (l & s) ? v[k] : v[k + s];
                v[k] = keep + __shfl_xor(send, s);
            }
        }
        // lane l now holds value index l (pair) or l & 15 (single tile; both 16-lane groups hold the same totals)
        const int idx = pair ? l : (l & 15);
        const int d = 32 * (t0 + (idx >> 4)) + 8 * ((idx & 15) >> 2) + 4 * h + (idx & 3);
        if ((pair || l < 16) && d < D) atomicAdd(bias_grad + d, v[0]);
    }
}

// Causal work balance: query block i needs i+1 key tiles.  A workgroup takes the PAIR (nb-1-x, x) -- heavy one
// first -- so every workgroup does nb+1 tiles (the middle block of an odd count runs alone).  grid.x = (nb+1)/2.
// When B*H is small (the default config at batch 1: 16 (batch, head) rows) the launcher gives every block its own workgroup
// instead (gridDim.x == nb, heaviest first): twice the workgroups, each half as long; with many rows the pairing is faster
// (same-box A/B at B*H = 1024: 303-317 us paired, 341-346 us unpaired).
__device__ __forceinline__ int pair_block(int ph, int nb, int x) {
    if ((int)gridDim.x == nb && nb > 1) return ph == 0 ? nb - 1 - x : -1;
    const int hi = nb - 1 - x;
    if (ph == 0) return hi;
    return x < hi ? x : -1;
}

// XCD-aware block mapping: consecutive workgroup ids go to different XCDs (id mod 8), so the gridDim.x workgroups
// that share one (batch, head)'s K/V (Q/dO) would land on different L2s.  Re-deal: XCD x takes (batch, head) rows
// x, x+8, ... and runs the gridDim.x blocks of a row on consecutive slots -> one L2 serves the row's tile re-reads.
// With H a multiple of 8 that alone would give every (batch, head) row of one XCD the SAME head index (by = 8k + xcd), i.e.
// the same 128-byte column slice of the [B,T,3E] tensor for every K/V/Q tile read through that L2 -- rows 3E*2 bytes apart,
// a fixed subset of its channels.  The head index is therefore rotated by the batch index (a bijection inside a batch).
__device__ __forceinline__ void xcd_block(int& bx, int& by, int H) {
    const int gx = gridDim.x, gy = gridDim.y;
    if (gy & 7) { bx = blockIdx.x; by = blockIdx.y; return; }
    const int L = blockIdx.x + gx * blockIdx.y;          // dispatch order: x fastest
    const int xcd = L & 7, slot = L >> 3;
    bx = slot % gx;
    by = (slot / gx) * 8 + xcd;
    const int bb = by / H;
    by = bb * H + (by % H + bb) % H;
}

// Block plan of the forward and dQ launches (plan_u >= 0; 1-D grid, B*H a multiple of 8).  All paired workgroups cost the same
// (nb+1 tiles), so a grid that is not a whole number of rounds over the resident slots (B*H = 1024: 4096 pairs over 768 slots =
// 5.33 rounds; B*H = 256: 1.33) ends with most of the chip idle.  The plan takes the first plan_u (batch, head) rows of every
// XCD out of the pairing: an XCD runs its paired rows first, then the single blocks of those rows heaviest level first
// (all rows' block nb-1, then nb-2, ...), so the launch ends on the cheapest jobs (longest-processing-time order).
// Workgroup L: xcd = L & 7, slot = L >> 3; gridDim.x = 8 * ((rows_per_xcd - plan_u) * pairs + plan_u * nb).
__device__ __forceinline__ void attn_job(int plan_u, int nb, int H, int& by, int& qb0, int& qb1) {
    if (plan_u < 0) {
        int bx;
        xcd_block(bx, by, H);
        qb0 = pair_block(0, nb, bx);
        qb1 = pair_block(1, nb, bx);
        return;
    }
    const int L = blockIdx.x, xcd = L & 7, slot = L >> 3;
    const int pairs = (nb + 1) >> 1;
    const int n_paired = (int)(gridDim.x >> 3) - plan_u * nb;
    int row;
    if (slot < n_paired) {
        row = plan_u + slot / pairs;
        const int x = slot % pairs, hi = nb - 1 - x;
        qb0 = hi;
        qb1 = x < hi ? x : -1;
    } else {
        const int s2 = slot - n_paired;
        row = s2 % plan_u;
        qb0 = nb - 1 - s2 / plan_u;
        qb1 = -1;
    }
    by = row * 8 + xcd;
    const int bb = by / H;
    by = bb * H + (by % H + bb) % H;
}

// =================================================================================================
// forward.  grid ((nb+1)/2, B*H), 256 threads: wave w owns query rows [qb*128 + 32w, +32)
// =================================================================================================
// AMASK: Transformer.call's attention_mask (transformer.py:774-779, 356-358): amask[b][key] = (1 - mask) * -1e4 is ADDED to the
// scaled, causally masked scores of every query of batch row b (forward passes only; the train loop never passes a mask).
// KS ("key split", small grids -- attn_key_split below): the workgroup owns ONE 32-row query block, its four waves take the four
// 64-key quarters of every staged 256-key tile and their (m, l, O) partials are merged through LDS at the end: a quarter of the
// serial tile walk per wave and four times the workgroups.  grid (ceil(T/32), B*H), heaviest block first.
template <typename T, int D, bool DROP, bool AMASK = false, bool KS = false>
__global__ __launch_bounds__(256, (KS ? 2 : Occ<T, D>::MINW_Q)) void attn_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ o,
                                                                          float* __restrict__ lse, int Tn, int H,
                                                                          float scale, DropCfg drop, int plan_u,
                                                                          const float* __restrict__ amask) {
    using G = Geo<T, D>;
    constexpr bool EXACT = AT<T>::EXACT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* Kb = reinterpret_cast<T*>(smem_raw);          // 2 x { K [KT][S] | V [KT][S] }
    static_assert(!KS || (!EXACT && !AMASK), "key split: throughput mode without a mask term");
    constexpr int KT = KS ? 256 : 64;                // keys per staged tile
    constexpr int QR = KS ? 32 : 128;                // query rows per workgroup
    constexpr int IMG = KT * G::S;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = KS ? wave * 64 : 0;               // this wave's keys inside a staged tile
    const int nb = cdiv(Tn, 128);
    int by, qb0, qb1;
    if constexpr (KS) {
        by = blockIdx.y;
        qb0 = (int)gridDim.x - 1 - (int)blockIdx.x;
        qb1 = -1;
    } else {
        attn_job(plan_u, nb, H, by, qb0, qb1);
    }
    const int b = by / H, hd = by % H;
    const int E = H * D;
    const int64_t rs = 3 * E;                        // row stride of qkv
    const T* qg = qkv + (int64_t)b * Tn * rs + hd * D;
    const T* kg = qg + E;
    const T* vg = qg + 2 * E;
    T* og = o + (int64_t)b * Tn * E + hd * D;
    const float c2 = scale * LOG2E_F, neg_big = -1e4f / scale;
    // Deferred rescale (throughput mode): the running maximum m is only raised -- and O, l rescaled -- when some row's new maximum
    // exceeds it by more than 2^RESCALE_LOG2 in the probability domain; until then the probabilities are taken against the stale
    // maximum (at most 2^RESCALE_LOG2, exact in fp32 sums and as bf16 operands) and O / l stays the same quotient.  With random
    // scores some row of a wave sets a new maximum in nearly every tile, so the exact vote rescaled (34 multiplies and an
    // exponential per lane) almost always; the deferred one does so on the first tile of a row and rarely after.
#define ATTN_RESCALE_LOG2 8.0f
    const float rescale_raw = ATTN_RESCALE_LOG2 / c2;
    const float* am = AMASK ? amask + (int64_t)b * Tn : nullptr;
    const float inv_scale = 1.0f / scale;           // throughput mode works on raw scores: the mask term goes in divided by the scale

    for (int ph = 0; ph < 2; ph++) {
        const int qb = ph == 0 ? qb0 : qb1;
        if (qb < 0) break;
        const int q0w = KS ? qb * 32 : qb * 128 + wave * 32;
        const int q = q0w + (lane & 31);
        const bool qvalid = q < Tn;
        frag_t<T> qf[G::NS];
        load_bfrags<T, D>(qf, qg, rs, q, qvalid, h);
        f32x16 oacc[G::DT];
#pragma unroll
        for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
            for (int r = 0; r < 16; r++) oacc[dt][r] = 0.f;
        float m = -INFINITY, lsum = 0.f;   // running max: scaled domain (parity mode) / raw domain (throughput mode)
        // With a mask term no key tile is skipped: a causally masked key sits at -1e4 + its mask term, and in a row whose allowed
        // keys are all masked out (a padding query) that is not negligible against the row maximum -- the reference's softmax
        // runs over all of them (transformer.py:351-360).
        const int kv_end = AMASK ? Tn : min(Tn, qb * QR + QR);
        const uint32_t rowh = attn_row_hash(drop.seed, drop.stream, (uint32_t)(by * Tn + q));

        Stager<T, D, KT> sk, sv;
        sk.load(kg, rs, 0, Tn, tid);
        sv.load(vg, rs, 0, Tn, tid);
        sk.store(Kb, tid);
        sv.store(Kb + IMG, tid);
        __syncthreads();
        // One 64-key tile.  `interior` (compile time) = the tile lies below the diagonal for EVERY wave of the workgroup:
        // that instance has no branch around an accumulating MFMA.  (With the skip/mask branches of the general form in
        // the only loop, hipcc carried the O^T accumulators through 64 v_mov_b64 per pair of tiles -- MFMA into a copy,
        // copy back at the join -- and waited out the MFMA pipeline before the copies.)
        auto tile = [&](auto interior, const int kts, const int it) __attribute__((always_inline)) {
            const T* Ks = Kb + (it & 1) * 2 * IMG + wk * G::S;
            const T* Vs = Ks + IMG;
            const bool more = kts + KT < kv_end;
            const int kt0 = kts + wk;                 // first key of this wave's 64
            if (more) {
                sk.load(kg, rs, kts + KT, Tn, tid);
                sv.load(vg, rs, kts + KT, Tn, tid);
            }
            // Fast path (throughput mode): all 64 keys of the tile are at or below every query of this wave -> no
            // masking; both 32-key sub-tiles go through ONE softmax step: 8 score MFMAs back to back, one row-max exchange
            // and one rescale vote per 64 keys, 32 exponentials, 8 PV MFMAs.
            const bool full64 = decltype(interior)::value || (!EXACT && (kt0 + 63 <= q0w) && (kt0 + 64 <= Tn));   // wave-uniform
            if (full64) {
                f32x16 s0, s1;
#pragma unroll
                for (int r = 0; r < 16; r++) { s0[r] = 0.f; s1[r] = 0.f; }
                s0 = mma_rows<T, D>(Ks, 0, qf, lane, s0);
                s1 = mma_rows<T, D>(Ks, 32, qf, lane, s1);
                if constexpr (AMASK) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        s0[r] += am[kt0 + rho(r, h)] * inv_scale;
                        s1[r] += am[kt0 + 32 + rho(r, h)] * inv_scale;
                    }
                }
                const float mloc = half_max(fmaxf(max16(s0), max16(s1)));
                const float mnew = fmaxf(m, mloc);
                if (!__all(mnew <= m + rescale_raw)) {
                    const float alpha = fast_exp2((m - mnew) * c2);
                    lsum *= alpha;
#pragma unroll
                    for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
                        for (int r = 0; r < 16; r++) oacc[dt][r] *= alpha;
                    m = mnew;
                }
                const float mc = m * c2;
                f32x2 ps = {0.f, 0.f};
                ps = exp2_scaled16(s0, c2, -mc, ps);
                ps = exp2_scaled16(s1, c2, -mc, ps);
                lsum += ps[0] + ps[1];
                if constexpr (DROP) {
                    mask16_qlane<true>(s0, rowh, kt0, h, drop.thr);
                    mask16_qlane<true>(s1, rowh, kt0 + 32, h, drop.thr);
                }
#pragma unroll
                for (int dt = 0; dt < G::DT; dt++) {
                    oacc[dt] = mma_acc_b<T, D>(Vs, 0, dt, s0, lane, oacc[dt]);
                    oacc[dt] = mma_acc_b<T, D>(Vs, 32, dt, s1, lane, oacc[dt]);
                }
            } else
#pragma unroll
            for (int sub = 0; sub < 2; sub++) {
                const int k0 = kt0 + 32 * sub;
                if ((!AMASK && k0 > q0w + 31) || k0 >= Tn) continue;          // wave-uniform: tile entirely masked
                f32x16 s;
#pragma unroll
                for (int r = 0; r < 16; r++) s[r] = 0.f;
                s = mma_rows<T, D>(Ks, 32 * sub, qf, lane, s);
                if constexpr (EXACT) {
                    // parity mode: the reference's arithmetic as written (scale, mask to exactly -1e4, exp)
                    float mloc = -INFINITY;
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        int key = k0 + rho(r, h);
                        float v = s[r] * scale;
                        if (key > q || key >= Tn) v = -1e4f;          // w*b - 1e4*(1-b), transformer.py:354
                        if constexpr (AMASK) v = key < Tn ? v + am[key] : -INFINITY;     // :356-358; keys past the end do not exist
                        s[r] = v;
                        mloc = fmaxf(mloc, v);
                    }
                    mloc = half_max(mloc);
                    const float mnew = fmaxf(m, mloc);
                    const float alpha = expf(m - mnew);
                    float ps = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        float p = expf(s[r] - mnew);
                        ps += p;
                        s[r] = p;
                    }
                    lsum = lsum * alpha + ps;
                    m = mnew;
#pragma unroll
                    for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
                        for (int r = 0; r < 16; r++) oacc[dt][r] *= alpha;
                } else {
                    // throughput mode: raw scores, the scale folded into ONE fma feeding v_exp_f32 (base 2), mask only
                    // on tiles touching the diagonal / sequence end, rescale only when some row's max actually grew.
                    const bool edge = (k0 + 31 > q0w) || (k0 + 32 > Tn);      // wave-uniform
                    if (edge) {
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            int key = k0 + rho(r, h);
                            if (key > q || key >= Tn) s[r] = neg_big;       // == -1e4 after scaling
                        }
                    }
                    if constexpr (AMASK) {
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const int key = k0 + rho(r, h);
                            s[r] = key < Tn ? s[r] + am[key] * inv_scale : -INFINITY;
                        }
                    }
                    float mloc = max16(s);
                    mloc = half_max(mloc);
                    const float mnew = fmaxf(m, mloc);
                    if (!__all(mnew <= m + rescale_raw)) {
                        const float alpha = fast_exp2((m - mnew) * c2);
                        lsum *= alpha;
#pragma unroll
                        for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
                            for (int r = 0; r < 16; r++) oacc[dt][r] *= alpha;
                        m = mnew;
                    }
                    const float mc = m * c2;
                    const f32x2 ps = exp2_scaled16(s, c2, -mc, f32x2{0.f, 0.f});
                    lsum += ps[0] + ps[1];
                }
                if constexpr (DROP) mask16_qlane<true>(s, rowh, k0, h, drop.thr);
#pragma unroll
                for (int dt = 0; dt < G::DT; dt++) oacc[dt] = mma_acc_b<T, D>(Vs, 32 * sub, dt, s, lane, oacc[dt]);
            }
            if (more) {
                T* nbuf = Kb + ((it & 1) ^ 1) * 2 * IMG;
                sk.store(nbuf, tid);
                sv.store(nbuf + IMG, tid);
            }
            __syncthreads();
        };
        int kt0 = 0, it = 0;
        const int interior_end = EXACT ? 0 : (qb * QR) / KT * KT;      // whole tiles below every query row of the block
        for (; kt0 < interior_end; kt0 += KT, it++) tile(std::true_type{}, kt0, it);
        for (; kt0 < kv_end; kt0 += KT, it++) tile(std::false_type{}, kt0, it);
        float ltot = half_sum(lsum);
        if constexpr (KS) {
            // merge the four waves' partial softmax states (the last tile's barrier has passed: the staging buffers are free)
            constexpr int NV = 2 + 16 * G::DT;
            float* mg = reinterpret_cast<float*>(smem_raw);
            if (wave > 0) {
                float* w = mg + (wave - 1) * NV * 64 + lane;
                w[0] = m;
                w[64] = ltot;
#pragma unroll
                for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) w[(2 + 16 * dt + r) * 64] = oacc[dt][r];
            }
            __syncthreads();
            if (wave > 0) continue;               // (single phase: leaves the loop)
            float mstar = m;
#pragma unroll
            for (int w = 0; w < 3; w++) mstar = fmaxf(mstar, mg[w * NV * 64 + lane]);
            const float a0 = fast_exp2((m - mstar) * c2);      // wave 0 always holds key 0: m is finite
            ltot *= a0;
#pragma unroll
            for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
                for (int r = 0; r < 16; r++) oacc[dt][r] *= a0;
#pragma unroll
            for (int w = 0; w < 3; w++) {
                const float* src = mg + w * NV * 64 + lane;
                const float aw = fast_exp2((src[0] - mstar) * c2);     // a wave without keys left m = -inf: factor 0
                ltot = fmaf(src[64], aw, ltot);
#pragma unroll
                for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) oacc[dt][r] = fmaf(src[(2 + 16 * dt + r) * 64], aw, oacc[dt][r]);
            }
            m = mstar;
        }
        const float inv = (DROP ? drop.scale : 1.0f) / ltot;
#pragma unroll
        for (int dt = 0; dt < G::DT; dt++) store_t_tile<T, D>(og, E, q, qvalid, dt, oacc[dt], inv, h);
        if (qvalid && h == 0) lse[(int64_t)by * Tn + q] = (EXACT ? m : m * scale) + logf(ltot);
    }
}


// =================================================================================================
// dQ.  same geometry as forward: dQ^T += K^T . dS^T,  dS^T = P^T * (dP^T - delta),  dP^T = V . dO^T
// With dropout (keep-scale f = 1/(1-p)):  dS = f * P * (M*dP~ - delta/f)  -> the f goes to the output scale.
// =================================================================================================
// KS: as in the forward -- one 32-row query block per workgroup, the waves split every staged 256-key tile, dQ partials summed in LDS.
// (the body is shared by attn_dq_kernel and the small-grid backward launch attn_bwd_ks_kernel, which passes its block in ks_blk)
template <typename T, int D, bool DROP, int KS>
__device__ __forceinline__ void attn_dq_body(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o,
                                             const float* __restrict__ lse, float* __restrict__ delta, T* __restrict__ dqkv,
                                             float* __restrict__ bias_grad, int Tn, int H, float scale, DropCfg drop, int plan_u,
                                             int ks_blk, const AttnLnRows lr = AttnLnRows()) {
    using G = Geo<T, D>;
    constexpr bool EXACT = AT<T>::EXACT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* Kb = reinterpret_cast<T*>(smem_raw);          // 2 x { K | V }
    static_assert(!KS || !EXACT, "key split: throughput mode");
    constexpr int KT = KS ? 256 : 64, QR = KS ? 32 : 128;
    constexpr int IMG = KT * G::S;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = KS ? wave * 64 : 0;
    const int nb = cdiv(Tn, 128);
    int by, qb0, qb1;
    if constexpr (KS) {
        by = blockIdx.y;
        qb0 = ks_blk;
        qb1 = -1;
    } else {
        attn_job(plan_u, nb, H, by, qb0, qb1);
    }
    const int b = by / H, hd = by % H;
    const int E = H * D;
    const int64_t rs = 3 * E;
    const T* qg = qkv + (int64_t)b * Tn * rs + hd * D;
    const T* kg = qg + E;
    const T* vg = qg + 2 * E;
    const T* dog = d_o + (int64_t)b * Tn * E + hd * D;
    T* dqg = dqkv + (int64_t)b * Tn * rs + hd * D;
    const float c2 = scale * LOG2E_F;
    const float keep_scale = DROP ? drop.scale : 1.0f;

    for (int ph = 0; ph < 2; ph++) {
        const int qb = ph == 0 ? qb0 : qb1;
        if (qb < 0) break;
        const int q0w = KS ? qb * 32 : qb * 128 + wave * 32;
        const int q = q0w + (lane & 31);
        const bool qvalid = q < Tn;
        frag_t<T> qf[G::NS], dof[G::NS];
        load_bfrags<T, D>(qf, qg, rs, q, qvalid, h);
        load_bfrags<T, D>(dof, dog, E, q, qvalid, h);
        const float lse_q = qvalid ? lse[(int64_t)by * Tn + q] : 0.f;
        // delta[q] = rowsum(dO . O) is computed here -- this lane already holds its half of the dO row
        // -- and stored for the dK/dV kernel that runs next on the stream (this replaced a separate 52 us pass per layer).
        // The O row is requested now and consumed after the first K/V tile has been staged, under that latency.
        frag_t<T> of[G::NS];
        load_bfrags<T, D>(of, o + (int64_t)b * Tn * E + hd * D, E, q, qvalid, h);
        const float lse2 = lse_q * LOG2E_F;
        f32x16 dq[G::DT];
#pragma unroll
        for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
            for (int r = 0; r < 16; r++) dq[dt][r] = 0.f;
        const int kv_end = min(Tn, qb * QR + QR);
        const uint32_t rowh = attn_row_hash(drop.seed, drop.stream, (uint32_t)(by * Tn + q));

        Stager<T, D, KT> sk, sv;
        sk.load(kg, rs, 0, Tn, tid);
        sv.load(vg, rs, 0, Tn, tid);
        sk.store(Kb, tid);
        sv.store(Kb + IMG, tid);
        float dsum = 0.f;
#pragma unroll
        for (int sidx = 0; sidx < G::NS; sidx++) {
            if constexpr (std::is_same<T, float>::value) {
                dsum += of[sidx] * dof[sidx];
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) dsum += (float)of[sidx][j] * (float)dof[sidx][j];
            }
        }
        dsum = half_sum(dsum);
        if (qvalid && h == 0 && (!KS || wave == 0)) delta[(int64_t)by * Tn + q] = dsum;
        const float del_q = (qvalid ? dsum : 0.f) / keep_scale;
        __syncthreads();
        // One 64-key tile.  `interior` (compile time) = every key of the tile lies at or below every query row of the block and
        // every row and key exists: that instance carries NO mask code.  (Round 3 had the mask in one loop under a wave-uniform
        // `if (edge)`: hipcc if-converted it -- 32 integer compares + 16 selects + ~17 scalar mask operations in the block of the
        // score MFMAs of EVERY sub-tile, a fifth of the kernel's vector instructions, needed on two tiles in eighteen.)
        auto tile = [&](auto interior, const int kts, const int it) __attribute__((always_inline)) {
            constexpr bool INT = decltype(interior)::value;
            const T* Ks = Kb + (it & 1) * 2 * IMG + wk * G::S;
            const T* Vs = Ks + IMG;
            const bool more = kts + KT < kv_end;
            const int kt0 = kts + wk;                 // first key of this wave's 64
            if (more) {
                sk.load(kg, rs, kts + KT, Tn, tid);
                sv.load(vg, rs, kts + KT, Tn, tid);
            }
#pragma unroll
            for (int sub = 0; sub < 2; sub++) {
                const int k0 = kt0 + 32 * sub;
                if (!INT && (k0 > q0w + 31 || k0 >= Tn)) continue;
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
                s = mma_rows<T, D>(Ks, 32 * sub, qf, lane, s);
                dp = mma_rows<T, D>(Vs, 32 * sub, dof, lane, dp);
                if constexpr (DROP) mask16_qlane(dp, rowh, k0, h, drop.thr);
                if constexpr (EXACT) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        int key = k0 + rho(r, h);
                        bool masked = (key > q) || (key >= Tn) || !qvalid;
                        float p = masked ? 0.f : expf(s[r] * scale - lse_q);
                        s[r] = p * (dp[r] - del_q);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; r++) s[r] = fast_exp2(fmaf(s[r], c2, -lse2));
                    if constexpr (!INT) {
                        const bool edge = (k0 + 31 > q0w) || (k0 + 32 > Tn) || (q0w + 32 > Tn);      // wave-uniform
                        if (edge) {
#pragma unroll
                            for (int r = 0; r < 16; r++) {
                                const int key = k0 + rho(r, h);
                                if ((key > q) || (key >= Tn) || !qvalid) s[r] = 0.f;
                            }
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 16; r++) s[r] *= dp[r] - del_q;
                }
#pragma unroll
                for (int dt = 0; dt < G::DT; dt++) dq[dt] = mma_acc_b<T, D>(Ks, 32 * sub, dt, s, lane, dq[dt]);
            }
            if (more) {
                T* nbuf = Kb + ((it & 1) ^ 1) * 2 * IMG;
                sk.store(nbuf, tid);
                sv.store(nbuf + IMG, tid);
            }
            __syncthreads();
        };
        int kt0 = 0, it = 0;
        const int interior_end = (EXACT || qb * QR + QR > Tn) ? 0 : (qb * QR) / KT * KT;     // whole tiles below every (existing) query row of the block
        for (; kt0 < interior_end; kt0 += KT, it++) tile(std::true_type{}, kt0, it);
        for (; kt0 < kv_end; kt0 += KT, it++) tile(std::false_type{}, kt0, it);
        if constexpr (KS) {
            // sum of the four waves' partial dQ^T tiles (the last tile's barrier has passed: the staging buffers are free)
            float* mg = reinterpret_cast<float*>(smem_raw);
            if (wave > 0) {
#pragma unroll
                for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) mg[(((wave - 1) * G::DT + dt) * 16 + r) * 64 + lane] = dq[dt][r];
            }
            __syncthreads();
            if (wave > 0) continue;               // (single phase: leaves the loop)
#pragma unroll
            for (int w = 0; w < 3; w++)
#pragma unroll
                for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) dq[dt][r] += mg[((w * G::DT + dt) * 16 + r) * 64 + lane];
        }
        // (lr: the stored rows carry the rstd of their token's LayerNorm as a factor; see AttnLnRows)
        const float row_rs = (lr.rstd && qvalid) ? lr.rstd[(int64_t)b * Tn + q] : 1.f;
#pragma unroll
        for (int dt = 0; dt < G::DT; dt++) store_t_tile<T, D>(dqg, rs, q, qvalid, dt, dq[dt], scale * keep_scale * row_rs, h);
        if (bias_grad) colsum_t_tiles<T, D>(bias_grad + hd * D, qvalid, dq, scale * keep_scale, h, lane);
    }
}
template <typename T, int D, bool DROP>
__global__ __launch_bounds__(256, (Occ<T, D>::MINW_Q))
void attn_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o, const float* __restrict__ lse,
                    float* __restrict__ delta, T* __restrict__ dqkv, float* __restrict__ bias_grad, int Tn, int H, float scale,
                    DropCfg drop, int plan_u) {
    attn_dq_body<T, D, DROP, 0>(qkv, o, d_o, lse, delta, dqkv, bias_grad, Tn, H, scale, drop, plan_u, 0);
}
// (the same with the stored rows scaled by their token's LayerNorm rstd: AttnLnRows, round 6)
template <typename T, int D, bool DROP>
__global__ __launch_bounds__(256, (Occ<T, D>::MINW_Q))
void attn_dq_ln_kernel(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o, const float* __restrict__ lse,
                    float* __restrict__ delta, T* __restrict__ dqkv, float* __restrict__ bias_grad, int Tn, int H, float scale,
                    DropCfg drop, int plan_u, AttnLnRows lr) {
    attn_dq_body<T, D, DROP, 0>(qkv, o, d_o, lse, delta, dqkv, bias_grad, Tn, H, scale, drop, plan_u, 0, lr);
}

// =================================================================================================
// dK, dV.  grid ((nb+1)/2, B*H): wave w owns keys [kb*128 + 32w, +32); loops over the query tiles at or below the
// diagonal.  Key block j needs nb-j query blocks -> paired (j, nb-1-j) like the forward.
// =================================================================================================
// KS (small grids): one 32-key block per workgroup (grid (ceil(T/32), B*H), key block 0 = the heaviest first), the four waves take
// the four 64-query quarters of every staged 256-query tile, dK / dV partials summed in LDS.
// KS == 2 takes delta[q] = rowsum(dO . O) from `o` itself (a 32- or 64-byte row per thread and staged tile) instead of from the dQ
// kernel: the two roles of a small backward then run side by side in ONE launch (attn_bwd_ks_kernel).
template <typename T, int D, bool DROP, int KS>
__device__ __forceinline__ void attn_dkv_body(const T* __restrict__ qkv, const T* __restrict__ d_o, const float* __restrict__ lse,
                                              const float* __restrict__ delta, T* __restrict__ dqkv, float* __restrict__ bias_grad,
                                              int Tn, int H, float scale, DropCfg drop, const T* __restrict__ o, int ks_blk,
                                              const AttnLnRows lr = AttnLnRows()) {
    using G = Geo<T, D>;
    constexpr bool EXACT = AT<T>::EXACT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* Qb = reinterpret_cast<T*>(smem_raw);          // 2 x { Q [QT][S] | dO [QT][S] }
    static_assert(!KS || !EXACT, "key split: throughput mode");
    constexpr int QT = KS ? 256 : 64;                // queries per staged tile
    constexpr int IMG = QT * G::S;
    float* Lb = reinterpret_cast<float*>(Qb + (KS ? 2 : 4) * IMG);     // 2 x { lse [QT] | delta/f [QT] | dropout row hash [QT] } (KS: 1 x)
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = KS ? wave * 64 : 0;               // this wave's queries inside a staged tile
    int bx, by;
    if constexpr (KS) {
        bx = ks_blk;
        by = blockIdx.y;
    } else {
        xcd_block(bx, by, H);
    }
    const int b = by / H, hd = by % H;
    const int E = H * D;
    const int64_t rs = 3 * E;
    const T* qg = qkv + (int64_t)b * Tn * rs + hd * D;
    const T* kg = qg + E;
    const T* vg = qg + 2 * E;
    const T* dog = d_o + (int64_t)b * Tn * E + hd * D;
    T* dkg = dqkv + (int64_t)b * Tn * rs + E + hd * D;
    T* dvg = dkg + E;
    const float c2 = scale * LOG2E_F;
    const float keep_scale = DROP ? drop.scale : 1.0f;
    const int nb = cdiv(Tn, 128);

    for (int ph = 0; ph < 2; ph++) {
        // light/heavy are mirrored w.r.t. the forward: key block 0 is the heavy one
        const int kb = (KS || ((int)gridDim.x == nb && nb > 1)) ? (ph == 0 ? bx : -1) : (ph == 0 ? bx : (bx < nb - 1 - bx ? nb - 1 - bx : -1));
        if (kb < 0) break;
        const int k0w = KS ? kb * 32 : kb * 128 + wave * 32;
        const int key = k0w + (lane & 31);
        const bool kvalid = key < Tn;
        frag_t<T> kf[G::NS], vf[G::NS];
        load_bfrags<T, D>(kf, kg, rs, key, kvalid, h);
        load_bfrags<T, D>(vf, vg, rs, key, kvalid, h);
        const uint32_t kgG = ((uint32_t)key >> 2) * ATTN_G;
        const uint32_t kC = (key & 3) == 0 ? ATTN_C0 : ((key & 3) == 1 ? ATTN_C1 : ((key & 3) == 2 ? ATTN_C2 : ATTN_C3));
        f32x16 dk[G::DT], dv[G::DT];
#pragma unroll
        for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
            for (int r = 0; r < 16; r++) { dk[dt][r] = 0.f; dv[dt][r] = 0.f; }

        Stager<T, D, QT> sq, so;
        float st_l = 0.f, st_d = 0.f;
        constexpr int ORW = KS == 2 ? D / AT<T>::VN : 1;
        Vec16<T> st_o[ORW], st_g[ORW];           // KS == 2: the thread's O and dO row of the next tile (delta is their dot product)
        const T* og_ks = KS == 2 ? o + (int64_t)b * Tn * E + hd * D : nullptr;
        // per-row scalars of tile qt (threads 0..63): raw loads only -- any arithmetic on the loaded value here would make
        // the compiler wait for it (and for the tile loads issued before it) ahead of the current tile's MFMAs; the
        // scale factors are applied in store_rows, after the tile's work.  Rows past Tn read a clamped (finite) row;
        // their probabilities are masked to zero.
        // Every wave issues them (same 256 bytes, L1 hits): with the loads under `if (tid < 64)` the wait-count pass
        // sized the waits in front of the MFMAs for the shorter path and made the other wave stall on a tile load.
        auto load_rows = [&](int qt) {
            const int qq = min(qt + (tid & (QT - 1)), Tn - 1);
            st_l = lse[(int64_t)by * Tn + qq];
            if constexpr (KS == 2) {
#pragma unroll
                for (int i = 0; i < ORW; i++) {
                    st_o[i] = ld16(og_ks + (int64_t)qq * E + i * AT<T>::VN);
                    st_g[i] = ld16(dog + (int64_t)qq * E + i * AT<T>::VN);
                }
            } else {
                st_d = delta[(int64_t)by * Tn + qq];
            }
        };
        auto store_rows = [&](float* dst, int qt) {
            if constexpr (KS == 2) {
                st_d = 0.f;
#pragma unroll
                for (int i = 0; i < ORW; i++)
#pragma unroll
                    for (int j = 0; j < AT<T>::VN; j++) st_d = fmaf(st_o[i].get(j), st_g[i].get(j), st_d);
            }
            if (tid < QT) {
                dst[tid] = st_l * (EXACT ? 1.0f : LOG2E_F);
                dst[QT + tid] = st_d / keep_scale;
                reinterpret_cast<uint32_t*>(dst)[2 * QT + tid] = attn_row_hash(drop.seed, drop.stream, (uint32_t)(by * Tn + qt + tid));
            }
        };
        const int qstart = KS ? (kb * 32) / 64 * 64 : kb * 128;
        sq.load(qg, rs, qstart, Tn, tid);
        so.load(dog, E, qstart, Tn, tid);
        load_rows(qstart);
        sq.store(Qb, tid);
        so.store(Qb + IMG, tid);
        store_rows(Lb, qstart);
        __syncthreads();
        // One 64-query tile.  `interior` (compile time) = every query row of the tile lies below every key of the block and every
        // row and key exists: no mask code in that instance (see the dQ kernel: the if-converted mask was a fifth of the vector
        // instructions of every sub-tile).
        auto tile = [&](auto interior, const int qts, const int it) __attribute__((always_inline)) {
            constexpr bool INT = decltype(interior)::value;
            // KS stages into ONE buffer (a barrier in front of the refill): 43 KiB of LDS at D = 16, three workgroups per CU -- the
            // double-buffered 86 KiB left one per CU and the 512 workgroups of the default configuration took two rounds
            const int sb = KS ? 0 : (it & 1);
            const T* Qs = Qb + sb * 2 * IMG + wq * G::S;
            const T* Os = Qs + IMG;
            const float* Ls = Lb + sb * 3 * QT + wq;
            const bool more = qts + QT < Tn;
            const int qt0 = qts + wq;                 // first query of this wave's 64
            if (more) {
                sq.load(qg, rs, qts + QT, Tn, tid);
                so.load(dog, E, qts + QT, Tn, tid);
                load_rows(qts + QT);
            }
#pragma unroll
            for (int sub = 0; sub < 2; sub++) {
                const int qb0 = qt0 + 32 * sub;
                if (!INT && (qb0 + 31 < k0w || qb0 >= Tn || k0w >= Tn)) continue;     // wave-uniform: all (q, key) pairs masked
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
                s = mma_rows<T, D>(Qs, 32 * sub, kf, lane, s);              // S[q][key]
                dp = mma_rows<T, D>(Os, 32 * sub, vf, lane, dp);            // dP~[q][key]
                // row constants of the 16 query rows this lane sees: rows 8g+4h .. +3 are consecutive -> 16-byte reads
                f32x4 lq[4], dq4[4];
                __attribute__((ext_vector_type(4))) uint32_t rh4[4];
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const int ql = 32 * sub + 8 * g + 4 * h;
                    lq[g] = *reinterpret_cast<const f32x4*>(Ls + ql);
                    dq4[g] = *reinterpret_cast<const f32x4*>(Ls + QT + ql);
                    if constexpr (DROP) rh4[g] = *reinterpret_cast<const __attribute__((ext_vector_type(4))) uint32_t*>(Ls + 2 * QT + ql);
                }
                f32x16 pt;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    if constexpr (EXACT) pt[r] = expf(s[r] * scale - lq[r >> 2][r & 3]);
                    else pt[r] = fast_exp2(fmaf(s[r], c2, -lq[r >> 2][r & 3]));        // lse*log2(e) in this mode
                }
                if constexpr (!INT) {
                    const bool edge = EXACT || (qb0 < k0w + 32) || (qb0 + 32 > Tn) || (k0w + 32 > Tn);   // wave-uniform
                    if (edge) {
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const int qq = qt0 + 32 * sub + rho(r, h);
                            if ((key > qq) || (qq >= Tn) || !kvalid) pt[r] = 0.f;
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float p = pt[r];
                    if constexpr (EXACT || !DROP) {
                        float dpv = dp[r];
                        float pd = p;
                        if constexpr (DROP) {
                            const bool keep = __umul24(rh4[r >> 2][r & 3] ^ kgG, kC) >= drop.thr;
                            dpv = keep ? dpv : 0.f;
                            pd = keep ? p : 0.f;
                        }
                        pt[r] = pd;                                   // (dropped) probabilities feed dV
                        s[r] = p * (dpv - dq4[r >> 2][r & 3]);        // dS/f feeds dK
                    } else {
                        // p (M dP~ - delta/f) = (M p) dP~ - p delta/f: ONE select (the masked probability, which dV needs anyway), a
                        // multiply and an fma instead of two selects, a subtract and a multiply
                        const bool keep = __umul24(rh4[r >> 2][r & 3] ^ kgG, kC) >= drop.thr;
                        const float pd = keep ? p : 0.f;
                        pt[r] = pd;
                        s[r] = fmaf(pd, dp[r], -(p * dq4[r >> 2][r & 3]));
                    }
                }
#pragma unroll
                for (int dt = 0; dt < G::DT; dt++) {
                    dv[dt] = mma_acc_b<T, D>(Os, 32 * sub, dt, pt, lane, dv[dt]);
                    dk[dt] = mma_acc_b<T, D>(Qs, 32 * sub, dt, s, lane, dk[dt]);
                }
            }
            if (more) {
                if constexpr (KS) __syncthreads();
                T* nbuf = Qb + (KS ? 0 : (sb ^ 1)) * 2 * IMG;
                sq.store(nbuf, tid);
                so.store(nbuf + IMG, tid);
                store_rows(Lb + (KS ? 0 : (sb ^ 1)) * 3 * QT, qts + QT);
            }
            __syncthreads();
        };
        // the diagonal block's tiles (masked), then the tiles below it (interior), then a ragged last tile (masked)
        int qt0 = qstart, it = 0;
        const int diag_end = EXACT ? Tn : min(Tn, KS ? k0w + 32 : qstart + 128);
        for (; qt0 < diag_end; qt0 += QT, it++) tile(std::false_type{}, qt0, it);
        for (; qt0 + QT <= Tn; qt0 += QT, it++) tile(std::true_type{}, qt0, it);
        for (; qt0 < Tn; qt0 += QT, it++) tile(std::false_type{}, qt0, it);
        if constexpr (KS) {
            // sum of the four waves' partial dK^T / dV^T tiles (the last tile's barrier has passed: the staging buffers are free)
            float* mg = reinterpret_cast<float*>(smem_raw);
            if (wave > 0) {
#pragma unroll
                for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        mg[(((wave - 1) * 2 * G::DT + 2 * dt) * 16 + r) * 64 + lane] = dk[dt][r];
                        mg[(((wave - 1) * 2 * G::DT + 2 * dt + 1) * 16 + r) * 64 + lane] = dv[dt][r];
                    }
            }
            __syncthreads();
            if (wave > 0) continue;               // (single phase: leaves the loop)
#pragma unroll
            for (int w = 0; w < 3; w++)
#pragma unroll
                for (int dt = 0; dt < G::DT; dt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        dk[dt][r] += mg[((w * 2 * G::DT + 2 * dt) * 16 + r) * 64 + lane];
                        dv[dt][r] += mg[((w * 2 * G::DT + 2 * dt + 1) * 16 + r) * 64 + lane];
                    }
        }
        const float row_rs = (lr.rstd && kvalid) ? lr.rstd[(int64_t)b * Tn + key] : 1.f;
#pragma unroll
        for (int dt = 0; dt < G::DT; dt++) {
            store_t_tile<T, D>(dkg, rs, key, kvalid, dt, dk[dt], scale * keep_scale * row_rs, h);
            store_t_tile<T, D>(dvg, rs, key, kvalid, dt, dv[dt], keep_scale * row_rs, h);
        }
        if (bias_grad) {
            colsum_t_tiles<T, D>(bias_grad + E + hd * D, kvalid, dk, scale * keep_scale, h, lane);
            colsum_t_tiles<T, D>(bias_grad + 2 * E + hd * D, kvalid, dv, keep_scale, h, lane);
        }
    }
}
template <typename T, int D, bool DROP>
__global__ __launch_bounds__(256, (Occ<T, D>::MINW)) void attn_dkv_kernel(const T* __restrict__ qkv, const T* __restrict__ d_o,
                                                                          const float* __restrict__ lse,
                                                                          const float* __restrict__ delta, T* __restrict__ dqkv,
                                                                          float* __restrict__ bias_grad, int Tn, int H, float scale,
                                                                          DropCfg drop) {
    attn_dkv_body<T, D, DROP, 0>(qkv, d_o, lse, delta, dqkv, bias_grad, Tn, H, scale, drop, nullptr, 0);
}
template <typename T, int D, bool DROP>
__global__ __launch_bounds__(256, (Occ<T, D>::MINW)) void attn_dkv_ln_kernel(const T* __restrict__ qkv, const T* __restrict__ d_o,
                                                                          const float* __restrict__ lse,
                                                                          const float* __restrict__ delta, T* __restrict__ dqkv,
                                                                          float* __restrict__ bias_grad, int Tn, int H, float scale,
                                                                          DropCfg drop, AttnLnRows lr) {
    attn_dkv_body<T, D, DROP, 0>(qkv, d_o, lse, delta, dqkv, bias_grad, Tn, H, scale, drop, nullptr, 0, lr);
}
// The whole backward of a small grid in one launch: grid (2 * ceil(T/32), B*H); even x = dK/dV of key block x/2, odd x = dQ of query
// block ceil(T/32) - 1 - x/2 -- the heaviest blocks of both roles first, the lightest last, so the second round of workgroups (two
// fit a CU) fills the slots the light ones leave.  (Side by side on two streams the pair lost to its event fork / join, NEGATIVE_RESULTS.)
template <typename T, int D, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_bwd_ks_kernel(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o,
                                                             const float* __restrict__ lse, float* __restrict__ delta, T* __restrict__ dqkv,
                                                             float* __restrict__ bias_grad, int Tn, int H, float scale, DropCfg drop) {
    const int x = blockIdx.x, nqb = (int)gridDim.x >> 1;
    if (x & 1) attn_dq_body<T, D, DROP, 1>(qkv, o, d_o, lse, delta, dqkv, bias_grad, Tn, H, scale, drop, -1, nqb - 1 - (x >> 1));
    else attn_dkv_body<T, D, DROP, 2>(qkv, d_o, lse, delta, dqkv, bias_grad, Tn, H, scale, drop, o, x >> 1);
}
// ... and as two launches where the merged grid would not be resident at once (the default configuration at T = 1024: 1024 workgroups on
// 512 slots took 59 us merged against 19 + 29 us apart); dK/dV then reads the delta the dQ launch stored.
template <typename T, int D, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_dq_ks_kernel(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o,
                                                            const float* __restrict__ lse, float* __restrict__ delta, T* __restrict__ dqkv,
                                                            float* __restrict__ bias_grad, int Tn, int H, float scale, DropCfg drop) {
    attn_dq_body<T, D, DROP, 1>(qkv, o, d_o, lse, delta, dqkv, bias_grad, Tn, H, scale, drop, -1, (int)gridDim.x - 1 - (int)blockIdx.x);
}
template <typename T, int D, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_dkv_ks_kernel(const T* __restrict__ qkv, const T* __restrict__ d_o, const float* __restrict__ lse,
                                                             const float* __restrict__ delta, T* __restrict__ dqkv, float* __restrict__ bias_grad,
                                                             int Tn, int H, float scale, DropCfg drop) {
    attn_dkv_body<T, D, DROP, 1>(qkv, d_o, lse, delta, dqkv, bias_grad, Tn, H, scale, drop, nullptr, (int)blockIdx.x);
}

// =================================================================================================
// host launchers.  What a launch becomes is decided in attn_plan.h (attn_plan_fwd / attn_plan_bwd); the code below asks the
// device the facts the plan needs, refuses before anything is enqueued and launches what the plan names.
// =================================================================================================
int colsum_run(void* stream, const void* X, int ldx, float* out, int rows, int cols, int dtype, float* det_ws, size_t det_ws_bytes);   // elementwise.hip

#define ATTN_GEO_IS(D) (attn_lds_stride(true, D) == Geo<bf16_t, D>::S && attn_lds_stride(false, D) == Geo<float, D>::S)
static_assert(ATTN_GEO_IS(16) && ATTN_GEO_IS(32) && ATTN_GEO_IS(64) && ATTN_GEO_IS(128), "attn_plan.h restates Geo<T, D>::S");

// COMPOSER_ATTN_KS=0 turns the key-split kernels off, =1 forces them wherever they exist (tests); COMPOSER_ATTN_BIAS_PASS=<MiB>
// moves the bound of the bias column-sum pass, 0 = never.  Both read once per process.
static AttnEnv attn_env() {
    static const AttnEnv env = [] {
        AttnEnv e;
        if (const char* v = getenv("COMPOSER_ATTN_KS")) e.ks_mode = atoi(v);
        if (const char* v = getenv("COMPOSER_ATTN_BIAS_PASS")) e.bias_pass_mib = atoi(v);
        return e;
    }();
    return env;
}
template <typename K> static int attn_wgs_per_cu(K kernel, size_t smem) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, smem) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
#define ATTN_OPTIN(kernel, bytes) HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)))
// LDS opt-in of the key-split kernels (4 * 256 staged rows), decided once per (type, head size) for all of them together: a device
// or driver that refuses it keeps the 128-row kernels, forward and backward alike (the GEMM ring falls back to its two-stage loop
// in the same situation) instead of failing every small-grid attention call.
template <typename T, int D> static bool attn_ks_available() {
    static const bool ok = [] {
        const int ks = (int)attn_ks_smem(true, D), kv = (int)attn_ks_kv_smem(true, D);
        const void* big[] = {(const void*)attn_fwd_kernel<T, D, true, false, true>, (const void*)attn_fwd_kernel<T, D, false, false, true>,
                             (const void*)attn_bwd_ks_kernel<T, D, true>, (const void*)attn_bwd_ks_kernel<T, D, false>,
                             (const void*)attn_dq_ks_kernel<T, D, true>, (const void*)attn_dq_ks_kernel<T, D, false>};
        const void* half[] = {(const void*)attn_dkv_ks_kernel<T, D, true>, (const void*)attn_dkv_ks_kernel<T, D, false>};
        bool good = true;
        for (const void* f : big) good = good && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, ks) == hipSuccess;
        for (const void* f : half) good = good && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kv) == hipSuccess;
        if (!good) (void)hipGetLastError();
        return good;
    }();
    return ok;
}
// The device facts of the 128-row kernels (KERNEL: CMP_ATTN_K_*): resident workgroups per CU of the kernel the block plan is for,
// asked once per (kernel, type, head size).  An image above 64 KiB needs its opt-in before the occupancy can be asked, so the opt-in
// of that kernel set stays here, ahead of the query, on every launch.
template <typename T, int D, int KERNEL> static int attn_rows_caps(AttnCaps* c) {
    constexpr size_t smem = attn_rows_smem(std::is_same<T, bf16_t>::value, D);
    if constexpr (KERNEL == CMP_ATTN_K_FWD) {
        if (attn_fwd_optin(smem)) {
            ATTN_OPTIN((attn_fwd_kernel<T, D, true>), smem);
            ATTN_OPTIN((attn_fwd_kernel<T, D, false>), smem);
        }
        static const int wgs_per_cu = attn_wgs_per_cu(attn_fwd_kernel<T, D, true>, smem);
        c->wgs_per_cu = wgs_per_cu;
    } else if constexpr (KERNEL == CMP_ATTN_K_DQ_LN) {
        if (attn_bwd_optin(smem)) {
            ATTN_OPTIN((attn_dq_ln_kernel<T, D, true>), smem);
            ATTN_OPTIN((attn_dq_ln_kernel<T, D, false>), smem);
            ATTN_OPTIN((attn_dkv_ln_kernel<T, D, true>), smem + ATTN_DKV_EXTRA);
            ATTN_OPTIN((attn_dkv_ln_kernel<T, D, false>), smem + ATTN_DKV_EXTRA);
        }
        static const int wgs_per_cu_ln = attn_wgs_per_cu(attn_dq_ln_kernel<T, D, true>, smem);
        c->wgs_per_cu = wgs_per_cu_ln;
    } else {
        if (attn_bwd_optin(smem)) {
            ATTN_OPTIN((attn_dq_kernel<T, D, true>), smem);
            ATTN_OPTIN((attn_dq_kernel<T, D, false>), smem);
            ATTN_OPTIN((attn_dkv_kernel<T, D, true>), smem + ATTN_DKV_EXTRA);
            ATTN_OPTIN((attn_dkv_kernel<T, D, false>), smem + ATTN_DKV_EXTRA);
        }
        static const int wgs_per_cu = attn_wgs_per_cu(attn_dq_kernel<T, D, true>, smem);
        c->wgs_per_cu = wgs_per_cu;
    }
    return CMP_OK;
}
// ... and of one launch: the key-split set first where it is built and the launch may use it; nothing of the 128-row kernels when
// the launch then takes the key split.
template <typename T, int D, bool BACKWARD> static int attn_caps(const AttnDesc& d, const AttnEnv& env, AttnCaps* c) {
    constexpr bool bf = std::is_same<T, bf16_t>::value;
    if constexpr (BACKWARD && bf) {
        if (d.ln.rstd) return attn_rows_caps<T, D, CMP_ATTN_K_DQ_LN>(c);
    }
    if constexpr (attn_ks_built(bf, D)) {
        if (BACKWARD || !d.amask) {
            c->ks_ok = attn_ks_available<T, D>();
            if (attn_key_split(d.T, d.B * d.H, D, bf, env, c->ks_ok)) return CMP_OK;
        }
    }
    return attn_rows_caps<T, D, BACKWARD ? CMP_ATTN_K_DQ : CMP_ATTN_K_FWD>(c);
}

// `DROP` inside the statement is the compile-time form of `drop`
#define DISPATCH_DROP(drop, ...)                                  \
    if (drop) { constexpr bool DROP = true; __VA_ARGS__; }        \
    else { constexpr bool DROP = false; __VA_ARGS__; }
// launch i of plan p on stream s between the timing marks of its class: `grid` and `lds` inside the statement are the plan's
#define ATTN_LAUNCH(i, ...)                                                    \
    do {                                                                       \
        const AttnLaunch& l_ = p.l[i];                                         \
        const dim3 grid(l_.grid_x, l_.grid_y);                                 \
        const size_t lds = l_.smem;                                            \
        if (l_.cls >= 0) PROF_START(l_.cls, s);                                \
        DISPATCH_DROP(p.drop, __VA_ARGS__)                                     \
        if (l_.cls >= 0) PROF_STOP(l_.cls, s, l_.work, l_.bytes);              \
        KERNEL_CHECK();                                                        \
    } while (0)

template <typename T, int D> static int launch_fwd(hipStream_t s, const AttnDesc& d) {
    constexpr bool bf = std::is_same<T, bf16_t>::value;
    const AttnEnv env = attn_env();
    AttnCaps caps;
    if (const int rc = attn_caps<T, D, false>(d, env, &caps)) return rc;
    const AttnPlan p = attn_plan_fwd(d, env, caps);
    const DropCfg drop = make_drop(d.p_drop, d.seed, d.rng_stream);
    const T* qkv = (const T*)d.qkv;
    T* o = (T*)d.o;
    switch (p.form) {
        case CMP_ATTN_FWD_KS:
            if constexpr (attn_ks_built(bf, D))
                ATTN_LAUNCH(0, attn_fwd_kernel<T, D, DROP, false, true><<<grid, 256, lds, s>>>(qkv, o, d.lse, d.T, d.H, d.scale, drop, -1, nullptr));
            return CMP_OK;
        case CMP_ATTN_FWD_ROWS:
            ATTN_LAUNCH(0, attn_fwd_kernel<T, D, DROP><<<grid, 256, lds, s>>>(qkv, o, d.lse, d.T, d.H, d.scale, drop, p.plan_u, nullptr));
            return CMP_OK;
        default:         // CMP_ATTN_FWD_MASK: the instances with the mask term take their opt-in here (the plain ones: attn_rows_caps)
            if (p.optin) {
                ATTN_OPTIN((attn_fwd_kernel<T, D, true, true>), p.l[0].smem);
                ATTN_OPTIN((attn_fwd_kernel<T, D, false, true>), p.l[0].smem);
            }
            ATTN_LAUNCH(0, attn_fwd_kernel<T, D, DROP, true><<<grid, 256, lds, s>>>(qkv, o, d.lse, d.T, d.H, d.scale, drop, p.plan_u, d.amask));
            return CMP_OK;
    }
}
template <typename T, int D> static int launch_bwd(hipStream_t s, const AttnDesc& d) {
    constexpr bool bf = std::is_same<T, bf16_t>::value;
    const AttnEnv env = attn_env();
    AttnCaps caps;
    if (const int rc = attn_caps<T, D, true>(d, env, &caps)) return rc;
    const AttnPlan p = attn_plan_bwd(d, env, caps);
    const DropCfg drop = make_drop(d.p_drop, d.seed, d.rng_stream);
    const T *qkv = (const T*)d.qkv, *o = (const T*)d.o, *d_o = (const T*)d.d_o;
    T* dqkv = (T*)d.dqkv;
    float* const bias = p.bias_fused ? d.bias_grad : nullptr;
    switch (p.form) {
        case CMP_ATTN_BWD_LN:
            if constexpr (bf) {
                ATTN_LAUNCH(0, attn_dq_ln_kernel<T, D, DROP><<<grid, 256, lds, s>>>(qkv, o, d_o, d.lse, d.delta, dqkv, bias, d.T, d.H, d.scale, drop, p.plan_u, d.ln));
                ATTN_LAUNCH(1, attn_dkv_ln_kernel<T, D, DROP><<<grid, 256, lds, s>>>(qkv, d_o, d.lse, d.delta, dqkv, bias, d.T, d.H, d.scale, drop, d.ln));
            }
            break;
        case CMP_ATTN_BWD_KS2:         // dK/dV reads the delta the dQ launch stored
            if constexpr (attn_ks_built(bf, D)) {
                ATTN_LAUNCH(0, attn_dq_ks_kernel<T, D, DROP><<<grid, 256, lds, s>>>(qkv, o, d_o, d.lse, d.delta, dqkv, bias, d.T, d.H, d.scale, drop));
                ATTN_LAUNCH(1, attn_dkv_ks_kernel<T, D, DROP><<<grid, 256, lds, s>>>(qkv, d_o, d.lse, d.delta, dqkv, bias, d.T, d.H, d.scale, drop));
            }
            break;
        case CMP_ATTN_BWD_KS1:
            if constexpr (attn_ks_built(bf, D))
                ATTN_LAUNCH(0, attn_bwd_ks_kernel<T, D, DROP><<<grid, 256, lds, s>>>(qkv, o, d_o, d.lse, d.delta, dqkv, bias, d.T, d.H, d.scale, drop));
            break;
        default:
            ATTN_LAUNCH(0, attn_dq_kernel<T, D, DROP><<<grid, 256, lds, s>>>(qkv, o, d_o, d.lse, d.delta, dqkv, bias, d.T, d.H, d.scale, drop, p.plan_u));
            ATTN_LAUNCH(1, attn_dkv_kernel<T, D, DROP><<<grid, 256, lds, s>>>(qkv, d_o, d.lse, d.delta, dqkv, bias, d.T, d.H, d.scale, drop));
            break;
    }
    if (p.bias_pass) return colsum_run(s, d.dqkv, 3 * d.H * d.D, d.bias_grad, d.B * d.T, 3 * d.H * d.D, CMP_BF16, nullptr, 0);
    return CMP_OK;
}

#define DISPATCH_D(T, fn, ...)                                                         \
    switch (d.D) {                                                                     \
        case 16: return fn<T, 16>(__VA_ARGS__);                                        \
        case 32: return fn<T, 32>(__VA_ARGS__);                                        \
        case 64: return fn<T, 64>(__VA_ARGS__);                                        \
        case 128: return fn<T, 128>(__VA_ARGS__);                                      \
    }
// refusals and the empty launch (attn_plan_check) come before the first question to the device; then the kernels of (dtype, D)
#define ATTN_RUN(backward, fn, ...)                                                    \
    do {                                                                               \
        const AttnPlan chk = attn_plan_check(d, backward);                             \
        if (chk.status != CMP_OK) {                                                    \
            cmp_set_error("%s", chk.msg);                                              \
            return chk.status;                                                         \
        }                                                                              \
        if (chk.empty) return CMP_OK;                                                  \
        if (d.dtype == CMP_BF16) { DISPATCH_D(bf16_t, fn, __VA_ARGS__) }               \
        else { DISPATCH_D(float, fn, __VA_ARGS__) }                                    \
        return CMP_ERR_INVALID;       /* (not reached: every other head size was refused) */ \
    } while (0)

int attn_fwd_run(void* stream, const AttnDesc& d) { ATTN_RUN(false, launch_fwd, (hipStream_t)stream, d); }

// the C ABI's positional arguments as a launch record
static AttnDesc attn_abi_desc(int dtype, int B, int T, int H, int D, int scale, float p_drop, uint64_t seed, uint32_t rng_stream, const void* qkv,
                              const void* o, const float* lse) {
    AttnDesc d;
    d.dtype = dtype; d.B = B; d.T = T; d.H = H; d.D = D;
    d.scale = scale ? 1.0f / sqrtf((float)D) : 1.0f;
    d.p_drop = p_drop; d.seed = seed; d.rng_stream = rng_stream;
    d.qkv = qkv; d.o = const_cast<void*>(o); d.lse = const_cast<float*>(lse);
    return d;
}
extern "C" int cmp_k_attn_fwd(void* stream, const void* qkv, void* o, float* lse, int B, int T, int H, int D, int scale,
                              int dtype, float p_drop, uint64_t seed, uint32_t rng_stream) {
    return attn_fwd_run(stream, attn_abi_desc(dtype, B, T, H, D, scale, p_drop, seed, rng_stream, qkv, o, lse));
}

// The attention probabilities themselves (Transformer(..., output_attention_weights=True), transformer.py:360-369, 808-809):
// out[b][h][i - q0][j] = dropout(softmax row i)[j] for the queries i in [q0, Tn), recomputed from q, k and the forward
// kernel's row log-sum-exp.  An inspection path (the [B,H,T,T] tensor the hot kernels never write): one workgroup per
// (batch, head, query), a thread per key, plain dot products.
template <typename T>
__global__ __launch_bounds__(256) void attn_probs_kernel(const T* __restrict__ qkv, const float* __restrict__ lse,
                                                         const float* __restrict__ amask, float* __restrict__ out, int q0, int Tn,
                                                         int H, int D, float scale, DropCfg drop) {
    const int bh = blockIdx.y, i = q0 + blockIdx.x, b = bh / H, hd = bh % H;
    const int E = H * D;
    const int64_t rs = 3 * E;
    const T* qrow = qkv + ((int64_t)b * Tn + i) * rs + hd * D;
    const float l = lse[(int64_t)bh * Tn + i];
    const uint32_t rowh = attn_row_hash(drop.seed, drop.stream, (uint32_t)(bh * Tn + i));
    float* orow = out + ((int64_t)bh * (Tn - q0) + (i - q0)) * Tn;
    for (int j = threadIdx.x; j < Tn; j += blockDim.x) {
        const T* krow = qkv + ((int64_t)b * Tn + j) * rs + E + hd * D;
        float sdot = 0.f;
        for (int d = 0; d < D; d++) sdot = fmaf(to_f32<T>(qrow[d]), to_f32<T>(krow[d]), sdot);
        float v = sdot * scale;
        if (j > i) v = -1e4f;                                          // :351-354
        if (amask) v += amask[(int64_t)b * Tn + j];                    // :356-358
        float pr = expf(v - l);                                        // :360
        if (drop.thr) pr = attn_elem_hash(rowh, (uint32_t)j) >= drop.thr ? pr * drop.scale : 0.f;     // :361
        orow[j] = pr;
    }
}

int attn_probs_run(void* stream, const AttnDesc& d, int q0, float* out) {
    if (d.B * (d.T - q0) <= 0) return CMP_OK;
    hipStream_t s = (hipStream_t)stream;
    const DropCfg drop = make_drop(d.p_drop, d.seed, d.rng_stream);
    const dim3 grid(d.T - q0, d.B * d.H);
    if (d.dtype == CMP_BF16) attn_probs_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)d.qkv, d.lse, d.amask, out, q0, d.T, d.H, d.D, d.scale, drop);
    else attn_probs_kernel<float><<<grid, 256, 0, s>>>((const float*)d.qkv, d.lse, d.amask, out, q0, d.T, d.H, d.D, d.scale, drop);
    KERNEL_CHECK();
    return CMP_OK;
}

int attn_bwd_run(void* stream, const AttnDesc& d) { ATTN_RUN(true, launch_bwd, (hipStream_t)stream, d); }

// One-shot for the kernel-level tests that call cmp_k_attn_bwd directly (per calling thread): the next cmp_k_attn_bwd also
// adds the column sums of [dQ | dK | dV] to out[0..3E) (the c_attn bias gradient).  The model driver sets AttnDesc::bias_grad itself.
static thread_local float* t_attn_bias_next = nullptr;
extern "C" int cmp_attn_bwd_bias_next(float* out) {
    t_attn_bias_next = out;
    return CMP_OK;
}

// ... and (round 6) stores its gradient rows scaled by rstd[token] (AttnLnRows, attn_plan.h)
static thread_local AttnLnRows t_attn_ln_next;
extern "C" int cmp_attn_bwd_ln_next(const float* rstd) {
    t_attn_ln_next = AttnLnRows{rstd};
    return CMP_OK;
}

extern "C" int cmp_k_attn_bwd(void* stream, const void* qkv, const void* o, const void* d_o, const float* lse,
                              float* delta_ws, void* dqkv, int B, int T, int H, int D, int scale, int dtype,
                              float p_drop, uint64_t seed, uint32_t rng_stream) {
    AttnDesc d = attn_abi_desc(dtype, B, T, H, D, scale, p_drop, seed, rng_stream, qkv, o, lse);
    d.d_o = d_o; d.delta = delta_ws; d.dqkv = dqkv;
    d.bias_grad = t_attn_bias_next;
    t_attn_bias_next = nullptr;
    d.ln = t_attn_ln_next;
    t_attn_ln_next = AttnLnRows();
    return attn_bwd_run(stream, d);
}

// the plan of the launch cmp_k_attn_fwd / cmp_k_attn_bwd would make of such a record on a device with these caps: no HIP call
extern "C" int cmp_attn_plan(int dtype, int B, int T, int H, int D, float p_drop, int has_amask, int want_bias, int has_ln_rows,
                             int backward, int wgs_per_cu, int ks_ok, cmp_attn_plan_info* out) {
    CMP_REQUIRE(out != nullptr, "attn_plan: out is null");
    static const float some = 0.f;            // any non-null address: the plan looks at null-ness only
    AttnDesc d;
    d.dtype = dtype; d.B = B; d.T = T; d.H = H; d.D = D; d.p_drop = p_drop;
    if (has_amask) d.amask = &some;
    if (want_bias) d.bias_grad = const_cast<float*>(&some);
    if (has_ln_rows) d.ln.rstd = &some;
    AttnCaps caps;
    caps.ks_ok = ks_ok != 0;
    caps.wgs_per_cu = wgs_per_cu;
    const AttnPlan p = backward ? attn_plan_bwd(d, attn_env(), caps) : attn_plan_fwd(d, attn_env(), caps);
    if (p.status != CMP_OK) {
        cmp_set_error("%s", p.msg);
        return p.status;
    }
    *out = cmp_attn_plan_info{p.form, p.drop, p.nlaunch, {(int)p.l[0].grid_x, (int)p.l[1].grid_x}, {(int)p.l[0].grid_y, (int)p.l[1].grid_y}, (int)p.block,
                              {(int64_t)p.l[0].smem, (int64_t)p.l[1].smem}, p.optin, p.plan_u, p.bias_fused, p.bias_pass, {p.l[0].cls, p.l[1].cls},
                              {p.l[0].work, p.l[1].work}, {p.l[0].bytes, p.l[1].bytes}, p.empty};
    return CMP_OK;
}
// what the launcher asks the current device about the kernels of (dtype, D): the key-split opt-in and the occupancy of `kernel`
template <typename T, int D> static int attn_caps_of(int kernel, AttnCaps* c) {
    constexpr bool bf = std::is_same<T, bf16_t>::value;
    if constexpr (attn_ks_built(bf, D)) c->ks_ok = attn_ks_available<T, D>();
    if (kernel == CMP_ATTN_K_FWD) return attn_rows_caps<T, D, CMP_ATTN_K_FWD>(c);
    if (kernel == CMP_ATTN_K_DQ) return attn_rows_caps<T, D, CMP_ATTN_K_DQ>(c);
    if constexpr (bf) {
        if (kernel == CMP_ATTN_K_DQ_LN) return attn_rows_caps<T, D, CMP_ATTN_K_DQ_LN>(c);
    }
    cmp_set_error("attn_caps: no kernel %d for dtype %d", kernel, bf ? CMP_BF16 : CMP_FP32);
    return CMP_ERR_INVALID;
}
extern "C" int cmp_attn_caps(int dtype, int D, int kernel, int* wgs_per_cu, int* ks_ok) {
    CMP_REQUIRE(wgs_per_cu && ks_ok, "attn_caps: null output");
    AttnDesc d;
    d.B = d.T = 1; d.D = D;
    const AttnPlan chk = attn_plan_check(d, false);
    if (chk.status != CMP_OK) {
        cmp_set_error("%s", chk.msg);
        return chk.status;
    }
    AttnCaps c;
    const int rc = [&]() -> int {
        if (dtype == CMP_BF16) { DISPATCH_D(bf16_t, attn_caps_of, kernel, &c) }
        else { DISPATCH_D(float, attn_caps_of, kernel, &c) }
        return CMP_ERR_INVALID;
    }();
    *wgs_per_cu = c.wgs_per_cu;
    *ks_ok = c.ks_ok;
    return rc;
}

