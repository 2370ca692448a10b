// score.hip -- per-row scoring of fp32 logits (include/composer_hip.h, "scoring"): log-probability of the target, its rank and the
// entropy of the row's distribution.  One read of the logits and nothing else: no gradient, no atomics, no LDS.
// A translation unit of its own: adding it leaves every kernel of the other sources instruction-identical (tools/isa_hash.py).
// The row reduction itself is score_rows.h's (evalpass.hip sums the same figures per event class).
#include "score_rows.h"

struct ScoreOut {
    float* logp;
    int32_t* rank;
    float* entropy;
};
__device__ __forceinline__ void score_store(const ScoreOut& o, int row, bool valid, float zy, float gmx, float s, float t, int cnt) {
    const float ls = logf(s);
    if (o.logp) o.logp[row] = valid ? score_logp(zy, gmx, ls) : 0.f;
    if (o.rank) o.rank[row] = valid ? cnt : -1;
    if (o.entropy) o.entropy[row] = ls - t * __builtin_amdgcn_rcpf(s);      // (v_rcp_f32: 1 ulp, against the bound's 1e-5)
}

template <bool VEC>
__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ z, int ldz, const int32_t* __restrict__ y,
                                                         ScoreOut out, int rows, int V) {
    const int lane = threadIdx.x & 63;
    score_walk_rows<VEC>(z, ldz, y, rows, V, blockDim.x >> 6, [&](int row, int, bool valid, float zy, float gmx, float s, float t, int cnt) {
        if (lane == 0) score_store(out, row, valid, zy, gmx, s, t, cnt);
    });
}

__global__ __launch_bounds__(256) void score_rows_wide_kernel(const float* __restrict__ z, int ldz, const int32_t* __restrict__ y,
                                                              ScoreOut out, int rows, int V) {
    const int lane = threadIdx.x & 63;
    score_walk_rows_wide(z, ldz, y, rows, V, blockDim.x >> 6, [&](int row, int, bool valid, float zy, float gmx, float s, float t, int cnt) {
        if (lane == 0) score_store(out, row, valid, zy, gmx, s, t, cnt);
    });
}

extern "C" int cmp_k_score_rows(void* stream, const float* logits, int ldz, const int32_t* y, float* logp, int32_t* rank,
                                float* entropy, int rows, int V) {
    CMP_REQUIRE(logits && y, "score_rows: null logits or targets");
    CMP_REQUIRE(V > 0 && V <= ldz && rows >= 0, "score_rows: V=%d ldz=%d rows=%d", V, ldz, rows);
    if (rows == 0 || (!logp && !rank && !entropy)) return CMP_OK;
    hipStream_t s = (hipStream_t)stream;
    const ScoreOut out = {logp, rank, entropy};
    const int grid = std::min(cdiv(rows, 4), 8192);
    const int form = score_rows_form(logits, ldz);
    if (form == 2)
        score_rows_wide_kernel<<<grid, 256, 0, s>>>(logits, ldz, y, out, rows, V);
    else if (form == 0)
        score_rows_kernel<true><<<grid, 256, 0, s>>>(logits, ldz, y, out, rows, V);
    else
        score_rows_kernel<false><<<grid, 256, 0, s>>>(logits, ldz, y, out, rows, V);
    KERNEL_CHECK();
    return CMP_OK;
}
