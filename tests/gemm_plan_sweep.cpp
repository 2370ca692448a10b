// Stand-alone sweep of gemm_plan (composer_amd/csrc/gemm_plan.h) under the host compiler: shows that the header needs no HIP
// and, with -fsanitize=address,undefined, that its 32/64-bit arithmetic does not overflow (tests/test_gemm_plan_host.py builds it).
#include "../composer_amd/csrc/gemm_plan.h"
#include <stdlib.h>

static long cases = 0, refused = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s: dtype=%d ta=%d tb=%d M=%d N=%d K=%d splitk=%d flags=%d\n", #c, d.dtype, d.ta, d.tb, d.M, d.N, d.K, d.splitk, d.flags); exit(1); } } while (0)

static void one(GemmDesc d, const GemmExtra& ex) {
    const GemmPlan p = gemm_plan(d, ex, GemmEnv());
    cases++;
    if (p.status != CMP_OK) { refused++; CHECK(p.msg[0] != 0); return; }
    CHECK(p.grid_x > 0 && p.grid_y > 0 && p.grid_z > 0 && p.block > 0);
    CHECK((int64_t)p.per * p.nsplit >= p.nk && (int64_t)p.per * (p.nsplit - 1) < p.nk);
    const int cap = ex.max_wgs > 0 ? ex.max_wgs : 256;
    if (p.family >= CMP_GEMM_FAM_TILE256) CHECK((int)p.grid_x <= (p.family == CMP_GEMM_FAM_P4_128 ? 2 * cap : cap));
    const int tile = (p.family == CMP_GEMM_FAM_TILE128 || p.family == CMP_GEMM_FAM_RING) ? 128 : 256;
    if (p.kind != EPI_GENERIC) CHECK(d.M % tile == 0 && d.N % tile == 0 && p.family >= CMP_GEMM_FAM_TILE128);
    CHECK(!p.colsum_fused || p.kind != EPI_GENERIC);
    CHECK((p.colsum_fused || p.colsum_pass) == (ex.colsum != nullptr) && !(p.colsum_fused && p.colsum_pass));
    if (p.slabs) CHECK((size_t)p.nsplit * d.M * d.N * 4 <= ex.slab_bytes && p.reduce_grid > 0);
    if ((d.flags & CMP_GEMM_GENERIC) && d.dtype == CMP_BF16) CHECK(p.family == CMP_GEMM_FAM_GENERIC);
}

int main() {
    const int sizes[] = {8, 136, 264, 512, 24576}, ks[] = {64, 72, 160, 200, 512}, flags[] = {0, 1, 2, 4, 8, 16, 48, 128}, splits[] = {1, 2, 5};
    float* const fake = (float*)0x1000;                 // never dereferenced
    for (int dtype = 0; dtype < 2; dtype++) for (int lay = 0; lay < 4; lay++) for (int M : sizes) for (int N : sizes) for (int K : ks)
    for (int epi = 0; epi < 8; epi++) for (int f : flags) for (int sk : splits) for (int ctx = 0; ctx < 2; ctx++) {
        GemmDesc d;
        d.dtype = dtype; d.ta = lay >> 1; d.tb = lay & 1; d.M = M; d.N = N; d.K = K; d.flags = f; d.splitk = sk;
        const int kp = (f & 1) ? (K + 63) / 64 * 64 : K;
        d.A = d.B = d.C = fake; d.lda = d.ta ? M : kp; d.ldb = d.tb ? kp : N; d.ldc = N + 16 * ctx;
        if (epi == 1 || epi == 2 || epi == 4 || epi == 5) d.bias = fake;
        if (epi == 2 || epi == 3) { d.act = epi - 1; d.aux = fake; d.ldaux = N; }
        if (epi == 4 || epi == 5) { d.resid = fake; d.ldr = N; }
        if (epi == 5) d.p_drop = 0.25f;
        if (epi == 6 || sk > 1) d.out_fp32 = 1;
        GemmExtra ex;
        if (epi == 7) ex.colsum = fake;
        if (ctx) { ex.max_wgs = 96; ex.slab_ws = fake; ex.slab_bytes = (size_t)3 * M * N * 4; }
        one(d, ex);
    }
    // the largest model shapes: M . N, the operand spans and nsplit . M . N . 4 in 64 bits
    const int big_splits[] = {1, 64, 4096};
    for (int lay = 0; lay < 4; lay++) for (int f : flags) for (int sk : big_splits) {
        GemmDesc d;
        d.ta = lay >> 1; d.tb = lay & 1; d.M = 131072; d.N = 2048; d.K = 131072; d.flags = f; d.splitk = sk; d.out_fp32 = sk > 1;
        d.A = d.B = d.C = fake; d.lda = d.ta ? d.M : d.K; d.ldb = d.tb ? d.K : d.N; d.ldc = d.N;
        GemmExtra ex;
        ex.slab_ws = fake; ex.slab_bytes = (size_t)1 << 42;
        one(d, ex);
    }
    printf("gemm_plan sweep ok: %ld cases, %ld refused\n", cases, refused);
    return 0;
}
