// copyguard.hip -- the scan in front of a guarded draw (include/composer_hip.h, "copy guard"): which columns would extend a verbatim
// training-set match of the row's last M events.  Integers only: the ban words are bitwise what composer_amd/novelty.py copy_bans
// computes on the host.  One scan launch serves all B rows and reads the corpus once; workgroups share nothing but the atomic ORs
// into the ban words and the atomic adds into the counters.  No spin loop; every trip count is bounded by M, B, N, velocity_n and
// the tile sizes; every global index is inside its array (the reads are listed at each load).
// A translation unit of its own: adding it leaves every kernel of the other sources instruction-identical.
#include "model.h"

#define CG_BLOCK 256
#define CG_PER 8                       // corpus positions per lane and grid-stride step: one 16-byte load plus one overlap id
#define CG_HT 512                      // buckets of the LDS table "last token of a window -> rows"
#define CG_NONE 0xFFFFu                // a history code that equals nothing; an empty bucket; the end of a chain
#define CG_KANY 1000                   // no note token met in the window yet: every k in [-N, N] can still match
#define CG_MAX_B 256
#define CG_MAX_M 64
#define CG_MAX_N 24

struct CgParams {
    int64_t n;
    int on0, off0, ts0, tsn;           // the dataset's layout: note bases, the TIME_SHIFT ids
    int vel0, veln;                    // the folded velocity range (veln = 0: none)
    int M, N, B, ld, V, nw;            // nw = ceil(V / 32) words per row
};

__device__ __forceinline__ int cg_fold(int id, const CgParams& P) { return (unsigned)(id - P.vel0) < (unsigned)P.veln ? P.vel0 : id; }
__device__ __forceinline__ bool cg_is_ts(int id, const CgParams& P) { return (unsigned)(id - P.ts0) < (unsigned)P.tsn; }
// the bucket of a folded code: with N > 0 every NOTE_ON (every NOTE_OFF) shares one, since a transposition moves a note inside its range
__device__ __forceinline__ int cg_bucket(int code, const CgParams& P) {
    if (P.N > 0) {
        if ((unsigned)(code - P.on0) < 128u) code = P.on0;
        else if ((unsigned)(code - P.off0) < 128u) code = P.off0;
    }
    return (code ^ (code >> 9)) & (CG_HT - 1);
}

// every word of both outputs: the row's words start as the chain's static words, its count at 0 (or stays: a chain's running counter)
__global__ __launch_bounds__(256) void copyguard_init_kernel(const uint32_t* __restrict__ sw, uint32_t* __restrict__ words,
                                                             unsigned long long* __restrict__ count, int B, int nw, int keep_count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B * nw) words[i] = sw ? sw[i % nw] : 0u;
    if (i < B && !keep_count) count[i] = 0ull;
}

// column v joins row r's bans: not a TIME_SHIFT, inside the vocabulary, an id a history token could be
__device__ __forceinline__ void cg_ban(uint32_t* __restrict__ words, unsigned long long* __restrict__ count, const CgParams& P, int r, int v) {
    if (v < 0 || v >= P.V || v >= 65535 || cg_is_ts(v, P)) return;
    const uint32_t bit = 1u << (v & 31);
    const uint32_t old = atomicOr(words + (size_t)r * P.nw + (v >> 5), bit);          // v < V: word v / 32 < nw
    if (!(old & bit)) atomicAdd(count + r, 1ull);
}

// Row r against corpus position p (M <= p < n): the window c[p - M .. p) against the row's M history codes, backwards, so that almost
// every candidate leaves at the first or second compare.  The first note token met fixes the only k that can still match.
__device__ __forceinline__ void cg_try(const uint16_t* __restrict__ ids, const uint32_t* __restrict__ sbits, const CgParams& P,
                                       const uint16_t* __restrict__ w, int r, int64_t p, int cn, uint32_t* __restrict__ words,
                                       unsigned long long* __restrict__ count) {
    int k = CG_KANY;
    for (int j = 0; j < P.M; j++) {
        const int hc = w[P.M - 1 - j];
        if (hc == (int)CG_NONE) return;
        const int cc = cg_fold((int)ids[p - 1 - j], P);                    // p - M <= p - 1 - j <= p - 1: inside [0, n)
        const unsigned pon = (unsigned)(hc - P.on0), poff = (unsigned)(hc - P.off0);
        if (pon < 128u || poff < 128u) {
            const int base = pon < 128u ? P.on0 : P.off0;
            const int d = cc - base;
            if ((unsigned)d >= 128u) return;                               // (the corpus pitch is in 0..127: p + k "stays inside")
            const int diff = d - (hc - base);
            if (k == CG_KANY) {
                if (diff > P.N || diff < -P.N) return;
                k = diff;
            } else if (diff != k) return;
        } else if (cc != hc) return;
    }
    if (sbits)
        for (int64_t q = p - P.M + 1; q <= p; q++)                         // 1 <= q <= p < n: word q / 32 < ceil(n / 32)
            if ((sbits[q >> 5] >> (int)(q & 31)) & 1u) return;
    if ((unsigned)(cn - P.vel0) < (unsigned)P.veln) {
        for (int v = P.vel0; v < P.vel0 + P.veln; v++) cg_ban(words, count, P, r, v);
        return;
    }
    const unsigned con = (unsigned)(cn - P.on0), coff = (unsigned)(cn - P.off0);
    if (con < 128u || coff < 128u) {
        const int base = con < 128u ? P.on0 : P.off0, q = cn - base;
        const int klo = k == CG_KANY ? -P.N : k, khi = k == CG_KANY ? P.N : k;
        for (int kk = klo; kk <= khi; kk++)
            if ((unsigned)(q - kk) < 128u) cg_ban(words, count, P, r, base + q - kk);
        return;
    }
    cg_ban(words, count, P, r, cn);
}

// Can history code hc stand for the folded corpus code cc under SOME k in [-N, N]?  The test of the two compares that are made on
// registers, in front of cg_try (which then decides with one k for the whole window).
__device__ __forceinline__ bool cg_may_equal(int hc, int cc, const CgParams& P) {
    const unsigned pon = (unsigned)(hc - P.on0), poff = (unsigned)(hc - P.off0);
    if (pon < 128u || poff < 128u) {
        const int base = pon < 128u ? P.on0 : P.off0;
        const int d = cc - base;
        const int diff = d - (hc - base);
        return (unsigned)d < 128u && diff <= P.N && diff >= -P.N;
    }
    return hc != (int)CG_NONE && cc == hc;
}

// win: [B][M] folded history codes.  a: ids' offset from a 16-byte boundary in elements; chunk ch covers the corpus indices
// ch * 8 - a .. ch * 8 - a + 7, so every chunk that lies wholly inside the stream is one aligned 16-byte load.
__global__ __launch_bounds__(CG_BLOCK) void copyguard_scan_kernel(const uint16_t* __restrict__ ids, const uint32_t* __restrict__ sbits,
                                                                  CgParams P, const int32_t* __restrict__ hist,
                                                                  const int32_t* __restrict__ lens, uint32_t* __restrict__ words,
                                                                  unsigned long long* __restrict__ count, int64_t nchunks, int a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t win[];
    __shared__ unsigned head[CG_HT];
    __shared__ uint16_t nxt[CG_MAX_B];
    const int tid = threadIdx.x;
    for (int i = tid; i < CG_HT; i += CG_BLOCK) head[i] = CG_NONE;
    for (int i = tid; i < P.B * P.M; i += CG_BLOCK) {
        const int r = i / P.M, j = i - r * P.M;
        const int len = min(max(lens[r], 0), P.ld);
        unsigned code = CG_NONE;
        if (len >= P.M) {
            const int id = hist[(size_t)r * P.ld + len - P.M + j];         // 0 <= len - M + j < len <= ld
            if (id >= 0 && id < 65535) code = (unsigned)cg_fold(id, P);
        }
        win[i] = (uint16_t)code;
    }
    __syncthreads();
    for (int r = tid; r < P.B; r += CG_BLOCK) {
        const unsigned last = win[r * P.M + P.M - 1];
        const int len = min(max(lens[r], 0), P.ld);
        if (len >= P.M && last != CG_NONE) nxt[r] = (uint16_t)atomicExch(&head[cg_bucket((int)last, P)], (unsigned)r);
    }
    __syncthreads();
    for (int64_t ch = (int64_t)blockIdx.x * CG_BLOCK + tid; ch < nchunks; ch += (int64_t)gridDim.x * CG_BLOCK) {
        const int64_t q0 = ch * CG_PER - a;
        unsigned t[CG_PER + 1];
        const unsigned tm1 = (q0 >= 1 && q0 - 1 < P.n) ? ids[q0 - 1] : 0u;    // the id in front of the chunk: the second compare of its first position
        if (q0 >= 0 && q0 + CG_PER <= P.n) {
            const uint4 v = *reinterpret_cast<const uint4*>(ids + q0);
            t[0] = v.x & 0xFFFFu; t[1] = v.x >> 16; t[2] = v.y & 0xFFFFu; t[3] = v.y >> 16;
            t[4] = v.z & 0xFFFFu; t[5] = v.z >> 16; t[6] = v.w & 0xFFFFu; t[7] = v.w >> 16;
        } else {
#pragma unroll
            for (int s = 0; s < CG_PER; s++) t[s] = (q0 + s >= 0 && q0 + s < P.n) ? ids[q0 + s] : 0u;
        }
        t[CG_PER] = (q0 + CG_PER >= 0 && q0 + CG_PER < P.n) ? ids[q0 + CG_PER] : 0u;
#pragma unroll
        for (int s = 0; s < CG_PER; s++) {
            const int64_t p = q0 + s + 1;                                  // t[s] = c[p - 1], t[s + 1] = c[p]
            if (p < P.M || p >= P.n) continue;
            const int cn = (int)t[s + 1];
            if (cg_is_ts(cn, P) && !((unsigned)(cn - P.vel0) < (unsigned)P.veln)) continue;       // a TIME_SHIFT continuation bans nothing
            const int c1 = cg_fold((int)t[s], P), c2 = cg_fold((int)(s ? t[s ? s - 1 : 0] : tm1), P);      // c[p - 1], c[p - 2] (read only when M >= 2: p >= 2)
            unsigned r = head[cg_bucket(c1, P)];
            for (int it = 0; r != CG_NONE && it < P.B; it++) {             // a chain holds every row at most once
                // the first two compares on registers and LDS alone: almost every row leaves here, without a global load
                const uint16_t* w = win + r * P.M;
                if (cg_may_equal(w[P.M - 1], c1, P) && (P.M < 2 || cg_may_equal(w[P.M - 2], c2, P)))
                    cg_try(ids, sbits, P, w, (int)r, p, cn, words, count);
                r = nxt[r];
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
int copy_guard_check(const char* who, int64_t n, const cmp_event_grammar* g, const cmp_copy_guard_opts* o) {
    CMP_REQUIRE(o->max_copy >= 1 && o->max_copy <= CG_MAX_M, "%s: max_copy=%d outside [1, %d]", who, o->max_copy, CG_MAX_M);
    CMP_REQUIRE(o->transpose >= 0 && o->transpose <= CG_MAX_N, "%s: transpose=%d outside [0, %d]", who, o->transpose, CG_MAX_N);
    CMP_REQUIRE(g, "%s: the dataset has no event layout: the rule has to know the TIME_SHIFT and the note ids", who);
    CMP_REQUIRE(g->time_shift_n >= 1 && g->time_shift0 >= 0, "%s: TIME_SHIFT ids [%d, %d): a layout names at least one", who,
                g->time_shift0, g->time_shift0 + g->time_shift_n);
    const cmp_novelty_opts no = {1, o->transpose, o->velocity0, o->velocity_n};
    return nov_check(who, n, g, 1, 1, &no);
}

int copy_guard_run(hipStream_t s, const DecGuardCfg& g, const int32_t* hist, const int32_t* lens, int B, int ld, int V,
                   const uint32_t* static_words, uint32_t* words_out, unsigned long long* count_out, bool accumulate) {
    CgParams P;
    P.n = g.n;
    P.on0 = g.layout.note_on0; P.off0 = g.layout.note_off0; P.ts0 = g.layout.time_shift0; P.tsn = g.layout.time_shift_n;
    P.vel0 = g.opts.velocity0; P.veln = g.opts.velocity_n;
    P.M = g.opts.max_copy; P.N = g.opts.transpose;
    P.B = B; P.ld = ld; P.V = V; P.nw = (V + 31) / 32;
    copyguard_init_kernel<<<cdiv(B * P.nw + B, 256), 256, 0, s>>>(static_words, words_out, count_out, B, P.nw, accumulate ? 1 : 0);
    KERNEL_CHECK();
    if (g.n <= P.M) return CMP_OK;                                         // no position p with M <= p < n
    const int a = (int)(((uintptr_t)g.ids & 15) / 2);
    const int64_t nchunks = cdiv64(g.n + a, CG_PER);
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(nchunks, CG_BLOCK), 2048);
    copyguard_scan_kernel<<<grid, CG_BLOCK, (size_t)B * P.M * 2, s>>>(g.ids, g.start_bits, P, hist, lens, words_out, count_out, nchunks, a);
    KERNEL_CHECK();
    return CMP_OK;
}

extern "C" int cmp_k_copy_bans(void* stream, const uint16_t* ids_dev, int64_t n, const uint32_t* start_bits_dev,
                               const cmp_event_grammar* layout, const cmp_copy_guard_opts* opts, const int32_t* hist_dev,
                               const int32_t* lens_dev, int B, int ld, int V, const uint32_t* static_words_dev, uint32_t* words_out,
                               int64_t* count_out) {
    CMP_REQUIRE(ids_dev && opts && hist_dev && lens_dev && words_out && count_out, "k_copy_bans: null argument");
    CMP_REQUIRE(((uintptr_t)ids_dev & 1) == 0, "k_copy_bans: ids_dev is not 2-byte aligned");
    CMP_REQUIRE(B >= 1 && B <= CG_MAX_B, "k_copy_bans: B=%d outside [1, %d]", B, CG_MAX_B);
    CMP_REQUIRE(ld >= 1, "k_copy_bans: ld=%d must be >= 1", ld);
    CMP_REQUIRE(V >= 1, "k_copy_bans: V=%d must be >= 1", V);
    CHECK_RC(copy_guard_check("k_copy_bans", n, layout, opts));
    DecGuardCfg g;
    g.ids = ids_dev;
    g.n = n;
    g.start_bits = start_bits_dev;
    g.layout = *layout;
    g.opts = *opts;
    return copy_guard_run((hipStream_t)stream, g, hist_dev, lens_dev, B, ld, V, static_words_dev, words_out,
                          (unsigned long long*)count_out, false);
}
