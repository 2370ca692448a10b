// novelty.hip -- the longest training-set match of every event of a query (include/composer_hip.h, "novelty check").  Integers only:
// every result is bitwise what composer_amd/novelty.py computes on the host.  One atomic maximum per LONG run, nothing else shared
// between workgroups; no spin loop, every trip count bounded by ld and the tile sizes.
// A translation unit of its own: adding it leaves every kernel of the other sources instruction-identical (tools/isa_hash.py).
#include "model.h"

#define NOV_BLOCK 256                  // diagonals per workgroup, one per lane
#define NOV_SCHUNK 512                 // query positions staged in LDS at a time
#define NOV_KT 7                       // transpositions per lane when N > 0 (one counter each; N = 0: one)
#define NOV_NOMATCH 0x10000            // a mapped query token that equals no corpus code
#define NOV_OUTSIDE 0x20000u           // the code of a corpus position outside [0, n): equals no query token
#define NOV_START 0x80000000u          // bit 31 of a staged corpus code: the position is a piece start
#define NOV_POS_MASK ((1ULL << 40) - 1)
#define NOV_MAX_B 256
#define NOV_MAX_LD 32768
#define NOV_MAX_N 24

struct NovParams {
    int64_t n;
    int on0, off0;             // note bases; far below 0 without a layout (no id is a note then)
    int vel0, veln;            // the folded velocity range (veln = 0: none)
    int min_match, nrank;      // nrank = 2 N + 1 transpositions, in rank order 0, -1, +1, -2, +2 ...
    int B, ld;
};

__device__ __forceinline__ int nov_rank_to_k(int r) { return (r & 1) ? -((r + 1) >> 1) : (r >> 1); }

__device__ __forceinline__ int nov_fold(int id, const NovParams& P) { return (unsigned)(id - P.vel0) < (unsigned)P.veln ? P.vel0 : id; }

// the staged code of corpus position p: the folded id, NOV_START on a piece start; NOV_OUTSIDE outside the stream.  The only reads
// of ids and sbits: p in [0, n), word p >> 5 < ceil(n / 32).
__device__ __forceinline__ uint32_t nov_code(const uint16_t* __restrict__ ids, const uint32_t* __restrict__ sbits, const NovParams& P, int64_t p) {
    if (p < 0 || p >= P.n) return NOV_OUTSIDE;
    uint32_t v = (uint32_t)nov_fold((int)ids[p], P);
    if (sbits && ((sbits[p >> 5] >> (int)(p & 31)) & 1u)) v |= NOV_START;
    return v;
}

// One lane per diagonal d = p - s, d in [-(ld - 1), n - 1]; a workgroup owns NOV_BLOCK consecutive diagonals and walks s from
// len - 1 down to 0, so that the running length in a lane's register IS m(s, p, k): a match adds one, a mismatch clears it, and a
// piece start at p clears what (s - 1, p - 1) would continue.  At a fixed s the lanes read consecutive staged codes (ds_read_b32,
// conflict-free); the query token, mapped under the group's KT transpositions when its chunk is staged, is read from one LDS address
// by the whole wave (a broadcast, one 16-byte row of 8 per position when KT = 7).  blockIdx.y picks KT consecutive ranks of the
// transposition.  A lane touches global memory only when a run has reached min_match and beats what a plain read of the key shows (a
// stale read costs an atomic, never a result).  The window of corpus codes is staged once for all B rows when ld fits one chunk,
// else per (row, chunk) -- 768 loads for 131072 cells.
template <int KT>
__global__ __launch_bounds__(NOV_BLOCK) void novelty_match_kernel(const uint16_t* __restrict__ ids, const uint32_t* __restrict__ sbits,
                                                                  NovParams P, const int32_t* __restrict__ x,
                                                                  const int32_t* __restrict__ lens, unsigned long long* keys,
                                                                  int64_t nblocks) {
    constexpr int KP = KT == 1 ? 1 : 8;                    // mapped tokens per query position in LDS: 16-byte rows when KT = 7
    __shared__ uint32_t lc[NOV_BLOCK + NOV_SCHUNK];
    __shared__ __attribute__((aligned(16))) int32_t lx[NOV_SCHUNK * KP];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * KT;
    const int nch = (P.ld + NOV_SCHUNK - 1) / NOV_SCHUNK;
    for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int64_t d0 = blk * NOV_BLOCK - (int64_t)(P.ld - 1);
        const int64_t d = d0 + tid;
        __syncthreads();                   // the previous block's readers are done
        if (nch == 1)
            for (int i = tid; i < NOV_BLOCK + P.ld - 1; i += NOV_BLOCK) lc[i] = nov_code(ids, sbits, P, d0 + i);
        for (int b = 0; b < P.B; b++) {
            const int len = min(max(lens[b], 0), P.ld);
            if (len == 0) continue;            // (block-uniform)
            const int32_t* __restrict__ xr = x + (int64_t)b * P.ld;
            unsigned long long* kr = keys + (int64_t)b * P.ld;
            int cnt[KT];
#pragma unroll
            for (int j = 0; j < KT; j++) cnt[j] = 0;
            for (int ch = (len - 1) / NOV_SCHUNK; ch >= 0; ch--) {
                const int s_lo = ch * NOV_SCHUNK, ns = min(len, s_lo + NOV_SCHUNK) - s_lo;      // 1 <= ns <= NOV_SCHUNK
                __syncthreads();               // the previous chunk's readers are done
                if (nch > 1)
                    for (int i = tid; i < NOV_BLOCK + ns - 1; i += NOV_BLOCK) lc[i] = nov_code(ids, sbits, P, d0 + s_lo + i);
                for (int i = tid; i < ns; i += NOV_BLOCK) {
                    const int id = xr[s_lo + i];                   // s_lo + i < len <= ld
                    const int xs = (id < 0 || id >= 65535) ? NOV_NOMATCH : nov_fold(id, P);
                    const unsigned pon = (unsigned)(xs - P.on0), poff = (unsigned)(xs - P.off0);       // (NOV_NOMATCH is no note)
                    const bool note = pon < 128u || poff < 128u;
                    const int pitch = (int)(pon < 128u ? pon : poff);
#pragma unroll
                    for (int j = 0; j < KP; j++) {                 // the token under every transposition of this group
                        const int k = nov_rank_to_k(r0 + j);
                        int xk = note ? ((unsigned)(pitch + k) < 128u ? xs + k : NOV_NOMATCH) : xs;
                        if (j >= KT || r0 + j >= P.nrank) xk = NOV_NOMATCH;
                        lx[i * KP + j] = xk;
                    }
                }
                __syncthreads();
                for (int t = ns - 1; t >= 0; t--) {
                    const uint32_t v = lc[tid + t];                // tid + t <= NOV_BLOCK + ns - 2: staged above
                    const uint32_t c = v & ~NOV_START;
                    int xk[KT];
#pragma unroll
                    for (int j = 0; j < KT; j++) xk[j] = lx[t * KP + j];           // one address for the whole wave: a broadcast read
                    int mx = 0;
#pragma unroll
                    for (int j = 0; j < KT; j++) {
                        cnt[j] = c == (uint32_t)xk[j] ? cnt[j] + 1 : 0;
                        mx = max(mx, cnt[j]);
                    }
                    if (mx >= P.min_match) {
                        // a run of >= 1 matched a real corpus position: 0 <= p < n, and s < len <= ld, b < B
                        const int s = s_lo + t;
                        const unsigned long long lowp = NOV_POS_MASK - (unsigned long long)(d + s);
#pragma unroll
                        for (int j = 0; j < KT; j++)
                            if (cnt[j] >= P.min_match) {
                                const unsigned long long key = ((unsigned long long)cnt[j] << 48) | ((unsigned long long)(255 - (r0 + j)) << 40) | lowp;
                                if (key > __atomic_load_n(kr + s, __ATOMIC_RELAXED)) atomicMax(kr + s, key);
                            }
                    }
                    if (v & NOV_START) {
#pragma unroll
                        for (int j = 0; j < KT; j++) cnt[j] = 0;
                    }
                }
            }
        }
    }
}

// key -> (len, pos, k), in place: pos holds the keys.  Every element of the three outputs is written.
__global__ __launch_bounds__(256) void novelty_unpack_kernel(const int32_t* __restrict__ lens, int B, int ld, int min_match, int64_t* pos,
                                                             int32_t* __restrict__ len_out, int32_t* __restrict__ k_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * ld) return;
    const int b = (int)(i / ld), s = (int)(i - (int64_t)b * ld);
    const int len = min(max(lens[b], 0), ld);
    const unsigned long long key = (unsigned long long)pos[i];
    const int m = (int)(key >> 48);
    if (s >= len || m < min_match) {
        len_out[i] = 0;
        pos[i] = -1;
        k_out[i] = 0;
    } else {
        len_out[i] = m;
        pos[i] = (int64_t)(NOV_POS_MASK - (key & NOV_POS_MASK));
        k_out[i] = nov_rank_to_k(255 - (int)((key >> 40) & 255));
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// every refusal that can be decided from the host arguments the bare launch and the dataset entry point share
int nov_check(const char* who, int64_t n, const cmp_event_grammar* g, int B, int ld, const cmp_novelty_opts* o) {
    CMP_REQUIRE(n >= 1 && n < (1LL << 40), "%s: n=%lld ids outside [1, 2^40)", who, (long long)n);
    CMP_REQUIRE(B >= 1 && B <= NOV_MAX_B, "%s: B=%d outside [1, %d]", who, B, NOV_MAX_B);
    CMP_REQUIRE(ld >= 1 && ld <= NOV_MAX_LD, "%s: ld=%d outside [1, %d]", who, ld, NOV_MAX_LD);
    CMP_REQUIRE(o->min_match >= 1, "%s: min_match=%d must be >= 1", who, o->min_match);
    CMP_REQUIRE(o->transpose >= 0 && o->transpose <= NOV_MAX_N, "%s: transpose=%d outside [0, %d]", who, o->transpose, NOV_MAX_N);
    CMP_REQUIRE(o->transpose == 0 || g, "%s: transpose=%d needs the event layout (which ids are notes)", who, o->transpose);
    CMP_REQUIRE(o->velocity_n >= 0 && o->velocity0 >= 0 && (int64_t)o->velocity0 + o->velocity_n <= 65536,
                "%s: velocity ids [%d, %lld) outside [0, 65536)", who, o->velocity0, (long long)o->velocity0 + o->velocity_n);
    if (g) {
        CMP_REQUIRE(g->note_on0 >= 0 && g->note_on0 + 128 <= 65536 && g->note_off0 >= 0 && g->note_off0 + 128 <= 65536,
                    "%s: note ids [%d, %d) / [%d, %d) outside [0, 65536)", who, g->note_on0, g->note_on0 + 128, g->note_off0,
                    g->note_off0 + 128);
        CMP_REQUIRE(g->note_on0 + 128 <= g->note_off0 || g->note_off0 + 128 <= g->note_on0, "%s: the note_on ids [%d, %d) overlap the "
                    "note_off ids [%d, %d)", who, g->note_on0, g->note_on0 + 128, g->note_off0, g->note_off0 + 128);
        const int bases[2] = {g->note_on0, g->note_off0};
        for (int i = 0; i < 2 && o->velocity_n > 0; i++)
            CMP_REQUIRE(o->velocity0 + o->velocity_n <= bases[i] || bases[i] + 128 <= o->velocity0, "%s: the velocity ids [%d, %d) overlap "
                        "the %s ids [%d, %d)", who, o->velocity0, o->velocity0 + o->velocity_n, i ? "note_off" : "note_on", bases[i],
                        bases[i] + 128);
    }
    return CMP_OK;
}

static int nov_launch(hipStream_t s, const uint16_t* ids_dev, int64_t n, const uint32_t* sbits, const cmp_event_grammar* g,
                      const int32_t* x_dev, const int32_t* lens_dev, int B, int ld, const cmp_novelty_opts* o, int32_t* len_out,
                      int64_t* pos_out, int32_t* k_out) {
    NovParams P;
    P.n = n;
    P.on0 = g ? g->note_on0 : -(1 << 20);
    P.off0 = g ? g->note_off0 : -(1 << 20);
    P.vel0 = o->velocity0;
    P.veln = o->velocity_n;
    P.min_match = o->min_match;
    P.nrank = 2 * o->transpose + 1;
    P.B = B;
    P.ld = ld;
    const int64_t cells = (int64_t)B * ld;
    HIP_CHECK(hipMemsetAsync(pos_out, 0, (size_t)cells * 8, s));           // key 0: no run yet
    const int64_t nblocks = cdiv64(n + ld - 1, NOV_BLOCK);                  // diagonals -(ld - 1) .. n - 1
    const unsigned gx = (unsigned)std::min<int64_t>(nblocks, 1 << 22);
    if (P.nrank == 1)
        novelty_match_kernel<1><<<dim3(gx, 1), NOV_BLOCK, 0, s>>>(ids_dev, sbits, P, x_dev, lens_dev, (unsigned long long*)pos_out, nblocks);
    else
        novelty_match_kernel<NOV_KT><<<dim3(gx, cdiv(P.nrank, NOV_KT)), NOV_BLOCK, 0, s>>>(ids_dev, sbits, P, x_dev, lens_dev,
                                                                                             (unsigned long long*)pos_out, nblocks);
    KERNEL_CHECK();
    novelty_unpack_kernel<<<(unsigned)cdiv64(cells, 256), 256, 0, s>>>(lens_dev, B, ld, P.min_match, pos_out, len_out, k_out);
    KERNEL_CHECK();
    return CMP_OK;
}

extern "C" int cmp_k_novelty(void* stream, const uint16_t* ids_dev, int64_t n, const uint32_t* start_bits_dev, const cmp_event_grammar* layout,
                             const int32_t* x_dev, const int32_t* lens_dev, int B, int ld, const cmp_novelty_opts* opts, int32_t* len_out,
                             int64_t* pos_out, int32_t* k_out) {
    CMP_REQUIRE(ids_dev && x_dev && lens_dev && opts && len_out && pos_out && k_out, "k_novelty: null argument");
    CHECK_RC(nov_check("k_novelty", n, layout, B, ld, opts));
    return nov_launch((hipStream_t)stream, ids_dev, n, start_bits_dev, layout, x_dev, lens_dev, B, ld, opts, len_out, pos_out, k_out);
}

extern "C" int cmp_dataset_set_pieces(cmp_dataset* d, const int64_t* starts, int n_pieces) {
    CMP_REQUIRE(d && starts, "dataset_set_pieces: null argument");
    CMP_REQUIRE(n_pieces >= 1, "dataset_set_pieces: n_pieces=%d must be >= 1", n_pieces);
    CMP_REQUIRE(starts[0] == 0, "dataset_set_pieces: the first start is %lld, not 0", (long long)starts[0]);
    for (int i = 0; i < n_pieces; i++) {
        CMP_REQUIRE(starts[i] >= 0 && starts[i] < d->n, "dataset_set_pieces: start %d = %lld outside [0, %lld)", i, (long long)starts[i],
                    (long long)d->n);
        CMP_REQUIRE(i == 0 || starts[i] >= starts[i - 1], "dataset_set_pieces: start %d = %lld below start %d = %lld: the list is not "
                    "sorted", i, (long long)starts[i], i - 1, (long long)starts[i - 1]);
    }
    std::vector<uint32_t> words((size_t)cdiv64(d->n, 32), 0u);
    for (int i = 0; i < n_pieces; i++) words[(size_t)(starts[i] >> 5)] |= 1u << (int)(starts[i] & 31);
    HIP_CHECK(hipSetDevice(d->ctx->device));
    HIP_CHECK(hipStreamSynchronize(d->ctx->stream));           // a launch that reads the list being replaced may be in flight
    uint32_t* buf = nullptr;
    HIP_CHECK(hipMalloc((void**)&buf, words.size() * 4));
    const hipError_t e = hipMemcpy(buf, words.data(), words.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(buf);
        HIP_CHECK(e);
    }
    if (d->start_bits_dev) (void)hipFree(d->start_bits_dev);
    d->start_bits_dev = buf;
    d->n_pieces = n_pieces;
    return CMP_OK;
}

extern "C" int cmp_novelty(cmp_dataset* d, const int32_t* x, const int32_t* lens, int B, int ld, const cmp_novelty_opts* opts,
                           int32_t* len_out, int64_t* pos_out, int32_t* k_out) {
    CMP_REQUIRE(d && x && lens && opts && len_out && pos_out && k_out, "novelty: null argument");
    const cmp_event_grammar* g = d->has_layout ? &d->layout : nullptr;
    CHECK_RC(nov_check("novelty", d->n, g, B, ld, opts));
    for (int b = 0; b < B; b++) {
        CMP_REQUIRE(lens[b] >= 1 && lens[b] <= ld, "novelty: row %d: length %d outside [1, ld = %d]", b, lens[b], ld);
        for (int s = 0; s < lens[b]; s++) {
            const int32_t id = x[(size_t)b * ld + s];
            CMP_REQUIRE(id >= 0 && id < 65535, "novelty: row %d, position %d: id %d outside [0, 65535)", b, s, id);
        }
    }
    HIP_CHECK(hipSetDevice(d->ctx->device));
    const size_t cells = (size_t)B * ld;
    // one allocation: pos (8-byte elements first), x, len, k, lens
    char* buf = nullptr;
    HIP_CHECK(hipMalloc((void**)&buf, cells * 20 + (size_t)B * 4));
    int64_t* pos = (int64_t*)buf;
    int32_t* xd = (int32_t*)(buf + cells * 8);
    int32_t* len_d = xd + cells;
    int32_t* k_d = len_d + cells;
    int32_t* lens_d = k_d + cells;
    hipStream_t s = d->ctx->stream;
    hipError_t e = hipMemcpyAsync(xd, x, cells * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(lens_d, lens, (size_t)B * 4, hipMemcpyHostToDevice, s);
    int rc = CMP_OK;
    if (e == hipSuccess) rc = nov_launch(s, d->ids_dev, d->n, d->start_bits_dev, g, xd, lens_d, B, ld, opts, len_d, pos, k_d);
    if (e == hipSuccess && rc == CMP_OK) e = hipMemcpyAsync(len_out, len_d, cells * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && rc == CMP_OK) e = hipMemcpyAsync(pos_out, pos, cells * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && rc == CMP_OK) e = hipMemcpyAsync(k_out, k_d, cells * 4, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    (void)hipFree(buf);
    if (rc != CMP_OK) return rc;
    HIP_CHECK(e);
    HIP_CHECK(e2);
    return CMP_OK;
}
