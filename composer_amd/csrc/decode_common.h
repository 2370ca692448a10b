// decode_common.h -- what the batch-1 decode chain (decode.hip) and the batched one (decode_batch.hip) share.  Device side: the
// wave reductions, the split-key attention record layout and the sampler -- both chains draw their ids through the same
// sample_block, so a batched row and a batch-1 decode see the same arithmetic for the same logits.  Host side (at the end): the
// per-row loop state, the row buffers and the transposed weights of a chain, and everything AROUND the per-token chains -- the
// prefill of one row, the slide, the begin-time checks, the graph capture -- written once (decode.hip) for both.
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

// ---- event grammar (composer_hip.h, "event-grammar decoding") ----------------------------------------------------------------
// The per-row state of the grammar beside the sampling parameters in DecRow: the caller's id layout, the rule bits and
// the fold of prompt ++ ids so far.  `layout` = 0: no layout was given (no dynamic rule, the state never moves); `active` = 0: no
// rule, no static bit and no budget -- the kernels that draw then call today's sampler and nothing else.
struct DecGrammar {
    int note_on0, note_off0, time_shift0, time_shift_n, sustain_on, sustain_off;
    unsigned rules;          // CMP_GRAMMAR_* bits (0 without a layout)
    int layout;
    int active;
    int pedal;
    unsigned sounding[4];    // bit p: pitch p sounds
    long long time_steps;    // sum over the TIME_SHIFT events of the sequence, id time_shift0 + j counting j + 1
};
// ---- timed generation (composer_hip.h, "timed generation"): the budget of a row beside its grammar state in DecRow --------------
struct DecBudget {
    long long t_end;         // time_steps(prompt) + the chain's time budget; 0: no time budget (the row stays in PLAY)
    int max_polyphony;       // 0: no cap
    int done_at;             // -1 until the state first becomes DONE, then the ids the row had produced at that moment
};
// the phase of a row: a pure function of its state (any: a pitch sounds or the pedal is down)
__host__ __device__ __forceinline__ int budget_phase(long long t_end, long long time_steps, bool any) {
    if (t_end == 0 || time_steps < t_end) return CMP_BUDGET_PLAY;
    return any ? CMP_BUDGET_ENDING : CMP_BUDGET_DONE;
}

// the transition NoteSequence.from_events implements, for one id: the prompt's fold in the begin functions (host)
static inline void grammar_step(DecGrammar& g, int id) {
    if (!g.layout) return;
    const unsigned on = (unsigned)(id - g.note_on0), off = (unsigned)(id - g.note_off0), ts = (unsigned)(id - g.time_shift0);
    if (on < 128u) g.sounding[on >> 5] |= 1u << (on & 31);
    else if (off < 128u) g.sounding[off >> 5] &= ~(1u << (off & 31));
    else if (ts < (unsigned)g.time_shift_n) g.time_steps += (long long)ts + 1;
    else if (id == g.sustain_on) g.pedal = 1;
    else if (id == g.sustain_off) g.pedal = 0;
}
// The state as the kernels that draw hold it: every word loaded into a register of its own BEFORE the draw (field by field: no
// copy of the struct, no array, nothing that would live in scratch memory).
struct GramRegs {
    int note_on0, note_off0, time_shift0, time_shift_n, sustain_on, sustain_off;
    unsigned rules;
    int layout, active, pedal;
    unsigned s0, s1, s2, s3;
    long long time_steps;
};
__device__ __forceinline__ GramRegs grammar_read(const DecGrammar* __restrict__ g) {
    GramRegs r;
    r.note_on0 = g->note_on0; r.note_off0 = g->note_off0; r.time_shift0 = g->time_shift0; r.time_shift_n = g->time_shift_n;
    r.sustain_on = g->sustain_on; r.sustain_off = g->sustain_off;
    r.rules = g->rules;
    r.layout = g->layout; r.active = g->active; r.pedal = g->pedal;
    r.s0 = g->sounding[0]; r.s1 = g->sounding[1]; r.s2 = g->sounding[2]; r.s3 = g->sounding[3];
    r.time_steps = g->time_steps;
    return r;
}
// The transition under a time budget (t_end != 0): in DONE the id is a filler and the state stays where it is; after a real id,
// done_at records the ids produced so far (`produced`, this one included) when the new state is DONE.  The new state's three
// terms -- pitches sounding, pedal, time -- are followed in registers from g0 (bit p of the sounding set in arithmetic, as
// ban_sounds reads it).
__device__ __forceinline__ void grammar_advance_timed(DecGrammar* __restrict__ gm, DecBudget* __restrict__ bd, const GramRegs& g0,
                                                      int id, int produced, long long t_end) {
    int cnt = __popc(g0.s0) + __popc(g0.s1) + __popc(g0.s2) + __popc(g0.s3), ped = g0.pedal;
    long long t = g0.time_steps;
    if (budget_phase(t_end, t, (cnt | ped) != 0) == CMP_BUDGET_DONE) return;
    const unsigned on = (unsigned)(id - g0.note_on0), off = (unsigned)(id - g0.note_off0), ts = (unsigned)(id - g0.time_shift0);
    if (on < 128u) {
        gm->sounding[on >> 5] |= 1u << (on & 31);
        cnt += 1;                                     // (one more or the same: not empty either way)
    } else if (off < 128u) {
        gm->sounding[off >> 5] &= ~(1u << (off & 31));
        const unsigned r = off & 31, i = off >> 5;
        cnt -= (int)((((g0.s0 >> r) & (unsigned)(i == 0u)) | ((g0.s1 >> r) & (unsigned)(i == 1u)) |
                      ((g0.s2 >> r) & (unsigned)(i == 2u)) | ((g0.s3 >> r) & (unsigned)(i == 3u))) & 1u);
    } else if (ts < (unsigned)g0.time_shift_n) {
        t += (long long)ts + 1;
        gm->time_steps = t;
    } else if (id == g0.sustain_on) {
        gm->pedal = ped = 1;
    } else if (id == g0.sustain_off) {
        gm->pedal = ped = 0;
    }
    if (budget_phase(t_end, t, (cnt | ped) != 0) == CMP_BUDGET_DONE) bd->done_at = produced;
}
// ... and the transition for the drawn id on the device, by ONE lane after every thread has read the state: g0 is the state the
// draw saw, gm the state in memory; only the word that changes is written (a note event updates its word of the sounding set in
// memory: which word is known only now, and a run-time choice between registers is what the compiler turns into scratch).
// The budget is not part of what the draw's threads load: t_end, constant since begin, is read here by the one lane, and only on
// a chain with a layout; without a time budget the transition is the code it was.
__device__ __forceinline__ void grammar_advance(DecGrammar* __restrict__ gm, DecBudget* __restrict__ bd, const GramRegs& g0, int id,
                                                int produced) {
    if (!g0.layout) return;
    const long long t_end = bd->t_end;
    if (t_end != 0) { grammar_advance_timed(gm, bd, g0, id, produced, t_end); return; }
    const unsigned on = (unsigned)(id - g0.note_on0), off = (unsigned)(id - g0.note_off0), ts = (unsigned)(id - g0.time_shift0);
    if (on < 128u) {
        gm->sounding[on >> 5] |= 1u << (on & 31);
    } else if (off < 128u) {
        gm->sounding[off >> 5] &= ~(1u << (off & 31));
    } else if (ts < (unsigned)g0.time_shift_n) {
        gm->time_steps = g0.time_steps + (long long)ts + 1;
    } else if (id == g0.sustain_on) {
        gm->pedal = 1;
    } else if (id == g0.sustain_off) {
        gm->pedal = 0;
    }
}

// What the ban predicate reads: a few words, the same in every lane of the workgroup (readfirstlane keeps them in scalar
// registers), snapshotted before the draw so that the lane that moves the state on afterwards races with no reader.
struct BanCtx {
    const unsigned* words;   // static bans, ceil(V / 32) words (all zero when unused)
    int note_on0, note_off0, sustain_on, sustain_off;
    unsigned rules;
    int pedal;
    unsigned s0, s1, s2, s3;
    // timed generation: the phase of the row, the TIME_SHIFT ids [ts_lo, ts_hi) that would pass t_end (PLAY; empty without a time
    // budget), whether the polyphony cap is reached (PLAY: no NOTE_ON), and the filler id of DONE
    int phase, ts_lo, ts_hi, no_on, time_shift0;
};
__device__ __forceinline__ int uni_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
// bd: the row's budget, loaded HERE -- on the banning path only, so a chain without grammar and budget (`active` = 0) reads none
// of it; t_end and max_polyphony are constant since begin, so there is no writer to race with
__device__ __forceinline__ BanCtx ban_load(const GramRegs& g, const DecBudget* __restrict__ bd, const unsigned* __restrict__ words) {
    BanCtx b;
    const long long t_end = bd->t_end;
    const int max_polyphony = bd->max_polyphony;
    b.words = words;
    b.note_on0 = uni_i(g.note_on0); b.note_off0 = uni_i(g.note_off0);
    b.sustain_on = uni_i(g.sustain_on); b.sustain_off = uni_i(g.sustain_off);
    b.rules = (unsigned)uni_i((int)g.rules);
    b.pedal = uni_i(g.pedal);
    b.s0 = (unsigned)uni_i((int)g.s0); b.s1 = (unsigned)uni_i((int)g.s1);
    b.s2 = (unsigned)uni_i((int)g.s2); b.s3 = (unsigned)uni_i((int)g.s3);
    // the budget's terms, once per workgroup from the uniform words above: the popcount of the sounding set, the phase, and the
    // number of TIME_SHIFT ids that stay allowed, min(time_shift_n, t_end - time_steps) (all of them without a time budget)
    const int cnt = __popc(b.s0) + __popc(b.s1) + __popc(b.s2) + __popc(b.s3);
    const long long left = t_end - g.time_steps;
    const int tsn = g.layout ? g.time_shift_n : 0;
    const int allow = (t_end != 0 && left < (long long)tsn) ? (int)(left > 0 ? left : 0) : tsn;
    b.phase = uni_i(budget_phase(t_end, g.time_steps, (cnt | b.pedal) != 0));
    b.time_shift0 = uni_i(g.time_shift0);
    b.ts_lo = uni_i(g.time_shift0 + allow);
    b.ts_hi = uni_i(g.time_shift0 + tsn);
    b.no_on = uni_i((max_polyphony > 0 && cnt >= max_polyphony) ? 1 : 0);
    return b;
}
// static bans only (cmp_k_sample_banned)
__device__ __forceinline__ BanCtx ban_static(const unsigned* __restrict__ words) {
    BanCtx b = {words, 0, 0, -1, -1, 0u, 0, 0u, 0u, 0u, 0u, CMP_BUDGET_PLAY, 0, 0, 0, -1};
    return b;
}
// bit p of the sounding set, in arithmetic alone (a select between the four words ends up as an indexed load from scratch)
__device__ __forceinline__ bool ban_sounds(const BanCtx& b, unsigned p) {
    const unsigned r = p & 31, i = p >> 5;
    const unsigned m = ((b.s0 >> r) & (unsigned)(i == 0u)) | ((b.s1 >> r) & (unsigned)(i == 1u)) |
                       ((b.s2 >> r) & (unsigned)(i == 2u)) | ((b.s3 >> r) & (unsigned)(i == 3u));
    return m & 1u;
}
// column c (0 <= c < V) cannot be drawn in this state
__device__ __forceinline__ bool banned(const BanCtx& b, int c) {
    if (b.phase != CMP_BUDGET_PLAY) {                 // (uniform) the static vector and the rule bits are not read here
        if (b.phase == CMP_BUDGET_DONE) return c != b.time_shift0;                    // the filler alone
        const unsigned p = (unsigned)(c - b.note_off0);                              // ENDING: only what releases
        if (p < 128u) return !ban_sounds(b, p);
        return !(c == b.sustain_off && b.pedal);
    }
    bool r = (b.words[c >> 5] >> (c & 31)) & 1u;
    r = r || (c >= b.ts_lo && c < b.ts_hi);           // a TIME_SHIFT that would pass t_end
    if (b.no_on) r = r || (unsigned)(c - b.note_on0) < 128u;                         // the polyphony cap is reached
    if (b.rules & CMP_GRAMMAR_NOTE_OFF_SOUNDING) {
        const unsigned p = (unsigned)(c - b.note_off0);
        if (p < 128u) r = r || !ban_sounds(b, p);
    }
    if (b.rules & CMP_GRAMMAR_NOTE_ON_SILENT) {
        const unsigned p = (unsigned)(c - b.note_on0);
        if (p < 128u) r = r || ban_sounds(b, p);
    }
    if (b.rules & CMP_GRAMMAR_PEDAL) r = r || (c == b.sustain_on && b.pedal) || (c == b.sustain_off && !b.pedal);
    return r;
}
// every read of a logit by the samplers: BAN = false is the load itself
template <bool BAN> __device__ __forceinline__ float z_at(const float* __restrict__ z, int c, const BanCtx& b) {
    if (BAN) return banned(b, c) ? -INFINITY : z[c];
    return z[c];
}

// The draw itself, shared by the per-token sampler and the kernel-level test entry (cmp_k_sample): every thread of a 256-thread
// workgroup returns the chosen id.  temperature <= 0: argmax, lowest index on ties (tf.argmax).  Otherwise Gumbel-max:
// argmax_c(z[c]/temperature + G_c), G_c = -log(-log(u_c)) with u_c a counter hash of (seed, draw counter, column) -- one
// draw from softmax(z / temperature) (tf.random.categorical, cli.py:671-673).  bv/bi: 4-entry LDS scratch.
// BAN: every logit is read through the ban predicate (a banned column reads -inf: the draw of the contract, by construction).
template <bool BAN>
__device__ __forceinline__ int sample_block_t(const float* __restrict__ z, int V, float temperature, unsigned seed, unsigned ctr,
                                              float* bv, int* bi, const BanCtx& ban) {
    const int tid = threadIdx.x;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    const float inv_t = temperature > 0.f ? 1.0f / temperature : 0.f;
    for (int c = tid; c < V; c += 256) {
        float v = z_at<BAN>(z, c, ban);
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
__device__ __forceinline__ int sample_block(const float* __restrict__ z, int V, float temperature, unsigned seed, unsigned ctr,
                                            float* bv, int* bi) {
    return sample_block_t<false>(z, V, temperature, seed, ctr, bv, bi, BanCtx{});
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
template <bool BAN>
__device__ __forceinline__ int sample_block_trunc_t(const float* __restrict__ z, int V, float temperature, int top_k, float top_p,
                                                    unsigned seed, unsigned ctr, float* bv, int* bi, unsigned char* lds,
                                                    const BanCtx& ban) {
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
        ks[c] = c < V ? trunc_key(z_at<BAN>(z, c, ban)) : 0u;        // padding: key 0 at an index above every column is never counted
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
        const double zmax = (double)z_at<BAN>(z, min((int)ord[0], V - 1), ban), dt = (double)temperature;
        for (int r = tid; r < kc; r += 256) q[r] = exp(((double)z_at<BAN>(z, min((int)ord[r], V - 1), ban) - zmax) / dt);
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
        float v = z_at<BAN>(z, c, ban);
        unsigned hsh = drop_hash(seed, 0xC0FFEEu + ctr, (uint64_t)c);
        float u = ((float)(hsh >> 9) + 0.5f) * (1.0f / 8388608.0f);
        v = v * inv_t - __logf(-__logf(u));
        if (v > best || (v == best && v > -INFINITY && c < arg)) { best = v; arg = c; }      // (a -inf column is never chosen)
    }
    const int id = block_argmax(best, arg, bv, bi);
    return min(max(id, 0), V - 1);
}

__device__ __forceinline__ int sample_block_trunc(const float* __restrict__ z, int V, float temperature, int top_k, float top_p,
                                                  unsigned seed, unsigned ctr, float* bv, int* bi, unsigned char* lds) {
    return sample_block_trunc_t<false>(z, V, temperature, top_k, top_p, seed, ctr, bv, bi, lds, BanCtx{});
}

// what every kernel that draws an id calls: the existing sampler unless a filter is on (uniform per workgroup)
__device__ __forceinline__ int sample_block_any(const float* __restrict__ z, int V, float temperature, int top_k, float top_p,
                                                unsigned seed, unsigned ctr, float* bv, int* bi, unsigned char* lds) {
    if (trunc_filters_on(V, temperature, top_k, top_p) && V <= TRUNC_MAX_V)
        return sample_block_trunc(z, V, temperature, top_k, top_p, seed, ctr, bv, bi, lds);
    return sample_block(z, V, temperature, seed, ctr, bv, bi);
}

// ... with the event grammar: the banning samplers only when a rule or a static bit is active (`active`, uniform per workgroup),
// so a chain without a grammar runs sample_block_any itself
__device__ __forceinline__ int sample_block_banned(const float* __restrict__ z, int V, float temperature, int top_k, float top_p,
                                                   unsigned seed, unsigned ctr, float* bv, int* bi, unsigned char* lds,
                                                   const BanCtx& ban) {
    if (trunc_filters_on(V, temperature, top_k, top_p) && V <= TRUNC_MAX_V)
        return sample_block_trunc_t<true>(z, V, temperature, top_k, top_p, seed, ctr, bv, bi, lds, ban);
    return sample_block_t<true>(z, V, temperature, seed, ctr, bv, bi, ban);
}
__device__ __forceinline__ int sample_block_grammar(const float* __restrict__ z, int V, float temperature, int top_k, float top_p,
                                                    unsigned seed, unsigned ctr, float* bv, int* bi, unsigned char* lds,
                                                    const GramRegs& g, const DecBudget* __restrict__ bd,
                                                    const unsigned* __restrict__ words) {
    if (uni_i(g.active)) return sample_block_banned(z, V, temperature, top_k, top_p, seed, ctr, bv, bi, lds, ban_load(g, bd, words));
    return sample_block_any(z, V, temperature, top_k, top_p, seed, ctr, bv, bi, lds);
}

// ---- host side of the grammar: what cmp_decode_grammar keeps per chain, and what the begin functions make of it ---------------
static inline int grammar_words(int V) { return (V + 31) / 32; }
// the state of a row whose sequence so far is its prompt
static inline DecGrammar grammar_begin(const DecGrammarCfg& c, const int32_t* prompt, int P) {
    DecGrammar g = {};
    g.note_on0 = g.note_off0 = g.time_shift0 = g.sustain_on = g.sustain_off = -1;
    if (c.has_layout) {
        g.note_on0 = c.g.note_on0; g.note_off0 = c.g.note_off0; g.time_shift0 = c.g.time_shift0; g.time_shift_n = c.g.time_shift_n;
        g.sustain_on = c.g.sustain_on; g.sustain_off = c.g.sustain_off;
        g.rules = (unsigned)c.g.rules;
        g.layout = 1;
    }
    bool any = false;
    for (uint32_t w : c.words) any = any || w != 0u;
    g.active = (g.rules != 0u || any) ? 1 : 0;
    for (int i = 0; i < P; i++) grammar_step(g, prompt[i]);
    return g;
}
// the chain's static bans into its device buffer (all zero when there are none), stream-ordered in front of the first draw
static inline hipError_t grammar_upload(const DecGrammarCfg& c, int V, unsigned* banw, hipStream_t s) {
    const size_t bytes = (size_t)grammar_words(V) * 4;
    if (c.words.empty()) return hipMemsetAsync(banw, 0, bytes, s);
    return hipMemcpyAsync(banw, c.words.data(), bytes, hipMemcpyHostToDevice, s);
}

// ---- the state of a chain ----------------------------------------------------------------------------------------------------
#define DECB_MAX_ROWS 256
#define DEC_GUARD_MAX_M 64

struct DecRow {          // device-resident per-row loop state (the captured chain does not depend on it); the batch-1 chain has one
    int pos;             // position id of the token about to be consumed (first member: all the batch-1 attention reads)
    int token;           // that token
    int produced;        // ids written to this row's slot of ids[]
    int advance;         // 1: kv mode (pos += 1 per step), 0: literal (pos stays 0)
    unsigned rng;        // sampling counter
    unsigned seed;       // (uint32)(seed + b).  Temperature and seed live here (not in kernel arguments) so that the captured
    float temperature;   // per-token graph does not depend on them and survives from one begin to the next.  <= 0: greedy
    int hold;            // sliding-window mode, batched chain: 1 while the row sits out a replay (its cache is full, pos == W):
                         // attention neither appends nor reads, the sampler leaves the row alone; the row's slide, run after the
                         // replay, clears it.  Always 0 on the batch-1 chain, whose kernels do not read it
    int top_k;           // truncated sampling, per row: 0 or >= V: off
    float top_p;         // 1: off
    DecGrammar gr;       // event grammar: layout, rules and the fold of the row's prompt ++ ids so far
    DecBudget bd;        // timed generation: where the row's time ends, its polyphony cap, when it was done
};

struct DecRowList {      // rows of one slide, by value in the kernel arguments: no host buffer has to outlive an enqueued step
    unsigned char row[DECB_MAX_ROWS];
};

struct DecLayerW { float *attn_wT, *proj_wT, *fc_wT, *pr_wT; };     // fp32, transposed to [N][K]

// The transposed weights a chain's GEMVs / projections read, and its static grammar bans: independent of the batch size, so their
// addresses outlive every captured chain.  Each chain has its OWN instance: a chain in mid-decode keeps the weights its begin saw
// when a parameter is set and the other chain then begins.
struct DecWeights {
    std::vector<DecLayerW> lw;
    unsigned* banw = nullptr;           // static bans of the event grammar, ceil(V / 32) words shared by all rows (zero: none)
    int64_t version = -1;               // cmp_model::param_version the transposes were made from
    std::vector<void*> allocs;
};

// Everything indexed by row, for capB rows (the batch-1 chain: one), and how far the rows have got (the same for every row).
struct DecRows {
    int capB = 0;                       // rows the buffers and caches hold
    int cap = 1 << 16;                  // ids per row
    DecRow* st = nullptr;
    int32_t* ids = nullptr;             // [capB][cap]
    float *x = nullptr, *u = nullptr, *qkv = nullptr, *att = nullptr, *r = nullptr, *g = nullptr, *logits = nullptr;
    // sliding-window mode: every row's prompt and its length stay on the device beside its ids, so that the tail a slide
    // re-encodes is gathered without a host round trip
    int32_t* prompts = nullptr;         // [capB][W]
    int32_t* plen = nullptr;            // [capB]
    std::vector<float*> kc, vc;         // per layer, [capB] x K [H][D/4][W][4], V [H][W][D]
    // copy guard (composer_hip.h, "copy guard"): the guard this decode began under (off: the buffers are not touched), every row's
    // own ban words -- what a guarded chain's samplers read in place of the static words --, its window of history ids and its counter
    DecGuardCfg guard;
    uint32_t* cgwords = nullptr;        // [capB][ceil(V / 32)]
    int32_t* cghist = nullptr;          // [capB][DEC_GUARD_MAX_M]
    int32_t* cglens = nullptr;          // [capB]
    unsigned long long* cgcount = nullptr;      // [capB] banned_columns
    std::vector<void*> allocs;          // sized by capB (replaced when a larger B is asked for)
    int B = 0, mode = 0;
    int keep = 0;                       // 0: plain kv / literal decode
    int produced = 0, returned = 0;
    bool begun = false;
    int64_t row_slides = 0, fwd_calls = 0;
};

struct DecodeState {                    // the batch-1 chain (decode.hip)
    DecWeights w;
    DecRows rows;                       // one row
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int pos = 0;                        // host mirror of the row's position (kv-mode window check; when to slide)
    bool built = false;                 // buffers allocated, chain captured (reused by later cmp_decode_begin calls)
    bool graph_on = false;
    int64_t guard_epoch = 0;            // DecGuardCfg::epoch the chain was captured under
};

struct DecodeBatchState {               // the batched chain (decode_batch.hip)
    DecWeights w;
    DecRows rows;
    std::map<int, std::pair<hipGraph_t, hipGraphExec_t>> graphs;     // captured chain per B
    bool graph_on = true;
    int64_t guard_epoch = 0;            // DecGuardCfg::epoch the chains were captured under
    std::vector<int> pos;               // host mirror of each row's position (kv-mode window check; which rows slide at which step)
};

template <typename Tp> static int dec_alloc(std::vector<void*>& list, Tp** p, size_t bytes) {
    void* q = nullptr;
    HIP_CHECK(hipMalloc(&q, bytes ? bytes : 16));
    list.push_back(q);
    *p = (Tp*)q;
    return CMP_OK;
}

// `enqueue` captured on the stream into a graph and instantiated; no graph is left behind when either step fails
template <typename F> static int dec_capture(hipStream_t s, F&& enqueue, hipGraph_t* graph, hipGraphExec_t* exec) {
    HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(s, &g);
    if (rc != CMP_OK) { if (g) hipGraphDestroy(g); return rc; }
    HIP_CHECK(e);
    hipGraphExec_t ex = nullptr;
    e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (e != hipSuccess) hipGraphDestroy(g);
    HIP_CHECK(e);
    *graph = g;
    *exec = ex;
    return CMP_OK;
}

// decode.hip, for both chains.  `who`: the caller's name as its refusals print it
bool dec_graph_enabled();                                                        // COMPOSER_NO_GRAPH=1: off
int dec_check_prompt(const char* who, int row, const int32_t* ids, int P, int V, int W);      // row < 0: the batch-1 chain's wording
int dec_check_keep(const char* who, int keep, int W);
int dec_require_begun(const char* who, bool begun, const char* begin_fn);
int dec_weights_refresh(cmp_model* m, DecWeights& w);       // allocated on first use; transposed again when a parameter has changed
void dec_rows_free(DecRows& R);
int dec_rows_alloc(cmp_model* m, DecRows& R, int B);
int dec_check_budget(const char* who, const DecGrammarCfg& c, const DecBudgetCfg& bc);      // the begin-time refusals of a budget
DecRow dec_row_init(int mode, int P, unsigned seed, float temperature, int top_k, float top_p, const DecGrammarCfg& c,
                    const DecBudgetCfg& bc, const int32_t* prompt, bool guarded = false);
int dec_prefill_row(cmp_model* m, DecRows& R, const DecWeights& w, int b, const int32_t* prompt, int P);
int dec_enqueue_slide(cmp_model* m, DecRows& R, const DecWeights& w, const DecRowList& rl, int nb);
// Copy guard: the scan in front of a draw of rows row0 .. row0 + nrows - 1 (nothing on an unguarded chain).  nb < 0: every row of the
// range that is not held draws; nb >= 0: the rows rl.row[0 .. nb) do.  Every other row of the range gets its static words alone.
int dec_enqueue_guard(cmp_model* m, DecRows& R, const DecWeights& w, const DecRowList& rl, int nb, int row0, int nrows);
// the ban words the samplers of a chain read, and their stride per row (0: one vector for all rows)
static inline const unsigned* dec_ban_words(const DecRows& R, const DecWeights& w) { return R.guard.on() ? R.cgwords : w.banw; }
static inline int dec_ban_stride(const cmp_model* m, const DecRows& R) { return R.guard.on() ? grammar_words(m->V) : 0; }
// decode_batch.hip: decb_sample_kernel for rows row0 .. row0 + nrows - 1 from `logits` (one row each, stride ldz)
int decb_launch_sample(cmp_model* m, DecRows& R, const DecWeights& w, const float* logits, int nrows, int row0, int first);
