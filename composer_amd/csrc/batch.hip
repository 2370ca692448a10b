// batch.hip -- train-time augmentation on the device (include/composer_hip.h, "device dataset"): one row of (x, y) per workgroup, cut
// out of the uint16 id stream in HBM, transposed and time-stretched by the row's plan.  Integers only: every result is bitwise what
// composer_amd/augment.py computes on the host.  No atomics, no scratch.
// A translation unit of its own: adding it leaves every kernel of the other sources instruction-identical (tools/isa_hash.py).
#include "model.h"

#define BATCH_BLOCK 256
#define BATCH_WAVES (BATCH_BLOCK / WAVE)

struct BatchLayout { int note_on0, note_off0, time_shift0, time_shift_n; };

// R(t) = (t f + 512) >> 10: the stretched time of unstretched time t, rounded once -- cumulative, so a span's emitted steps sum to
// R(total) whatever its runs are
__device__ __forceinline__ int64_t batch_R(int64_t t, int f) { return (t * (int64_t)f + 512) >> 10; }

__device__ __forceinline__ int batch_transpose(int id, const BatchLayout& L, int k) {
    const unsigned pon = (unsigned)(id - L.note_on0), poff = (unsigned)(id - L.note_off0);
    if (pon < 128u) return L.note_on0 + min(max((int)pon + k, 0), 127);
    if (poff < 128u) return L.note_off0 + min(max((int)poff + k, 0), 127);
    return id;
}

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// inclusive scans across the 64 lanes of a wave (ds_bpermute shuffles; every lane takes part)
__device__ __forceinline__ int64_t wave_scan_sum64(int64_t v, int lane) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int64_t u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}
__device__ __forceinline__ int64_t wave_scan_max64(int64_t v, int lane) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int64_t u = __shfl_up(v, o);
        if (lane >= o) v = max64(v, u);
    }
    return v;
}
__device__ __forceinline__ int wave_scan_sum32(int v, int lane) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// out[q] of a row, q in [0, W]: x[q] = out[q] for q < W, y[q - 1] = out[q] for q >= 1
__device__ __forceinline__ void batch_put(int32_t* __restrict__ xr, int32_t* __restrict__ yr, int W, int q, int id) {
    if (q < W) xr[q] = id;
    if (q >= 1) yr[q - 1] = id;
}

// One workgroup per row.  The span src = ids[offset : offset + S], S = min(2 (W + 1), n - offset), is walked in chunks of 256 tokens, one
// token per thread, with three block scans per chunk carried from chunk to chunk:
//   time      inclusive sum of the TIME_SHIFT steps: the unstretched time after token i;
//   run start inclusive max of (time at a non-shift token, else -1): time never decreases, so that is the time at the LAST non-shift
//             token, where the run a shift token belongs to began (no such token yet: 0, the span's start);
//   count     exclusive sum of the tokens each source token emits: a non-shift token 1 (itself, transposed), the LAST token of a run
//             ceil(d / M) with d = R(time) - R(run start), every other shift token 0.
// A thread writes its tokens at its exclusive count, positions below W + 1 only; the walk ends once W + 1 tokens exist.  A span that
// emits fewer takes the copy path (the f = 1024 row: src[: W + 1] transposed) in a block-uniform branch, after a barrier.
__global__ __launch_bounds__(BATCH_BLOCK) void batch_rows_kernel(const uint16_t* __restrict__ ids, int64_t n, BatchLayout L,
                                                                 const cmp_batch_row* __restrict__ plan, int W,
                                                                 int32_t* __restrict__ x, int32_t* __restrict__ y,
                                                                 int32_t* __restrict__ status) {
    // (two barriers per chunk: a wave cannot reach the next write of an array before every wave has read it)
    __shared__ int64_t wt[BATCH_WAVES], wm[BATCH_WAVES];
    __shared__ int wc[BATCH_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const cmp_batch_row pr = plan[b];
    const int64_t off = pr.offset;
    const int k = pr.transpose, f = pr.stretch_q10;
    const int need = W + 1;
    int32_t* st = status + 2 * (int64_t)b;
    // a row the host entry points would have refused (the bare launch cannot read a device plan): nothing of the stream is read
    if (off < 0 || off > n - need || f < 512 || f > 1536 || k < -127 || k > 127) {
        if (tid == 0) { st[0] = 0; st[1] = CMP_BATCH_REFUSED; }
        return;
    }
    const uint16_t* __restrict__ src = ids + off;
    int32_t* __restrict__ xr = x + (int64_t)b * W;
    int32_t* __restrict__ yr = y + (int64_t)b * W;
    const int64_t S = min64((int64_t)2 * need, n - off);
    const int M = L.time_shift_n;
    int total = need;
    if (f != 1024) {
        int64_t carry_t = 0, carry_m = 0;
        int carry_c = 0;
        for (int64_t base = 0; base < S && carry_c < need; base += BATCH_BLOCK) {
            const int64_t i = base + tid;
            int id = -1;
            bool shift = false, run_end = false;
            int steps = 0;
            if (i < S) {
                id = src[i];
                const unsigned j = (unsigned)(id - L.time_shift0);
                shift = j < (unsigned)M;
                steps = shift ? (int)j + 1 : 0;
                if (shift) run_end = i + 1 == S || (unsigned)((int)src[i + 1] - L.time_shift0) >= (unsigned)M;
            }
            const bool plain = i < S && !shift;
            const int64_t lt = wave_scan_sum64(steps, lane);                      // time inside this wave's 64 tokens
            const int64_t lm = wave_scan_max64(plain ? lt : -1, lane);            // ... at its last non-shift token so far, or -1
            if (lane == WAVE - 1) { wt[wave] = lt; wm[wave] = lm; }
            __syncthreads();
            int64_t pre_t = carry_t, in_m = carry_m, my_t = 0, my_m = 0;
#pragma unroll
            for (int w = 0; w < BATCH_WAVES; w++) {
                if (w == wave) { my_t = pre_t; my_m = in_m; }
                const int64_t m_w = wm[w];
                if (m_w >= 0) in_m = pre_t + m_w;
                pre_t += wt[w];
            }
            carry_t = pre_t;
            carry_m = in_m;
            const int64_t t1 = my_t + lt;
            const int64_t t0 = lm >= 0 ? my_t + lm : my_m;
            int e = plain ? 1 : 0;
            int64_t d = 0;
            if (run_end) {
                d = batch_R(t1, f) - batch_R(t0, f);
                e = (int)min64((d + M - 1) / M, need);                     // (more than W + 1 tokens of one run are never written)
            }
            const int lc = wave_scan_sum32(e, lane);
            if (lane == WAVE - 1) wc[wave] = lc;
            __syncthreads();
            int pre_c = carry_c, my_c = 0;
#pragma unroll
            for (int w = 0; w < BATCH_WAVES; w++) {
                if (w == wave) my_c = pre_c;
                pre_c += wc[w];
            }
            carry_c = min(pre_c, need);
            int q = my_c + lc - e;
            if (plain) {
                if (q < need) batch_put(xr, yr, W, q, batch_transpose(id, L, k));
            } else if (run_end) {
                // d // M tokens of M steps, then the remainder (notes.py's chunking of one shift)
                const int64_t full = d / M;
                const int rem = (int)(d - full * M);
                const int stop = min(q + e, need);
                for (int j = 0; q < stop; q++, j++)
                    batch_put(xr, yr, W, q, L.time_shift0 + ((int64_t)j < full ? M : rem) - 1);
            }
        }
        total = carry_c;
    }
    bool fallback = false;
    if (total < need || f == 1024) {
        fallback = f != 1024;
        __syncthreads();               // the walk's stores to this row come before the copy's
        for (int q = tid; q < need; q += BATCH_BLOCK) batch_put(xr, yr, W, q, batch_transpose(src[q], L, k));
    }
    if (tid == 0) { st[0] = total; st[1] = fallback ? CMP_BATCH_FALLBACK : 0; }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// the grammar's layout rules (cmp_decode_grammar) for the four fields the augmentation reads and the sustain pair, against V ids
static int batch_layout_check(const char* who, const cmp_event_grammar* g, int64_t V) {
    CMP_REQUIRE((g->rules & ~CMP_GRAMMAR_ALL) == 0, "%s: unknown rule bits 0x%x (known: 0x%x)", who, g->rules, CMP_GRAMMAR_ALL);
    CMP_REQUIRE(g->time_shift_n >= 1, "%s: time_shift_n=%d must be >= 1", who, g->time_shift_n);
    CMP_REQUIRE((g->sustain_on < 0) == (g->sustain_off < 0), "%s: sustain_on=%d without sustain_off=%d (or the reverse): both ids, or -1 "
                "for both", who, g->sustain_on, g->sustain_off);
    CMP_REQUIRE(g->sustain_on >= -1 && g->sustain_off >= -1, "%s: sustain ids %d / %d: an id, or -1 for both", who, g->sustain_on,
                g->sustain_off);
    struct R { const char* name; int64_t lo, n; };
    const R rg[5] = {{"note_on", g->note_on0, 128}, {"note_off", g->note_off0, 128}, {"time_shift", g->time_shift0, g->time_shift_n},
                     {"sustain_on", g->sustain_on, 1}, {"sustain_off", g->sustain_off, 1}};
    const int nr = g->sustain_on < 0 ? 3 : 5;
    for (int i = 0; i < nr; i++)
        CMP_REQUIRE(rg[i].lo >= 0 && rg[i].lo + rg[i].n <= V, "%s: %s ids [%lld, %lld) outside the vocabulary [0, %lld)", who, rg[i].name,
                    (long long)rg[i].lo, (long long)(rg[i].lo + rg[i].n), (long long)V);
    for (int i = 0; i < nr; i++)
        for (int j = i + 1; j < nr; j++)
            CMP_REQUIRE(rg[i].lo + rg[i].n <= rg[j].lo || rg[j].lo + rg[j].n <= rg[i].lo, "%s: the %s ids [%lld, %lld) overlap the %s ids "
                        "[%lld, %lld)", who, rg[i].name, (long long)rg[i].lo, (long long)(rg[i].lo + rg[i].n), rg[j].name,
                        (long long)rg[j].lo, (long long)(rg[j].lo + rg[j].n));
    return CMP_OK;
}

static int batch_rows_launch(hipStream_t s, const uint16_t* ids_dev, int64_t n, const cmp_event_grammar* g, const cmp_batch_row* plan_dev,
                             int B, int W, int32_t* x, int32_t* y, int32_t* status) {
    // no layout: identity plans only, which never look at it
    const BatchLayout L = g ? BatchLayout{g->note_on0, g->note_off0, g->time_shift0, g->time_shift_n} : BatchLayout{-1, -1, -1, 1};
    batch_rows_kernel<<<B, BATCH_BLOCK, 0, s>>>(ids_dev, n, L, plan_dev, W, x, y, status);
    KERNEL_CHECK();
    return CMP_OK;
}

static const int64_t BATCH_MAX_W = (1 << 20);       // 256 threads x (W + 1) emitted tokens, the most a chunk can count, stay inside an int

extern "C" int cmp_k_batch_rows(void* stream, const uint16_t* ids_dev, int64_t n, const cmp_event_grammar* layout,
                                const cmp_batch_row* plan_dev, int B, int W, int32_t* x, int32_t* y, int32_t* status) {
    CMP_REQUIRE(ids_dev && plan_dev && x && y && status, "k_batch_rows: null argument");
    CMP_REQUIRE(B >= 0 && W >= 1 && W <= BATCH_MAX_W && n >= (int64_t)W + 1, "k_batch_rows: B=%d W=%d n=%lld (a row needs W + 1 ids)", B, W,
                (long long)n);
    if (layout) CHECK_RC(batch_layout_check("k_batch_rows", layout, 65536));
    if (B == 0) return CMP_OK;
    return batch_rows_launch((hipStream_t)stream, ids_dev, n, layout, plan_dev, B, W, x, y, status);
}

int batch_plan_check(const char* who, const cmp_dataset* ds, const cmp_batch_row* plan, int B, int W, int V) {
    CMP_REQUIRE(B >= 1 && W >= 1 && W <= BATCH_MAX_W, "%s: B=%d W=%d", who, B, W);
    CMP_REQUIRE(ds->n >= (int64_t)W + 1, "%s: the dataset holds %lld ids, a row of W=%d needs %d", who, (long long)ds->n, W, W + 1);
    const int64_t last = ds->n - ((int64_t)W + 1);
    bool identity = true;
    for (int b = 0; b < B; b++) {
        const cmp_batch_row& r = plan[b];
        CMP_REQUIRE(r.offset >= 0 && r.offset <= last, "%s: row %d: offset %lld outside [0, %lld] (n=%lld, W=%d)", who, b,
                    (long long)r.offset, (long long)last, (long long)ds->n, W);
        CMP_REQUIRE(r.stretch_q10 >= 512 && r.stretch_q10 <= 1536, "%s: row %d: stretch %d/1024 outside [512, 1536]", who, b, r.stretch_q10);
        CMP_REQUIRE(r.transpose >= -127 && r.transpose <= 127, "%s: row %d: transpose %d outside [-127, 127]", who, b, r.transpose);
        identity = identity && r.transpose == 0 && r.stretch_q10 == 1024;
    }
    CMP_REQUIRE(identity || ds->has_layout, "%s: a plan that transposes or stretches needs a dataset created with a layout", who);
    if (V > 0) {
        CMP_REQUIRE(ds->max_id < V, "%s: the dataset's largest id %d is outside the model's vocabulary [0, %d)", who, ds->max_id, V);
        if (ds->has_layout) CHECK_RC(batch_layout_check(who, &ds->layout, V));
    }
    return CMP_OK;
}

int batch_rows_run(hipStream_t s, const cmp_dataset* ds, const cmp_batch_row* plan_dev, int B, int W, int32_t* x, int32_t* y,
                   int32_t* status) {
    return batch_rows_launch(s, ds->ids_dev, ds->n, ds->has_layout ? &ds->layout : nullptr, plan_dev, B, W, x, y, status);
}

extern "C" int cmp_dataset_create(cmp_ctx* ctx, const uint16_t* ids, int64_t n, const cmp_event_grammar* layout, cmp_dataset** out) {
    CMP_REQUIRE(ctx && ids && out, "dataset_create: null argument");
    CMP_REQUIRE(n >= 2, "dataset_create: n=%lld ids (a row needs at least 2)", (long long)n);
    if (layout) CHECK_RC(batch_layout_check("dataset_create", layout, 65536));
    int mx = 0;
    for (int64_t i = 0; i < n; i++) mx = std::max(mx, (int)ids[i]);
    HIP_CHECK(hipSetDevice(ctx->device));
    cmp_dataset* d = new cmp_dataset();
    d->ctx = ctx;
    d->n = n;
    d->max_id = mx;
    d->has_layout = layout != nullptr;
    if (layout) d->layout = *layout;
    hipError_t e = hipMalloc((void**)&d->ids_dev, (size_t)n * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpy(d->ids_dev, ids, (size_t)n * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d->ids_dev) (void)hipFree(d->ids_dev);
        delete d;
        HIP_CHECK(e);
    }
    *out = d;
    return CMP_OK;
}

extern "C" int cmp_dataset_destroy(cmp_dataset* d) {
    if (!d) return CMP_OK;
    hipSetDevice(d->ctx->device);
    hipStreamSynchronize(d->ctx->stream);          // a train step that reads the stream may still be in flight
    if (d->ids_dev) (void)hipFree(d->ids_dev);
    if (d->start_bits_dev) (void)hipFree(d->start_bits_dev);
    delete d;
    return CMP_OK;
}

extern "C" int cmp_dataset_batch(cmp_dataset* d, const cmp_batch_row* plan, int B, int W, int32_t* x_host, int32_t* y_host,
                                 int32_t* status_host) {
    CMP_REQUIRE(d && plan && x_host && y_host, "dataset_batch: null argument");
    CHECK_RC(batch_plan_check("dataset_batch", d, plan, B, W, 0));
    HIP_CHECK(hipSetDevice(d->ctx->device));
    const size_t row_b = (size_t)W * 4, plan_b = (size_t)B * sizeof(cmp_batch_row), xy_b = (size_t)B * row_b, st_b = (size_t)B * 8;
    // one allocation: plan, x, y, status (each a multiple of 8 bytes long)
    const size_t xy_pad = (xy_b + 7) & ~(size_t)7;
    char* buf = nullptr;
    HIP_CHECK(hipMalloc((void**)&buf, plan_b + 2 * xy_pad + st_b));
    cmp_batch_row* plan_dev = (cmp_batch_row*)buf;
    int32_t* x = (int32_t*)(buf + plan_b);
    int32_t* y = (int32_t*)(buf + plan_b + xy_pad);
    int32_t* st = (int32_t*)(buf + plan_b + 2 * xy_pad);
    hipStream_t s = d->ctx->stream;
    hipError_t e = hipMemcpyAsync(plan_dev, plan, plan_b, hipMemcpyHostToDevice, s);
    int rc = CMP_OK;
    if (e == hipSuccess) rc = batch_rows_run(s, d, plan_dev, B, W, x, y, st);
    if (e == hipSuccess && rc == CMP_OK) e = hipMemcpyAsync(x_host, x, xy_b, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && rc == CMP_OK) e = hipMemcpyAsync(y_host, y, xy_b, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && rc == CMP_OK && status_host) e = hipMemcpyAsync(status_host, st, st_b, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    (void)hipFree(buf);
    if (rc != CMP_OK) return rc;
    HIP_CHECK(e);
    HIP_CHECK(e2);
    return CMP_OK;
}
