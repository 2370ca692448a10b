// evalpass.hip -- the validation pass (include/composer_hip.h, "validation pass"): held-out loss of a whole split in HBM, summed per
// event class on the device.  Windows of the fixed grid are cut out of the id stream, the inference forward pass runs on them, and
// every logits row is reduced by score_rows.h's walk (the figures cmp_k_score_rows stores) into per-workgroup partial tables that one
// workgroup folds by index.  One pass over the logits; no atomics, no spin loop, no scratch; the launch boundary is the only
// dependency between workgroups.
// A translation unit of its own: adding it leaves every kernel of the other sources instruction-identical (tools/isa_hash.py).
#include "model.h"
#include "score_rows.h"

#define EVAL_SLOTS 9                    // 8 classes and "every other id"
#define EVAL_MAX_PARTS 1024             // workgroups of eval_rows_kernel = partial tables of one launch
#define EVAL_STRIPES 16                 // eval_fold_kernel: 16 threads per slot, thread j of them adds parts j, j + 16, ...

// the device image of cmp_eval_table, also the layout of a partial table
struct EvalTable {
    double nll[EVAL_SLOTS];
    long long count[EVAL_SLOTS];
    long long correct[EVAL_SLOTS];
};
static_assert(sizeof(EvalTable) == sizeof(cmp_eval_table), "EvalTable is cmp_eval_table");

// class of a target id inside [0, V): lane j < K.n holds range j (lo, hi) and the wave votes -- the range that holds y, else K.n
__device__ __forceinline__ int eval_class_of(int n, int lane, int lo, int hi, int y) {
    const unsigned long long in = __ballot(lane < n && y >= lo && y < hi);
    return in ? __builtin_ctzll(in) : n;
}

// Lane c of a wave keeps the sums of class c over the rows the wave walks: a row's figures are the same in every lane, so the lane
// that owns the row's class adds them (no run-time index into a register array).  A wave's rows come in ascending order.  The four
// waves' sums meet in LDS and thread c adds them in wave order into partial table blockIdx.x, every word of which is written.
// FORM: score_rows_form.
template <int FORM>
__global__ __launch_bounds__(256) void eval_rows_kernel(const float* __restrict__ z, int ldz, const int32_t* __restrict__ y, int rows,
                                                        int V, cmp_eval_classes K, EvalTable* __restrict__ parts) {
    __shared__ double sh_nll[4][EVAL_SLOTS];
    __shared__ int sh_cnt[4][EVAL_SLOTS], sh_cor[4][EVAL_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int my_lo = K.lo[lane & 7], my_hi = K.hi[lane & 7];
    double nll = 0.0;
    int cnt = 0, cor = 0;
    auto sink = [&](int, int yy, bool valid, float zy, float gmx, float s, float, int rank) {
        const int cls = valid ? eval_class_of(K.n, lane, my_lo, my_hi, yy) : -1;      // a target outside [0, V) is counted nowhere
        if (lane == cls) {
            nll += (double)-score_logp(zy, gmx, logf(s));
            cnt += 1;
            cor += rank == 0 ? 1 : 0;
        }
    };
    if (FORM == 2)
        score_walk_rows_wide(z, ldz, y, rows, V, 4, sink);
    else
        score_walk_rows<FORM == 0>(z, ldz, y, rows, V, 4, sink);
    if (lane < EVAL_SLOTS) { sh_nll[wave][lane] = nll; sh_cnt[wave][lane] = cnt; sh_cor[wave][lane] = cor; }
    __syncthreads();
    if (threadIdx.x < EVAL_SLOTS) {
        const int c = threadIdx.x;
        double a = 0.0;
        long long n = 0, k = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { a += sh_nll[w][c]; n += sh_cnt[w][c]; k += sh_cor[w][c]; }
        EvalTable& p = parts[blockIdx.x];
        p.nll[c] = a; p.count[c] = n; p.correct[c] = k;
    }
}

// One workgroup: thread (j, c) = (tid / 16, tid % 16), c < 9, adds the parts j, j + 16, ... of slot c in ascending order, thread c
// then adds the 16 stripes in ascending order and adds the result INTO the table.  The order is a function of nparts alone.
__global__ __launch_bounds__(256) void eval_fold_kernel(const EvalTable* __restrict__ parts, int nparts, EvalTable* __restrict__ table) {
    __shared__ double sh_nll[EVAL_STRIPES][EVAL_SLOTS];
    __shared__ long long sh_cnt[EVAL_STRIPES][EVAL_SLOTS], sh_cor[EVAL_STRIPES][EVAL_SLOTS];
    const int c = threadIdx.x & 15, j = threadIdx.x >> 4;
    if (c < EVAL_SLOTS) {
        double a = 0.0;
        long long n = 0, k = 0;
        for (int p = j; p < nparts; p += EVAL_STRIPES) { a += parts[p].nll[c]; n += parts[p].count[c]; k += parts[p].correct[c]; }
        sh_nll[j][c] = a; sh_cnt[j][c] = n; sh_cor[j][c] = k;
    }
    __syncthreads();
    if (threadIdx.x < EVAL_SLOTS) {
        const int s = threadIdx.x;
        double a = 0.0;
        long long n = 0, k = 0;
#pragma unroll
        for (int q = 0; q < EVAL_STRIPES; q++) { a += sh_nll[q][s]; n += sh_cnt[q][s]; k += sh_cor[q][s]; }
        table->nll[s] += a; table->count[s] += n; table->correct[s] += k;
    }
}

// x[r, t] = ids[(first + r)(T + 1) + t], y[r, t] = ids[(first + r)(T + 1) + t + 1]: B windows of the fixed grid (the caller has checked
// that the last one ends inside the stream)
__global__ __launch_bounds__(256) void eval_windows_kernel(const uint16_t* __restrict__ ids, int64_t first, int B, int T,
                                                           int32_t* __restrict__ x, int32_t* __restrict__ y) {
    const int n = B * T;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int r = i / T, t = i - r * T;
        const uint16_t* w = ids + (first + r) * ((int64_t)T + 1);
        x[i] = w[t];
        y[i] = w[t + 1];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
static int eval_parts(int rows) { return std::min(cdiv(rows, 4), EVAL_MAX_PARTS); }

static int eval_classes_check(const char* who, const cmp_eval_classes* k, int V) {
    if (!k) return CMP_OK;
    CMP_REQUIRE(k->n >= 0 && k->n <= 8, "%s: %d classes (at most 8)", who, k->n);
    for (int i = 0; i < k->n; i++) {
        CMP_REQUIRE(k->lo[i] >= 0 && k->hi[i] <= V && k->lo[i] < k->hi[i], "%s: class %d: ids [%d, %d) are empty or outside the vocabulary "
                    "[0, %d)", who, i, k->lo[i], k->hi[i], V);
        for (int j = 0; j < i; j++)
            CMP_REQUIRE(k->hi[i] <= k->lo[j] || k->hi[j] <= k->lo[i], "%s: class %d [%d, %d) overlaps class %d [%d, %d)", who, i, k->lo[i],
                        k->hi[i], j, k->lo[j], k->hi[j]);
    }
    return CMP_OK;
}

static int eval_rows_launch(hipStream_t s, const float* logits, int ldz, const int32_t* y, int rows, int V, const cmp_eval_classes* classes,
                            EvalTable* table, EvalTable* parts) {
    cmp_eval_classes K = {};
    if (classes) K = *classes;
    const int grid = eval_parts(rows);
    const int form = score_rows_form(logits, ldz);
    if (form == 2)
        eval_rows_kernel<2><<<grid, 256, 0, s>>>(logits, ldz, y, rows, V, K, parts);
    else if (form == 0)
        eval_rows_kernel<0><<<grid, 256, 0, s>>>(logits, ldz, y, rows, V, K, parts);
    else
        eval_rows_kernel<1><<<grid, 256, 0, s>>>(logits, ldz, y, rows, V, K, parts);
    KERNEL_CHECK();
    eval_fold_kernel<<<1, 256, 0, s>>>(parts, grid, table);
    KERNEL_CHECK();
    return CMP_OK;
}

extern "C" int64_t cmp_k_eval_rows_ws(int rows) { return (int64_t)std::max(1, eval_parts(std::max(rows, 0))) * sizeof(EvalTable); }

extern "C" int cmp_k_eval_rows(void* stream, const float* logits, int ldz, const int32_t* y, int rows, int V,
                               const cmp_eval_classes* classes, void* table_dev, void* ws_dev) {
    CMP_REQUIRE(logits && y && table_dev && ws_dev, "eval_rows: null argument");
    CMP_REQUIRE(V > 0 && V <= ldz && rows >= 0, "eval_rows: V=%d ldz=%d rows=%d", V, ldz, rows);
    CMP_REQUIRE(((uintptr_t)table_dev & 7) == 0 && ((uintptr_t)ws_dev & 7) == 0, "eval_rows: the table and the workspace must be 8-byte "
                "aligned");
    CHECK_RC(eval_classes_check("eval_rows", classes, V));
    if (rows == 0) return CMP_OK;
    return eval_rows_launch((hipStream_t)stream, logits, ldz, y, rows, V, classes, (EvalTable*)table_dev, (EvalTable*)ws_dev);
}

// The pass.  Nothing that lasts is written (cmp_score's list): x_dev / y_dev, the activations and the logits are the scratch every
// forward pass rewrites, the table and the partial tables are the pass's own.
extern "C" int cmp_eval_dataset(cmp_model* m, cmp_dataset* ds, int64_t first_window, int64_t n_windows, int T, int batch,
                                const cmp_eval_classes* classes, cmp_eval_table* out) {
    CMP_REQUIRE(m && ds && out, "eval_dataset: null argument");
    CMP_REQUIRE(ds->ctx == m->ctx, "eval_dataset: the dataset and the model belong to different contexts");
    CMP_REQUIRE(ds->max_id < m->V, "eval_dataset: the dataset's largest id %d is outside the model's vocabulary [0, %d)", ds->max_id, m->V);
    const int max_T = std::min(m->W, m->cfg.max_seq);
    CMP_REQUIRE(T >= 1 && T <= max_T, "eval_dataset: T=%d outside [1, min(window_size, max_seq) = %d]", T, max_T);
    CMP_REQUIRE(batch >= 1 && batch <= std::max(1, m->cfg.max_batch), "eval_dataset: batch=%d outside [1, max_batch = %d]", batch,
                std::max(1, m->cfg.max_batch));
    CMP_REQUIRE(first_window >= 0 && n_windows >= 1 && first_window <= ds->n / ((int64_t)T + 1) &&
                n_windows <= ds->n / ((int64_t)T + 1) - first_window,
                "eval_dataset: windows [%lld, %lld + %lld) of %d + 1 ids lie outside the stream of %lld ids (%lld windows)",
                (long long)first_window, (long long)first_window, (long long)n_windows, T, (long long)ds->n,
                (long long)(ds->n / ((int64_t)T + 1)));
    CHECK_RC(eval_classes_check("eval_dataset", classes, m->V));
    HIP_CHECK(hipSetDevice(m->ctx->device));
    CHECK_RC(ensure_workspace(m, batch, T));
    if (!m->eval_buf) CHECK_RC(dev_alloc(m, &m->eval_buf, (size_t)(1 + EVAL_MAX_PARTS) * sizeof(EvalTable)));
    EvalTable* table = (EvalTable*)m->eval_buf;
    EvalTable* parts = table + 1;
    hipStream_t s = m->ctx->stream;
    HIP_CHECK(hipStreamSynchronize(s));                 // a train step may be in flight: the pass starts on an idle stream
    HIP_CHECK(hipMemsetAsync(table, 0, sizeof(EvalTable), s));
    for (int64_t w0 = 0; w0 < n_windows; w0 += batch) {
        const int B = (int)std::min<int64_t>(batch, n_windows - w0);        // the last batch is ragged, not dropped
        const int rows = B * T;
        eval_windows_kernel<<<std::min(cdiv(rows, 256), 1024), 256, 0, s>>>(ds->ids_dev, first_window + w0, B, T, m->x_dev, m->y_dev);
        KERNEL_CHECK();
        CHECK_RC(model_forward(m, m->x_dev, B, T, false, 0));
        CHECK_RC(eval_rows_launch(s, m->logits, m->ldz, m->y_dev, rows, m->V, classes, table, parts));
    }
    HIP_CHECK(hipMemcpyAsync(out, table, sizeof(EvalTable), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return CMP_OK;
}
