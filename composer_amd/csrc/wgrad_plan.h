// wgrad_plan.h -- the ONE decision of the grouped weight-gradient launch (gemm.hip: gemm_wgrad_group_kernel): whether a list of
// problems fits the kernel, whether one grouped launch beats one split-K launch per problem, and the item table -- which
// (tile, K range) pairs exist and in which order they are dealt out.  Pure host code: no HIP header, no HIP call, no environment
// variable; pointers are looked at for 16-byte alignment only.  gemm.hip: wgrad_group_run builds the plan and launches it;
// model.hip: backward() asks it BEFORE it enqueues a block (whether the bias gradients can ride on the launch);
// cmp_wgrad_group_plan shows it to the CPU tests (tests/test_wgrad_group_plan_host.py).
//
// All T output tiles (of all problems) are cut into the SAME s = floor(G / T) K ranges; item lin = range * T + tile, dealt to the
// XCD groups in consecutive runs like every persistent launch here: the workgroups of an XCD contract the same rows of
// different tiles in step, so its L2 fetches each operand panel once.  (A stream-K cut -- one contiguous range of exactly
// T * nk / G k-steps per workgroup -- was built first and measured: every workgroup equally long, but the ranges of an XCD start
// at unrelated rows, nothing is shared through L2, and the launch took 890 us at K = 131072 where this form is predicted at
// ~800 and four split-K launches take 902-954; at C4's 108 tiles it lost 3.6 % of the step.)
// Cost model in k-steps of 32 (tools/kbench.py wgradgroup: 0.91 us per k-step, 54 us = 59 k-steps of atomic epilogue per launch):
// grouped = ceil(nk / s) * rounds + 59 against the sum over problems of nk / split_p + 59 -- the grouped launch is used when it wins.
//
// The bias sums that ride on the launch (WgradProblem::bias) rest on one property of the table, which the CPU test sweeps: the
// K ranges of a tile cover [0, nk) exactly once, so the items of the tiles in tile row 0 (m0 == 0) of a problem cover every
// (column tile, k-step) of its B operand exactly once.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <vector>

#define WG_MAXP 8               // problems per grouped launch
#define WG_BK 32                // k-step of the kernel (gemm_plan.h: P_BK)

// One launch for several split-K weight gradients that contract over the same K rows (gemm.hip: gemm_wgrad_group_kernel):
// problem i is C_i[M_i, N_i] (fp32, accumulated into) += A_i^T . B_i with A_i stored [K, M_i] and B_i stored [K, N_i], bf16.
// bias (null: none): bias[0..N_i) += the column sums of B_i over the K rows, by the same launch (the float-atomic form only).
struct WgradProblem { const void* A; int lda; const void* B; int ldb; float* C; int ldc; int M, N; float* bias = nullptr; };

enum { WG_FITS = 0, WG_REFUSE_NPROB = 1, WG_REFUSE_K = 2, WG_REFUSE_WGS = 3, WG_REFUSE_SLAB = 4, WG_REFUSE_SHAPE = 5, WG_REFUSE_LD = 6,
       WG_REFUSE_ALIGN = 7, WG_REFUSE_SPAN = 8, WG_REFUSE_TABLE = 9 };

struct WgPlanTile { int prob, m0, n0, ranges; };          // ranges: K ranges the tile really has
struct WgPlanItem { int tile, kt0, kt1, idx; };           // k-steps [kt0, kt1); idx: index of this range among the tile's
struct WgPlan {
    int refusal = WG_FITS;       // != WG_FITS: outside the grouped kernel's domain; nothing below is filled
    bool taken = false;          // fits, and the cost model (or `force`) chooses the grouped launch
    int G = 0;                   // workgroups the launch may use (a multiple of 8)
    int T = 0, nk = 0;           // output tiles of all problems, k-steps
    int nitems = 0, grid = 0;
    int max_split = 0, longest = 0;       // most K ranges of a tile; longest item in k-steps
    int nslots = 0;              // last-arriver form: workspace slots (one per K range of a multi-range tile)
    std::vector<WgPlanTile> tiles;
    std::vector<WgPlanItem> order;        // K-range-major: range j of every tile that has one, tile by tile
    std::vector<int> slot0;               // first workspace slot of a tile
    // item table position -> index into `order`: the XCD group of position p is p & 7, and a group's positions hold consecutive items
    int lin_of(int item) const {
        const int q = nitems >> 3, r = nitems & 7, x = item & 7;
        return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (item >> 3);
    }
};

static inline int wg_cdiv(int a, int b) { return (a + b - 1) / b; }

// max_wgs: cap on the grid (0 = all 256); slab_ws: the caller asked for slab split-K (deterministic without the last-arriver
// workspace); force: take the grouped launch whatever the cost model says (kernel-level entry points).
static inline WgPlan wgrad_group_plan(const WgradProblem* probs, int nprob, int K, int max_wgs, bool slab_ws, bool force) {
    WgPlan p;
    p.G = (max_wgs > 0 ? std::min(max_wgs, 256) : 256) & ~7;
    const int G = p.G;
    if (nprob < 1 || nprob > WG_MAXP) { p.refusal = WG_REFUSE_NPROB; return p; }
    if (K < WG_BK || K % WG_BK != 0) { p.refusal = WG_REFUSE_K; return p; }
    if (G < 8) { p.refusal = WG_REFUSE_WGS; return p; }
    if (slab_ws) { p.refusal = WG_REFUSE_SLAB; return p; }
    for (int i = 0; i < nprob; i++) {
        const WgradProblem& q = probs[i];
        if (q.M <= 0 || q.N <= 0 || q.M >= 65536 - 256 || q.N >= 65536 - 256) { p.refusal = WG_REFUSE_SHAPE; return p; }
        if (q.lda % 8 || q.ldb % 8) { p.refusal = WG_REFUSE_LD; return p; }
        if (((uintptr_t)q.A & 15) || ((uintptr_t)q.B & 15)) { p.refusal = WG_REFUSE_ALIGN; return p; }
        if ((int64_t)K * q.lda * 2 >= 0x7FFFFFF0ll || (int64_t)K * q.ldb * 2 >= 0x7FFFFFF0ll) { p.refusal = WG_REFUSE_SPAN; return p; }
    }
    for (int i = 0; i < nprob; i++)
        for (int tm = 0; tm < wg_cdiv(probs[i].M, 256); tm++)
            for (int tn = 0; tn < wg_cdiv(probs[i].N, 256); tn++) p.tiles.push_back({i, tm * 256, tn * 256, 0});
    const int T = (int)p.tiles.size(), nk = K / WG_BK;
    p.T = T;
    p.nk = nk;
    // Split count: every split of every tile is one more partial 256x256 f32 tile through the float-atomic unit (~1.3 TB/s),
    // every split less is a longer k-loop per workgroup.  With few tokens the atomics win: the reference's default configuration
    // (1 024 tokens, 12 tiles) ran 21 splits = 64 MB of atomics for 32 k-steps of work, 44 us per block; the minimum of
    //   ceil(nk / s) * 0.91 us + T * s * 256 KiB / 1.3 TB/s          (tools/kbench.py wgradgroup, same constants as below)
    // over s <= G / T is 4 splits there (~17 us) and stays at G / T for the benchmark shapes (K = 32 768 ... 131 072 tokens).
    // (the last-arriver form takes the same cut: K ranges finer than one item per workgroup -- 7 ranges in 3 rounds at C4's 108
    //  tiles -- measured 917 us without its reduction reads and 967 with them against 934 for the float-atomic form's 2 ranges)
    int sp = 1;
    {
        const int smax = std::max(1, std::min(G / std::max(1, T), nk));
        double best = 1e30;
        for (int c = 1; c <= smax; c++) {
            const double t = (double)wg_cdiv(nk, c) * 0.91 + (double)T * c * 262144.0 / 1.3e6;
            if (t < best * 0.999) { best = t; sp = c; }
        }
    }
    // Workgroups left over by the common split count (C2: 256 - 48 * 5 = 16) go to whole PROBLEMS, smallest first, as one
    // more split each (tiles that share operand panels keep the same K ranges): their items are shorter, finish early and
    // put their share of the atomic traffic out before the final burst; the longest item is unchanged.
    std::vector<int> tiles_of(nprob, 0), split_of(nprob, sp);
    for (const WgPlanTile& t : p.tiles) tiles_of[t.prob]++;
    {
        int spare = G - T * sp;
        std::vector<int> byt(nprob);
        for (int i = 0; i < nprob; i++) byt[i] = i;
        std::stable_sort(byt.begin(), byt.end(), [&](int a, int b) { return tiles_of[a] < tiles_of[b]; });
        for (int i : byt)
            if (T * sp <= G && sp + 1 <= nk && tiles_of[i] <= spare) { split_of[i] = sp + 1; spare -= tiles_of[i]; }
    }
    // items in K-range-major order (range j of every problem that has one, tile by tile): consecutive items = one XCD's group
    for (int i = 0; i < nprob; i++) p.max_split = std::max(p.max_split, split_of[i]);
    for (int j = 0; j < p.max_split; j++)
        for (int t = 0; t < T; t++) {
            const int spt = split_of[p.tiles[t].prob], chunk = wg_cdiv(nk, spt);
            if (j * chunk >= nk) continue;              // a chunk that starts behind nk does not exist
            p.order.push_back({t, j * chunk, std::min(nk, (j + 1) * chunk), p.tiles[t].ranges});
            p.tiles[t].ranges += 1;
            p.longest = std::max(p.longest, std::min(nk, (j + 1) * chunk) - j * chunk);
        }
    p.nitems = (int)p.order.size();
    if (p.max_split > 255 || T > 4095) { p.refusal = WG_REFUSE_TABLE; return p; }       // (the meta word's fields; far outside any model shape)
    p.slot0.assign(T, 0);                        // single-range tiles need no slot
    for (int t = 0; t < T; t++) { p.slot0[t] = p.nslots; if (p.tiles[t].ranges > 1) p.nslots += p.tiles[t].ranges; }
    p.grid = std::min(p.nitems, G);
    {   // is one grouped launch cheaper than one split-K launch per problem?  (model above; K-independent overhead in k-steps)
        const double ov = 59.0;
        const double grouped = (double)p.longest * wg_cdiv(p.nitems, G) + ov;
        double separate = 0.0;
        for (int i = 0; i < nprob; i++) {
            const int t = wg_cdiv(probs[i].M, 256) * wg_cdiv(probs[i].N, 256);
            const int si = std::max(1, std::min(G / std::max(1, t), nk));
            separate += (double)wg_cdiv(nk, si) * wg_cdiv(t * si, G) + ov;
        }
        p.taken = force || grouped < separate;
    }
    return p;
}
