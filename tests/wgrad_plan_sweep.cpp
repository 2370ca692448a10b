// Stand-alone sweep of composer_amd/csrc/wgrad_plan.h (host compiler, no HIP include path; run under ASan + UBSan by
// tests/test_wgrad_group_plan_host.py).  For every problem list the plan takes: every (tile, k-step) is covered exactly once, the
// items of tile row 0 of a problem cover every (column tile, k-step) of its B operand exactly once (what makes the bias sums that
// ride on the launch correct), the item-table order is a permutation of the K-range-major order, and the counts agree.
#include "../composer_amd/csrc/wgrad_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check(const std::vector<WgradProblem>& pr, int K, int max_wgs) {
    const WgPlan p = wgrad_group_plan(pr.data(), (int)pr.size(), K, max_wgs, false, true);
    if (p.refusal != WG_FITS) return;
    EXPECT(p.taken, "force must take a fitting list");
    EXPECT(p.nitems == (int)p.order.size() && p.T == (int)p.tiles.size() && p.nk == K / WG_BK, "counts");
    EXPECT(p.grid == (p.nitems < p.G ? p.nitems : p.G) && p.G % 8 == 0 && p.G <= 256, "grid");
    std::vector<std::vector<int>> cover((size_t)p.T, std::vector<int>((size_t)p.nk, 0));
    std::vector<int> seen_idx((size_t)p.T, 0);
    int longest = 0;
    for (const WgPlanItem& it : p.order) {
        EXPECT(it.tile >= 0 && it.tile < p.T && it.kt0 >= 0 && it.kt0 < it.kt1 && it.kt1 <= p.nk, "item range");
        EXPECT(it.idx == seen_idx[(size_t)it.tile], "K ranges of a tile are numbered in order");
        seen_idx[(size_t)it.tile]++;
        for (int k = it.kt0; k < it.kt1; k++) cover[(size_t)it.tile][(size_t)k]++;
        if (it.kt1 - it.kt0 > longest) longest = it.kt1 - it.kt0;
    }
    EXPECT(longest == p.longest, "longest");
    int nslots = 0;
    for (int t = 0; t < p.T; t++) {
        EXPECT(seen_idx[(size_t)t] == p.tiles[(size_t)t].ranges && p.tiles[(size_t)t].ranges >= 1 && p.tiles[(size_t)t].ranges <= p.max_split, "ranges");
        for (int k = 0; k < p.nk; k++) EXPECT(cover[(size_t)t][(size_t)k] == 1, "tile %d k-step %d covered %d times", t, k, cover[(size_t)t][(size_t)k]);
        EXPECT(p.slot0[(size_t)t] == nslots, "slot0");
        if (p.tiles[(size_t)t].ranges > 1) nslots += p.tiles[(size_t)t].ranges;
    }
    EXPECT(nslots == p.nslots, "nslots");
    // tiles: every (problem, tile row, tile column) once; tile row 0 of problem i = one tile per column tile
    for (size_t i = 0; i < pr.size(); i++) {
        const int tn = wg_cdiv(pr[i].N, 256), tm = wg_cdiv(pr[i].M, 256);
        std::vector<int> grid((size_t)tm * tn, 0);
        std::vector<std::vector<int>> bcover((size_t)tn, std::vector<int>((size_t)p.nk, 0));
        for (int t = 0; t < p.T; t++) {
            const WgPlanTile& tl = p.tiles[(size_t)t];
            if (tl.prob != (int)i) continue;
            EXPECT(tl.m0 % 256 == 0 && tl.n0 % 256 == 0 && tl.m0 < pr[i].M && tl.n0 < pr[i].N, "tile origin");
            grid[(size_t)(tl.m0 / 256) * tn + tl.n0 / 256]++;
        }
        for (int g : grid) EXPECT(g == 1, "tile listed %d times", g);
        for (const WgPlanItem& it : p.order) {
            const WgPlanTile& tl = p.tiles[(size_t)it.tile];
            if (tl.prob != (int)i || tl.m0 != 0) continue;
            for (int k = it.kt0; k < it.kt1; k++) bcover[(size_t)(tl.n0 / 256)][(size_t)k]++;
        }
        for (int c = 0; c < tn; c++)
            for (int k = 0; k < p.nk; k++) EXPECT(bcover[(size_t)c][(size_t)k] == 1, "problem %zu column tile %d k-step %d summed %d times", i, c, k, bcover[(size_t)c][(size_t)k]);
    }
    // item-table order: a permutation
    std::vector<int> hit((size_t)p.nitems, 0);
    for (int item = 0; item < p.nitems; item++) {
        const int lin = p.lin_of(item);
        EXPECT(lin >= 0 && lin < p.nitems, "lin_of out of range");
        if (lin >= 0 && lin < p.nitems) hit[(size_t)lin]++;
    }
    for (int h : hit) EXPECT(h == 1, "lin_of is no permutation");
}

int main() {
    const int dims[] = {8, 64, 136, 256, 264, 520, 1000, 1536, 2048, 3072};
    const int Ks[] = {32, 96, 128, 1024, 4096, 32768, 131072};
    const int wgs[] = {0, 8, 100, 208, 256, 1000};
    long planned = 0;
    unsigned seed = 12345;
    auto rnd = [&seed](int n) { seed = seed * 1664525u + 1013904223u; return (int)((seed >> 8) % (unsigned)n); };
    for (int K : Ks)
        for (int w : wgs)
            for (int rep = 0; rep < 40; rep++) {
                const int n = 1 + rnd(WG_MAXP);
                std::vector<WgradProblem> pr;
                for (int i = 0; i < n; i++) {
                    const int M = dims[rnd(10)], N = dims[rnd(10)];
                    pr.push_back(WgradProblem{(const void*)0x1000, M + 8 * rnd(2), (const void*)0x2000, N + 16 * rnd(2), nullptr, N, M, N});
                }
                check(pr, K, w);
                planned++;
            }
    // the block shapes of the benchmark configurations (E, tokens)
    const int blocks[][2] = {{512, 131072}, {512, 32768}, {768, 65536}, {64, 96}};
    for (auto& b : blocks) {
        const int E = b[0], M = b[1];
        std::vector<WgradProblem> pr = {{(const void*)0x1000, 4 * E, (const void*)0x1000, E, nullptr, E, 4 * E, E},
                                        {(const void*)0x1000, E, (const void*)0x1000, 4 * E, nullptr, 4 * E, E, 4 * E},
                                        {(const void*)0x1000, E, (const void*)0x1000, E, nullptr, E, E, E},
                                        {(const void*)0x1000, E, (const void*)0x1000, 3 * E, nullptr, 3 * E, E, 3 * E}};
        check(pr, M, 0);
        const WgPlan p = wgrad_group_plan(pr.data(), 4, M, 0, false, false);
        EXPECT(p.refusal == WG_FITS && p.taken, "the block of E=%d at %d tokens takes the grouped launch", E, M);
        planned++;
    }
    // refusals touch nothing of the list beyond what they judge
    {
        WgradProblem one{(const void*)0x1000, 64, (const void*)0x1000, 64, nullptr, 64, 64, 64};
        EXPECT(wgrad_group_plan(&one, 0, 64, 0, false, true).refusal == WG_REFUSE_NPROB, "nprob 0");
        EXPECT(wgrad_group_plan(&one, 9, 64, 0, false, true).refusal == WG_REFUSE_NPROB, "nprob 9");
        EXPECT(wgrad_group_plan(&one, 1, 48, 0, false, true).refusal == WG_REFUSE_K, "K no multiple of 32");
        EXPECT(wgrad_group_plan(&one, 1, 64, 7, false, true).refusal == WG_REFUSE_WGS, "7 workgroups");
        EXPECT(wgrad_group_plan(&one, 1, 64, 0, true, true).refusal == WG_REFUSE_SLAB, "slab");
    }
    if (failures) { printf("wgrad_plan sweep: %d failures\n", failures); return 1; }
    printf("wgrad_plan sweep ok: %ld lists\n", planned);
    return 0;
}
