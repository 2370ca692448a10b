// Stand-alone sweep of attn_plan_fwd / attn_plan_bwd (composer_amd/csrc/attn_plan.h) under the host compiler: shows that the header
// needs no HIP and, with -fsanitize=address,undefined, that its 32/64-bit arithmetic does not overflow up to B = 512, T = 4096,
// H = 16, D = 128 (tests/test_attn_plan_host.py builds it).
#include "../composer_amd/csrc/attn_plan.h"
#include <stdlib.h>

static long cases = 0, refused = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s: bwd=%d dtype=%d B=%d T=%d H=%d D=%d p=%g amask=%d bias=%d ln=%d wgs=%d ks=%d\n", #c, backward, d.dtype, d.B, d.T, d.H, d.D, d.p_drop, d.amask != nullptr, d.bias_grad != nullptr, d.ln.rstd != nullptr, caps.wgs_per_cu, caps.ks_ok); exit(1); } } while (0)

static void one(const AttnDesc& d, const AttnEnv& env, const AttnCaps& caps, bool backward) {
    const AttnPlan p = backward ? attn_plan_bwd(d, env, caps) : attn_plan_fwd(d, env, caps);
    cases++;
    if (p.status != CMP_OK) { refused++; CHECK(p.msg[0] != 0); return; }
    if (p.empty) { CHECK(d.B * d.T == 0); return; }
    const bool bf16 = d.dtype == CMP_BF16, ks = p.form == CMP_ATTN_FWD_KS || p.form == CMP_ATTN_BWD_KS1 || p.form == CMP_ATTN_BWD_KS2;
    CHECK(backward ? p.form >= CMP_ATTN_BWD_LN && p.form <= CMP_ATTN_BWD_ROWS : p.form >= CMP_ATTN_FWD_KS && p.form <= CMP_ATTN_FWD_ROWS);
    CHECK(p.nlaunch == ((p.form >= CMP_ATTN_BWD_LN && p.form != CMP_ATTN_BWD_KS1) ? 2 : 1) && p.block == 256);
    size_t top = 0;
    for (int i = 0; i < p.nlaunch; i++) {
        CHECK(p.l[i].grid_x > 0 && p.l[i].grid_y > 0 && p.l[i].smem > 0 && p.l[i].smem <= 160 * 1024);
        CHECK((p.l[i].cls >= 3 && p.l[i].work > 0 && p.l[i].bytes > 0) || (p.form == CMP_ATTN_FWD_MASK && p.l[i].cls == -1));
        top = p.l[i].smem > top ? p.l[i].smem : top;
    }
    CHECK(p.optin == (top > 65536));
    if (ks) CHECK(bf16 && d.D <= 32 && d.T >= 64 && caps.ks_ok && !d.amask && !d.ln.rstd && env.ks_mode != 0 && p.plan_u == -1);
    CHECK((p.form == CMP_ATTN_BWD_LN) == (backward && d.ln.rstd != nullptr) && (p.form == CMP_ATTN_FWD_MASK) == (!backward && d.amask != nullptr));
    CHECK(p.bias_fused + p.bias_pass == (backward && d.bias_grad != nullptr) && !(p.bias_pass && !bf16));
    const int BH = d.B * d.H, nb = (d.T + 127) / 128, pairs = (nb + 1) / 2;
    if (p.plan_u >= 0) {
        CHECK(!ks && caps.wgs_per_cu >= 1 && BH % 8 == 0 && p.plan_u > 0 && p.plan_u < BH / 8 && p.l[0].grid_y == 1);
        CHECK((int64_t)p.l[0].grid_x == 8ll * ((int64_t)(BH / 8 - p.plan_u) * pairs + (int64_t)p.plan_u * nb));
    } else if (!ks) {
        CHECK(p.l[0].grid_y == (unsigned)BH && (p.l[0].grid_x == (unsigned)nb || p.l[0].grid_x == (unsigned)pairs));
    }
}

int main() {
    static const float some = 0.f;
    float* const fake = const_cast<float*>(&some);      // never dereferenced
    const int Bs[] = {0, 1, 2, 3, 8, 40, 128, 512}, Ts[] = {1, 33, 63, 64, 96, 128, 129, 600, 1000, 1024, 2048, 4096}, Hs[] = {1, 4, 8, 12, 16},
              Ds[] = {16, 32, 48, 64, 128};
    const float ps[] = {0.f, 1e-12f, 0.1f};
    for (int backward = 0; backward < 2; backward++) for (int dtype = 0; dtype < 2; dtype++) for (int B : Bs) for (int T : Ts) for (int H : Hs)
    for (int D : Ds) for (float pd : ps) for (int opt = 0; opt < 4; opt++) for (int wgs = 0; wgs <= 4; wgs++) for (int ks = 0; ks < 2; ks++)
    for (int mode = -1; mode <= 1; mode++) for (int mib = 0; mib <= 16; mib += 16) {
        AttnDesc d;
        d.dtype = dtype; d.B = B; d.T = T; d.H = H; d.D = D; d.p_drop = pd;
        if (!backward && (opt & 1)) d.amask = fake;
        if (backward && (opt & 1)) d.bias_grad = fake;
        if (backward && (opt & 2)) d.ln.rstd = fake;
        AttnEnv env;
        env.ks_mode = mode; env.bias_pass_mib = mib;
        AttnCaps caps;
        caps.ks_ok = ks != 0; caps.wgs_per_cu = wgs;
        one(d, env, caps, backward != 0);
    }
    printf("attn_plan sweep ok: %ld cases, %ld refused\n", cases, refused);
    return 0;
}
