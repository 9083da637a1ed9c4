// test_ct_eval.cpp -- the coarse tracker's per-evaluation host/device functions (ldso_amd/csrc/ct_eval.h) as a
// stand-alone host program: ct_eval_setup, ct_finish_res and ct_finish_gs_entry on fixed poses, affine pairs
// and sums, bit for bit against the straightforward statements written out here -- the 3x3 product and
// fromToVecExposure for the setup, the symmetric float 9x9 and the two scaling loops of
// Accumulator9::finish + CoarseTracker.cc:725-740 for the finish.  Header only: no HIP runtime call, no
// library, so the same source builds under -fsanitize=address,undefined (make sanitize-ct-eval).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../ldso_amd/csrc/ct_eval.h"

using namespace ldso_ct;

namespace {

int g_fail = 0;
long long g_checks = 0;
std::string g_case;
#define CHECK(cond)                                                                                            \
    do {                                                                                                       \
        g_checks++;                                                                                            \
        if (!(cond) && g_fail++ < 40) std::printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
    } while (0)

struct Lcg {
    uint64_t s;
    double next() {  // in [-1, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(int32_t)(s >> 32) / 2147483648.0;
    }
};

template <typename T>
bool same_bits(const T &a, const T &b) {
    return std::memcmp(&a, &b, sizeof(T)) == 0;
}

void check_setup(const char *name, const double *T, const float *Ki, float expR, float expN, float ra, float rb, float a,
                 float b, float cutoff) {
    g_case = name;
    CtPose p;
    CtEvalTerms e;
    std::memset(&p, 0xff, sizeof p);
    ct_eval_setup(T, Ki, expR, expN, ra, rb, a, b, cutoff, p, e);
    // CoarseTracker.cc:555-558: (R * Ki[lvl]).cast<float>() of the float R, t as float
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            const float rki = (float)T[4 * i] * Ki[j] + (float)T[4 * i + 1] * Ki[3 + j] + (float)T[4 * i + 2] * Ki[6 + j];
            CHECK(same_bits(p.RKi[3 * i + j], rki));
        }
        CHECK(same_bits(p.t[i], (float)T[4 * i + 3]));
    }
    // AffLight::fromToVecExposure
    float eR = expR, eN = expN;
    if (eR == 0 || eN == 0) eR = eN = 1;
    const float aLL = expf(a - ra) * eN / eR, bLL = b - aLL * rb;
    CHECK(same_bits(p.aLL, aLL) && same_bits(p.bLL, bLL));
    CHECK(p.pad[0] == 0 && p.pad[1] == 0);
    CHECK(same_bits(e.gs_a, aLL) && same_bits(e.gs_b0, rb) && same_bits(e.cutoffTH, cutoff));
    CHECK(same_bits(e.maxEnergy, 2 * 9.0f * cutoff - 9.0f * 9.0f));  // setting_huberTH = 9
}

void check_finish(const char *name, const double *res, const double *gs, int n_warped) {
    g_case = name;
    double rs[6];
    ct_finish_res(res, rs);
    const float E = (float)res[0], sT = (float)res[3], sRT = (float)res[4], sNum = (float)res[5];
    const int nE = (int)res[1], nSat = (int)res[2];
    const double want[6] = {E, (double)nE, sT / (sNum + 0.1), 0, sRT / (sNum + 0.1), nSat / (float)nE};
    for (int k = 0; k < 6; k++) CHECK(same_bits(rs[k], want[k]));
    // the float 9x9 from the upper triangle, then H(r, cc) * (1 / n) * scale[cc] * scale[r] and b likewise
    float H[9][9];
    int k = 0;
    for (int r = 0; r < 9; r++)
        for (int cc = r; cc < 9; cc++, k++) H[r][cc] = H[cc][r] = (float)gs[k];
    const int nw = (n_warped + 3) / 4 * 4;
    const double inv_n = (double)(1.0f / nw);
    const float scale[8] = {0.5f, 0.5f, 0.5f, 1.0f, 1.0f, 1.0f, 10.0f, 1000.0f};
    for (int r = 0; r < 8; r++) {
        for (int cc = 0; cc < 8; cc++)
            CHECK(same_bits(ct_finish_gs_entry(gs, n_warped, r, cc), (double)H[r][cc] * inv_n * scale[cc] * scale[r]));
        CHECK(same_bits(ct_finish_gs_entry(gs, n_warped, r, 8), (double)H[r][8] * inv_n * scale[r]));
    }
}

}  // namespace

int main() {
    for (int k = 0; k < 8; k++) {
        g_case = "scale table";
        const float scale[8] = {0.5f, 0.5f, 0.5f, 1.0f, 1.0f, 1.0f, 10.0f, 1000.0f};  // Settings.h:29-35
        CHECK(kCtScale[k] == scale[k]);
    }
    Lcg rng{12345};
    for (int it = 0; it < 200; it++) {
        // a small rotation about a random axis (first order is enough: the setup only casts and multiplies)
        const double w[3] = {0.05 * rng.next(), 0.05 * rng.next(), 0.05 * rng.next()};
        const double T[12] = {1, -w[2], w[1], 0.3 * rng.next(), w[2], 1, -w[0], 0.3 * rng.next(), -w[1], w[0], 1, 0.3 * rng.next()};
        const float f = 200.f + 300.f * (float)(0.5 + 0.5 * rng.next()), cx = 319.5f + (float)rng.next(), cy = 239.5f;
        const float Ki[9] = {1 / f, 0, -cx / f, 0, 1 / (f * 1.1f), -cy / (f * 1.1f), 0, 0, 1};
        const bool zero_exposure = it % 17 == 0;
        check_setup(zero_exposure ? "setup, zero exposure" : "setup", T, Ki, zero_exposure ? 0.f : 1.0f + 0.2f * (float)rng.next(),
                    0.9f + 0.2f * (float)rng.next(), 0.1f * (float)rng.next(), 5.f * (float)rng.next(),
                    0.3f * (float)rng.next(), 20.f * (float)rng.next(), 20.f * (float)(1 << (it % 4)));
        double res[kResParts], gs[kGsParts];
        const int n = it == 0 ? 0 : 1 + (int)(3000 * (0.5 + 0.5 * rng.next()));  // it 0: a level without a point
        res[0] = n * 40.0 * (1 + rng.next());
        res[1] = n;
        res[2] = n / 7;
        res[3] = n * 1e-3 * (1 + rng.next());
        res[4] = n * 2e-3 * (1 + rng.next());
        res[5] = 2 * (n / 32);
        res[6] = n - n / 7;
        res[7] = 0;
        for (int k = 0; k < kGsParts; k++) gs[k] = n * 1e3 * rng.next();
        check_finish(n ? "finish" : "finish, no point", res, gs, (int)res[6]);
    }
    std::printf("ok: %lld checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
