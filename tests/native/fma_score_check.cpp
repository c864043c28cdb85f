// Check of the fast-path pair score (kg_common.h header): the node operands R and F come from the real
// kg_finalize_fit_r / kg_finalize_la_r on a one-node plane set, the pair value is fma(∓pr, R, F) with the
// kernels' two saturating converts (lr_q's int + max 0, cvt_u32_sat) and the MostAllocated min(q, 100), and
// the result must equal the int64 formula of the plugins on every node the finalize functions admit to the
// fast path (no slow bit).  Domains: step edges (req and req ± 1 around every quotient k of every cap class,
// caps up to KG_CAP_LIMIT − 1), bases up to KG_VAL_LIMIT − 1 (clamped scores), random fill, and negative
// bases with base + pr in [0, cap] (which the finalize functions must hand to the exact path).  F is also
// recomputed through kg_divmod64_fp (the device's quotient) and must have the same bits.
// Then the three weight-sum divisions against s / W for every W in 1..600 and every s in 0..100·W.
// Prints "checked N bad M slow S" (S: pairs left to the exact path); exit status 1 on any mismatch.
// Built and run by tests/test_score_edges_cpu.py.
#include "kg_common.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

static long n_checked = 0, n_bad = 0, n_slow = 0, n_neg = 0, n_neg_slow = 0;

static int sat_i32(double x) {   // v_cvt_i32_f64: truncates, saturates
    if (!(x > -2147483648.0)) return INT32_MIN;
    if (x >= 2147483647.0) return INT32_MAX;
    return (int)x;
}
static uint32_t sat_u32(double x) {   // v_cvt_u32_f64: truncates, negatives to 0, saturates
    if (!(x > 0.0)) return 0u;
    if (x >= 4294967295.0) return 0xFFFFFFFFu;
    return (uint32_t)x;
}

// the plugins' int64 formulas (Go division truncates; every operand here is non-negative where it divides)
static int64_t least_i(int64_t req, int64_t a) { return (a == 0 || req > a) ? 0 : (a - req) * 100 / a; }
static int64_t most_i(int64_t req, int64_t a) { return a == 0 ? 0 : (req > a ? a : req) * 100 / a; }

static double scaled_ratio_dev(int64_t num, int64_t den) {   // kg_scaled_ratio with the device's quotient
    int64_t q, r;
    kg_divmod64_fp(num * 100, den, q, r);
    return (double)q + ((double)r / (double)den + KG_EPS);
}

static void report(const char *what, int64_t a, int64_t base, int64_t pr, long got, long want) {
    if (n_bad < 12) printf("bad %s cap %ld base %ld pr %ld got %ld want %ld\n", what, (long)a, (long)base, (long)pr, got, want);
    n_bad++;
}

struct Planes {
    kg_node_row row;
    int64_t free_[KG_NUM_RES], metric_ns;
    double fit_R[KG_NUM_RES], fit_F[KG_NUM_RES], la_R[2], la_F[4];
    uint32_t dflags, fmask;
    kg_planes pl;
    Planes() {
        memset(&row, 0, sizeof row);
        pl = kg_planes{&row, free_, fit_R, fit_F, la_R, la_F, &metric_ns, &dflags, &fmask, 1};
    }
};
static Planes P;
static kg_consts C_least, C_most;

// one (cap, base, pr) through every fast-path form: Fit Least / Most on a native (r = 0: NonZeroRequested) and a
// scalar resource (r = 3: Requested), LoadAware on both usage variants.  neg: a negative-base case.
static void check(int64_t a, int64_t base, int64_t pr, bool neg) {
    const int64_t req = base + pr;
    for (int most = 0; most < 2; most++) {
        const kg_consts &c = most ? C_most : C_least;
        const int r = (n_checked & 1) ? 3 : 0;
        P.row.alloc[r] = a;
        P.row.alloc_present = 1u << 3;
        if (r < 2) P.row.nonzero_requested[r] = base;
        P.row.requested[r] = r < 2 ? 0 : base;
        double R, F;
        const uint32_t f = kg_finalize_fit_r(c, P.pl, 0, P.row, r, nullptr, &R, &F);
        n_checked++;
        n_neg += neg;
        if (!(f & 2u)) { report("fit not scored", a, base, pr, f, 2); continue; }
        if (f & 1u) {
            n_slow++;
            n_neg_slow += neg;
            if (!neg) report("fit slow inside the bounds", a, base, pr, f, 2);
            continue;
        }
        const double Fd = most ? scaled_ratio_dev(base, a) : scaled_ratio_dev(a - base, a);
        if (memcmp(&Fd, &F, sizeof F) != 0) report("fit F host/device quotient", a, base, pr, 0, 0);
        const double v = std::fma(most ? (double)pr : -(double)pr, R, F);
        int q1 = sat_i32(v);
        q1 = q1 > 0 ? q1 : 0;
        uint32_t q2 = sat_u32(v);
        if (most) {
            q1 = q1 < 100 ? q1 : 100;
            q2 = q2 < 100u ? q2 : 100u;
        }
        const int64_t want = most ? most_i(req, a) : least_i(req, a);
        if (q1 != want) report(most ? "fit most (int)" : "fit least (int)", a, base, pr, q1, (long)want);
        if ((int64_t)q2 != want) report(most ? "fit most (u32)" : "fit least (u32)", a, base, pr, q2, (long)want);
    }
    {   // LoadAware: variant 0 carries the base, variant 1 a base one lower (another operand of the same step)
        const int r = (int)(n_checked & 1);
        const int64_t base1 = base > 0 ? base - 1 : base;
        P.row.la_alloc[r] = a;
        P.row.la_used[0][r] = base;
        P.row.la_used[1][r] = base1;
        double R, F0, F1;
        const uint32_t f = kg_finalize_la_r(C_least, P.pl, 0, P.row, r, &R, &F0, &F1);
        n_checked++;
        n_neg += neg;
        if (f) {
            n_slow++;
            n_neg_slow += neg;
            if (!neg || f != 3u) report("loadaware slow bits", a, base, pr, f, neg ? 3 : 0);
            return;
        }
        for (int v = 0; v < 2; v++) {
            const int64_t b = v ? base1 : base;
            const double F = v ? F1 : F0, Fd = scaled_ratio_dev(a - b, a);
            if (memcmp(&Fd, &F, sizeof F) != 0) report("loadaware F host/device quotient", a, b, pr, 0, 0);
            const double x = std::fma(-(double)pr, R, F);
            int q1 = sat_i32(x);
            q1 = q1 > 0 ? q1 : 0;
            const uint32_t q2 = sat_u32(x);
            const int64_t want = least_i(b + pr, a);
            if (q1 != want) report("loadaware (int)", a, b, pr, q1, (long)want);
            if ((int64_t)q2 != want) report("loadaware (u32)", a, b, pr, q2, (long)want);
        }
    }
}

static int64_t ceil_div(int64_t n, int64_t d) { return (n + d - 1) / d; }

int main(int argc, char **argv) {
    const long iters = argc > 1 ? atol(argv[1]) : 400000;
    std::mt19937_64 g(7);
    memset(&C_least, 0, sizeof C_least);
    for (int r = 0; r < KG_NUM_RES; r++) C_least.fit_w[r] = 1;
    C_most = C_least;
    C_most.fit_most = 1;
    const int64_t CAPL = KG_CAP_LIMIT, VALL = KG_VAL_LIMIT;
    const int64_t caps[] = {CAPL - 1, CAPL - 3, (1LL << 40) + 1, 1000000000039LL, 3 * (1LL << 39) - 1, 1, 2, 3, 7, 99,
                            100, 101, 12800, 1LL << 36, CAPL - 2, (1LL << 40) - 1, 2199023254720LL};
    auto rnd = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(g() % (uint64_t)(hi - lo + 1)); };   // [lo, hi]
    auto rnd_log = [&](int64_t hi) { int64_t m = 1LL << (1 + g() % 50); if (m > hi) m = hi; return rnd(0, m); };

    // 1. step edges: every cap class and random caps, every quotient k, both strategies' steps
    //    (LeastAllocated: the largest req with quotient k is a − ceil(k·a/100); MostAllocated: the smallest is
    //    ceil(k·a/100)), the pod request anywhere in [0, req] (base = req − pr ≥ 0), and req − 1, req, req + 1
    const int ncaps = (int)(sizeof caps / sizeof caps[0]);
    for (long it = 0; it < iters; it++) {
        const int64_t a = it % 3 == 0 ? caps[(it / 3) % ncaps]
                        : it % 3 == 1 ? CAPL - 1 - (int64_t)(g() % (1u << 20)) : 1 + rnd_log(CAPL - 2);
        const int64_t k = (it / 7) % 101;
        const int64_t edge = (it & 8) ? ceil_div(k * a, 100) : a - ceil_div(k * a, 100);
        for (int64_t d = -1; d <= 1; d++) {
            const int64_t req = edge + d;
            if (req < 0) continue;
            const int64_t pr = (it & 16) ? rnd(0, req) : (req < (1LL << 34) ? rnd(0, req) : rnd(0, 1LL << 34));
            check(a, req - pr, pr, false);
        }
    }
    // 2. bases and requests up to KG_VAL_LIMIT − 1 (base > cap: LeastAllocated clamps to 0, MostAllocated to 100)
    for (long it = 0; it < iters; it++) {
        const int64_t a = (it & 1) ? caps[(it / 2) % ncaps] : 1 + rnd_log(CAPL - 2);
        const int64_t base = (it & 2) ? VALL - 1 - rnd_log(VALL - 1) : rnd_log(VALL - 1);
        const int64_t pr = (it & 4) ? VALL - 1 - rnd_log(VALL - 1) : rnd_log(VALL - 1);
        check(a, base, pr, false);
    }
    // 3. random fill inside the cap
    for (long it = 0; it < iters; it++) {
        const int64_t a = 1 + rnd_log(CAPL - 2);
        const int64_t req = rnd(0, a + a / 8 + 1);
        const int64_t pr = rnd(0, req);
        check(a, req - pr, pr, false);
    }
    // 4. negative bases in (−KG_VAL_LIMIT, 0) with base + pr in [0, cap] (three recorded tuples first): the
    //    finalize functions must leave them to the exact path; a pair they admit is checked like any other
    check(6, -531169216302749LL, 531169216302750LL, true);
    check(13, -295819977655557LL, 295819977655560LL, true);
    check(2199023254720LL, -462544787795525LL, 463754250585621LL, true);
    for (long it = 0; it < iters; it++) {
        const int64_t a = (it & 1) ? caps[(it / 2) % ncaps] : 1 + rnd_log(CAPL - 2);
        const int64_t base = -1 - rnd_log(VALL - 2);
        const int64_t k = (it / 5) % 101;
        const int64_t edge = a - ceil_div(k * a, 100);
        int64_t req = (it & 2) ? edge + (int64_t)(g() % 3) - 1 : rnd(0, a);
        if (req < 0) req = 0;
        const int64_t pr = req - base;
        if (pr >= VALL) continue;
        check(a, base, pr, true);
    }
    printf("pairs: negative-base %ld of which left to the exact path %ld\n", n_neg, n_neg_slow);

    // 5. the weight-sum divisions: s = Σ w·q ≤ 100·W
    long n_w = 0;
    for (uint32_t W = 1; W <= 600; W++) {
        const uint32_t magic = (uint32_t)((0x80000000ULL + W - 1) / W);   // kg_pod_dev::fit_magic, kg_consts::la_magic
        const float rcp = 1.0f / (float)W;                                // kg_pod_hot_t::fit_rcp, kg_consts::la_rcp
        const bool pow2 = (W & (W - 1)) == 0;
        const uint32_t shift = (uint32_t)__builtin_ctz(W);
        for (uint32_t s = 0; s <= 100 * W; s++) {
            const uint32_t want = s / W;
            const uint32_t m = (uint32_t)(((uint64_t)(s << 1) * magic) >> 32);   // __umulhi(s << 1, magic)
            const uint32_t f = (uint32_t)fmaf((float)s, rcp, 0x1p-12f);          // div_w<false>
            n_w++;
            if (m != want || f != want || (pow2 && (s >> shift) != want)) {
                if (n_bad < 12) printf("bad weight division W %u s %u: umulhi %u fmaf %u want %u\n", W, s, m, f, want);
                n_bad++;
            }
        }
    }
    n_checked += n_w;
    printf("checked %ld bad %ld slow %ld\n", n_checked, n_bad, n_slow);
    return n_bad != 0;
}
