// Stand-alone check of the robust kernels of csrc/posegraph.h, built by tests/test_posegraph_robust_host.py
// with plain g++ and again with -fsanitize=address,undefined (no GPU, no library):
//
//  1. pg_rho_weight against central differences of rho restated in long double, for Huber, Cauchy and Geman-McClure at
//     s = 0, c^2 (1 -+ 2^-40) and 1e12, and pg_rho against that restatement (8 ulps).  At s = 0 the difference is the
//     one-sided second-order one.  Steps and bounds: up to c^2, h = c^2 2^-30; a difference across Huber's joint errs by
//     h |jump of rho''| / 2 = h / (4 c^2) = 2.3e-10, rounding adds 2^-63 rho / h = 1e-10: tol 1e-9.  At 1e12, h = s 2^-8:
//     truncation (h / s)^2 = 1.5e-5 of rho', rounding 1e-6 of it for Geman-McClure (rho' = 2.8e-22): tol 1e-4 of rho'.
//     Huber's weight is exactly 1 at and below c^2, and below 1 above it.
//  2. One robust Gauss-Newton step of the host path's pieces (pg_linearize, pg_robustify, PgHostChain, the capacitance
//     solve) on a chain of 9 poses with two closures, one of them far off, against a dense elimination of
//     H = sum_odom J^T J + sum_closures rho' J^T J built from the UNSCALED linearisations, for every kernel: 1e-10 relative;
//     and g against central differences of the robust F itself (g is half its gradient): 1e-6 of its largest entry.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "posegraph.h"

using namespace sageicp;

static unsigned long long g_seed = 88172645463325252ull;
static double rnd() {            // xorshift, uniform in (-1, 1)
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return (double)(g_seed >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static long double rho_l(uint32_t kernel, long double c2, long double s) {
    if (kernel == 1u) return s <= c2 ? s : 2.0L * sqrtl(c2 * s) - c2;
    if (kernel == 2u) return c2 * log1pl(s / c2);
    if (kernel == 3u) return c2 * s / (c2 + s);
    return s;
}

static void check_weights() {
    const double c2 = 16.81;
    const double points[] = {0.0, c2 * (1.0 - 0x1p-40), c2 * (1.0 + 0x1p-40), 1e12};
    for (uint32_t kernel = 1; kernel <= 3; ++kernel)
        for (double s : points) {
            const bool far = s > 2.0 * c2;
            const long double h = far ? (long double)s * 0x1p-8L : (long double)c2 * 0x1p-30L;
            long double fd;
            if (s == 0.0) fd = (-3.0L * rho_l(kernel, c2, 0.0L) + 4.0L * rho_l(kernel, c2, h) - rho_l(kernel, c2, 2.0L * h)) / (2.0L * h);
            else fd = (rho_l(kernel, c2, s + h) - rho_l(kernel, c2, s - h)) / (2.0L * h);
            const double w = pg_rho_weight(kernel, c2, s);
            const double tol = far ? 1e-4 * w : 1e-9;
            std::printf("kernel %u s %-22.17g rho' %.17g, the difference %.17Lg (tol %.3g)\n", kernel, s, w, fd, tol);
            CHECK(std::isfinite(w) && w > 0.0 && w <= 1.0, "kernel %u: weight %.17g at s = %.17g", kernel, w, s);
            CHECK(std::fabs((double)(fd - (long double)w)) <= tol, "kernel %u: rho' %.17g against %.17Lg at s = %.17g", kernel, w, fd, s);
            const long double want = rho_l(kernel, c2, s);
            CHECK(std::fabs((double)((long double)pg_rho(kernel, c2, s) - want)) <= 8.0 * 0x1p-52 * (double)want, "kernel %u: rho at s = %.17g", kernel, s);
        }
    CHECK(pg_rho_weight(1u, c2, 0.0) == 1.0 && pg_rho_weight(1u, c2, c2) == 1.0 && pg_rho_weight(1u, c2, c2 * (1.0 - 0x1p-40)) == 1.0,
          "Huber's weight is not exactly 1 at or below c^2");
    CHECK(pg_rho_weight(1u, c2, c2 * (1.0 + 0x1p-40)) < 1.0 && pg_rho_weight(1u, c2, c2 * (1.0 + 0x1p-40)) >= 1.0 - 0x1p-40,
          "Huber's weight just above c^2");
    CHECK(pg_rho(0u, c2, 3.5) == 3.5 && pg_rho_weight(0u, c2, 3.5) == 1.0, "kernel 0 is the identity");
    CHECK(pg_rho_weight(2u, c2, 0.0) == 1.0 && pg_rho_weight(3u, c2, 0.0) == 1.0 && pg_rho(2u, c2, 0.0) == 0.0 && pg_rho(3u, c2, 0.0) == 0.0,
          "the kernels at s = 0");
}

static void dense_solve(std::vector<double> A, std::vector<double> b, size_t N, std::vector<double> &x) {
    for (size_t k = 0; k < N; ++k) {
        size_t p = k;
        for (size_t i = k + 1; i < N; ++i)
            if (std::fabs(A[i * N + k]) > std::fabs(A[p * N + k])) p = i;
        if (p != k) {
            for (size_t j = 0; j < N; ++j) std::swap(A[k * N + j], A[p * N + j]);
            std::swap(b[k], b[p]);
        }
        for (size_t i = k + 1; i < N; ++i) {
            const double f = A[i * N + k] / A[k * N + k];
            if (f == 0.0) continue;
            for (size_t j = k; j < N; ++j) A[i * N + j] -= f * A[k * N + j];
            b[i] -= f * b[k];
        }
    }
    x.assign(N, 0.0);
    for (size_t i = N; i-- > 0;) {
        double v = b[i];
        for (size_t j = i + 1; j < N; ++j) v -= A[i * N + j] * x[j];
        x[i] = v / A[i * N + i];
    }
}

struct Edge { uint32_t a, b; double zinv[7]; };

static double robust_cost(const std::vector<Edge> &E, size_t odo, const std::vector<double> &x, const double *L, uint32_t kernel, double c2) {
    double F = 0.0;
    for (size_t e = 0; e < E.size(); ++e) {
        const double s = pg_edge_cost(E[e].zinv, &x[7 * E[e].a], &x[7 * E[e].b], L);
        F += e >= odo ? pg_rho(kernel, c2, s) : s;
    }
    return F;
}

static void check_step(uint32_t kernel) {
    const uint32_t n = 9, m = n - 1, c = 2;                      // the anchor is pose 0: free index f = k - 1
    const double c2 = 16.81;
    g_seed = 88172645463325252ull + kernel;
    std::vector<double> x(7 * n);
    for (uint32_t k = 0; k < n; ++k) {
        const double t[6] = {1.0 * k + 0.1 * rnd(), 0.2 * rnd(), 0.1 * rnd(), 0.05 * rnd(), 0.05 * rnd(), 0.1 * k + 0.05 * rnd()};
        se3_exp(t, &x[7 * k]);
    }
    double L[36];
    for (int i = 0; i < 36; ++i) L[i] = 0.0;
    for (int i = 0; i < 6; ++i) L[i * 6 + i] = i < 3 ? 10.0 : 50.0;
    std::vector<Edge> E;
    auto add = [&](uint32_t a, uint32_t b, double noise_t, double noise_r) {
        Edge e{a, b, {}};
        double D[7], N[7], Z[7];
        const double t[6] = {noise_t * rnd(), noise_t * rnd(), noise_t * rnd(), noise_r * rnd(), noise_r * rnd(), noise_r * rnd()};
        pg_between(&x[7 * a], &x[7 * b], D);
        se3_exp(t, N);
        se3_mul(D, N, Z);
        se3_inv(Z, e.zinv);
        E.push_back(e);
    };
    for (uint32_t k = 0; k + 1 < n; ++k) add(k, k + 1, 0.02, 0.004);
    add(1, 7, 0.05, 0.01);                                       // inside c^2 or near it
    add(6, 2, 3.0, 0.2);                                         // far outside, reversed
    const size_t odo = n - 1;
    std::vector<PgEdgeLin> raw(E.size()), lin(E.size());
    std::vector<double> wt(E.size(), 1.0);
    for (size_t e = 0; e < E.size(); ++e) {
        pg_linearize(E[e].zinv, &x[7 * E[e].a], &x[7 * E[e].b], L, raw[e]);
        lin[e] = raw[e];
        if (e >= odo) {
            const double s = pg_dot6(raw[e].w, raw[e].w);
            wt[e] = pg_rho_weight(kernel, c2, s);
            const double r = pg_robustify(kernel, c2, lin[e]);
            CHECK(std::fabs(r - pg_rho(kernel, c2, s)) <= 1e-15 * (1.0 + r), "pg_robustify's rho");
            std::printf("kernel %u closure %zu: s %.6g weight %.6g\n", kernel, e - odo, s, wt[e]);
        }
    }
    // dense: H and g from the unscaled blocks and rho'
    const size_t N = 6 * m;
    std::vector<double> H(N * N, 0.0), g(N, 0.0);
    for (size_t e = 0; e < E.size(); ++e) {
        const double (*J[2])[6] = {raw[e].A, raw[e].B};
        const uint32_t v[2] = {E[e].a, E[e].b};
        for (int p = 0; p < 2; ++p) {
            if (v[p] == 0) continue;
            for (int i = 0; i < 6; ++i) {
                for (int k = 0; k < 6; ++k) g[6 * (v[p] - 1) + i] += wt[e] * J[p][k][i] * raw[e].w[k];
                for (int q = 0; q < 2; ++q) {
                    if (v[q] == 0) continue;
                    for (int j = 0; j < 6; ++j)
                        for (int k = 0; k < 6; ++k) H[(6 * (v[p] - 1) + i) * N + 6 * (v[q] - 1) + j] += wt[e] * J[p][k][i] * J[q][k][j];
                }
            }
        }
    }
    std::vector<double> mg(N), want;
    for (size_t i = 0; i < N; ++i) mg[i] = -g[i];
    dense_solve(H, mg, N, want);
    // g against central differences of the robust F: dF/d delta = 2 g
    double gscale = 0.0, gworst = 0.0;
    for (size_t i = 0; i < N; ++i) gscale = std::fmax(gscale, std::fabs(g[i]));
    for (size_t i = 0; i < N; ++i) {
        const double h = 1e-6;
        double d[6] = {0, 0, 0, 0, 0, 0};
        std::vector<double> xp = x, xm = x;
        d[i % 6] = h;
        pg_retract(&x[7 * (i / 6 + 1)], d, 1.0, &xp[7 * (i / 6 + 1)]);
        pg_retract(&x[7 * (i / 6 + 1)], d, -1.0, &xm[7 * (i / 6 + 1)]);
        const double fd = (robust_cost(E, odo, xp, L, kernel, c2) - robust_cost(E, odo, xm, L, kernel, c2)) / (2.0 * h);
        gworst = std::fmax(gworst, std::fabs(fd - 2.0 * g[i]));
    }
    std::printf("kernel %u: g against the differences of F, worst %.3g of %.3g\n", kernel, gworst, 2.0 * gscale);
    CHECK(gworst <= 1e-6 * 2.0 * gscale, "kernel %u: g is not half the gradient of the robust F (%.3g of %.3g)", kernel, gworst, gscale);
    // the host path's pieces on the scaled linearisations
    PgHostChain T;
    T.resize(m);
    std::vector<double> gs(N, 0.0);
    for (uint32_t f = 0; f < m; ++f) {
        const uint32_t k = f + 1;
        double gv[6] = {0, 0, 0, 0, 0, 0};
        pg_zero(T.D[f].v);
        pg_zero(T.Eb[f].v);
        pg_add_atb(lin[k - 1].B, lin[k - 1].B, 1.0, T.D[f].v);
        pg_add_atv(lin[k - 1].B, lin[k - 1].w, 1.0, gv);
        if (k + 1 < n) {
            pg_add_atb(lin[k].A, lin[k].A, 1.0, T.D[f].v);
            pg_add_atv(lin[k].A, lin[k].w, 1.0, gv);
            pg_add_atb(lin[k].A, lin[k].B, 1.0, T.Eb[f].v);
        }
        for (uint32_t ce = 0; ce < c; ++ce) {
            const PgEdgeLin &l = lin[odo + ce];
            if (E[odo + ce].a == k) pg_add_atv(l.A, l.w, 1.0, gv);
            if (E[odo + ce].b == k) pg_add_atv(l.B, l.w, 1.0, gv);
        }
        for (int i = 0; i < 6; ++i) gs[6 * f + i] = gv[i];
    }
    for (size_t i = 0; i < N; ++i) CHECK(std::fabs(gs[i] - g[i]) <= 1e-12 * (1.0 + gscale), "g from the scaled blocks at %zu", i);
    CHECK(T.factor(), "the chain was refused");
    const size_t rank = 6 * c, K = 1 + rank;
    std::vector<double> U(N * rank, 0.0);
    for (uint32_t ce = 0; ce < c; ++ce)
        for (int sc = 0; sc < 6; ++sc)
            for (int r = 0; r < 6; ++r) {
                if (E[odo + ce].a) U[(6 * (E[odo + ce].a - 1) + r) * rank + 6 * ce + sc] = lin[odo + ce].A[sc][r];
                if (E[odo + ce].b) U[(6 * (E[odo + ce].b - 1) + r) * rank + 6 * ce + sc] = lin[odo + ce].B[sc][r];
            }
    std::vector<double> X(N * K), Gm(rank * K), z(rank), C;
    for (size_t i = 0; i < N; ++i) {
        X[i * K] = -gs[i];
        for (size_t k = 0; k < rank; ++k) X[i * K + 1 + k] = U[i * rank + k];
    }
    T.solve(X.data(), K);
    for (size_t r = 0; r < rank; ++r)
        for (size_t col = 0; col < K; ++col) {
            double s = 0.0;
            for (size_t i = 0; i < N; ++i) s += U[i * rank + r] * X[i * K + col];
            Gm[r * K + col] = s;
        }
    CHECK(pg_solve_capacitance(Gm.data(), static_cast<uint32_t>(rank), C, z.data()), "the capacitance system was refused");
    std::vector<double> d(N);
    for (size_t i = 0; i < N; ++i) {
        double v = -gs[i];
        for (size_t k = 0; k < rank; ++k) v -= U[i * rank + k] * z[k];
        d[i] = v;
    }
    T.solve(d.data(), 1);
    double worst = 0.0, scale = 0.0;
    for (size_t i = 0; i < N; ++i) {
        worst = std::fmax(worst, std::fabs(d[i] - want[i]));
        scale = std::fmax(scale, std::fabs(want[i]));
    }
    std::printf("kernel %u: the robust step against the dense one, worst %.3g of %.3g\n", kernel, worst, scale);
    CHECK(worst <= 1e-10 * scale, "kernel %u: the robust step differs from the dense one by %.3g (scale %.3g)", kernel, worst, scale);
}

int main() {
    check_weights();
    for (uint32_t kernel = 0; kernel <= 3; ++kernel) check_step(kernel);
    std::printf(g_fail ? "posegraph_robust_check: %d FAILED\n" : "posegraph_robust_check: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
