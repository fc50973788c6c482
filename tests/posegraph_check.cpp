// Stand-alone check of csrc/posegraph.h, built by tests/test_posegraph_host.py with plain g++ and again with
// -fsanitize=address,undefined (no GPU, no library):
//
//  1. Jr^-1(r) and the two Jacobians of an edge (pg_linearize with L = I) against central differences of the residual
//     itself, at rotation angles of the residual from 1e-9 rad to 3.1 rad, on both sides of kPgSeriesAngle.
//     Step h = 1e-5: the difference quotient's own error is h^2/6 |r'''| + 2^-53 |r| / h ~ 2e-11 (1 + |r|) for moderate
//     residuals; near pi the logarithm's derivatives grow like 1 / (pi - th), so the bound is scaled by that:
//         tol = 1e-8 * (1 + |r|) / min(1, pi - th)
//     The approximation Jr^-1 = I is off by about |r| / 2: it fails this check by seven orders of magnitude at 0.5 rad
//     (printed as "identity would be off by").
//  2. PgHostChain (block Thomas) plus pg_solve_capacitance (Woodbury) against a dense Gaussian elimination with partial
//     pivoting of T + U U^T, for chains of 1, 2, 3 and 40 block rows and ranks 0, 6 and 18.  The blocks are those of a
//     weighted chain (diagonal dominance 3), cond ~ 1e3: the two solutions agree to 1e-10 relative.
//  3. pg_spd_inv6 against the identity, and the bitwise symmetry of its result.
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

static const double kPi = 3.14159265358979323846;

static void unit_L(double *L) {
    for (int i = 0; i < 36; ++i) L[i] = 0.0;
    for (int i = 0; i < 6; ++i) L[i * 6 + i] = 1.0;
}

// the residual of an edge with x_a, x_b perturbed on the right by da, db
static void residual(const double *Zinv, const double *xa, const double *xb, const double *da, const double *db, double r[6]) {
    double a2[7], b2[7], D[7];
    pg_retract(xa, da, 1.0, a2);
    pg_retract(xb, db, 1.0, b2);
    pg_residual(Zinv, a2, b2, r, D);
}

static void check_jacobians(double angle, double trans) {
    // x_a, x_b arbitrary; Z chosen so that the residual is exp-coordinates (trans * u, angle * w)
    double ta[6] = {3.0 * rnd(), 3.0 * rnd(), rnd(), 0.4 * rnd(), 0.4 * rnd(), 2.0 * rnd()};
    double tb[6] = {3.0 * rnd(), 3.0 * rnd(), rnd(), 0.4 * rnd(), 0.4 * rnd(), 2.0 * rnd()};
    double xa[7], xb[7], D[7], R[7], Rinv[7], Z[7], Zinv[7];
    se3_exp(ta, xa);
    se3_exp(tb, xb);
    double w[3] = {rnd(), rnd(), rnd()};
    const double wn = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double want[6] = {trans * rnd(), trans * rnd(), trans * rnd(), angle * w[0] / wn, angle * w[1] / wn, angle * w[2] / wn};
    se3_exp(want, R);
    // Zinv * D = R  ->  Z = D * R^-1
    pg_between(xa, xb, D);
    se3_inv(R, Rinv);
    se3_mul(D, Rinv, Z);
    se3_inv(Z, Zinv);
    double L[36];
    unit_L(L);
    PgEdgeLin lin;
    pg_linearize(Zinv, xa, xb, L, lin);
    double rn = 0.0;
    for (int i = 0; i < 6; ++i) rn += lin.w[i] * lin.w[i];
    rn = std::sqrt(rn);
    const double th = std::sqrt(lin.w[3] * lin.w[3] + lin.w[4] * lin.w[4] + lin.w[5] * lin.w[5]);
    CHECK(std::fabs(th - angle) <= 1e-9 * (1.0 + angle), "the residual's angle %.17g, wanted %.17g", th, angle);
    const double tol = 1e-8 * (1.0 + rn) / std::fmin(1.0, kPi - th);
    const double h = 1e-5;
    double worst = 0.0, ident = 0.0;
    for (int side = 0; side < 2; ++side)
        for (int j = 0; j < 6; ++j) {
            double dp[6] = {0, 0, 0, 0, 0, 0}, dm[6] = {0, 0, 0, 0, 0, 0}, zero[6] = {0, 0, 0, 0, 0, 0}, rp[6], rm[6];
            dp[j] = h;
            dm[j] = -h;
            residual(Zinv, xa, xb, side ? zero : dp, side ? dp : zero, rp);
            residual(Zinv, xa, xb, side ? zero : dm, side ? dm : zero, rm);
            for (int i = 0; i < 6; ++i) {
                const double fd = (rp[i] - rm[i]) / (2.0 * h);
                const double got = side ? lin.B[i][j] : lin.A[i][j];
                worst = std::fmax(worst, std::fabs(fd - got));
                if (side) ident = std::fmax(ident, std::fabs(fd - (i == j ? 1.0 : 0.0)));
            }
        }
    std::printf("jacobians: angle %-8.3g |r| %-8.3g worst %.3g (tol %.3g); identity would be off by %.3g\n", angle, rn, worst, tol, ident);
    CHECK(worst <= tol, "a Jacobian differs from the central difference by %.3g > %.3g at angle %.3g", worst, tol, angle);
    // Jr^-1 on its own is the b side's Jacobian
    double J[6][6];
    pg_jr_inv(lin.w, J);
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) CHECK(J[i][j] == lin.B[i][j], "pg_jr_inv and pg_linearize differ at (%d, %d)", i, j);
}

static void check_series_joins_closed_form() {
    // the two branches of the coefficients on either side of the threshold
    double a2s, a4s, a2c, a4c;
    const double lo = kPgSeriesAngle * (1.0 - 1e-12), hi = kPgSeriesAngle * (1.0 + 1e-12);
    pg_jr_inv_coeffs(lo * lo, a2s, a4s);
    pg_jr_inv_coeffs(hi * hi, a2c, a4c);
    std::printf("coefficients at the threshold: a2 %.17g / %.17g, a4 %.17g / %.17g\n", a2s, a2c, a4s, a4c);
    CHECK(std::fabs(a2s - a2c) <= 1e-13, "a2 jumps by %.3g at the threshold", std::fabs(a2s - a2c));
    CHECK(std::fabs(a4s - a4c) <= 1e-12, "a4 jumps by %.3g at the threshold", std::fabs(a4s - a4c));
}

static void check_inverse() {
    double worst = 0.0;
    for (int t = 0; t < 50; ++t) {
        double B[6][6], M[6][6], I[6][6], P[6][6];
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) B[i][j] = rnd() + (i == j ? 2.0 : 0.0);
        pg_zero(M);
        pg_add_abt(B, B, 1.0, M);
        CHECK(pg_spd_inv6(M, I), "pg_spd_inv6 refused a positive definite block");
        pg_zero(P);
        pg_add_ab(M, I, 1.0, P);
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) {
                worst = std::fmax(worst, std::fabs(P[i][j] - (i == j ? 1.0 : 0.0)));
                CHECK(I[i][j] == I[j][i], "the inverse is not symmetric to the bit");
            }
    }
    std::printf("pg_spd_inv6: |M M^-1 - I| worst %.3g\n", worst);
    CHECK(worst <= 1e-11, "pg_spd_inv6 is off by %.3g", worst);
    double Z[6][6], I[6][6];
    pg_zero(Z);
    CHECK(!pg_spd_inv6(Z, I), "pg_spd_inv6 accepted the zero block");
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

static void check_solve(size_t m, size_t rank) {
    const size_t N = 6 * m;
    // T = sum over chain edges of [A B]^T [A B] + 3 I per block row: block tridiagonal, SPD
    PgHostChain T;
    T.resize(m);
    for (size_t f = 0; f < m; ++f) {
        pg_zero(T.D[f].v);
        pg_zero(T.Eb[f].v);
        for (int i = 0; i < 6; ++i) T.D[f].v[i][i] = 3.0;
    }
    for (size_t f = 0; f + 1 < m; ++f) {
        double A[6][6], B[6][6];
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) { A[i][j] = rnd(); B[i][j] = rnd(); }
        pg_add_atb(A, A, 1.0, T.D[f].v);
        pg_add_atb(B, B, 1.0, T.D[f + 1].v);
        pg_add_atb(A, B, 1.0, T.Eb[f].v);
    }
    std::vector<double> U(N * rank), g(N);
    for (auto &v : U) v = (rnd() > 0.6) ? rnd() : 0.0;
    for (auto &v : g) v = rnd();
    // dense H = T + U U^T
    std::vector<double> H(N * N, 0.0);
    for (size_t f = 0; f < m; ++f)
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) {
                H[(6 * f + i) * N + 6 * f + j] = T.D[f].v[i][j];
                if (f + 1 < m) {
                    H[(6 * f + i) * N + 6 * (f + 1) + j] = T.Eb[f].v[i][j];
                    H[(6 * (f + 1) + j) * N + 6 * f + i] = T.Eb[f].v[i][j];
                }
            }
    for (size_t i = 0; i < N; ++i)
        for (size_t j = 0; j < N; ++j)
            for (size_t k = 0; k < rank; ++k) H[i * N + j] += U[i * rank + k] * U[j * rank + k];
    std::vector<double> want;
    dense_solve(H, g, N, want);
    // Woodbury: Y = T^-1 [g | U], Gm = U^T Y, z = (I + Gm[:, 1:])^-1 Gm[:, 0], x = T^-1 (g - U z)
    CHECK(T.factor(), "the chain was refused");
    const size_t K = 1 + rank;
    std::vector<double> X(N * K), Gm(rank * K), z(rank), C;
    for (size_t i = 0; i < N; ++i) {
        X[i * K] = g[i];
        for (size_t k = 0; k < rank; ++k) X[i * K + 1 + k] = U[i * rank + k];
    }
    T.solve(X.data(), K);
    for (size_t r = 0; r < rank; ++r)
        for (size_t col = 0; col < K; ++col) {
            double s = 0.0;
            for (size_t i = 0; i < N; ++i) s += U[i * rank + r] * X[i * K + col];
            Gm[r * K + col] = s;
        }
    if (rank) CHECK(pg_solve_capacitance(Gm.data(), static_cast<uint32_t>(rank), C, z.data()), "the capacitance system was refused");
    std::vector<double> x(N);
    for (size_t i = 0; i < N; ++i) {
        double v = g[i];
        for (size_t k = 0; k < rank; ++k) v -= U[i * rank + k] * z[k];
        x[i] = v;
    }
    T.solve(x.data(), 1);
    double worst = 0.0, scale = 0.0;
    for (size_t i = 0; i < N; ++i) {
        worst = std::fmax(worst, std::fabs(x[i] - want[i]));
        scale = std::fmax(scale, std::fabs(want[i]));
    }
    std::printf("solve: m %-3zu rank %-3zu worst %.3g of %.3g\n", m, rank, worst, scale);
    CHECK(worst <= 1e-10 * scale, "the structured solve differs from the dense one by %.3g (scale %.3g), m %zu rank %zu", worst, scale, m, rank);
}

int main() {
    const double angles[] = {0.0, 1e-9, 1e-5, 1e-3, 0.1, 0.2499, 0.2501, 0.5, 1.5, 2.5, 3.0, 3.1};
    for (double a : angles) {
        check_jacobians(a, 0.3);
        check_jacobians(a, 5.0);
    }
    check_series_joins_closed_form();
    check_inverse();
    const size_t ms[] = {1, 2, 3, 40}, ranks[] = {0, 6, 18};
    for (size_t m : ms)
        for (size_t r : ranks) check_solve(m, r);
    std::printf(g_fail ? "posegraph_check: %d FAILED\n" : "posegraph_check: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
