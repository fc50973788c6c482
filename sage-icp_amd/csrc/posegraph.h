// Pose-graph optimisation of a trajectory: a chain of odometry edges plus a few loop closures (include/sageicp.h "pose
// graph").  This header holds the per-edge arithmetic and the 6x6 block algebra that the host path
// (capi_posegraph.hip) and the kernels (posegraph.hip) share, SAGE_HD, compilable by plain g++ as se3_math.h is, and
// below them the launchers of posegraph.hip (hipcc only).
//
//   residual   r_e(x) = se3_log(Z_e^-1 * (x_a^-1 x_b)),  tangent (upsilon, omega), se3_math.h's
//   cost       F(x) = sum_e r_e^T Omega_e r_e = sum_e |L_e^T r_e|^2,  Omega_e = L_e L_e^T (unpivoted Cholesky)
//   update     x_k <- x_k * se3_exp(delta_k)                         (right perturbation)
//   Jacobians  dr/d delta_b = Jr^-1(r),  dr/d delta_a = -Jr^-1(r) Ad((x_a^-1 x_b)^-1)      (exact)
//
// x_a^-1 x_b is formed as (conj(q_a) q_b, R_a^T (t_b - t_a)): the difference of the translations first, so the relative
// transform of two poses at UTM coordinates carries the rounding of their distance, not of their coordinates.  Everything
// an edge contributes is a function of relative transforms only.
//
// Jr^-1 of SE(3).  With ad = ad(r) = [[W, V], [0, W]] (W = hat(omega), V = hat(upsilon)), Jl^-1 = ad / (exp(ad) - 1)
// = -ad/2 + g(ad), g(x) = (x/2) coth(x/2) even; Jr^-1(r) = Jl^-1(-r) = I + ad/2 + g(ad).  ad satisfies
// ad (ad^2 + th^2)^2 = 0 (th = |omega|), so g(ad) = I + a2 ad^2 + a4 ad^4 with the Hermite conditions at x = i th:
//     gamma = (th/2) cot(th/2),   eta = (th / (4 sin^2(th/2)) - cot(th/2)/2) / (2 th)
//     a4 = (1 - gamma - eta th^2) / th^4,   a2 = (2 (1 - gamma) - eta th^2) / th^2
// In 3x3 blocks Jr^-1 = [[A, B], [0, A]]:  A = I + W/2 + (a2 - a4 th^2) W^2  (a2 - a4 th^2 = (1 - gamma)/th^2, SO(3)'s),
//     B = V/2 + a2 S + a4 (W^2 S + S W^2),  S = W V + V W.
// The numerator of a4 cancels to O(th^4) from terms of O(1), so the closed form loses th^-4 ulps; below kPgSeriesAngle
// the Bernoulli series is used instead (a2 = 1/12 - th^4/30240 - ..., a4 = -1/720 - th^2/15120 - ...: four terms, whose
// truncation at 0.25 rad is below 1e-14 of a4).  se3_log's own threshold (1e-10) would leave the closed form 1e-8 wrong
// at 1e-8 rad: the Jacobian test of tests/posegraph_check.cpp decides this.
//
// 6x6 blocks are double[6][6] indexed by compile-time constants only (every loop is unrolled; see se3_math.h for why a
// dynamically indexed block ends up in scratch memory on the device).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include <vector>

#include "se3_math.h"

namespace sageicp {

constexpr uint32_t kPgMaxClosures = 256;
constexpr double kPgSeriesAngle = 0.25;
constexpr int kPgRefineRounds = 2;           // rounds of delta += H^-1 (-g - H delta) after the Woodbury solve (capi_posegraph.hip)

// ---- 6x6 blocks ------------------------------------------------------------------------------------------------------------
SAGE_HD inline void pg_zero(double (&M)[6][6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) M[i][j] = 0.0;
}
// O (+)= s * A^T B   /   A B   /   A B^T
SAGE_HD inline void pg_add_atb(const double (&A)[6][6], const double (&B)[6][6], double s, double (&O)[6][6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) v += A[k][i] * B[k][j];
            O[i][j] += s * v;
        }
}
SAGE_HD inline void pg_add_ab(const double (&A)[6][6], const double (&B)[6][6], double s, double (&O)[6][6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) v += A[i][k] * B[k][j];
            O[i][j] += s * v;
        }
}
SAGE_HD inline void pg_add_abt(const double (&A)[6][6], const double (&B)[6][6], double s, double (&O)[6][6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) v += A[i][k] * B[j][k];
            O[i][j] += s * v;
        }
}
// o (+)= s * A v   /   A^T v
SAGE_HD inline void pg_add_av(const double (&A)[6][6], const double (&v)[6], double s, double (&o)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) t += A[i][k] * v[k];
        o[i] += s * t;
    }
}
SAGE_HD inline void pg_add_atv(const double (&A)[6][6], const double (&v)[6], double s, double (&o)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) t += A[k][i] * v[k];
        o[i] += s * t;
    }
}

// Unpivoted Cholesky M = L L^T of a symmetric 6x6 (the lower triangle is read); false if a pivot is not positive (or NaN).
SAGE_HD inline bool pg_chol6(const double (&M)[6][6], double (&L)[6][6]) {
    bool ok = true;
    pg_zero(L);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = M[j][j];
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k < j) d -= L[j][k] * L[j][k];
        ok = ok && d > 0.0 && d <= 1.7976931348623157e308;
        const double s = sqrt(d);
        L[j][j] = s;
#pragma unroll
        for (int i = 0; i < 6; ++i)
            if (i > j) {
                double v = M[i][j];
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (k < j) v -= L[i][k] * L[j][k];
                L[i][j] = v / s;
            }
    }
    return ok;
}

// The inverse of a symmetric positive definite 6x6: M = L L^T, N = L^-1, M^-1 = N^T N (symmetric to the bit: the two
// triangles are the same sums).  false as pg_chol6.
SAGE_HD inline bool pg_spd_inv6(const double (&M)[6][6], double (&Inv)[6][6]) {
    double L[6][6], N[6][6];
    const bool ok = pg_chol6(M, L);
    pg_zero(N);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        N[j][j] = 1.0 / L[j][j];
#pragma unroll
        for (int i = 0; i < 6; ++i)
            if (i > j) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (k >= j && k < i) v -= L[i][k] * N[k][j];
                N[i][j] = v / L[i][i];
            }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j)
            if (j <= i) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (k >= i) v += N[k][i] * N[k][j];
                Inv[i][j] = v;
                Inv[j][i] = v;
            }
    return ok;
}

// ---- SE(3) pieces ----------------------------------------------------------------------------------------------------------
// O = A^-1 B, the translations subtracted first
SAGE_HD inline void pg_between(const double A[7], const double B[7], double O[7]) {
    const double ax = -A[0], ay = -A[1], az = -A[2], aw = A[3];
    const double bx = B[0], by = B[1], bz = B[2], bw = B[3];
    double x = aw * bx + ax * bw + ay * bz - az * by;
    double y = aw * by - ax * bz + ay * bw + az * bx;
    double z = aw * bz + ax * by - ay * bx + az * bw;
    double w = aw * bw - ax * bx - ay * by - az * bz;
    const double inv = 1.0 / sqrt(x * x + y * y + z * z + w * w);
    const double qi[4] = {ax, ay, az, aw};
    double R[9], t[3];
    quat_to_mat(qi, R);
    const double d[3] = {B[4] - A[4], B[5] - A[5], B[6] - A[6]}, zero[3] = {0.0, 0.0, 0.0};
    mat_apply(R, zero, d, t);
    O[0] = x * inv; O[1] = y * inv; O[2] = z * inv; O[3] = w * inv;
    O[4] = t[0]; O[5] = t[1]; O[6] = t[2];
}

SAGE_HD inline void pg_hat(const double w[3], double (&H)[3][3]) {
    H[0][0] = 0.0;   H[0][1] = -w[2]; H[0][2] = w[1];
    H[1][0] = w[2];  H[1][1] = 0.0;   H[1][2] = -w[0];
    H[2][0] = -w[1]; H[2][1] = w[0];  H[2][2] = 0.0;
}
SAGE_HD inline void pg_mul3(const double (&A)[3][3], const double (&B)[3][3], double (&O)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) O[i][j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j];
}

// the coefficients of g(ad) = I + a2 ad^2 + a4 ad^4 (header above)
SAGE_HD inline void pg_jr_inv_coeffs(double th2, double &a2, double &a4) {
    const double th = sqrt(th2);
    if (th < kPgSeriesAngle) {
        const double t4 = th2 * th2;
        a2 = 1.0 / 12.0 - t4 * (1.0 / 30240.0 + th2 * (1.0 / 604800.0 + th2 * (1.0 / 15966720.0)));
        a4 = -1.0 / 720.0 - th2 * (1.0 / 15120.0 + th2 * (1.0 / 403200.0 + th2 * (1.0 / 11975040.0)));
    } else {
        const double half = 0.5 * th, sh = sin(half), ch = cos(half);
        const double cot = ch / sh;
        const double gamma = half * cot;
        const double eta = (th / (4.0 * sh * sh) - 0.5 * cot) / (2.0 * th);
        a4 = ((1.0 - gamma) - eta * th2) / (th2 * th2);
        a2 = (2.0 * (1.0 - gamma) - eta * th2) / th2;
    }
}

// Jr^-1(r) as its two 3x3 blocks: [[A, B], [0, A]]
SAGE_HD inline void pg_jr_inv_blocks(const double r[6], double (&A)[3][3], double (&B)[3][3]) {
    const double u[3] = {r[0], r[1], r[2]}, w[3] = {r[3], r[4], r[5]};
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    double a2, a4;
    pg_jr_inv_coeffs(th2, a2, a4);
    double W[3][3], V[3][3], W2[3][3], WV[3][3], VW[3][3], S[3][3], W2S[3][3], SW2[3][3];
    pg_hat(w, W);
    pg_hat(u, V);
    pg_mul3(W, W, W2);
    pg_mul3(W, V, WV);
    pg_mul3(V, W, VW);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S[i][j] = WV[i][j] + VW[i][j];
    pg_mul3(W2, S, W2S);
    pg_mul3(S, W2, SW2);
    const double cA = a2 - a4 * th2;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            A[i][j] = ((i == j) ? 1.0 : 0.0) + 0.5 * W[i][j] + cA * W2[i][j];
            B[i][j] = 0.5 * V[i][j] + a2 * S[i][j] + a4 * (W2S[i][j] + SW2[i][j]);
        }
}

// Jr^-1(r), full (the check program's)
SAGE_HD inline void pg_jr_inv(const double r[6], double (&J)[6][6]) {
    double A[3][3], B[3][3];
    pg_jr_inv_blocks(r, A, B);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            J[i][j] = A[i][j];
            J[i][j + 3] = B[i][j];
            J[i + 3][j] = 0.0;
            J[i + 3][j + 3] = A[i][j];
        }
}

// ---- an edge ---------------------------------------------------------------------------------------------------------------
// r = se3_log(Zinv * (x_a^-1 x_b)); D = x_a^-1 x_b
SAGE_HD inline void pg_residual(const double Zinv[7], const double xa[7], const double xb[7], double r[6], double D[7]) {
    double E[7];
    pg_between(xa, xb, D);
    se3_mul(Zinv, D, E);
    se3_log(E, r);
}

// w = L^T r (L: row-major lower 6x6, 36 doubles)
SAGE_HD inline void pg_whiten(const double *L, const double r[6], double (&w)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k >= i) v += L[k * 6 + i] * r[k];
        w[i] = v;
    }
}
SAGE_HD inline double pg_dot6(const double (&a)[6], const double (&b)[6]) {
    return ((a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3])) + (a[4] * b[4] + a[5] * b[5]);
}

// the edge's term of F
SAGE_HD inline double pg_edge_cost(const double Zinv[7], const double xa[7], const double xb[7], const double *L) {
    double r[6], D[7], w[6];
    pg_residual(Zinv, xa, xb, r, D);
    pg_whiten(L, r, w);
    return pg_dot6(w, w);
}

// ---- robust kernels on closure edges -----------------------------------------------------------------------
// s = r^T Omega r of a closure, c2 = scale^2.  rho(s) replaces s in F; rho'(s) is the edge's IRLS weight: A, B, w scaled
// by sqrt(rho') make g the exact gradient of F and H = sum rho' J^T J positive definite (no second-order term).
// 0 none, 1 Huber, 2 Cauchy, 3 Geman-McClure (sageicp.h's SAGEICP_GRAPH_KERNEL_*).
SAGE_HD inline double pg_rho(uint32_t kernel, double c2, double s) {
    if (kernel == 1u) return s <= c2 ? s : 2.0 * sqrt(c2 * s) - c2;
    if (kernel == 2u) return c2 * log1p(s / c2);
    if (kernel == 3u) return c2 * s / (c2 + s);
    return s;
}
SAGE_HD inline double pg_rho_weight(uint32_t kernel, double c2, double s) {
    if (kernel == 1u) return s <= c2 ? 1.0 : sqrt(c2 / s);
    if (kernel == 2u) return 1.0 / (1.0 + s / c2);
    if (kernel == 3u) {
        const double t = c2 / (c2 + s);
        return t * t;
    }
    return 1.0;
}

// The whitened linearisation of an edge: A = L^T dr/d delta_a, B = L^T dr/d delta_b, w = L^T r.  Its terms of
// H = sum J^T Omega J and g = sum J^T Omega r are then A^T A, A^T B, B^T B and A^T w, B^T w.
struct PgEdgeLin {
    double A[6][6], B[6][6], w[6];
};
SAGE_HD inline void pg_linearize(const double Zinv[7], const double xa[7], const double xb[7], const double *L, PgEdgeLin &o) {
    double r[6], D[7], Di[7];
    pg_residual(Zinv, xa, xb, r, D);
    pg_whiten(L, r, o.w);
    double JA[3][3], JB[3][3];
    pg_jr_inv_blocks(r, JA, JB);
    // Ad(D^-1) = [[R, T R], [0, R]], R and t of D^-1, T = hat(t)
    se3_inv(D, Di);
    double Rf[9], R[3][3], T[3][3], TR[3][3], AR[3][3], ATR[3][3], BR[3][3];
    quat_to_mat(Di, Rf);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = Rf[3 * i + j];
    const double t[3] = {Di[4], Di[5], Di[6]};
    pg_hat(t, T);
    pg_mul3(T, R, TR);
    pg_mul3(JA, R, AR);
    pg_mul3(JA, TR, ATR);
    pg_mul3(JB, R, BR);
    double Ja[6][6], Jb[6][6];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Jb[i][j] = JA[i][j];       Jb[i][j + 3] = JB[i][j];
            Jb[i + 3][j] = 0.0;        Jb[i + 3][j + 3] = JA[i][j];
            Ja[i][j] = -AR[i][j];      Ja[i][j + 3] = -(ATR[i][j] + BR[i][j]);
            Ja[i + 3][j] = 0.0;        Ja[i + 3][j + 3] = -AR[i][j];
        }
    // L^T J: row i sums k >= i; the lower-left block of J is zero
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double va = 0.0, vb = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (k >= i && !(k >= 3 && j < 3)) {
                    va += L[k * 6 + i] * Ja[k][j];
                    vb += L[k * 6 + i] * Jb[k][j];
                }
            o.A[i][j] = va;
            o.B[i][j] = vb;
        }
}

// a closure's linearisation under the kernel: scaled by sqrt(rho'(s)), s = |w|^2 before; returns rho(s)
SAGE_HD inline double pg_robustify(uint32_t kernel, double c2, PgEdgeLin &o) {
    const double s = pg_dot6(o.w, o.w);
    const double sw = sqrt(pg_rho_weight(kernel, c2, s));
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            o.A[i][j] *= sw;
            o.B[i][j] *= sw;
        }
        o.w[i] *= sw;
    }
    return pg_rho(kernel, c2, s);
}

// t = A d_a + B d_b + w: the edge's linear model of its whitened residual under the steps of its two poses
SAGE_HD inline void pg_edge_model(const PgEdgeLin &l, const double (&da)[6], const double (&db)[6], double (&t)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) t[i] = l.w[i];
    pg_add_av(l.A, da, 1.0, t);
    pg_add_av(l.B, db, 1.0, t);
}

// x <- x * se3_exp(s * d), the quaternion renormalised (se3_mul)
SAGE_HD inline void pg_retract(const double x[7], const double d[6], double s, double o[7]) {
    double sd[6], E[7];
#pragma unroll
    for (int i = 0; i < 6; ++i) sd[i] = s * d[i];
    se3_exp(sd, E);
    se3_mul(x, E, o);
}

// the free index of vertex k with `anchor` eliminated (the anchor has none)
SAGE_HD inline uint32_t pg_free_of(uint32_t k, uint32_t anchor) { return k < anchor ? k : k - 1u; }
SAGE_HD inline uint32_t pg_vertex_of(uint32_t f, uint32_t anchor) { return f < anchor ? f : f + 1u; }

// ---- the host path's two solves (plain C++; capi_posegraph.hip drives them, tests/posegraph_check.cpp holds them to a dense
// solve) -------------------------------------------------------------------------------------------------------------------
struct PgBlk { double v[6][6]; };

// A block tridiagonal SPD matrix of m 6x6 block rows: D the diagonal, Eb[f] the block (f, f + 1) (Eb[m - 1] unused).
// Sequential block Thomas: S_0 = D_0, S_f = D_f - E_{f-1}^T S_{f-1}^-1 E_{f-1}; Lf_f = E_{f-1}^T S_{f-1}^-1.
struct PgHostChain {
    std::vector<PgBlk> D, Eb, Sinv, Lf;
    void resize(size_t m) { D.resize(m); Eb.resize(m); Sinv.resize(m); Lf.resize(m); }
    bool factor() {
        bool ok = true;
        for (size_t f = 0; f < D.size(); ++f) {
            PgBlk S = D[f];
            pg_zero(Lf[f].v);
            if (f) {
                pg_add_atb(Eb[f - 1].v, Sinv[f - 1].v, 1.0, Lf[f].v);
                pg_add_ab(Lf[f].v, Eb[f - 1].v, -1.0, S.v);
            }
            ok = pg_spd_inv6(S.v, Sinv[f].v) && ok;
        }
        return ok;
    }
    // X (6m x K, row-major) <- T^-1 X
    void solve(double *X, size_t K) const {
        const size_t m = D.size();
        std::vector<double> tmp(6 * K);
        for (size_t f = 1; f < m; ++f) {
            double *cur = X + 6 * f * K;
            const double *prev = cur - 6 * K;
            for (int i = 0; i < 6; ++i)
                for (int k = 0; k < 6; ++k) {
                    const double l = Lf[f].v[i][k];
                    for (size_t col = 0; col < K; ++col) cur[i * K + col] -= l * prev[k * K + col];
                }
        }
        for (size_t f = m; f-- > 0;) {
            double *cur = X + 6 * f * K;
            if (f + 1 < m) {
                const double *next = cur + 6 * K;
                for (int i = 0; i < 6; ++i)
                    for (int k = 0; k < 6; ++k) {
                        const double ev = Eb[f].v[i][k];
                        for (size_t col = 0; col < K; ++col) cur[i * K + col] -= ev * next[k * K + col];
                    }
            }
            std::fill(tmp.begin(), tmp.end(), 0.0);
            for (int i = 0; i < 6; ++i)
                for (int k = 0; k < 6; ++k) {
                    const double sv = Sinv[f].v[i][k];
                    for (size_t col = 0; col < K; ++col) tmp[i * K + col] += sv * cur[k * K + col];
                }
            std::copy(tmp.begin(), tmp.end(), cur);
        }
    }
};

// z = C^-1 b for the factor pg_solve_capacitance left in C; b[i * stride]
inline void pg_resolve_capacitance(const std::vector<double> &C, uint32_t r, const double *b, size_t stride, double *z) {
    for (uint32_t i = 0; i < r; ++i) {
        const double *ci = C.data() + static_cast<size_t>(i) * r;
        double v = b[i * stride];
        for (uint32_t k = 0; k < i; ++k) v -= ci[k] * z[k];
        z[i] = v / ci[i];
    }
    for (uint32_t i = r; i-- > 0;) {
        double v = z[i];
        for (uint32_t k = i + 1; k < r; ++k) v -= C[static_cast<size_t>(k) * r + i] * z[k];
        z[i] = v / C[static_cast<size_t>(i) * r + i];
    }
}

// z = (I + Gm[:, 1:])^-1 Gm[:, 0]: dense Cholesky of the capacitance matrix (its lower triangle), r = 6c, ld = 1 + r
inline bool pg_solve_capacitance(const double *Gm, uint32_t r, std::vector<double> &C, double *z) {
    const size_t ld = 1 + static_cast<size_t>(r);
    C.assign(static_cast<size_t>(r) * r, 0.0);
    for (uint32_t i = 0; i < r; ++i)
        for (uint32_t j = 0; j <= i; ++j) C[static_cast<size_t>(i) * r + j] = Gm[i * ld + 1 + j] + (i == j ? 1.0 : 0.0);
    for (uint32_t j = 0; j < r; ++j) {
        double *cj = C.data() + static_cast<size_t>(j) * r;
        double d = cj[j];
        for (uint32_t k = 0; k < j; ++k) d -= cj[k] * cj[k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double s = std::sqrt(d);
        cj[j] = s;
        for (uint32_t i = j + 1; i < r; ++i) {
            double *ci = C.data() + static_cast<size_t>(i) * r;
            double v = ci[j];
            for (uint32_t k = 0; k < j; ++k) v -= ci[k] * cj[k];
            ci[j] = v / s;
        }
    }
    pg_resolve_capacitance(C, r, Gm, ld, z);
    return true;
}

// ---- the device side (posegraph.hip) -----------------------------------------------------------------------------------------
// Layouts.  E = n - 1 + c edges: odometry edge k = (k, k + 1) first, then the closures in the caller's order.  m = n - 1
// free vertices.  Everything per edge or per vertex is field-major (field * count + index), so that neighbouring lanes
// read neighbouring doubles.
//   lin    78 fields per edge: A (36, row-major), B (36), w (6)
//   T      block cyclic reduction: level l has m_l nodes at node offset o_l (m_0 = m, m_{l+1} = m_l / 2,
//          until 0), `nodes` in all (< 2 m).  Per node 36 doubles in each of D (diagonal), E (coupling to the next node,
//          zero at the last), DP (the inverse of D at even nodes, P = E_p^T D_p^-1 at odd ones), Q (E_i D_q^-1 at odd).
//   X      right-hand sides: ((o_l + node) * 6 + row) * K + col, K columns of a chunk.
constexpr int kPgLinFields = 78;
constexpr int kPgMaxLevels = 34;
constexpr unsigned kPgBlocks = 1024;         // every launch: work beyond 1024 x 256 items is reached by striding
constexpr size_t kPgChunkBytes = size_t(512) << 20;   // what X may take: the columns of a chunk follow from it

struct PgLevels {
    uint32_t count;
    uint32_t m[kPgMaxLevels], off[kPgMaxLevels];
    uint32_t nodes;
};
inline PgLevels pg_levels(uint32_t m) {
    PgLevels L{};
    uint32_t off = 0;
    while (m > 0 && L.count < kPgMaxLevels) {
        L.m[L.count] = m;
        L.off[L.count] = off;
        off += m;
        m /= 2;
        ++L.count;
    }
    L.nodes = off;
    return L;
}

#if defined(__HIPCC__)
struct PgGraph {
    uint32_t n, c, anchor, m, E;     // poses, closures, the anchor, free vertices, edges
    const double *zinv;              // E x 7: Z_e^-1
    const double *L;                 // Cholesky factors: odometry (1 or n - 1, by l_stride) then the closures
    uint32_t l_stride;               // 0 or 36
    const uint32_t *ca, *cb;         // c: the closures' vertices
    uint32_t kernel;                 // the closures' robust kernel (pg_rho); 0: the plain kernels are launched
    double c2;                       // its scale^2 at the current stage
};
struct PgSystem {
    double *lin;                     // 78 x E
    double *g;                       // 6 x m   (sum J^T Omega r: half of F's gradient)
    double *D, *E, *DP, *Q;          // 36 x nodes each
    uint32_t nodes;
    uint32_t *bad;                   // set to 1 by the factor when a diagonal block is not positive definite
};
hipError_t pg_linearize_all(const PgGraph &G, const double *x, const PgSystem &S, double *edge_cost, hipStream_t s);
hipError_t pg_assemble(const PgGraph &G, const PgSystem &S, hipStream_t s);
hipError_t pg_factor(const PgSystem &S, const PgLevels &lv, hipStream_t s);
// X level 0 <- columns [col0, col0 + K) of [-g | U]
hipError_t pg_rhs_columns(const PgGraph &G, const PgSystem &S, uint32_t col0, uint32_t K, double *X, hipStream_t s);
// X level 0 <- -g - U z
hipError_t pg_rhs_final(const PgGraph &G, const PgSystem &S, const double *z, double *X, hipStream_t s);
hipError_t pg_apply(const PgSystem &S, const PgLevels &lv, uint32_t K, double *X, hipStream_t s);
// Gm[(6 e + s) * ld + col0 + col] = (U^T X)[6 e + s][col], ld = 1 + 6 c
hipError_t pg_capacitance(const PgGraph &G, const PgSystem &S, const double *X, uint32_t col0, uint32_t K, double *Gm, hipStream_t s);
// q = g + H delta (field-major, as g), summed from the edges' blocks; X level 0 (K = 1) <- -q
hipError_t pg_residual(const PgGraph &G, const PgSystem &S, const double *delta, double *q, double *X, hipStream_t s);
// delta += X level 0 (K = 1)
hipError_t pg_accumulate(const PgGraph &G, const double *X, double *delta, hipStream_t s);
// out = x * exp(step * delta), the anchor's bytes copied; delta: 6 per free vertex, as X level 0 with K = 1
hipError_t pg_update(const PgGraph &G, const double *x, const double *delta, double step, double *out, hipStream_t s);
hipError_t pg_cost(const PgGraph &G, const double *x, double *edge_cost, hipStream_t s);
// *out = the sum (max of |.| if absmax) of v[0 .. count) by a fixed tree: slabs (kPgBlocks doubles), then one workgroup
hipError_t pg_reduce(const double *v, uint64_t count, bool absmax, double *slabs, double *out, hipStream_t s);
#endif

}  // namespace sageicp
