// The pose-graph optimiser on the host side of libsageicp_hip.so (posegraph.h): the checks, the
// Gauss-Newton driver with its backtracking, the host path (sequential block Thomas plus the low-rank closure: what runs
// without a device, and the yardstick of the device path), the device path's driver over posegraph.hip's launchers, and
// the C entries.  Host code only.
//
// Both paths solve H delta = -g, H = T + U U^T, by Woodbury: Y = T^-1 [-g | U] in chunks of columns, of which only
// Gm = U^T Y is kept; C = I + Gm[:, 1:] (6c x 6c, dense, Cholesky on the host); z = C^-1 Gm[:, 0];
// delta = T^-1 (-g - U z); then kPgRefineRounds rounds of delta += H^-1 (-g - H delta) by the same factors, the residual
// summed edge by edge.  Waits of the device path: one per outer iteration (Gm and, at the first, F), with closures one per
// refinement round (U^T T^-1 of the residual, for C^-1 on the host), one per backtracking trial (F and |delta|_inf), one
// at the end (the gradient and the poses).
#include "capi_internal.h"
#include "posegraph.h"

namespace sageicp_impl {
namespace {

struct Problem {
    uint32_t n = 0, c = 0, anchor = 0, m = 0, E = 0;
    uint32_t l_stride = 0;
    std::vector<double> zinv;        // E x 7
    std::vector<double> L;           // odometry (1 or n - 1), then the closures: 36 each, row-major lower
    std::vector<uint32_t> ca, cb;
    const double *l_of(uint32_t e) const {
        if (e < n - 1u) return L.data() + static_cast<size_t>(l_stride) * e;
        return L.data() + (l_stride ? size_t(36) * (n - 1u) : size_t(36)) + size_t(36) * (e - (n - 1u));
    }
    void ends(uint32_t e, uint32_t &a, uint32_t &b) const {
        if (e < n - 1u) { a = e; b = e + 1u; }
        else { a = ca[e - (n - 1u)]; b = cb[e - (n - 1u)]; }
    }
};

bool zero_quat(const double *T) { return T[0] == 0.0 && T[1] == 0.0 && T[2] == 0.0 && T[3] == 0.0; }

// symmetric to the bit, positive definite by an unpivoted Cholesky: L out
bool info_factor(const double *info, double *L_out) {
    if (!finite_n(info, 36)) return false;
    double M[6][6], L[6][6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            if (std::memcmp(&info[i * 6 + j], &info[j * 6 + i], sizeof(double)) != 0) return false;
            M[i][j] = info[i * 6 + j];
        }
    if (!pg_chol6(M, L)) return false;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) L_out[i * 6 + j] = L[i][j];
    return finite_n(L_out, 36);
}

int check_poses(const double *poses, uint64_t n, const char *what) {
    if (!finite_n(poses, 7 * n)) return fail(SAGEICP_ERR_INVALID, std::string("graph: ") + what + " is not finite");
    for (uint64_t k = 0; k < n; ++k)
        if (zero_quat(poses + 7 * k)) return fail(SAGEICP_ERR_INVALID, std::string("graph: a quaternion of norm 0 in ") + what);
    return SAGEICP_OK;
}

// every refusal that does not depend on where the problem is solved; nothing is written before it has passed
int make_problem(const double *poses, uint64_t n, const double *odom_info, uint32_t stride, const sageicp_graph_edge *cl, uint32_t c,
                 uint64_t anchor, Problem &P) {
    if (!poses || !odom_info || (c && !cl)) return fail(SAGEICP_ERR_INVALID, "graph: null argument");
    if (n < 2) return fail(SAGEICP_ERR_INVALID, "graph: needs n >= 2 poses");
    if (stride != 0 && stride != 36) return fail(SAGEICP_ERR_INVALID, "graph: odom_info_stride is 0 or 36");
    if (anchor >= n) return fail(SAGEICP_ERR_INVALID, "graph: anchor >= n");
    if (n > 0x80000000ull) return fail(SAGEICP_ERR_CAPACITY, "graph: more than 2^31 poses");
    if (c > kPgMaxClosures) return fail(SAGEICP_ERR_CAPACITY, "graph: more than 256 closures");
    if (int rc = check_poses(poses, n, "poses")) return rc;
    P.n = static_cast<uint32_t>(n);
    P.c = c;
    P.anchor = static_cast<uint32_t>(anchor);
    P.m = P.n - 1u;
    P.E = P.n - 1u + c;
    P.l_stride = stride;
    const size_t lo = stride ? n - 1 : 1;
    P.L.resize(36 * (lo + c));
    for (size_t k = 0; k < lo; ++k)
        if (!info_factor(odom_info + 36 * k, P.L.data() + 36 * k))
            return fail(SAGEICP_ERR_INVALID, "graph: odom_info is not finite, symmetric to the bit and positive definite");
    P.ca.resize(c);
    P.cb.resize(c);
    P.zinv.resize(7 * static_cast<size_t>(P.E));
    for (uint32_t e = 0; e < c; ++e) {
        const sageicp_graph_edge &g = cl[e];
        if (g.a == g.b || g.a >= n || g.b >= n) return fail(SAGEICP_ERR_INVALID, "graph: a closure needs a != b, both below n");
        if (!finite_n(g.z, 7) || zero_quat(g.z)) return fail(SAGEICP_ERR_INVALID, "graph: a closure's z is not finite, or its quaternion is 0");
        if (!info_factor(g.info, P.L.data() + 36 * (lo + e)))
            return fail(SAGEICP_ERR_INVALID, "graph: a closure's info is not finite, symmetric to the bit and positive definite");
        P.ca[e] = static_cast<uint32_t>(g.a);
        P.cb[e] = static_cast<uint32_t>(g.b);
        se3_inv(g.z, P.zinv.data() + 7 * static_cast<size_t>(P.n - 1u + e));
    }
    for (uint32_t k = 0; k + 1u < P.n; ++k) {
        double Z[7];
        pg_between(poses + 7 * static_cast<size_t>(k), poses + 7 * static_cast<size_t>(k + 1u), Z);
        se3_inv(Z, P.zinv.data() + 7 * static_cast<size_t>(k));
    }
    if (!finite_n(P.zinv.data(), P.zinv.size())) return fail(SAGEICP_ERR_INVALID, "graph: a relative pose is not finite");
    return SAGEICP_OK;
}

double cost_at(const Problem &P, const double *x, double *per_edge) {
    double F = 0.0;
    for (uint32_t e = 0; e < P.E; ++e) {
        uint32_t a, b;
        P.ends(e, a, b);
        const double v = pg_edge_cost(P.zinv.data() + 7 * static_cast<size_t>(e), x + 7 * static_cast<size_t>(a),
                                      x + 7 * static_cast<size_t>(b), P.l_of(e));
        if (per_edge) per_edge[e] = v;
        F += v;
    }
    return F;
}

// columns of X a chunk may hold: kPgChunkBytes, one column at the least, all of them at the most
uint32_t chunk_columns(size_t rows_of_x, uint32_t total) {
    const size_t per = rows_of_x * sizeof(double);
    const size_t k = std::max<size_t>(1, kPgChunkBytes / std::max<size_t>(per, 1));
    return static_cast<uint32_t>(std::min<size_t>(k, total));
}

// ---- the host path ---------------------------------------------------------------------------------------------------------
class HostSolver {
public:
    explicit HostSolver(const Problem &p) : P(p) {}
    int init(const double *initial) {
        x.assign(initial, initial + 7 * static_cast<size_t>(P.n));
        xt.resize(x.size());
        lin.resize(P.E);
        T.resize(P.m);
        g.resize(6 * static_cast<size_t>(P.m));
        delta.resize(6 * static_cast<size_t>(P.m));
        return SAGEICP_OK;
    }
    // linearise at x: F there; then delta
    int direction(double &F) {
        F = linearize();
        assemble();
        if (!T.factor()) return fail(SAGEICP_ERR_INVALID, "graph: the chain's normal matrix is not positive definite");
        const uint32_t r = 6u * P.c, total = 1u + r;
        const uint32_t K = chunk_columns(6 * static_cast<size_t>(P.m), total);
        Gm.assign(static_cast<size_t>(r) * total, 0.0);
        if (P.c) {
            X.resize(6 * static_cast<size_t>(P.m) * K);
            for (uint32_t col0 = 0; col0 < total; col0 += K) {
                const uint32_t k = std::min(K, total - col0);
                rhs_columns(col0, k);
                T.solve(X.data(), k);
                capacitance(col0, k);
            }
            z.resize(r);
            if (!pg_solve_capacitance(Gm.data(), r, Cm, z.data())) return fail(SAGEICP_ERR_INVALID, "graph: the capacitance system is not positive definite");
        }
        X.resize(std::max(X.size(), 6 * static_cast<size_t>(P.m)));
        rhs.resize(6 * static_cast<size_t>(P.m));
        for (size_t i = 0; i < rhs.size(); ++i) rhs[i] = -g[i];
        finish_solve();
        std::copy(X.begin(), X.begin() + 6 * static_cast<size_t>(P.m), delta.begin());
        // Refinement: Woodbury is accurate in delta but leaves a residual of cond(C) 2^-53, not 2^-53, of the system's terms
        // (1e-7 of them on a chain of 4 097 poses).  delta += H^-1 (-g - H delta), the residual summed from the edges' own
        // blocks, kPgRefineRounds times.
        for (int round = 0; round < kPgRefineRounds; ++round) {
            residual();
            if (P.c) {
                std::copy(rhs.begin(), rhs.end(), X.begin());
                T.solve(X.data(), 1);
                capacitance(0, 1);
                pg_resolve_capacitance(Cm, r, Gm.data(), total, z.data());
            }
            finish_solve();
            for (size_t i = 0; i < delta.size(); ++i) delta[i] += X[i];
        }
        return SAGEICP_OK;
    }
    int trial(double s, double &F, double &dmax) {
        dmax = 0.0;
        for (double d : delta) {
            const double a = std::fabs(d);
            if (a > dmax || a != a) dmax = a;
        }
        for (uint32_t k = 0; k < P.n; ++k) {
            double *o = xt.data() + 7 * static_cast<size_t>(k);
            const double *xk = x.data() + 7 * static_cast<size_t>(k);
            if (k == P.anchor) std::memcpy(o, xk, 7 * sizeof(double));
            else pg_retract(xk, delta.data() + 6 * static_cast<size_t>(pg_free_of(k, P.anchor)), s, o);
        }
        F = cost_at(P, xt.data(), nullptr);
        return SAGEICP_OK;
    }
    void accept() { x.swap(xt); }
    int finish(double &grad_max, double *poses_out) {
        linearize();
        assemble();
        grad_max = 0.0;
        for (double v : g) {
            const double a = std::fabs(v);
            if (a > grad_max || a != a) grad_max = a;
        }
        grad_max *= 2.0;
        std::memcpy(poses_out, x.data(), x.size() * sizeof(double));
        return SAGEICP_OK;
    }

private:
    double linearize() {
        double F = 0.0;
        for (uint32_t e = 0; e < P.E; ++e) {
            uint32_t a, b;
            P.ends(e, a, b);
            pg_linearize(P.zinv.data() + 7 * static_cast<size_t>(e), x.data() + 7 * static_cast<size_t>(a),
                         x.data() + 7 * static_cast<size_t>(b), P.l_of(e), lin[e]);
            F += pg_dot6(lin[e].w, lin[e].w);
        }
        return F;
    }
    void assemble() {
        for (uint32_t f = 0; f < P.m; ++f) {
            const uint32_t k = pg_vertex_of(f, P.anchor);
            double gv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            pg_zero(T.D[f].v);
            pg_zero(T.Eb[f].v);
            if (k >= 1u) {
                pg_add_atb(lin[k - 1u].B, lin[k - 1u].B, 1.0, T.D[f].v);
                pg_add_atv(lin[k - 1u].B, lin[k - 1u].w, 1.0, gv);
            }
            if (k + 1u < P.n) {
                pg_add_atb(lin[k].A, lin[k].A, 1.0, T.D[f].v);
                pg_add_atv(lin[k].A, lin[k].w, 1.0, gv);
                if (k + 1u != P.anchor) pg_add_atb(lin[k].A, lin[k].B, 1.0, T.Eb[f].v);
            }
            for (uint32_t ce = 0; ce < P.c; ++ce) {
                const PgEdgeLin &l = lin[P.n - 1u + ce];
                if (P.ca[ce] == k) pg_add_atv(l.A, l.w, 1.0, gv);
                if (P.cb[ce] == k) pg_add_atv(l.B, l.w, 1.0, gv);
            }
            for (int i = 0; i < 6; ++i) g[6 * static_cast<size_t>(f) + i] = gv[i];
        }
    }
    // X <- T^-1 (rhs - U z)
    void finish_solve() {
        for (uint32_t f = 0; f < P.m; ++f) {
            double v[6];
            for (int i = 0; i < 6; ++i) v[i] = rhs[6 * static_cast<size_t>(f) + i];
            const uint32_t k = pg_vertex_of(f, P.anchor);
            for (uint32_t ce = 0; ce < P.c; ++ce) {
                const bool at_a = P.ca[ce] == k, at_b = P.cb[ce] == k;
                if (!at_a && !at_b) continue;
                const PgEdgeLin &l = lin[P.n - 1u + ce];
                double zz[6];
                for (int s = 0; s < 6; ++s) zz[s] = z[6 * ce + s];
                pg_add_atv(at_a ? l.A : l.B, zz, -1.0, v);
            }
            for (int i = 0; i < 6; ++i) X[6 * static_cast<size_t>(f) + i] = v[i];
        }
        T.solve(X.data(), 1);
    }
    // edge e's J delta + w (the anchor's delta is zero)
    void edge_lin(uint32_t e, double (&t)[6]) const {
        uint32_t a, b;
        P.ends(e, a, b);
        double da[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, db[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < 6; ++i) {
            if (a != P.anchor) da[i] = delta[6 * static_cast<size_t>(pg_free_of(a, P.anchor)) + i];
            if (b != P.anchor) db[i] = delta[6 * static_cast<size_t>(pg_free_of(b, P.anchor)) + i];
        }
        pg_edge_model(lin[e], da, db, t);
    }
    // rhs <- -(g + H delta) = -sum J^T (J delta + w), a vertex's edges in assemble()'s order
    void residual() {
        for (uint32_t f = 0; f < P.m; ++f) {
            const uint32_t k = pg_vertex_of(f, P.anchor);
            double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[6];
            if (k >= 1u) {
                edge_lin(k - 1u, t);
                pg_add_atv(lin[k - 1u].B, t, 1.0, acc);
            }
            if (k + 1u < P.n) {
                edge_lin(k, t);
                pg_add_atv(lin[k].A, t, 1.0, acc);
            }
            for (uint32_t ce = 0; ce < P.c; ++ce) {
                if (P.ca[ce] != k && P.cb[ce] != k) continue;
                const uint32_t e = P.n - 1u + ce;
                edge_lin(e, t);
                pg_add_atv(P.ca[ce] == k ? lin[e].A : lin[e].B, t, 1.0, acc);
            }
            for (int i = 0; i < 6; ++i) rhs[6 * static_cast<size_t>(f) + i] = -acc[i];
        }
    }
    void rhs_columns(uint32_t col0, uint32_t K) {
        std::fill(X.begin(), X.begin() + 6 * static_cast<size_t>(P.m) * K, 0.0);
        for (uint32_t col = 0; col < K; ++col) {
            const uint32_t gc = col0 + col;
            if (gc == 0u) {
                for (size_t i = 0; i < 6 * static_cast<size_t>(P.m); ++i) X[i * K + col] = -g[i];
                continue;
            }
            const uint32_t ce = (gc - 1u) / 6u, sc = (gc - 1u) % 6u;
            const PgEdgeLin &l = lin[P.n - 1u + ce];
            if (P.ca[ce] != P.anchor) {
                const size_t f = pg_free_of(P.ca[ce], P.anchor);
                for (int r = 0; r < 6; ++r) X[(6 * f + r) * K + col] = row_of(l.A, sc)[r];
            }
            if (P.cb[ce] != P.anchor) {
                const size_t f = pg_free_of(P.cb[ce], P.anchor);
                for (int r = 0; r < 6; ++r) X[(6 * f + r) * K + col] = row_of(l.B, sc)[r];
            }
        }
    }
    static const double *row_of(const double (&M)[6][6], uint32_t s) { return M[s]; }
    void capacitance(uint32_t col0, uint32_t K) {
        const size_t ld = 1 + 6 * static_cast<size_t>(P.c);
        for (uint32_t row = 0; row < 6u * P.c; ++row) {
            const uint32_t ce = row / 6u, sc = row % 6u;
            const PgEdgeLin &l = lin[P.n - 1u + ce];
            for (uint32_t col = 0; col < K; ++col) {
                double sum = 0.0;
                if (P.ca[ce] != P.anchor) {
                    const size_t f = pg_free_of(P.ca[ce], P.anchor);
                    for (int r = 0; r < 6; ++r) sum += row_of(l.A, sc)[r] * X[(6 * f + r) * K + col];
                }
                if (P.cb[ce] != P.anchor) {
                    const size_t f = pg_free_of(P.cb[ce], P.anchor);
                    for (int r = 0; r < 6; ++r) sum += row_of(l.B, sc)[r] * X[(6 * f + r) * K + col];
                }
                Gm[row * ld + col0 + col] = sum;
            }
        }
    }

    const Problem &P;
    std::vector<double> x, xt, g, delta, rhs, X, Gm, Cm, z;
    std::vector<PgEdgeLin> lin;
    PgHostChain T;
};

// ---- the device path -------------------------------------------------------------------------------------------------------
class DeviceSolver {
public:
    explicit DeviceSolver(const Problem &p) : P(p) {}
    ~DeviceSolver() {
        if (stream) (void)hipStreamSynchronize(stream.get());    // before the buffers go
    }
    int init(const double *initial) {
        HIPCHK(stream.create());
        s = stream.get();
        lv = pg_levels(P.m);
        const size_t n = P.n, E = P.E, m = P.m, nodes = lv.nodes, r = 6 * static_cast<size_t>(P.c), total = 1 + r;
        K = chunk_columns(6 * nodes, static_cast<uint32_t>(total));
        HIPCHK(d_x.reserve(7 * n)); HIPCHK(d_xt.reserve(7 * n));
        HIPCHK(d_zinv.reserve(7 * E)); HIPCHK(d_L.reserve(P.L.size()));
        HIPCHK(d_ca.reserve(std::max<size_t>(1, P.c))); HIPCHK(d_cb.reserve(std::max<size_t>(1, P.c)));
        HIPCHK(d_lin.reserve(kPgLinFields * E)); HIPCHK(d_g.reserve(6 * m));
        HIPCHK(d_D.reserve(36 * nodes)); HIPCHK(d_E.reserve(36 * nodes)); HIPCHK(d_DP.reserve(36 * nodes)); HIPCHK(d_Q.reserve(36 * nodes));
        HIPCHK(d_X.reserve(6 * nodes * K));
        HIPCHK(d_delta.reserve(6 * m)); HIPCHK(d_q.reserve(6 * m)); HIPCHK(h_col.reserve(std::max<size_t>(1, r)));
        HIPCHK(d_Gm.reserve(std::max<size_t>(1, r * total))); HIPCHK(d_z.reserve(std::max<size_t>(1, r)));
        HIPCHK(d_ecost.reserve(E)); HIPCHK(d_slabs.reserve(kPgBlocks)); HIPCHK(d_out.reserve(2)); HIPCHK(d_bad.reserve(1)); HIPCHK(h_bad.reserve(1));
        HIPCHK(h_Gm.reserve(std::max<size_t>(1, r * total))); HIPCHK(h_z.reserve(std::max<size_t>(1, r))); HIPCHK(h_out.reserve(2));
        HIPCHK(hipMemcpyAsync(d_x.data(), initial, 7 * n * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_zinv.data(), P.zinv.data(), 7 * E * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_L.data(), P.L.data(), P.L.size() * sizeof(double), hipMemcpyHostToDevice, s));
        if (P.c) {
            HIPCHK(hipMemcpyAsync(d_ca.data(), P.ca.data(), P.c * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(d_cb.data(), P.cb.data(), P.c * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        }
        // the reduced levels' D and E, and the unused halves of DP and Q, are written before they are read; X's levels
        // likewise (posegraph.hip)
        G = PgGraph{P.n, P.c, P.anchor, P.m, P.E, d_zinv.data(), d_L.data(), P.l_stride, d_ca.data(), d_cb.data()};
        HIPCHK(hipMemsetAsync(d_bad.data(), 0, sizeof(uint32_t), s));
        S = PgSystem{d_lin.data(), d_g.data(), d_D.data(), d_E.data(), d_DP.data(), d_Q.data(), lv.nodes, d_bad.data()};
        return SAGEICP_OK;
    }
    int direction(double &F) {
        const uint32_t r = 6u * P.c, total = 1u + r;
        HIPCHK(pg_linearize_all(G, d_x.data(), S, d_ecost.data(), s));
        HIPCHK(pg_reduce(d_ecost.data(), P.E, false, d_slabs.data(), d_out.data(), s));
        HIPCHK(hipMemcpyAsync(h_out.data(), d_out.data(), sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(pg_assemble(G, S, s));
        HIPCHK(pg_factor(S, lv, s));
        if (P.c) {
            for (uint32_t col0 = 0; col0 < total; col0 += K) {
                const uint32_t k = std::min(K, total - col0);
                HIPCHK(pg_rhs_columns(G, S, col0, k, d_X.data(), s));
                HIPCHK(pg_apply(S, lv, k, d_X.data(), s));
                HIPCHK(pg_capacitance(G, S, d_X.data(), col0, k, d_Gm.data(), s));
            }
            HIPCHK(hipMemcpyAsync(h_Gm.data(), d_Gm.data(), static_cast<size_t>(r) * total * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipMemcpyAsync(h_bad.data(), d_bad.data(), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                 // the iteration's one wait
        F = h_out.data()[0];
        if (h_bad.data()[0]) return fail(SAGEICP_ERR_INVALID, "graph: the chain's normal matrix is not positive definite");
        if (P.c) {
            if (!pg_solve_capacitance(h_Gm.data(), r, Cm, h_z.data())) return fail(SAGEICP_ERR_INVALID, "graph: the capacitance system is not positive definite");
            HIPCHK(hipMemcpyAsync(d_z.data(), h_z.data(), r * sizeof(double), hipMemcpyHostToDevice, s));
        }
        HIPCHK(pg_rhs_final(G, S, d_z.data(), d_X.data(), s));
        HIPCHK(pg_apply(S, lv, 1u, d_X.data(), s));
        HIPCHK(hipMemcpyAsync(d_delta.data(), d_X.data(), 6 * static_cast<size_t>(P.m) * sizeof(double), hipMemcpyDeviceToDevice, s));
        // the refinement (HostSolver::direction): with closures each round has a wait of its own, for C^-1 on the host
        PgSystem Sq = S;
        Sq.g = d_q.data();
        for (int round = 0; round < kPgRefineRounds; ++round) {
            HIPCHK(pg_residual(G, S, d_delta.data(), d_q.data(), d_X.data(), s));
            if (P.c) {
                HIPCHK(pg_apply(S, lv, 1u, d_X.data(), s));
                HIPCHK(pg_capacitance(G, S, d_X.data(), 0u, 1u, d_Gm.data(), s));
                HIPCHK(hipMemcpy2DAsync(h_col.data(), sizeof(double), d_Gm.data(), static_cast<size_t>(total) * sizeof(double), sizeof(double), r,
                                        hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                pg_resolve_capacitance(Cm, r, h_col.data(), 1, h_z.data());
                HIPCHK(hipMemcpyAsync(d_z.data(), h_z.data(), r * sizeof(double), hipMemcpyHostToDevice, s));
            }
            HIPCHK(pg_rhs_final(G, Sq, d_z.data(), d_X.data(), s));
            HIPCHK(pg_apply(S, lv, 1u, d_X.data(), s));
            HIPCHK(pg_accumulate(G, d_X.data(), d_delta.data(), s));
        }
        HIPCHK(pg_reduce(d_delta.data(), 6 * static_cast<uint64_t>(P.m), true, d_slabs.data(), d_out.data() + 1, s));
        return SAGEICP_OK;
    }
    int trial(double step, double &F, double &dmax) {
        HIPCHK(pg_update(G, d_x.data(), d_delta.data(), step, d_xt.data(), s));
        HIPCHK(pg_cost(G, d_xt.data(), d_ecost.data(), s));
        HIPCHK(pg_reduce(d_ecost.data(), P.E, false, d_slabs.data(), d_out.data(), s));
        HIPCHK(hipMemcpyAsync(h_out.data(), d_out.data(), 2 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                 // the trial's one wait
        F = h_out.data()[0];
        dmax = h_out.data()[1];
        return SAGEICP_OK;
    }
    void accept() { std::swap(d_x, d_xt); }
    int finish(double &grad_max, double *poses_out) {
        HIPCHK(pg_linearize_all(G, d_x.data(), S, d_ecost.data(), s));
        HIPCHK(pg_assemble(G, S, s));
        HIPCHK(pg_reduce(d_g.data(), 6 * static_cast<uint64_t>(P.m), true, d_slabs.data(), d_out.data(), s));
        HIPCHK(hipMemcpyAsync(h_out.data(), d_out.data(), sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(poses_out, d_x.data(), 7 * static_cast<size_t>(P.n) * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        grad_max = 2.0 * h_out.data()[0];
        return SAGEICP_OK;
    }

private:
    const Problem &P;
    // (the buffers first, the stream last: it goes first, after its work has been waited for)
    DevBuf<double> d_x, d_xt, d_zinv, d_L, d_lin, d_g, d_D, d_E, d_DP, d_Q, d_X, d_delta, d_q, d_Gm, d_z, d_ecost, d_slabs, d_out;
    DevBuf<uint32_t> d_ca, d_cb, d_bad;
    PinnedBuf<double> h_Gm, h_col, h_z, h_out;
    PinnedBuf<uint32_t> h_bad;
    std::vector<double> Cm;
    OwnedStream stream;
    hipStream_t s = nullptr;
    PgLevels lv{};
    PgGraph G{};
    PgSystem S{};
    uint32_t K = 1;
};

// ---- Gauss-Newton with backtracking, over either path -------------------------------------------------------------------------
template <class Solver>
int gauss_newton(Solver &sv, uint32_t edges, const sageicp_graph_params &prm, sageicp_graph_info &info, double *poses_tmp) {
    double F = 0.0;
    info.status = 2;
    for (uint32_t it = 0; it < prm.max_iterations; ++it) {
        double F_lin = 0.0;
        if (int rc = sv.direction(F_lin)) return rc;
        if (it == 0) {
            if (!std::isfinite(F_lin)) return fail(SAGEICP_ERR_INVALID, "graph: the cost at the start is not finite");
            F = info.cost_initial = F_lin;
        }
        bool accepted = false;
        double step = 1.0, dmax = 0.0;
        for (uint32_t h = 0; h <= prm.max_halvings; ++h, step *= 0.5) {
            double F_try = 0.0;
            if (int rc = sv.trial(step, F_try, dmax)) return rc;
            // The full step is also taken where F cannot tell: every edge's term carries the rounding of its relative pose
            // times a whitened gradient that is not small (the edges' gradients cancel only in the sum at a vertex), so two
            // evaluations of F near one point differ by tens of ulps — (E + 64) 2^-52 F bounds it, as the tests' comparisons
            // of F do — and within some 1e-8 of the minimiser a Newton step's decrease lies below that.  Held to F_try < F
            // alone, whether such a step was taken, halved or refused (status 1) was decided by rounding.  (Never above the
            // start: cost_final <= cost_initial stays a property of every return.)
            const double noise = (static_cast<double>(edges) + 64.0) * 0x1p-52 * F;
            if (F_try < F || (h == 0 && F_try < F + noise && F_try <= info.cost_initial)) {
                sv.accept();
                F = F_try;
                accepted = true;
                break;
            }
            ++info.halvings;
        }
        if (!accepted) {
            info.status = 1;
            break;
        }
        ++info.iterations;
        info.step_last = step * dmax;
        if (info.step_last <= prm.step_tol) {
            info.status = 0;
            break;
        }
    }
    if (prm.max_iterations == 0) {                       // (nothing linearised: F is asked for on its own)
        double F_lin = 0.0;
        if (int rc = sv.direction(F_lin)) return rc;
        F = info.cost_initial = F_lin;
    }
    info.cost_final = F;
    return sv.finish(info.grad_max, poses_tmp);
}

int optimize(const double *poses, uint64_t n, const double *odom_info, uint32_t stride, const sageicp_graph_edge *cl, uint32_t c,
             const double *initial, const sageicp_graph_params *params, double *poses_out, double *corr_out, sageicp_graph_info *info_out) {
    sageicp_graph_params prm;
    sageicp_graph_params_default(&prm);
    if (params) prm = *params;
    if (!poses_out) return fail(SAGEICP_ERR_INVALID, "graph: null argument");
    if (prm.where > 2u) return fail(SAGEICP_ERR_INVALID, "graph: where is 0 (auto), 1 (host) or 2 (device)");
    if (!(prm.step_tol >= 0.0)) return fail(SAGEICP_ERR_INVALID, "graph: step_tol is negative or not a number");
    Problem P;
    if (int rc = make_problem(poses, n, odom_info, stride, cl, c, prm.anchor, P)) return rc;
    if (initial)
        if (int rc = check_poses(initial, n, "initial")) return rc;
    const double *start = initial ? initial : poses;
    uint32_t where = prm.where;
    if (where == 2u) {
        if (int rc = require_device()) return rc;
    } else if (where == 0u) {
        where = (n >= SAGEICP_GRAPH_AUTO_POSES && sageicp_device_count() > 0) ? 2u : 1u;
    }
    // ---- nothing of the caller's is written before the optimiser has ended well ----
    sageicp_graph_info info{};
    info.where = where;
    std::vector<double> out(7 * static_cast<size_t>(n));
    int rc;
    if (where == 2u) {
        DeviceSolver sv(P);
        rc = sv.init(start);
        if (!rc) rc = gauss_newton(sv, P.E, prm, info, out.data());
    } else {
        HostSolver sv(P);
        rc = sv.init(start);
        if (!rc) rc = gauss_newton(sv, P.E, prm, info, out.data());
    }
    if (rc) return rc;
    if (!finite_n(out.data(), out.size())) return fail(SAGEICP_ERR_INVALID, "graph: the optimum is not finite");
    const double I[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    const double *pa = poses + 7 * static_cast<size_t>(P.anchor), *sa = start + 7 * static_cast<size_t>(P.anchor);
    const bool anchor_kept = std::memcmp(pa, sa, 7 * sizeof(double)) == 0;
    std::memcpy(out.data() + 7 * static_cast<size_t>(P.anchor), sa, 7 * sizeof(double));
    double shift = 0.0;
    for (uint64_t k = 0; k < n; ++k) {
        const double *o = out.data() + 7 * k, *p = poses + 7 * k;
        const double dx = o[4] - p[4], dy = o[5] - p[5], dz = o[6] - p[6];
        shift = std::max(shift, std::sqrt((dx * dx + dy * dy) + dz * dz));
        if (corr_out) {
            double *C = corr_out + 7 * k;
            if (k == P.anchor && anchor_kept) {
                std::memcpy(C, I, sizeof(I));
            } else {
                double inv[7], Ck[7];
                se3_inv(p, inv);
                se3_mul(o, inv, Ck);
                std::memcpy(C, Ck, sizeof(Ck));
            }
        }
    }
    info.max_shift = shift;
    std::memmove(poses_out, out.data(), out.size() * sizeof(double));
    if (info_out) *info_out = info;
    return SAGEICP_OK;
}

}  // namespace
}  // namespace sageicp_impl

extern "C" {

void sageicp_graph_params_default(sageicp_graph_params *p) {
    if (!p) return;
    sageicp_graph_params d{};
    d.anchor = 0;
    d.max_iterations = 50;
    d.max_halvings = 10;
    d.step_tol = 1e-9;
    d.where = 0;
    *p = d;
}

int sageicp_graph_edge_from_closed(const double *poses, uint64_t n, uint64_t i, uint64_t j, const double closed[7],
                                   const double info[36], sageicp_graph_edge *out) {
    if (!poses || !closed || !info || !out) return fail(SAGEICP_ERR_INVALID, "graph edge: null argument");
    if (i >= n || j >= n || i == j) return fail(SAGEICP_ERR_INVALID, "graph edge: needs i != j, both below n");
    if (!finite_n(poses + 7 * i, 7) || !finite_n(closed, 7) || zero_quat(poses + 7 * i) || zero_quat(closed))
        return fail(SAGEICP_ERR_INVALID, "graph edge: a pose is not finite, or its quaternion is 0");
    double L[36];
    if (!info_factor(info, L)) return fail(SAGEICP_ERR_INVALID, "graph edge: info is not finite, symmetric to the bit and positive definite");
    sageicp_graph_edge e{};
    e.a = i;
    e.b = j;
    pg_between(poses + 7 * i, closed, e.z);
    if (!finite_n(e.z, 7)) return fail(SAGEICP_ERR_INVALID, "graph edge: the relative pose is not finite");
    std::memcpy(e.info, info, sizeof(e.info));
    *out = e;
    return SAGEICP_OK;
}

int sageicp_graph_cost(const double *poses, uint64_t n, const double *odom_info, uint32_t odom_info_stride,
                       const sageicp_graph_edge *closures, uint32_t c, const double *at, double *cost, double *per_edge) {
    if (!at || !cost) return fail(SAGEICP_ERR_INVALID, "graph: null argument");
    Problem P;
    if (int rc = make_problem(poses, n, odom_info, odom_info_stride, closures, c, 0, P)) return rc;
    if (int rc = check_poses(at, n, "at")) return rc;
    std::vector<double> pe(P.E);
    const double F = cost_at(P, at, pe.data());
    if (per_edge) std::memcpy(per_edge, pe.data(), pe.size() * sizeof(double));
    *cost = F;
    return SAGEICP_OK;
}

int sageicp_graph_optimize(const double *poses, uint64_t n, const double *odom_info, uint32_t odom_info_stride,
                           const sageicp_graph_edge *closures, uint32_t c, const double *initial, const sageicp_graph_params *params,
                           double *poses_out, double *corrections_out, sageicp_graph_info *info) {
    return optimize(poses, n, odom_info, odom_info_stride, closures, c, initial, params, poses_out, corrections_out, info);
}

int sageicp_pipeline_graph_optimize(const sageicp_pipeline *p, const double *odom_info, uint32_t odom_info_stride,
                                    const sageicp_graph_edge *closures, uint32_t c, const sageicp_graph_params *params,
                                    double *corrections_out, double *poses_out, sageicp_graph_info *info) {
    if (!p || !corrections_out) return fail(SAGEICP_ERR_INVALID, "sageicp_pipeline_graph_optimize: null argument");
    const uint64_t n = sageicp_pipeline_num_poses(p);
    std::vector<double> poses(7 * static_cast<size_t>(n)), out(7 * static_cast<size_t>(n));
    for (uint64_t k = 0; k < n; ++k)
        if (int rc = sageicp_pipeline_pose(p, k, poses.data() + 7 * k)) return rc;
    if (int rc = optimize(poses.data(), n, odom_info, odom_info_stride, closures, c, nullptr, params, out.data(), corrections_out, info))
        return rc;
    if (poses_out) std::memcpy(poses_out, out.data(), out.size() * sizeof(double));
    return SAGEICP_OK;
}

}  // extern "C"
