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
//
// Robust kernels on the closures: Problem::kernel and the solver's scale make linearize() / k_pg_lin<true>
// scale a closure's A, B, w by sqrt(rho') and the costs take rho(s); everything after the linearisation is unchanged.
// The scale continuation runs gn_stage() once per stage; its schedule comes from the closures' terms at the start,
// evaluated here on the host, so neither path waits for it.  An annealed device call waits once more, for the final
// kernel's F at the start.
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
    uint32_t kernel = 0;             // the closures' robust kernel (posegraph.h pg_rho); its scale is the solver's, per stage
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

// kernel 0: the plain F; otherwise the closures' terms under pg_rho(kernel, c2, .)
double cost_at(const Problem &P, const double *x, double *per_edge, uint32_t kernel = 0, double c2 = 0.0) {
    double F = 0.0;
    for (uint32_t e = 0; e < P.E; ++e) {
        uint32_t a, b;
        P.ends(e, a, b);
        double v = pg_edge_cost(P.zinv.data() + 7 * static_cast<size_t>(e), x + 7 * static_cast<size_t>(a),
                                x + 7 * static_cast<size_t>(b), P.l_of(e));
        if (kernel && e >= P.n - 1u) v = pg_rho(kernel, c2, v);
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
        F = cost_at(P, xt.data(), nullptr, P.kernel, c2);
        return SAGEICP_OK;
    }
    void accept() { x.swap(xt); }
    void set_scale2(double v) { c2 = v; }
    // F at x under the current scale, nothing else touched
    int cost_here(double &F) {
        F = cost_at(P, x.data(), nullptr, P.kernel, c2);
        return SAGEICP_OK;
    }
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
            if (P.kernel && e >= P.n - 1u) F += pg_robustify(P.kernel, c2, lin[e]);
            else F += pg_dot6(lin[e].w, lin[e].w);
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
    double c2 = 0.0;
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
        G = PgGraph{P.n, P.c, P.anchor, P.m, P.E, d_zinv.data(), d_L.data(), P.l_stride, d_ca.data(), d_cb.data(), P.kernel, 0.0};
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
    void set_scale2(double v) { G.c2 = v; }
    // F at x under the current scale: one wait, once per annealed call
    int cost_here(double &F) {
        HIPCHK(pg_cost(G, d_x.data(), d_ecost.data(), s));
        HIPCHK(pg_reduce(d_ecost.data(), P.E, false, d_slabs.data(), d_out.data(), s));
        HIPCHK(hipMemcpyAsync(h_out.data(), d_out.data(), sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        F = h_out.data()[0];
        return SAGEICP_OK;
    }
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
// One stage: at most max_iterations iterations at the solver's current scale.  iterations, halvings and step_last of `info`
// go on counting; F_first is F where the stage began, F the cost where it ended, status as sageicp_graph_info's.
template <class Solver>
int gn_stage(Solver &sv, uint32_t edges, uint32_t max_iterations, const sageicp_graph_params &prm, sageicp_graph_info &info,
             double &F_first, double &F, uint32_t &status) {
    F = 0.0;
    status = 2;
    for (uint32_t it = 0; it < max_iterations; ++it) {
        double F_lin = 0.0;
        if (int rc = sv.direction(F_lin)) return rc;
        if (it == 0) {
            if (!std::isfinite(F_lin)) return fail(SAGEICP_ERR_INVALID, "graph: the cost at the start is not finite");
            F = F_first = F_lin;
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
            if (F_try < F || (h == 0 && F_try < F + noise && F_try <= F_first)) {
                sv.accept();
                F = F_try;
                accepted = true;
                break;
            }
            ++info.halvings;
        }
        if (!accepted) {
            status = 1;
            break;
        }
        ++info.iterations;
        info.step_last = step * dmax;
        if (info.step_last <= prm.step_tol) {
            status = 0;
            break;
        }
    }
    if (max_iterations == 0) {                           // (nothing linearised: F is asked for on its own)
        double F_lin = 0.0;
        if (int rc = sv.direction(F_lin)) return rc;
        F = F_first = F_lin;
    }
    return SAGEICP_OK;
}

// What a robust call adds to the problem (sageicp_graph_robust, checked) and what it reports
struct Robust {
    uint32_t kernel = 0;
    bool anneal = false;
    double c2 = 0.0, factor = 2.0;
    uint32_t stage_iterations = 3;
    double s0 = 0.0;                 // the largest closure term at the start (host, fp64): it alone fixes the schedule
    double c2_first = 0.0;
    uint32_t stages = 1;
};
constexpr uint32_t kPgMaxStages = 1024;

// The stages c2 f^m, ..., c2 f, c2 (m the smallest count with c2 f^m >= s0; one stage without anneal), each but the last
// under stage_iterations, the last under max_iterations.  cost_initial and cost_final are the final scale's F.
template <class Solver>
int gauss_newton(Solver &sv, uint32_t edges, const sageicp_graph_params &prm, Robust &rb, sageicp_graph_info &info, double *poses_tmp) {
    double F_first = 0.0, F = 0.0;
    if (!rb.kernel) {
        if (int rc = gn_stage(sv, edges, prm.max_iterations, prm, info, F_first, F, info.status)) return rc;
        info.cost_initial = F_first;
        info.cost_final = F;
        return sv.finish(info.grad_max, poses_tmp);
    }
    std::vector<double> scale2(1, rb.c2);
    if (rb.anneal)
        while (scale2.back() < rb.s0) scale2.push_back(scale2.back() * rb.factor);
    rb.stages = static_cast<uint32_t>(scale2.size());
    rb.c2_first = scale2.back();
    if (rb.stages > 1u) {
        sv.set_scale2(rb.c2);
        if (int rc = sv.cost_here(info.cost_initial)) return rc;
        if (!std::isfinite(info.cost_initial)) return fail(SAGEICP_ERR_INVALID, "graph: the cost at the start is not finite");
    }
    for (uint32_t st = rb.stages; st-- > 0;) {
        sv.set_scale2(scale2[st]);
        if (int rc = gn_stage(sv, edges, st ? rb.stage_iterations : prm.max_iterations, prm, info, F_first, F, info.status)) return rc;
    }
    if (rb.stages == 1u) info.cost_initial = F_first;
    info.cost_final = F;
    return sv.finish(info.grad_max, poses_tmp);
}

int optimize(const double *poses, uint64_t n, const double *odom_info, uint32_t stride, const sageicp_graph_edge *cl, uint32_t c,
             const double *initial, const sageicp_graph_params *params, double *poses_out, double *corr_out, sageicp_graph_info *info_out,
             const sageicp_graph_robust *robust = nullptr, double *chi2_out = nullptr, double *weight_out = nullptr,
             sageicp_graph_robust_info *rinfo_out = nullptr) {
    sageicp_graph_params prm;
    sageicp_graph_params_default(&prm);
    if (params) prm = *params;
    if (!poses_out) return fail(SAGEICP_ERR_INVALID, "graph: null argument");
    Robust rb;
    if (robust) {
        if (robust->kernel > 3u) return fail(SAGEICP_ERR_INVALID, "graph: robust kernel is 0 (none), 1 (Huber), 2 (Cauchy) or 3 (Geman-McClure)");
        if (robust->anneal > 1u) return fail(SAGEICP_ERR_INVALID, "graph: robust anneal is 0 or 1");
        if (!std::isfinite(robust->scale) || !(robust->scale > 0.0)) return fail(SAGEICP_ERR_INVALID, "graph: robust scale is not finite and above 0");
        if (!std::isfinite(robust->anneal_factor) || !(robust->anneal_factor > 1.0))
            return fail(SAGEICP_ERR_INVALID, "graph: robust anneal_factor is not finite and above 1");
        if (robust->stage_iterations == 0u) return fail(SAGEICP_ERR_INVALID, "graph: robust stage_iterations is 0");
        rb.kernel = robust->kernel;
        rb.anneal = robust->anneal == 1u;
        rb.c2 = rb.c2_first = robust->scale * robust->scale;
        rb.factor = robust->anneal_factor;
        rb.stage_iterations = robust->stage_iterations;
        if (!std::isfinite(rb.c2) || !(rb.c2 > 0.0)) return fail(SAGEICP_ERR_INVALID, "graph: the square of robust scale is not finite and above 0");
    }
    if (prm.where > 2u) return fail(SAGEICP_ERR_INVALID, "graph: where is 0 (auto), 1 (host) or 2 (device)");
    if (!(prm.step_tol >= 0.0)) return fail(SAGEICP_ERR_INVALID, "graph: step_tol is negative or not a number");
    Problem P;
    if (int rc = make_problem(poses, n, odom_info, stride, cl, c, prm.anchor, P)) return rc;
    if (initial)
        if (int rc = check_poses(initial, n, "initial")) return rc;
    const double *start = initial ? initial : poses;
    P.kernel = rb.kernel;
    if (rb.kernel && rb.anneal) {
        for (uint32_t e = P.n - 1u; e < P.E; ++e)
            rb.s0 = std::max(rb.s0, pg_edge_cost(P.zinv.data() + 7 * static_cast<size_t>(e), start + 7 * static_cast<size_t>(P.ca[e - (P.n - 1u)]),
                                                 start + 7 * static_cast<size_t>(P.cb[e - (P.n - 1u)]), P.l_of(e)));
        if (!std::isfinite(rb.s0)) return fail(SAGEICP_ERR_INVALID, "graph: the cost at the start is not finite");
        double v = rb.c2;
        uint32_t m = 1;
        for (; v < rb.s0; v *= rb.factor)
            if (++m > kPgMaxStages) return fail(SAGEICP_ERR_CAPACITY, "graph: the anneal needs more than 1024 stages");
    }
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
        if (!rc) rc = gauss_newton(sv, P.E, prm, rb, info, out.data());
    } else {
        HostSolver sv(P);
        rc = sv.init(start);
        if (!rc) rc = gauss_newton(sv, P.E, prm, rb, info, out.data());
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
    // the closures' raw terms at poses_out and their weights under the final scale (host, fp64: sageicp_graph_cost's terms)
    sageicp_graph_robust_info ri{};
    ri.scale2_first = rb.c2_first;
    ri.stages = rb.stages;
    for (uint32_t ce = 0; ce < P.c; ++ce) {
        const uint32_t e = P.n - 1u + ce;
        const double sv = pg_edge_cost(P.zinv.data() + 7 * static_cast<size_t>(e), out.data() + 7 * static_cast<size_t>(P.ca[ce]),
                                       out.data() + 7 * static_cast<size_t>(P.cb[ce]), P.l_of(e));
        const double w = pg_rho_weight(rb.kernel, rb.c2, sv);
        if (w < 0.5) ++ri.outliers;
        if (chi2_out) chi2_out[ce] = sv;
        if (weight_out) weight_out[ce] = w;
    }
    std::memmove(poses_out, out.data(), out.size() * sizeof(double));
    if (info_out) *info_out = info;
    if (rinfo_out) *rinfo_out = ri;
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
    return sageicp_pipeline_graph_optimize_robust(p, odom_info, odom_info_stride, closures, c, params, corrections_out, poses_out, info,
                                                  nullptr, nullptr, nullptr, nullptr);
}

void sageicp_graph_robust_default(sageicp_graph_robust *r) {
    if (!r) return;
    sageicp_graph_robust d{};
    d.kernel = SAGEICP_GRAPH_KERNEL_NONE;
    d.anneal = 0;
    d.scale = std::sqrt(16.81);
    d.anneal_factor = 2.0;
    d.stage_iterations = 3;
    *r = d;
}

int sageicp_graph_optimize_robust(const double *poses, uint64_t n, const double *odom_info, uint32_t odom_info_stride,
                                  const sageicp_graph_edge *closures, uint32_t c, const double *initial, const sageicp_graph_params *params,
                                  double *poses_out, double *corrections_out, sageicp_graph_info *info, const sageicp_graph_robust *robust,
                                  double *closure_chi2_out, double *closure_weight_out, sageicp_graph_robust_info *rinfo) {
    return optimize(poses, n, odom_info, odom_info_stride, closures, c, initial, params, poses_out, corrections_out, info, robust,
                    closure_chi2_out, closure_weight_out, rinfo);
}

int sageicp_pipeline_graph_optimize_robust(const sageicp_pipeline *p, const double *odom_info, uint32_t odom_info_stride,
                                           const sageicp_graph_edge *closures, uint32_t c, const sageicp_graph_params *params,
                                           double *corrections_out, double *poses_out, sageicp_graph_info *info,
                                           const sageicp_graph_robust *robust, double *closure_chi2_out, double *closure_weight_out,
                                           sageicp_graph_robust_info *rinfo) {
    if (!p || !corrections_out) return fail(SAGEICP_ERR_INVALID, "sageicp_pipeline_graph_optimize: null argument");
    const uint64_t n = sageicp_pipeline_num_poses(p);
    std::vector<double> poses(7 * static_cast<size_t>(n)), out(7 * static_cast<size_t>(n));
    for (uint64_t k = 0; k < n; ++k)
        if (int rc = sageicp_pipeline_pose(p, k, poses.data() + 7 * k)) return rc;
    if (int rc = optimize(poses.data(), n, odom_info, odom_info_stride, closures, c, nullptr, params, out.data(), corrections_out, info,
                          robust, closure_chi2_out, closure_weight_out, rinfo))
        return rc;
    if (poses_out) std::memcpy(poses_out, out.data(), out.size() * sizeof(double));
    return SAGEICP_OK;
}

// ---- an edge's information from a quality report (host, fp64) -------------------------------------------------
int sageicp_graph_info_from_quality(const sageicp_quality *q, const double closed[7], double gain, double info_out[36]) {
    if (!q || !closed || !info_out) return fail(SAGEICP_ERR_INVALID, "graph info: null argument");
    if (!q->covariance_valid) return fail(SAGEICP_ERR_INVALID, "graph info: the report has no valid covariance");
    if (!finite_n(q->JTJ, 36) || !std::isfinite(q->sum_w_r2) || !finite_n(closed, 7) || !std::isfinite(gain))
        return fail(SAGEICP_ERR_INVALID, "graph info: an input is not finite");
    if (zero_quat(closed)) return fail(SAGEICP_ERR_INVALID, "graph info: the quaternion of closed is 0");
    if (!(gain > 0.0)) return fail(SAGEICP_ERR_INVALID, "graph info: gain is not above 0");
    const double s2 = q->sum_w_r2 / (3.0 * static_cast<double>(q->n_pairs) - 6.0);
    if (!(s2 > 0.0) || !std::isfinite(s2)) return fail(SAGEICP_ERR_INVALID, "graph info: s2 = sum_w_r2 / (3 n_pairs - 6) is not above 0");
    // Ad(closed) = [[R, hat(t) R], [0, R]] in (upsilon, omega): the report's left tangent xi from the edge's right one, xi = Ad eta
    const double qn = std::sqrt((closed[0] * closed[0] + closed[1] * closed[1]) + (closed[2] * closed[2] + closed[3] * closed[3]));
    const double qu[4] = {closed[0] / qn, closed[1] / qn, closed[2] / qn, closed[3] / qn};
    double Rf[9], R[3][3], T[3][3], TR[3][3], Ad[6][6], M[6][6], W[6][6], O[6][6];
    quat_to_mat(qu, Rf);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = Rf[3 * i + j];
    const double t[3] = {closed[4], closed[5], closed[6]};
    pg_hat(t, T);
    pg_mul3(T, R, TR);
    pg_zero(Ad);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Ad[i][j] = R[i][j];
            Ad[i][j + 3] = TR[i][j];
            Ad[i + 3][j + 3] = R[i][j];
        }
    const double k = gain / s2;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) M[i][j] = k * q->JTJ[6 * i + j];
    pg_zero(W);
    pg_zero(O);
    pg_add_ab(M, Ad, 1.0, W);
    pg_add_atb(Ad, W, 1.0, O);
    double sym[36], L[36];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) sym[6 * i + j] = i <= j ? 0.5 * (O[i][j] + O[j][i]) : 0.0;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < i; ++j) sym[6 * i + j] = sym[6 * j + i];
    if (!info_factor(sym, L)) return fail(SAGEICP_ERR_INVALID, "graph info: the result is not finite and positive definite (register in a local frame)");
    std::memcpy(info_out, sym, sizeof(sym));
    return SAGEICP_OK;
}

}  // extern "C"
