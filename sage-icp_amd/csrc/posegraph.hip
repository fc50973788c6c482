// The device side of the pose-graph optimiser (gfx950) — see posegraph.h and DESIGN.md D19.
//
//   linearise   k_pg_lin      a lane per edge: A, B, w and the edge's cost; <true>: the closures under a robust kernel (D20)
//   assemble    k_pg_asm      a lane per free vertex gathers its two odometry edges and, in the caller's order, its closures
//   factor      k_pg_inv, k_pg_red    per level of the block cyclic reduction: invert the even diagonals, reduce onto the odd
//   apply       k_pg_fwd, k_pg_bwd    per level, a lane per (node, column) of a chunk of right-hand sides
//   low rank    k_pg_rhs_cols, k_pg_cap, k_pg_rhs_final     columns of [-g | U] in, U^T T^-1 [-g | U] out, -g - U z in
//   refine      k_pg_resid, k_pg_acc          g + H delta per free vertex from its edges' blocks; delta += the correction
//   step        k_pg_update, k_pg_cost, k_pg_red1 -> k_pg_red2
//
// Phases are kernel boundaries on one stream.  No atomic, no barrier across workgroups, no wait inside a kernel; every
// sum is a fixed tree (a lane's strided run, the workgroup's LDS tree, one workgroup over the slabs), so the same input
// gives the same bytes.  Every loop is bounded by an argument and every index by the counts in PgGraph / PgLevels, which
// are what the host reserved the buffers by.  6x6 blocks are registers: compile-time indices only (posegraph.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "posegraph.h"

namespace sageicp {

namespace {

__device__ __forceinline__ void ld36(const double *__restrict__ base, size_t count, size_t idx, double (&M)[6][6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) M[i][j] = base[static_cast<size_t>(i * 6 + j) * count + idx];
}
__device__ __forceinline__ void st36(double *__restrict__ base, size_t count, size_t idx, const double (&M)[6][6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) base[static_cast<size_t>(i * 6 + j) * count + idx] = M[i][j];
}
__device__ __forceinline__ void ld6(const double *__restrict__ base, size_t count, size_t idx, double (&v)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = base[static_cast<size_t>(i) * count + idx];
}
// a column's six rows of a node of X
__device__ __forceinline__ void ldx(const double *__restrict__ X, size_t node, uint32_t K, uint32_t col, double (&v)[6]) {
#pragma unroll
    for (int r = 0; r < 6; ++r) v[r] = X[(node * 6 + r) * K + col];
}
__device__ __forceinline__ void stx(double *__restrict__ X, size_t node, uint32_t K, uint32_t col, const double (&v)[6]) {
#pragma unroll
    for (int r = 0; r < 6; ++r) X[(node * 6 + r) * K + col] = v[r];
}

__device__ __forceinline__ void edge_of(const PgGraph &G, uint32_t e, uint32_t &a, uint32_t &b, const double *&L) {
    if (e < G.n - 1u) {
        a = e;
        b = e + 1u;
        L = G.L + static_cast<size_t>(G.l_stride) * e;
    } else {
        const uint32_t ce = e - (G.n - 1u);
        a = G.ca[ce];
        b = G.cb[ce];
        L = G.L + (G.l_stride ? static_cast<size_t>(36) * (G.n - 1u) : size_t(36)) + static_cast<size_t>(36) * ce;
    }
}

#define PG_STRIDE(i, count)                                                                          \
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < (count);            \
         i += static_cast<uint64_t>(gridDim.x) * 256)

// Robust: the closures (e >= n - 1) under G.kernel at G.c2 (posegraph.h pg_robustify); the plain kernels hold none of it
template <bool Robust>
__global__ __launch_bounds__(256) void k_pg_lin(PgGraph G, const double *__restrict__ x, double *__restrict__ lin,
                                                double *__restrict__ edge_cost) {
    PG_STRIDE(e64, G.E) {
        const uint32_t e = static_cast<uint32_t>(e64);
        uint32_t a, b;
        const double *L;
        edge_of(G, e, a, b, L);
        PgEdgeLin o;
        pg_linearize(G.zinv + 7 * static_cast<size_t>(e), x + 7 * static_cast<size_t>(a), x + 7 * static_cast<size_t>(b), L, o);
        double cost;
        if (Robust && e >= G.n - 1u) cost = pg_robustify(G.kernel, G.c2, o);
        else cost = pg_dot6(o.w, o.w);
        st36(lin, G.E, e, o.A);
        st36(lin + static_cast<size_t>(36) * G.E, G.E, e, o.B);
#pragma unroll
        for (int i = 0; i < 6; ++i) lin[static_cast<size_t>(72 + i) * G.E + e] = o.w[i];
        edge_cost[e] = cost;
    }
}

template <bool Robust>
__global__ __launch_bounds__(256) void k_pg_cost(PgGraph G, const double *__restrict__ x, double *__restrict__ edge_cost) {
    PG_STRIDE(e64, G.E) {
        const uint32_t e = static_cast<uint32_t>(e64);
        uint32_t a, b;
        const double *L;
        edge_of(G, e, a, b, L);
        const double cost = pg_edge_cost(G.zinv + 7 * static_cast<size_t>(e), x + 7 * static_cast<size_t>(a),
                                         x + 7 * static_cast<size_t>(b), L);
        edge_cost[e] = (Robust && e >= G.n - 1u) ? pg_rho(G.kernel, G.c2, cost) : cost;
    }
}

__global__ __launch_bounds__(256) void k_pg_asm(PgGraph G, PgSystem S) {
    const double *linA = S.lin, *linB = S.lin + static_cast<size_t>(36) * G.E, *linW = S.lin + static_cast<size_t>(72) * G.E;
    PG_STRIDE(f64, G.m) {
        const uint32_t f = static_cast<uint32_t>(f64), k = pg_vertex_of(f, G.anchor);
        double D[6][6], Eb[6][6], g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        pg_zero(D);
        pg_zero(Eb);
        if (k >= 1u) {                                   // edge (k - 1, k): its B side
            double B[6][6], w[6];
            ld36(linB, G.E, k - 1u, B);
            ld6(linW, G.E, k - 1u, w);
            pg_add_atb(B, B, 1.0, D);
            pg_add_atv(B, w, 1.0, g);
        }
        if (k + 1u < G.n) {                              // edge (k, k + 1): its A side, and the coupling to k + 1
            double A[6][6], w[6];
            ld36(linA, G.E, k, A);
            ld6(linW, G.E, k, w);
            pg_add_atb(A, A, 1.0, D);
            pg_add_atv(A, w, 1.0, g);
            if (k + 1u != G.anchor) {
                double B[6][6];
                ld36(linB, G.E, k, B);
                pg_add_atb(A, B, 1.0, Eb);
            }
        }
        for (uint32_t ce = 0; ce < G.c; ++ce) {          // the closures' terms of g, in the caller's order
            const uint32_t e = G.n - 1u + ce;
            if (G.ca[ce] == k) {
                double A[6][6], w[6];
                ld36(linA, G.E, e, A);
                ld6(linW, G.E, e, w);
                pg_add_atv(A, w, 1.0, g);
            }
            if (G.cb[ce] == k) {
                double B[6][6], w[6];
                ld36(linB, G.E, e, B);
                ld6(linW, G.E, e, w);
                pg_add_atv(B, w, 1.0, g);
            }
        }
        st36(S.D, S.nodes, f, D);
        st36(S.E, S.nodes, f, Eb);
#pragma unroll
        for (int i = 0; i < 6; ++i) S.g[static_cast<size_t>(i) * G.m + f] = g[i];
    }
}

// ---- the factor: level (o, ml) -> (o2, m2 = ml / 2) ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pg_inv(PgSystem S, uint32_t o, uint32_t ml) {
    const uint32_t evens = (ml + 1u) / 2u;
    PG_STRIDE(t, evens) {
        const size_t p = static_cast<size_t>(o) + 2u * static_cast<uint32_t>(t);
        double D[6][6], I[6][6];
        ld36(S.D, S.nodes, p, D);
        if (!pg_spd_inv6(D, I)) *S.bad = 1u;             // (every lane that writes, writes the same word)
        st36(S.DP, S.nodes, p, I);
    }
}

__global__ __launch_bounds__(256) void k_pg_red(PgSystem S, uint32_t o, uint32_t ml, uint32_t o2, uint32_t m2) {
    PG_STRIDE(j64, m2) {
        const uint32_t j = static_cast<uint32_t>(j64), i = 2u * j + 1u, p = 2u * j, q = 2u * j + 2u;
        double Dn[6][6], En[6][6], P[6][6], Q[6][6];
        pg_zero(P);
        pg_zero(Q);
        pg_zero(En);
        ld36(S.D, S.nodes, o + i, Dn);
        {
            double Ep[6][6], Dp[6][6];
            ld36(S.E, S.nodes, o + p, Ep);
            ld36(S.DP, S.nodes, o + p, Dp);
            pg_add_atb(Ep, Dp, 1.0, P);                  // P = E_p^T D_p^-1
            pg_add_ab(P, Ep, -1.0, Dn);
        }
        if (q < ml) {
            double Ei[6][6], Dq[6][6];
            ld36(S.E, S.nodes, o + i, Ei);
            ld36(S.DP, S.nodes, o + q, Dq);
            pg_add_ab(Ei, Dq, 1.0, Q);                   // Q = E_i D_q^-1
            pg_add_abt(Q, Ei, -1.0, Dn);
            if (q + 1u < ml) {
                double Eq[6][6];
                ld36(S.E, S.nodes, o + q, Eq);
                pg_add_ab(Q, Eq, -1.0, En);
            }
        }
        st36(S.DP, S.nodes, o + i, P);
        st36(S.Q, S.nodes, o + i, Q);
        st36(S.D, S.nodes, o2 + j, Dn);
        st36(S.E, S.nodes, o2 + j, En);
    }
}

// ---- the apply -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pg_fwd(PgSystem S, uint32_t o, uint32_t ml, uint32_t o2, uint32_t m2, uint32_t K,
                                                double *__restrict__ X) {
    const uint64_t items = static_cast<uint64_t>(m2) * K;
    PG_STRIDE(idx, items) {
        const uint32_t j = static_cast<uint32_t>(idx / K), col = static_cast<uint32_t>(idx % K);
        const uint32_t i = 2u * j + 1u, p = 2u * j, q = 2u * j + 2u;
        double v[6], b[6], M[6][6];
        ldx(X, static_cast<size_t>(o) + i, K, col, v);
        ldx(X, static_cast<size_t>(o) + p, K, col, b);
        ld36(S.DP, S.nodes, o + i, M);
        pg_add_av(M, b, -1.0, v);
        if (q < ml) {
            ldx(X, static_cast<size_t>(o) + q, K, col, b);
            ld36(S.Q, S.nodes, o + i, M);
            pg_add_av(M, b, -1.0, v);
        }
        stx(X, static_cast<size_t>(o2) + j, K, col, v);
    }
}

// level (o, ml) from the solved level at o2 (not read when ml == 1); in place: a lane reads and writes its own node's slot
__global__ __launch_bounds__(256) void k_pg_bwd(PgSystem S, uint32_t o, uint32_t ml, uint32_t o2, uint32_t K,
                                                double *__restrict__ X) {
    const uint64_t items = static_cast<uint64_t>(ml) * K;
    PG_STRIDE(idx, items) {
        const uint32_t node = static_cast<uint32_t>(idx / K), col = static_cast<uint32_t>(idx % K);
        double v[6];
        if (node & 1u) {
            ldx(X, static_cast<size_t>(o2) + (node - 1u) / 2u, K, col, v);
        } else {
            double b[6], M[6][6];
#pragma unroll
            for (int r = 0; r < 6; ++r) v[r] = 0.0;
            ldx(X, static_cast<size_t>(o) + node, K, col, b);
            ld36(S.DP, S.nodes, o + node, M);
            pg_add_av(M, b, 1.0, v);
            if (node >= 1u) {
                ldx(X, static_cast<size_t>(o2) + (node - 2u) / 2u, K, col, b);
                ld36(S.Q, S.nodes, o + node - 1u, M);
                pg_add_atv(M, b, -1.0, v);
            }
            if (node + 1u < ml) {
                ldx(X, static_cast<size_t>(o2) + node / 2u, K, col, b);
                ld36(S.DP, S.nodes, o + node + 1u, M);
                pg_add_atv(M, b, -1.0, v);
            }
        }
        stx(X, static_cast<size_t>(o) + node, K, col, v);
    }
}

// ---- the low-rank part -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pg_rhs_cols(PgGraph G, PgSystem S, uint32_t col0, uint32_t K, double *__restrict__ X) {
    const uint64_t items = static_cast<uint64_t>(G.m) * K;
    PG_STRIDE(idx, items) {
        const uint32_t f = static_cast<uint32_t>(idx / K), col = static_cast<uint32_t>(idx % K), gc = col0 + col;
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (gc == 0u) {
#pragma unroll
            for (int r = 0; r < 6; ++r) v[r] = -S.g[static_cast<size_t>(r) * G.m + f];
        } else if (gc - 1u < 6u * G.c) {
            const uint32_t ce = (gc - 1u) / 6u, sc = (gc - 1u) % 6u, e = G.n - 1u + ce, k = pg_vertex_of(f, G.anchor);
            // U's block row of vertex k in the closure's columns is A^T (B^T): column sc of it is row sc of A (B)
            if (G.ca[ce] == k) {
#pragma unroll
                for (int r = 0; r < 6; ++r) v[r] = S.lin[static_cast<size_t>(sc * 6u + r) * G.E + e];
            } else if (G.cb[ce] == k) {
#pragma unroll
                for (int r = 0; r < 6; ++r) v[r] = S.lin[static_cast<size_t>(36u + sc * 6u + r) * G.E + e];
            }
        }
        stx(X, f, K, col, v);
    }
}

__global__ __launch_bounds__(256) void k_pg_rhs_final(PgGraph G, PgSystem S, const double *__restrict__ z, double *__restrict__ X) {
    PG_STRIDE(f64, G.m) {
        const uint32_t f = static_cast<uint32_t>(f64), k = pg_vertex_of(f, G.anchor);
        double v[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) v[r] = -S.g[static_cast<size_t>(r) * G.m + f];
        for (uint32_t ce = 0; ce < G.c; ++ce) {
            const bool at_a = G.ca[ce] == k, at_b = G.cb[ce] == k;
            if (at_a || at_b) {
                const uint32_t e = G.n - 1u + ce;
                double M[6][6], zz[6];
                ld36(S.lin + (at_a ? size_t(0) : static_cast<size_t>(36) * G.E), G.E, e, M);
#pragma unroll
                for (int s = 0; s < 6; ++s) zz[s] = z[6u * ce + s];
                pg_add_atv(M, zz, -1.0, v);
            }
        }
        stx(X, f, 1u, 0u, v);
    }
}

__global__ __launch_bounds__(256) void k_pg_cap(PgGraph G, PgSystem S, const double *__restrict__ X, uint32_t col0, uint32_t K,
                                                double *__restrict__ Gm) {
    const uint64_t items = static_cast<uint64_t>(6u * G.c) * K;
    const uint32_t ld = 1u + 6u * G.c;
    PG_STRIDE(idx, items) {
        const uint32_t row = static_cast<uint32_t>(idx / K), col = static_cast<uint32_t>(idx % K);
        if (col0 + col >= ld) continue;
        const uint32_t ce = row / 6u, sc = row % 6u, e = G.n - 1u + ce;
        const uint32_t a = G.ca[ce], b = G.cb[ce];
        double sum = 0.0;
        if (a != G.anchor) {
            double x[6];
            ldx(X, pg_free_of(a, G.anchor), K, col, x);
#pragma unroll
            for (int r = 0; r < 6; ++r) sum += S.lin[static_cast<size_t>(sc * 6u + r) * G.E + e] * x[r];
        }
        if (b != G.anchor) {
            double x[6];
            ldx(X, pg_free_of(b, G.anchor), K, col, x);
#pragma unroll
            for (int r = 0; r < 6; ++r) sum += S.lin[static_cast<size_t>(36u + sc * 6u + r) * G.E + e] * x[r];
        }
        Gm[static_cast<size_t>(row) * ld + col0 + col] = sum;
    }
}

// ---- the refinement --------------------------------------------------------------------------------------------------------
// acc += J^T (A d_a + B d_b + w) of edge e = (a, b), J its A (at_a) or B block; delta: 6 per free vertex, the anchor's zero
__device__ __forceinline__ void add_edge_model(const PgGraph &G, const PgSystem &S, const double *__restrict__ delta, uint32_t e,
                                               uint32_t a, uint32_t b, bool at_a, double (&acc)[6]) {
    PgEdgeLin l;
    ld36(S.lin, G.E, e, l.A);
    ld36(S.lin + static_cast<size_t>(36) * G.E, G.E, e, l.B);
    ld6(S.lin + static_cast<size_t>(72) * G.E, G.E, e, l.w);
    double da[6], db[6], t[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        da[i] = a == G.anchor ? 0.0 : delta[static_cast<size_t>(pg_free_of(a, G.anchor)) * 6 + i];
        db[i] = b == G.anchor ? 0.0 : delta[static_cast<size_t>(pg_free_of(b, G.anchor)) * 6 + i];
    }
    pg_edge_model(l, da, db, t);
    if (at_a) pg_add_atv(l.A, t, 1.0, acc);
    else pg_add_atv(l.B, t, 1.0, acc);
}

// a lane per free vertex, its edges in k_pg_asm's order
__global__ __launch_bounds__(256) void k_pg_resid(PgGraph G, PgSystem S, const double *__restrict__ delta, double *__restrict__ q,
                                                  double *__restrict__ X) {
    PG_STRIDE(f64, G.m) {
        const uint32_t f = static_cast<uint32_t>(f64), k = pg_vertex_of(f, G.anchor);
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (k >= 1u) add_edge_model(G, S, delta, k - 1u, k - 1u, k, false, acc);
        if (k + 1u < G.n) add_edge_model(G, S, delta, k, k, k + 1u, true, acc);
        for (uint32_t ce = 0; ce < G.c; ++ce) {
            const uint32_t a = G.ca[ce], b = G.cb[ce];
            if (a == k || b == k) add_edge_model(G, S, delta, G.n - 1u + ce, a, b, a == k, acc);
        }
        double v[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            q[static_cast<size_t>(i) * G.m + f] = acc[i];
            v[i] = -acc[i];
        }
        stx(X, f, 1u, 0u, v);
    }
}

__global__ __launch_bounds__(256) void k_pg_acc(uint64_t count, const double *__restrict__ X, double *__restrict__ delta) {
    PG_STRIDE(i, count) delta[i] += X[i];
}

// ---- the step --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pg_update(PgGraph G, const double *__restrict__ x, const double *__restrict__ delta,
                                                   double step, double *__restrict__ out) {
    PG_STRIDE(k64, G.n) {
        const uint32_t k = static_cast<uint32_t>(k64);
        const double *xk = x + 7 * static_cast<size_t>(k);
        double o[7];
        if (k == G.anchor) {
#pragma unroll
            for (int i = 0; i < 7; ++i) o[i] = xk[i];
        } else {
            const size_t f = pg_free_of(k, G.anchor);
            double xi[7], d[6];
#pragma unroll
            for (int i = 0; i < 7; ++i) xi[i] = xk[i];
#pragma unroll
            for (int i = 0; i < 6; ++i) d[i] = delta[f * 6 + i];
            pg_retract(xi, d, step, o);
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) out[7 * static_cast<size_t>(k) + i] = o[i];
    }
}

template <bool AbsMax>
__device__ __forceinline__ double red_op(double acc, double v) {
    if (AbsMax) {
        v = fabs(v);
        return (v > acc || v != v) ? v : acc;            // a NaN stays
    }
    return acc + v;
}
template <bool AbsMax>
__device__ __forceinline__ double block_tree(double acc) {
    __shared__ double sh[256];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned o = 128; o; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] = red_op<AbsMax>(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    return sh[0];
}
template <bool AbsMax>
__global__ __launch_bounds__(256) void k_pg_red1(const double *__restrict__ v, uint64_t count, double *__restrict__ slabs) {
    double acc = 0.0;
    PG_STRIDE(i, count) acc = red_op<AbsMax>(acc, v[i]);
    const double r = block_tree<AbsMax>(acc);
    if (threadIdx.x == 0) slabs[blockIdx.x] = r;
}
template <bool AbsMax>
__global__ __launch_bounds__(256) void k_pg_red2(const double *__restrict__ slabs, uint32_t nb, double *__restrict__ out) {
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < nb; i += 256) acc = red_op<AbsMax>(acc, slabs[i]);
    const double r = block_tree<AbsMax>(acc);
    if (threadIdx.x == 0) *out = r;
}

inline unsigned grid_for(uint64_t items) {
    return static_cast<unsigned>(std::min<uint64_t>(kPgBlocks, (items + 255) / 256));
}

}  // namespace

hipError_t pg_linearize_all(const PgGraph &G, const double *x, const PgSystem &S, double *edge_cost, hipStream_t s) {
    if (!G.E) return hipSuccess;
    if (G.kernel) hipLaunchKernelGGL(k_pg_lin<true>, dim3(grid_for(G.E)), dim3(256), 0, s, G, x, S.lin, edge_cost);
    else hipLaunchKernelGGL(k_pg_lin<false>, dim3(grid_for(G.E)), dim3(256), 0, s, G, x, S.lin, edge_cost);
    return hipGetLastError();
}

hipError_t pg_cost(const PgGraph &G, const double *x, double *edge_cost, hipStream_t s) {
    if (!G.E) return hipSuccess;
    if (G.kernel) hipLaunchKernelGGL(k_pg_cost<true>, dim3(grid_for(G.E)), dim3(256), 0, s, G, x, edge_cost);
    else hipLaunchKernelGGL(k_pg_cost<false>, dim3(grid_for(G.E)), dim3(256), 0, s, G, x, edge_cost);
    return hipGetLastError();
}

hipError_t pg_assemble(const PgGraph &G, const PgSystem &S, hipStream_t s) {
    if (!G.m) return hipSuccess;
    hipLaunchKernelGGL(k_pg_asm, dim3(grid_for(G.m)), dim3(256), 0, s, G, S);
    return hipGetLastError();
}

hipError_t pg_factor(const PgSystem &S, const PgLevels &lv, hipStream_t s) {
    for (uint32_t l = 0; l < lv.count; ++l) {
        const uint32_t ml = lv.m[l], o = lv.off[l];
        hipLaunchKernelGGL(k_pg_inv, dim3(grid_for((ml + 1u) / 2u)), dim3(256), 0, s, S, o, ml);
        if (l + 1 < lv.count)
            hipLaunchKernelGGL(k_pg_red, dim3(grid_for(lv.m[l + 1])), dim3(256), 0, s, S, o, ml, lv.off[l + 1], lv.m[l + 1]);
    }
    return hipGetLastError();
}

hipError_t pg_rhs_columns(const PgGraph &G, const PgSystem &S, uint32_t col0, uint32_t K, double *X, hipStream_t s) {
    if (!G.m || !K) return hipSuccess;
    hipLaunchKernelGGL(k_pg_rhs_cols, dim3(grid_for(static_cast<uint64_t>(G.m) * K)), dim3(256), 0, s, G, S, col0, K, X);
    return hipGetLastError();
}

hipError_t pg_rhs_final(const PgGraph &G, const PgSystem &S, const double *z, double *X, hipStream_t s) {
    if (!G.m) return hipSuccess;
    hipLaunchKernelGGL(k_pg_rhs_final, dim3(grid_for(G.m)), dim3(256), 0, s, G, S, z, X);
    return hipGetLastError();
}

hipError_t pg_apply(const PgSystem &S, const PgLevels &lv, uint32_t K, double *X, hipStream_t s) {
    if (!lv.count || !K) return hipSuccess;
    for (uint32_t l = 0; l + 1 < lv.count; ++l)
        hipLaunchKernelGGL(k_pg_fwd, dim3(grid_for(static_cast<uint64_t>(lv.m[l + 1]) * K)), dim3(256), 0, s, S, lv.off[l], lv.m[l],
                           lv.off[l + 1], lv.m[l + 1], K, X);
    for (uint32_t l = lv.count; l-- > 0;) {
        const uint32_t o2 = l + 1 < lv.count ? lv.off[l + 1] : 0u;
        hipLaunchKernelGGL(k_pg_bwd, dim3(grid_for(static_cast<uint64_t>(lv.m[l]) * K)), dim3(256), 0, s, S, lv.off[l], lv.m[l], o2, K, X);
    }
    return hipGetLastError();
}

hipError_t pg_capacitance(const PgGraph &G, const PgSystem &S, const double *X, uint32_t col0, uint32_t K, double *Gm, hipStream_t s) {
    if (!G.c || !K) return hipSuccess;
    hipLaunchKernelGGL(k_pg_cap, dim3(grid_for(static_cast<uint64_t>(6u * G.c) * K)), dim3(256), 0, s, G, S, X, col0, K, Gm);
    return hipGetLastError();
}

hipError_t pg_residual(const PgGraph &G, const PgSystem &S, const double *delta, double *q, double *X, hipStream_t s) {
    if (!G.m) return hipSuccess;
    hipLaunchKernelGGL(k_pg_resid, dim3(grid_for(G.m)), dim3(256), 0, s, G, S, delta, q, X);
    return hipGetLastError();
}

hipError_t pg_accumulate(const PgGraph &G, const double *X, double *delta, hipStream_t s) {
    if (!G.m) return hipSuccess;
    const uint64_t count = 6 * static_cast<uint64_t>(G.m);
    hipLaunchKernelGGL(k_pg_acc, dim3(grid_for(count)), dim3(256), 0, s, count, X, delta);
    return hipGetLastError();
}

hipError_t pg_update(const PgGraph &G, const double *x, const double *delta, double step, double *out, hipStream_t s) {
    hipLaunchKernelGGL(k_pg_update, dim3(grid_for(G.n)), dim3(256), 0, s, G, x, delta, step, out);
    return hipGetLastError();
}

hipError_t pg_reduce(const double *v, uint64_t count, bool absmax, double *slabs, double *out, hipStream_t s) {
    const unsigned nb = std::max(1u, grid_for(count));
    if (absmax) {
        hipLaunchKernelGGL(k_pg_red1<true>, dim3(nb), dim3(256), 0, s, v, count, slabs);
        hipLaunchKernelGGL(k_pg_red2<true>, dim3(1), dim3(256), 0, s, slabs, nb, out);
    } else {
        hipLaunchKernelGGL(k_pg_red1<false>, dim3(nb), dim3(256), 0, s, v, count, slabs);
        hipLaunchKernelGGL(k_pg_red2<false>, dim3(1), dim3(256), 0, s, slabs, nb, out);
    }
    return hipGetLastError();
}

}  // namespace sageicp
