// Header shim for the pose-graph optimiser of libsageicp_hip.so (include/sageicp.h "pose graph"): several
// loop closures minimised at once.  Poses and corrections are (qx, qy, qz, qw, tx, ty, tz), as VoxelHashMap's
// CorrectedPointcloud takes them: the corrections returned here go straight into it.
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "sageicp.h"

namespace sage_icp {

using Pose7 = std::array<double, 7>;
using Information = std::array<double, 36>;      // row-major 6x6, symmetric positive definite, tangent (upsilon, omega)

// A closure of the graph: pose b seen from pose a, z = T_a_b.
struct GraphEdge {
    sageicp_graph_edge edge{};
    GraphEdge() = default;
    GraphEdge(uint64_t a, uint64_t b, const Pose7 &z, const Information &info) {
        edge.a = a;
        edge.b = b;
        for (std::size_t k = 0; k < 7; ++k) edge.z[k] = z[k];
        for (std::size_t k = 0; k < 36; ++k) edge.info[k] = info[k];
    }
    // "pose j really is at `closed`, in pose i's frame of the world": what Relocalize returns against a map recalled
    // around pose i (sageicp_graph_edge_from_closed)
    static GraphEdge FromClosed(const std::vector<Pose7> &poses, uint64_t i, uint64_t j, const Pose7 &closed, const Information &info) {
        GraphEdge e;
        if (poses.empty() || sageicp_graph_edge_from_closed(poses.front().data(), poses.size(), i, j, closed.data(), info.data(), &e.edge) != SAGEICP_OK)
            throw std::runtime_error(std::string("sage_icp::GraphEdge::FromClosed: ") + sageicp_last_error());
        return e;
    }
};
static_assert(sizeof(GraphEdge) == sizeof(sageicp_graph_edge), "a vector of GraphEdge is an array of sageicp_graph_edge");

struct GraphResult {
    std::vector<Pose7> corrections, poses;
    sageicp_graph_info info{};
};

// poses optimised under their own odometry (information odom_info for every edge) and all closures; params: NULL = defaults
inline GraphResult OptimizeGraph(const std::vector<Pose7> &poses, const std::vector<GraphEdge> &closures, const Information &odom_info,
                                 const sageicp_graph_params *params = nullptr) {
    GraphResult r;
    r.corrections.resize(poses.size());
    r.poses.resize(poses.size());
    const sageicp_graph_edge *cl = closures.empty() ? nullptr : &closures.front().edge;
    const int rc = poses.empty() ? SAGEICP_ERR_INVALID
                                 : sageicp_graph_optimize(poses.front().data(), poses.size(), odom_info.data(), 0, cl,
                                                          static_cast<uint32_t>(closures.size()), nullptr, params, r.poses.front().data(),
                                                          r.corrections.front().data(), &r.info);
    if (rc != SAGEICP_OK) throw std::runtime_error(std::string("sage_icp::OptimizeGraph: ") + (poses.empty() ? "no poses" : sageicp_last_error()));
    return r;
}

// ---- robust kernels on the closures; an edge's information from a quality report ----------------------------
// The kernel a false place match is down-weighted by.  Huber bounds its pull; Cauchy and GemanMcClure reject it.
struct RobustKernel {
    sageicp_graph_robust robust{};
    RobustKernel() { sageicp_graph_robust_default(&robust); }
    static RobustKernel Huber(double scale = 0.0) { return Of(SAGEICP_GRAPH_KERNEL_HUBER, scale, false); }
    static RobustKernel Cauchy(double scale = 0.0, bool anneal = false) { return Of(SAGEICP_GRAPH_KERNEL_CAUCHY, scale, anneal); }
    static RobustKernel GemanMcClure(double scale = 0.0, bool anneal = true) { return Of(SAGEICP_GRAPH_KERNEL_GM, scale, anneal); }

private:
    static RobustKernel Of(uint32_t kernel, double scale, bool anneal) {      // scale 0: the default (chi-square, 6 dof, 99 %)
        RobustKernel k;
        k.robust.kernel = kernel;
        k.robust.anneal = anneal ? 1u : 0u;
        if (scale != 0.0) k.robust.scale = scale;
        return k;
    }
};

struct RobustGraphResult : GraphResult {
    std::vector<double> closure_chi2, closure_weight;            // per closure, in the caller's order; weight < 0.5: drop the match
    sageicp_graph_robust_info robust_info{};
};

inline RobustGraphResult OptimizeGraph(const std::vector<Pose7> &poses, const std::vector<GraphEdge> &closures, const Information &odom_info,
                                       const RobustKernel &kernel, const sageicp_graph_params *params = nullptr) {
    RobustGraphResult r;
    r.corrections.resize(poses.size());
    r.poses.resize(poses.size());
    r.closure_chi2.resize(closures.size() + 1);
    r.closure_weight.resize(closures.size() + 1);
    const sageicp_graph_edge *cl = closures.empty() ? nullptr : &closures.front().edge;
    const int rc = poses.empty() ? SAGEICP_ERR_INVALID
                                 : sageicp_graph_optimize_robust(poses.front().data(), poses.size(), odom_info.data(), 0, cl,
                                                                 static_cast<uint32_t>(closures.size()), nullptr, params,
                                                                 r.poses.front().data(), r.corrections.front().data(), &r.info,
                                                                 &kernel.robust, r.closure_chi2.data(), r.closure_weight.data(),
                                                                 &r.robust_info);
    if (rc != SAGEICP_OK) throw std::runtime_error(std::string("sage_icp::OptimizeGraph: ") + (poses.empty() ? "no poses" : sageicp_last_error()));
    r.closure_chi2.resize(closures.size());
    r.closure_weight.resize(closures.size());
    return r;
}

// The information of the edge FromClosed makes of `closed`, from the quality report at `closed` (Relocalize's);
// gain: the caller's noise model (ICP covariances are overconfident)
inline Information EdgeInfoFromQuality(const sageicp_quality &quality, const Pose7 &closed, double gain = 1.0) {
    Information info{};
    if (sageicp_graph_info_from_quality(&quality, closed.data(), gain, info.data()) != SAGEICP_OK)
        throw std::runtime_error(std::string("sage_icp::EdgeInfoFromQuality: ") + sageicp_last_error());
    return info;
}

}  // namespace sage_icp
