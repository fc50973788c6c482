// A caller of the header shim's robust pose-graph extension (tests/test_posegraph_robust_host.py type-checks it against the
// stand-in Eigen): two places recognised again, one of them possibly a false match; each edge's information from the quality
// report of its relocalisation, the closures optimised under a redescending kernel, the rejected match counted out.
#include <array>

#include "sage_icp/core/PoseGraph.hpp"
#include "sage_icp/core/VoxelHashMap.hpp"

std::size_t rows_after_robust_closures(const sage_icp::VoxelHashMap &local_map, const std::vector<sage_icp::Pose7> &poses,
                                       const std::vector<Eigen::Vector3d> &positions, const sage_icp::Pose7 &closed_a,
                                       const sageicp_quality &quality_a, const sage_icp::Pose7 &closed_b,
                                       const sageicp_quality &quality_b, const sage_icp::Information &odom_info) {
    std::vector<sage_icp::GraphEdge> closures;
    closures.push_back(sage_icp::GraphEdge::FromClosed(poses, 0, poses.size() - 1, closed_a,
                                                       sage_icp::EdgeInfoFromQuality(quality_a, closed_a, 0.01)));
    closures.push_back(sage_icp::GraphEdge::FromClosed(poses, 5, poses.size() - 3, closed_b, sage_icp::EdgeInfoFromQuality(quality_b, closed_b)));
    sageicp_graph_params params;
    sageicp_graph_params_default(&params);
    params.where = 1;
    const sage_icp::RobustGraphResult r = sage_icp::OptimizeGraph(poses, closures, odom_info, sage_icp::RobustKernel::GemanMcClure(), &params);
    std::size_t kept = 0;
    for (double w : r.closure_weight) kept += w >= 0.5 ? 1u : 0u;
    const sage_icp::RobustGraphResult h = sage_icp::OptimizeGraph(poses, closures, odom_info, sage_icp::RobustKernel::Huber(3.0));
    const sage_icp::RobustGraphResult c = sage_icp::OptimizeGraph(poses, closures, odom_info, sage_icp::RobustKernel::Cauchy());
    return local_map.CorrectedPointcloud(positions, r.corrections).size() + kept + r.robust_info.outliers + h.info.iterations +
           c.closure_chi2.size();
}
