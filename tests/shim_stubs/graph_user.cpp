// A caller of the header shim's pose-graph extension (tests/test_posegraph_host.py type-checks it against the stand-in
// Eigen): two places recognised again, both closures optimised at once, the session's map exported re-posed.
#include <array>

#include "sage_icp/core/PoseGraph.hpp"
#include "sage_icp/core/VoxelHashMap.hpp"

std::size_t rows_after_two_closures(const sage_icp::VoxelHashMap &local_map, const std::vector<sage_icp::Pose7> &poses,
                                    const std::vector<Eigen::Vector3d> &positions, const sage_icp::Pose7 &closed_a,
                                    const sage_icp::Pose7 &closed_b, const sage_icp::Information &info) {
    std::vector<sage_icp::GraphEdge> closures;
    closures.push_back(sage_icp::GraphEdge::FromClosed(poses, 0, poses.size() - 1, closed_a, info));
    closures.push_back(sage_icp::GraphEdge::FromClosed(poses, 5, poses.size() - 3, closed_b, info));
    closures.emplace_back(1, 2, sage_icp::Pose7{0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0}, info);
    sageicp_graph_params params;
    sageicp_graph_params_default(&params);
    params.where = 1;
    const sage_icp::GraphResult r = sage_icp::OptimizeGraph(poses, closures, info, &params);
    return local_map.CorrectedPointcloud(positions, r.corrections).size() + r.info.iterations;
}
