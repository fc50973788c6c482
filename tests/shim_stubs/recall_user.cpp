// A caller of the header shim's Recall extension (tests/test_recall_host.py type-checks it against the stand-in Eigen):
// a place recognised after the local map evicted it is recalled from the session's map and searched.
#include <tuple>

#include "sage_icp/core/VoxelHashMap.hpp"

std::size_t correspondences_at_a_recalled_place(const sage_icp::VoxelHashMap &local_map, const Eigen::Vector3d &place, double radius,
                                                const std::vector<Eigen::Vector4d> &scan) {
    const sage_icp::VoxelHashMap recalled = local_map.Recall(place, radius);
    const auto pairs = recalled.GetCorrespondences(scan, 1.0, 0.5);
    return std::get<0>(pairs).size() + recalled.Pointcloud().size();
}
