// A caller of the header shim's RebuiltMap extension (tests/test_rebuild_host.py type-checks it against the stand-in Eigen):
// after a loop closure the corrected session is rebuilt into a map, whole and around a place, and searched.
#include <array>
#include <tuple>
#include <vector>

#include "sage_icp/core/VoxelHashMap.hpp"

std::size_t correspondences_against_the_rebuilt_session(const sage_icp::VoxelHashMap &local_map,
                                                        const std::vector<Eigen::Vector3d> &positions,
                                                        const std::vector<std::array<double, 7>> &corrections,
                                                        const Eigen::Vector3d &place, double radius,
                                                        const std::vector<Eigen::Vector4d> &scan) {
    const sage_icp::VoxelHashMap whole = local_map.RebuiltMap(positions, corrections);
    const sage_icp::VoxelHashMap around = local_map.RebuiltMap(positions, corrections, place, radius);
    const auto pairs = around.GetCorrespondences(scan, 1.0, 0.5);
    return std::get<0>(pairs).size() + whole.Pointcloud().size();
}
