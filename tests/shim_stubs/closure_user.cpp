// A caller of the header shim's CorrectedPointcloud extension (tests/test_closure_host.py type-checks it against the
// stand-in Eigen): after a loop closure the session's map is exported with every voxel moved by the correction of the
// pose it was seen from.
#include <array>

#include "sage_icp/core/VoxelHashMap.hpp"

std::size_t rows_of_the_corrected_session(const sage_icp::VoxelHashMap &local_map, const std::vector<Eigen::Vector3d> &positions,
                                          const std::vector<std::array<double, 7>> &corrections) {
    const std::vector<Eigen::Vector4d> corrected = local_map.CorrectedPointcloud(positions, corrections);
    return corrected.size() - local_map.SessionPointcloud().size();
}
