// OPTIONAL replacement for the reference header cpp/sage_icp/core/Deskew.hpp (lines 32-35): the same free function,
// running on the MI355X through the C ABI of libsageicp_hip.so (deskew.hip, sageicp_deskew_scan).
//
// Opt-in: this header lives in its own include root (sage-icp_amd/shim_deskew), like shim_preprocessing.  With that
// root added and core/Deskew.cpp dropped from the build, the reference's pipeline (pipeline/sageICP.cpp:36-52) deskews
// on the GPU when its config sets deskew: true.  delta = (start_pose.inverse() * finish_pose).log() is formed on the
// host with the library's SE(3) restatement, each point is moved on the device by exp((t - 0.5) * delta) — the
// exponential and point action of the ICP update.  Unlike the reference, a non-finite timestamp, pose
// or point, or fewer timestamps than points, throws instead of being undefined behaviour.
#pragma once

#include <Eigen/Core>
#include <sophus/se3.hpp>
#include <stdexcept>
#include <string>
#include <vector>

#include "sage_icp/core/VoxelHashMap.hpp"
#include "sageicp.h"

namespace sage_icp {

// core/Deskew.cpp:31-50
inline std::vector<Eigen::Vector4d> DeSkewScan(const std::vector<Eigen::Vector4d> &frame,
                                               const std::vector<double> &timestamps,
                                               const Sophus::SE3d &start_pose,
                                               const Sophus::SE3d &finish_pose) {
    if (timestamps.size() < frame.size())
        throw std::runtime_error("sage_icp::DeSkewScan: fewer timestamps than points");
    std::vector<Eigen::Vector4d> out(frame.size());
    if (sageicp_deskew_scan(frame.empty() ? nullptr : frame.front().data(),
                            timestamps.empty() ? nullptr : timestamps.data(), frame.size(), start_pose.data(),
                            finish_pose.data(), out.empty() ? nullptr : out.front().data(),
                            VoxelHashMap::Device()) != SAGEICP_OK)
        throw std::runtime_error(std::string("sage_icp::DeSkewScan: ") + sageicp_last_error());
    return out;
}

}  // namespace sage_icp
