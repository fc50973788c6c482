// OPTIONAL replacement for the reference header cpp/sage_icp/core/Preprocessing.hpp
// (NeSC-IV/sage-icp @ 2024_10_08, lines 33-45): the same two free functions, running on the
// MI355X through the C ABI of libsageicp_hip.so (preprocess.hip).
//
// Opt-in: this header lives in its own include root (sage-icp_amd/shim_preprocessing) and is NOT
// part of the drop-in for the registration hot path.  Adding that root moves Preprocess() and
// VoxelDownsample() onto the GPU for every configuration of the reference's launch files: with
// dynamic_vehicle_filter == true (the default SemanticKITTI launches, ros/launch/odometry.launch.py:50
// and its _360 / _raw variants) Preprocess() runs the Euclidean-clustering vehicle filter of
// Preprocessing.cpp:95-172 on the device (sageicp_preprocess_dynamic; no PCL needed), with it false
// (odometry_gt.launch.py) the crop of :173-187.  Deskewing (core/Deskew.cpp) is not part of this header.
// VoxelDownsample() returns the survivors in the reference's order — the bucket order of its
// tsl::robin_map, replayed by the library (csrc/robin_order.hpp) — unless
// sageicp_set_downsample_order(0) selects the faster group-by-group input order.
#pragma once

#include <Eigen/Core>
#include <stdexcept>
#include <string>
#include <vector>

#include "sage_icp/core/VoxelHashMap.hpp"
#include "sageicp.h"

namespace sage_icp {

// core/Preprocessing.cpp:44-84
inline std::vector<Eigen::Vector4d> VoxelDownsample(const std::vector<Eigen::Vector4d> &frame,
                                                    const std::vector<std::vector<int>> &voxel_labels,
                                                    const std::vector<double> &voxel_size,
                                                    double vox_scale) {
    std::vector<int> counts, labels;
    for (const auto &g : voxel_labels) {
        counts.push_back(static_cast<int>(g.size()));
        labels.insert(labels.end(), g.begin(), g.end());
    }
    std::vector<Eigen::Vector4d> out(frame.size());
    uint64_t n = 0;
    if (sageicp_voxel_downsample(frame.empty() ? nullptr : frame.front().data(), frame.size(),
                                 static_cast<int>(voxel_size.size()), counts.data(), labels.data(),
                                 voxel_size.data(), vox_scale,
                                 out.empty() ? nullptr : out.front().data(), &n,
                                 VoxelHashMap::Device()) != SAGEICP_OK)
        throw std::runtime_error(std::string("sage_icp::VoxelDownsample: ") + sageicp_last_error());
    out.resize(n);
    return out;
}

// core/Preprocessing.cpp:86-187
inline std::vector<Eigen::Vector4d> Preprocess(const std::vector<Eigen::Vector4d> &frame,
                                               double max_range, double min_range,
                                               double label_max_range, bool dynamic_vehicle_filter,
                                               double dy_th, const std::vector<int> &dynamic_labels,
                                               const std::vector<int> &lankmark) {
    std::vector<Eigen::Vector4d> out(frame.size());
    uint64_t n = 0;
    const double *in = frame.empty() ? nullptr : frame.front().data();
    double *o = out.empty() ? nullptr : out.front().data();
    const int rc = dynamic_vehicle_filter
                       ? sageicp_preprocess_dynamic(in, frame.size(), max_range, min_range, label_max_range, dy_th,
                                                    dynamic_labels.data(), static_cast<int>(dynamic_labels.size()),
                                                    lankmark.data(), static_cast<int>(lankmark.size()), o, &n,
                                                    nullptr, VoxelHashMap::Device())
                       : sageicp_preprocess(in, frame.size(), max_range, min_range, label_max_range, o, &n,
                                            VoxelHashMap::Device());
    if (rc != SAGEICP_OK) throw std::runtime_error(std::string("sage_icp::Preprocess: ") + sageicp_last_error());
    out.resize(n);
    return out;
}

}  // namespace sage_icp
