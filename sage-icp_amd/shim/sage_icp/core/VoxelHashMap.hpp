// Drop-in replacement for the reference header cpp/sage_icp/core/VoxelHashMap.hpp
// (NeSC-IV/sage-icp @ 2024_10_08, lines 35-107): the same `sage_icp::VoxelHashMap` value type —
// constructor, member functions and public data members — implemented over the C ABI of
// libsageicp_hip.so (include/sageicp.h).  pipeline/sageICP.{hpp,cpp} and
// ros/ros2/OdometryServer.cpp compile against it unchanged; only the `map_` member (a
// tsl::robin_map in the reference, touched by nothing outside the struct) is replaced by an
// opaque handle to the host-authoritative map + HBM mirror.
//
// Value semantics are preserved: copy construction / copy assignment deep-copy the map
// (sageicp_map_clone) as OdometryServer.cpp:104 (`odometry_ = sageICP(config_)`) requires.
// A HIP failure has no analogue in the reference (its hot path has no error channel), so a
// non-zero ABI return is surfaced as std::runtime_error.
#pragma once

#include <Eigen/Core>
#include <sophus/se3.hpp>
#include <array>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "sageicp.h"

namespace sage_icp {

struct VoxelHashMap {
    using Vector4dVector = std::vector<Eigen::Vector4d>;
    using Vector4dVectorTuple = std::tuple<Vector4dVector, Vector4dVector>;
    using Voxel = Eigen::Vector3i;

    explicit VoxelHashMap(double voxel_size, double max_distance, int basic_points_per_voxel,
                          int critical_points_per_voxel, std::vector<int> basic_parts_labels)
        : voxel_size_(voxel_size),
          max_distance_(max_distance),
          basic_points_per_voxel_(basic_points_per_voxel),
          critical_points_per_voxel_{critical_points_per_voxel},
          basic_parts_labels_{std::move(basic_parts_labels)},
          map_(sageicp_map_create(voxel_size_, max_distance_, basic_points_per_voxel_,
                                  critical_points_per_voxel_, basic_parts_labels_.data(),
                                  static_cast<int>(basic_parts_labels_.size()), Device())) {
        if (!map_) throw std::runtime_error(std::string("sageicp_map_create: ") + sageicp_last_error());
#ifndef SAGE_ICP_SHIM_FAST_MAP
        // The drop-in node keeps the voxels the reference keeps: RemovePointsFarFromLocation erases while it
        // iterates its robin_map (VoxelHashMap.cpp:176-184), so the entry a deletion shifts into the bucket just
        // erased survives until a later frame, and Pointcloud() lists bucket order (:132-142).  A map in
        // reference-order mode reproduces both exactly (include/sageicp.h, sageicp_map_set_reference_order); since
        // round 6 its Update() runs on the GPU as well — the device inserts and finds the far voxels, the host replays
        // only the voxels concerned on its copy of the bucket array — at 0.38 ms per streamed frame against 0.25 ms
        // for -DSAGE_ICP_SHIM_FAST_MAP (every out-of-range voxel removed at once, block-pool order); poses are the
        // same on every stream measured.
        if (sageicp_map_set_reference_order(map_, 1) != 0) {
            const std::string why = sageicp_last_error();
            sageicp_map_destroy(map_);
            map_ = nullptr;
            throw std::runtime_error("sageicp_map_set_reference_order: " + why);
        }
#endif
    }

    VoxelHashMap(const VoxelHashMap &o)
        : voxel_size_(o.voxel_size_),
          max_distance_(o.max_distance_),
          basic_points_per_voxel_(o.basic_points_per_voxel_),
          critical_points_per_voxel_(o.critical_points_per_voxel_),
          basic_parts_labels_(o.basic_parts_labels_),
          map_(sageicp_map_clone(o.map_)) {
        // a failed clone (HIP out of memory, device error) must not pass for an empty map
        if (!map_) throw std::runtime_error(std::string("sageicp_map_clone: ") + sageicp_last_error());
    }
    VoxelHashMap(VoxelHashMap &&o) noexcept
        : voxel_size_(o.voxel_size_),
          max_distance_(o.max_distance_),
          basic_points_per_voxel_(o.basic_points_per_voxel_),
          critical_points_per_voxel_(o.critical_points_per_voxel_),
          basic_parts_labels_(std::move(o.basic_parts_labels_)),
          map_(o.map_) {
        o.map_ = nullptr;
    }
    VoxelHashMap &operator=(VoxelHashMap o) noexcept {   // copy-and-swap: copy and move assignment
        swap(o);
        return *this;
    }
    ~VoxelHashMap() { sageicp_map_destroy(map_); }

    // core/VoxelHashMap.cpp:48-130
    Vector4dVectorTuple GetCorrespondences(const Vector4dVector &points,
                                           double max_correspondance_distance, double th) const {
        Vector4dVector src(points.size()), tgt(points.size());
        uint64_t n = 0;
        Check(sageicp_get_correspondences(map_, Data(points), points.size(),
                                          max_correspondance_distance, th, Data(src), Data(tgt), &n,
                                          nullptr),
              "GetCorrespondences");
        src.resize(n);
        tgt.resize(n);
        return std::make_tuple(std::move(src), std::move(tgt));
    }
    inline void Clear() { Check(sageicp_map_clear(map_), "Clear"); }
    inline bool Empty() const { return sageicp_map_empty(map_) != 0; }
    void Update(const Vector4dVector &points, const Eigen::Vector3d &origin) {
        Check(sageicp_map_update(map_, Data(points), points.size(), origin.data()), "Update");
    }
    // the per-frame map update (pipeline/sageICP.cpp:89) runs on the GPU against the HBM-resident
    // map; same voxel blocks as the host entry sageicp_map_update_pose()
    void Update(const Vector4dVector &points, const Sophus::SE3d &pose) {
        Check(sageicp_map_update_pose_device(map_, Data(points), points.size(), pose.data()), "Update");
    }
    void AddPoints(const Vector4dVector &points) {
        Check(sageicp_map_add_points(map_, Data(points), points.size()), "AddPoints");
    }
    void RemovePointsFarFromLocation(const Eigen::Vector3d &origin) {
        Check(sageicp_map_remove_far(map_, origin.data()), "RemovePointsFarFromLocation");
    }
    Vector4dVector Pointcloud() const {
        Vector4dVector out(sageicp_map_size(map_));
        sageicp_map_pointcloud(map_, Data(out), out.size());
        return out;
    }

    double voxel_size_;
    double max_distance_;
    int basic_points_per_voxel_;
    int critical_points_per_voxel_;
    std::vector<int> basic_parts_labels_;

    // ---- not part of the reference surface -------------------------------------------------
    const sageicp_map *handle() const { return map_; }     // used by the Registration.hpp shim
    // The archive (include/sageicp.h; SAGEICP_MAP_ARCHIVE=1 switches it on for a caller that cannot be changed): every
    // voxel the map evicted, as recorded, and the session's map — the latest generation of every evicted voxel the map
    // does not hold, then Pointcloud().
    Vector4dVector ArchivedPointcloud() const { return ArchiveRows(SAGEICP_ARCHIVE_ALL, "ArchivedPointcloud"); }
    Vector4dVector SessionPointcloud() const { return ArchiveRows(SAGEICP_SESSION, "SessionPointcloud"); }
    // The session's map after a loop closure (include/sageicp.h "loop closure"): SessionPointcloud()'s rows,
    // each moved by the correction of the pose its voxel belongs to.  positions[s]: the sensor position of the update with
    // serial s; corrections[s]: C_s of sageicp_closure_corrections as (qx, qy, qz, qw, tx, ty, tz), one per position.
    Vector4dVector CorrectedPointcloud(const std::vector<Eigen::Vector3d> &positions,
                                       const std::vector<std::array<double, 7>> &corrections) const {
        if (positions.empty() || positions.size() != corrections.size())
            throw std::runtime_error("sage_icp::VoxelHashMap::CorrectedPointcloud: one correction per position, at least one");
        const double *pos = positions.front().data(), *corr = corrections.front().data();
        uint64_t n = 0;
        Check(sageicp_map_session_corrected(map_, SAGEICP_SESSION, 0, pos, corr, positions.size(), nullptr, 0, &n),
              "CorrectedPointcloud");
        Vector4dVector out(n);
        Check(sageicp_map_session_corrected(map_, SAGEICP_SESSION, 0, pos, corr, positions.size(), Data(out), out.size(), &n),
              "CorrectedPointcloud");
        return out;
    }
    // Recall (include/sageicp.h): the voxels of the session's map whose first point lies within `radius` of
    // `center`, as a map of max_distance = radius that can be searched — what Relocalize takes when a place was
    // recognised after the local map evicted it.  The returned map is filled on the device and is in block-pool order
    // (a recall's destination is never in reference-order mode).
    VoxelHashMap Recall(const Eigen::Vector3d &center, double radius) const {
        sageicp_map *dst = sageicp_map_create(voxel_size_, radius, basic_points_per_voxel_, critical_points_per_voxel_,
                                              basic_parts_labels_.data(), static_cast<int>(basic_parts_labels_.size()), Device());
        if (!dst) throw std::runtime_error(std::string("sageicp_map_create: ") + sageicp_last_error());
        int rc = sageicp_map_set_reference_order(dst, 0);      // (SAGEICP_MAP_REFERENCE_ORDER=1 would have switched it on)
        if (rc == SAGEICP_OK) rc = sageicp_map_recall(map_, center.data(), radius, dst, nullptr);
        if (rc != SAGEICP_OK) {
            const std::string why = sageicp_last_error();
            sageicp_map_destroy(dst);
            throw std::runtime_error("sage_icp::VoxelHashMap::Recall: " + why);
        }
        return VoxelHashMap(*this, radius, dst);
    }
    // The session rebuilt (include/sageicp.h "session rebuild"): CorrectedPointcloud()'s rows voxelised
    // again under this map's retention policy, on the device, as a map that can be searched — a street driven twice is in
    // it once.  With (center, radius): only the voxels whose first point lies within `radius` of `center`, as a map of
    // max_distance = radius; without: everything, max_distance as this map's.  Block-pool order, like Recall's.
    VoxelHashMap RebuiltMap(const std::vector<Eigen::Vector3d> &positions, const std::vector<std::array<double, 7>> &corrections) const {
        return Rebuilt(positions, corrections, nullptr, max_distance_);
    }
    VoxelHashMap RebuiltMap(const std::vector<Eigen::Vector3d> &positions, const std::vector<std::array<double, 7>> &corrections,
                            const Eigen::Vector3d &center, double radius) const {
        return Rebuilt(positions, corrections, center.data(), radius);
    }
    // HIP device ordinal for maps created by this process (one process per GPU); set it before
    // the first map is constructed, e.g. from LOCAL_RANK.
    static int &Device() {
        // the library this process loaded must speak the ABI this header was written against
        // (struct layouts are part of it): checked once, before the first map exists
        static const bool abi_ok = [] {
            if (sageicp_abi_version() != SAGEICP_ABI_VERSION)
                throw std::runtime_error("libsageicp_hip.so speaks ABI version " +
                                         std::to_string(sageicp_abi_version()) + ", the header shim " +
                                         std::to_string(SAGEICP_ABI_VERSION));
            return true;
        }();
        (void)abi_ok;
        static int device = 0;
        return device;
    }

private:
    // a handle that already exists, with the parameters of `like` (Recall)
    VoxelHashMap(const VoxelHashMap &like, double max_distance, sageicp_map *handle)
        : voxel_size_(like.voxel_size_),
          max_distance_(max_distance),
          basic_points_per_voxel_(like.basic_points_per_voxel_),
          critical_points_per_voxel_(like.critical_points_per_voxel_),
          basic_parts_labels_(like.basic_parts_labels_),
          map_(handle) {}
    // Eigen::Vector4d is four contiguous doubles, so a vector of them is the ABI's double[n][4]
    static const double *Data(const Vector4dVector &v) { return v.empty() ? nullptr : v.front().data(); }
    static double *Data(Vector4dVector &v) { return v.empty() ? nullptr : v.front().data(); }
    static void Check(int rc, const char *what) {
        if (rc != SAGEICP_OK)
            throw std::runtime_error(std::string("sage_icp::VoxelHashMap::") + what + ": " +
                                     sageicp_last_error());
    }
    VoxelHashMap Rebuilt(const std::vector<Eigen::Vector3d> &positions, const std::vector<std::array<double, 7>> &corrections,
                         const double *center, double radius) const {
        if (positions.empty() || positions.size() != corrections.size())
            throw std::runtime_error("sage_icp::VoxelHashMap::RebuiltMap: one correction per position, at least one");
        sageicp_map *dst = sageicp_map_create(voxel_size_, radius, basic_points_per_voxel_, critical_points_per_voxel_,
                                              basic_parts_labels_.data(), static_cast<int>(basic_parts_labels_.size()), Device());
        if (!dst) throw std::runtime_error(std::string("sageicp_map_create: ") + sageicp_last_error());
        const int rc = sageicp_map_session_rebuild(map_, SAGEICP_SESSION, positions.front().data(), corrections.front().data(),
                                                   positions.size(), center, radius, dst, nullptr);
        if (rc != SAGEICP_OK) {
            const std::string why = sageicp_last_error();
            sageicp_map_destroy(dst);
            throw std::runtime_error("sage_icp::VoxelHashMap::RebuiltMap: " + why);
        }
        return VoxelHashMap(*this, radius, dst);
    }
    Vector4dVector ArchiveRows(int which, const char *what) const {
        uint64_t n = 0;
        Check(sageicp_map_archive_rows(map_, which, 0, nullptr, 0, &n), what);
        Vector4dVector out(n);
        Check(sageicp_map_archive_rows(map_, which, 0, Data(out), out.size(), &n), what);
        return out;
    }
    void swap(VoxelHashMap &o) noexcept {
        std::swap(voxel_size_, o.voxel_size_);
        std::swap(max_distance_, o.max_distance_);
        std::swap(basic_points_per_voxel_, o.basic_points_per_voxel_);
        std::swap(critical_points_per_voxel_, o.critical_points_per_voxel_);
        basic_parts_labels_.swap(o.basic_parts_labels_);
        std::swap(map_, o.map_);
    }

    sageicp_map *map_;
};

}  // namespace sage_icp
