// The field-name rules of sage-icp_amd/shim_ros/sageicp_msg.hpp on a stub message type (no ROS headers), the way a node
// would use it (tests/test_pointcloud2_host.py).  Prints one line per case: "<case> ok ..." or "<case> error: <text>".
// No device is needed: layouts, the output's field table, and an empty frame through the C ABI.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <map>
#include <string>
#include <vector>

#include "sageicp_msg.hpp"

namespace stub {
struct PointField {
    std::string name;
    uint32_t offset = 0;
    uint8_t datatype = 0;
    uint32_t count = 0;
};
struct PointCloud2 {
    uint32_t height = 1, width = 0;
    std::vector<PointField> fields;
    bool is_bigendian = false;
    uint32_t point_step = 0, row_step = 0;
    std::vector<uint8_t> data;
};
}  // namespace stub

using sageicp::msg::kFloat32;
using sageicp::msg::kFloat64;
using sageicp::msg::kUint32;
using sageicp::msg::kUint8;

static stub::PointCloud2 make(std::vector<stub::PointField> fields, uint32_t step) {
    stub::PointCloud2 m;
    m.fields = std::move(fields);
    m.point_step = step;
    return m;
}

static void show(const char *name, const stub::PointCloud2 &m, bool want_time) {
    try {
        const sageicp_msg_layout l = sageicp::msg::layout_of(m, want_time);
        std::printf("%s ok step=%u x=%u y=%u z=%u label=%u/%d time=%d/%u\n", name, l.point_step, l.x_offset, l.y_offset,
                    l.z_offset, l.label_offset, l.label_dtype, l.time_kind, l.time_offset);
    } catch (const std::exception &e) {
        std::printf("%s error: %s\n", name, e.what());
    }
}

int main() {
    const std::vector<stub::PointField> xyz = {{"x", 0, kFloat32, 1}, {"y", 4, kFloat32, 1}, {"z", 8, kFloat32, 1}};
    auto with = [&](std::vector<stub::PointField> more) {
        std::vector<stub::PointField> f = xyz;
        f.insert(f.end(), more.begin(), more.end());
        return f;
    };
    // five fields: a UINT8 label; another count: a FLOAT32 label
    show("five_u8", make(with({{"label", 12, kUint8, 1}, {"rgb", 13, kUint32, 1}}), 21), false);
    show("five_f32", make(with({{"label", 12, kFloat32, 1}, {"rgb", 16, kUint32, 1}}), 20), false);
    show("four_f32", make(with({{"label", 12, kFloat32, 1}}), 16), false);
    show("four_u8", make(with({{"label", 12, kUint8, 1}}), 13), false);
    show("x_f64", make({{"x", 0, kFloat64, 1}, {"y", 8, kFloat32, 1}, {"z", 12, kFloat32, 1}, {"label", 16, kFloat32, 1}}, 20), false);
    show("no_label", make(xyz, 12), false);
    // the time field: the last of t / timestamp / time wins
    const auto six = with({{"label", 12, kFloat32, 1}, {"t", 16, kUint32, 1}, {"time", 24, kFloat64, 1}});
    show("last_time", make(six, 32), true);
    show("time_not_asked", make(six, 32), false);
    show("last_t", make(with({{"label", 12, kFloat32, 1}, {"time", 16, kFloat64, 1}, {"timestamp", 24, kUint32, 1}}), 28), true);
    show("no_time", make(with({{"label", 12, kFloat32, 1}}), 16), true);
    // (x, y, z, label and one more are five fields: these carry a ring field as well)
    show("t_f64", make(with({{"label", 12, kFloat32, 1}, {"ring", 16, kUint8, 1}, {"t", 20, kFloat64, 1}}), 28), true);
    show("time_u32", make(with({{"label", 12, kFloat32, 1}, {"ring", 16, kUint8, 1}, {"time", 20, kUint32, 1}}), 24), true);
    show("five_with_t", make(with({{"label", 12, kUint8, 1}, {"t", 16, kUint32, 1}}), 20), true);
    {
        stub::PointCloud2 m = make(with({{"label", 12, kFloat32, 1}}), 16);
        m.is_bigendian = true;
        show("bigendian", m, false);
    }
    // the outgoing message
    stub::PointCloud2 out;
    sageicp::msg::prepare_output(out, 7);
    std::printf("prepare_output step=%u width=%u height=%u row_step=%u data=%zu fields=", out.point_step, out.width,
                out.height, out.row_step, out.data.size());
    for (const auto &f : out.fields) std::printf("%s:%u:%d:%u,", f.name.c_str(), f.offset, static_cast<int>(f.datatype), f.count);
    std::printf("\n");
    // ... is read back as a five-field message
    show("round_trip", out, false);
    const std::map<int, int> color_list = {{0, 0}, {40, 0xff00ff}, {300, 5}};
    const sageicp::msg::Colors colors(color_list);
    std::printf("colors n=%u\n", colors.get().n);

    // an empty frame through the wrapper: a pose is pushed, nothing needs a device
    const int basic[1] = {40};
    const int counts[1] = {1}, labels[1] = {40};
    const double sizes[1] = {1.0};
    sageicp_pipeline_config cfg{};
    cfg.voxel_size_map = 1.0; cfg.max_range = 100.0; cfg.min_range = 5.0; cfg.label_max_range = 50.0;
    cfg.local_map_range = 100.0; cfg.basic_points_per_voxel = 20; cfg.critical_points_per_voxel = 20;
    cfg.basic_parts_labels = basic; cfg.n_basic_parts_labels = 1;
    cfg.min_motion_th = 0.1; cfg.initial_threshold = 2.0; cfg.sem_th = 0.05;
    cfg.n_groups = 1; cfg.group_label_counts = counts; cfg.group_labels = labels; cfg.group_voxel_size = sizes;
    cfg.device = 0; cfg.map_update_on_device = 1;
    sageicp_pipeline *p = sageicp_pipeline_create(&cfg);
    if (!p) {
        std::printf("pipeline error: %s\n", sageicp_last_error());
        return 1;
    }
    stub::PointCloud2 empty = make(with({{"label", 12, kUint8, 1}, {"rgb", 13, kUint32, 1}}), 21);
    double pose[7];
    try {
        const uint64_t n_source = sageicp::msg::register_frame(p, empty, false, pose);
        std::printf("empty_frame ok n_source=%llu poses=%llu\n", static_cast<unsigned long long>(n_source),
                    static_cast<unsigned long long>(sageicp_pipeline_num_poses(p)));
        stub::PointCloud2 src;
        sageicp::msg::source_to(p, colors, src);
        std::printf("empty_source ok width=%u data=%zu\n", src.width, src.data.size());
    } catch (const std::exception &e) {
        std::printf("empty_frame error: %s\n", e.what());
    }
    sageicp_pipeline_destroy(p);
    return 0;
}
