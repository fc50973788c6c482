// sensor_msgs/PointCloud2 in and out of libsageicp_hip.so (include/sageicp.h, "PointCloud2 payloads"): what the odometry
// node does with ros/ros2/Utils.hpp's PointCloud2ToEigen, GetTimestamps and EigenToPointCloud2, on top of the C ABI.
//
// Header-only and duck-typed on the message type — .fields[i].{name, offset, datatype, count}, .point_step, .height,
// .width, .row_step, .data, .is_bigendian — so it needs no ROS headers: sensor_msgs::msg::PointCloud2 fits, and so does
// any struct with those members.  INTEGRATION.md section 6e shows the node's three call sites on top of it.
//
// The field-name rules are the reference's:
//   x, y, z, label   found by name (the first of a name, as sensor_msgs' iterators take it); each must be declared
//                    FLOAT32, except that label must be UINT8 when the message has exactly five fields and FLOAT32
//                    otherwise (the fields.size() == 5 switch of Utils.hpp:167);
//   time             the LAST field named t, timestamp or time; t and timestamp must be UINT32 (normalised by their
//                    maximum), time must be FLOAT64 (taken as it is); without one: the reference's error text, raised
//                    only when stamps are asked for;
//   where the reference would read a field through a type other than its declared one it reinterprets bytes; here that
//   is refused with an error that names the field; a big-endian message is refused.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "sageicp.h"

namespace sageicp {
namespace msg {

// sensor_msgs/PointField datatype codes
constexpr int kUint8 = SAGEICP_MSG_FIELD_UINT8, kUint32 = SAGEICP_MSG_FIELD_UINT32, kFloat32 = SAGEICP_MSG_FIELD_FLOAT32,
              kFloat64 = SAGEICP_MSG_FIELD_FLOAT64;
// GetTimestampField's text, ros/ros2/Utils.hpp:63
constexpr const char *kNoTimeField = "Field 't', 'timestamp', or 'time'  does not exist";

namespace detail {
inline const char *type_name(int datatype) {
    static const char *const names[9] = {"datatype 0", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "FLOAT32", "FLOAT64"};
    return datatype >= 1 && datatype <= 8 ? names[datatype] : "an unknown datatype";
}
template <class Field>
uint32_t field_as(const Field &f, int datatype, const std::string &why = "") {
    if (static_cast<int>(f.datatype) != datatype)
        throw std::runtime_error("field '" + std::string(f.name) + "' is declared " + type_name(static_cast<int>(f.datatype)) +
                                 "; it is read as " + type_name(datatype) + why +
                                 " (the reference would reinterpret its bytes)");
    return static_cast<uint32_t>(f.offset);
}
template <class Msg>
const auto &named(const Msg &m, const char *name) {
    for (const auto &f : m.fields)
        if (f.name == name) return f;
    throw std::runtime_error(std::string("Field ") + name + " does not exist");
}
inline void check(int rc, const char *what) {
    if (rc != SAGEICP_OK) throw std::runtime_error(std::string(what) + ": " + sageicp_last_error());
}
}  // namespace detail

// the layout of an incoming message by the rules above; want_time: the stamps will be read (deskew is on)
template <class Msg>
sageicp_msg_layout layout_of(const Msg &m, bool want_time) {
    if (m.is_bigendian) throw std::runtime_error("a big-endian PointCloud2 is not supported");
    sageicp_msg_layout l{};
    l.point_step = static_cast<uint32_t>(m.point_step);
    l.x_offset = detail::field_as(detail::named(m, "x"), kFloat32);
    l.y_offset = detail::field_as(detail::named(m, "y"), kFloat32);
    l.z_offset = detail::field_as(detail::named(m, "z"), kFloat32);
    if (m.fields.size() == 5) {
        l.label_offset = detail::field_as(detail::named(m, "label"), kUint8, " in a message of exactly five fields");
        l.label_dtype = SAGEICP_DTYPE_UINT8;
    } else {
        l.label_offset = detail::field_as(detail::named(m, "label"), kFloat32,
                                          " in a message of " + std::to_string(m.fields.size()) + " fields");
        l.label_dtype = SAGEICP_DTYPE_FLOAT32;
    }
    if (want_time) {
        const std::decay_t<decltype(m.fields[0])> *tf = nullptr;
        for (const auto &f : m.fields)
            if (f.name == "t" || f.name == "timestamp" || f.name == "time") tf = &f;
        if (!tf || !tf->count) throw std::runtime_error(kNoTimeField);
        if (tf->name == "time") {
            l.time_offset = detail::field_as(*tf, kFloat64);
            l.time_kind = 2;
        } else {
            l.time_offset = detail::field_as(*tf, kUint32);
            l.time_kind = 1;
        }
    }
    return l;
}

// CreatePointCloud2Msg (Utils.hpp:104-128) for n points: the five fields, point_step 21, one row; data sized (the
// header is the caller's)
template <class Msg>
void prepare_output(Msg &m, size_t n) {
    sageicp_msg_field table[8];
    const uint32_t k = sageicp_msg_output_fields(table, 8);
    m.fields.clear();
    m.fields.resize(k);
    for (uint32_t i = 0; i < k; ++i) {
        m.fields[i].name = table[i].name;
        m.fields[i].offset = table[i].offset;
        m.fields[i].datatype = static_cast<decltype(m.fields[i].datatype)>(table[i].datatype);
        m.fields[i].count = table[i].count;
    }
    m.is_bigendian = false;
    m.point_step = SAGEICP_MSG_POINT_STEP;
    m.height = 1;
    m.width = static_cast<decltype(m.width)>(n);
    m.row_step = static_cast<decltype(m.row_step)>(n * SAGEICP_MSG_POINT_STEP);
    m.data.resize(n * SAGEICP_MSG_POINT_STEP);
}

// the node's color_list (std::map<int, int> or any range of pairs) as the ABI's key / value arrays
class Colors {
public:
    template <class Map>
    explicit Colors(const Map &color_list) {
        for (const auto &kv : color_list) {
            keys_.push_back(static_cast<int32_t>(kv.first));
            values_.push_back(static_cast<int32_t>(kv.second));
        }
    }
    sageicp_msg_colors get() const {
        return sageicp_msg_colors{keys_.data(), values_.data(), static_cast<uint32_t>(keys_.size())};
    }

private:
    std::vector<int32_t> keys_, values_;
};

// PointCloud2ToEigen + GetTimestamps + RegisterFrame of a message in host memory (OdometryServer.cpp:160-167):
// deskew says whether the pipeline deskews (sageicp_pipeline_set_deskew), which is when the stamps are read.
// Returns n_source; throws with the library's text on error.
template <class Msg>
uint64_t register_frame(sageicp_pipeline *p, const Msg &m, bool deskew, double pose_out[7], sageicp_stats *stats = nullptr) {
    const sageicp_msg_layout l = layout_of(m, deskew);
    const uint64_t n = static_cast<uint64_t>(m.height) * m.width;      // (the reference's iterators ignore row_step)
    uint64_t n_source = 0;
    detail::check(sageicp_pipeline_register_frame_msg(p, m.data.empty() ? nullptr : m.data.data(), m.data.size(), n, &l,
                                                      pose_out, nullptr, nullptr, &n_source, stats),
                  "sageicp::msg::register_frame");
    return n_source;
}

// EigenToPointCloud2(frame, header, color_list) of the registered source cloud (OdometryServer.cpp:214)
template <class Msg>
void source_to(const sageicp_pipeline *p, const Colors &colors, Msg &out) {
    uint64_t n = 0;
    detail::check(sageicp_pipeline_source(p, nullptr, 0, &n), "sageicp::msg::source_to");
    prepare_output(out, n);
    const sageicp_msg_colors c = colors.get();
    detail::check(sageicp_pipeline_source_msg(p, &c, out.data.data(), n, &n), "sageicp::msg::source_to");
}

// EigenToPointCloud2(local_map, header, color_list) of a map (OdometryServer.cpp:219; the pipeline's:
// sageicp_pipeline_local_map)
template <class Msg>
void map_to(const sageicp_map *map, const Colors &colors, Msg &out) {
    uint64_t n = sageicp_map_size(map);
    prepare_output(out, n);
    const sageicp_msg_colors c = colors.get();
    detail::check(sageicp_map_pointcloud_msg(map, &c, out.data.data(), n, &n), "sageicp::msg::map_to");
}

}  // namespace msg
}  // namespace sageicp
