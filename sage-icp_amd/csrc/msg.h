// sensor_msgs/PointCloud2 payloads on the device (msg.hip): the two conversions at the ends of the reference's odometry
// node (ros/ros2/Utils.hpp:55-198).
//   k_msg_unpack   PointCloud2ToEigen + GetTimestamps: n records of point_step bytes, float32 x / y / z, a uint8 or
//                  float32 label and a uint32 or float64 stamp at arbitrary byte offsets, into the library's Point4 rows
//                  (and fp64 stamps).  Every value is a plain (double) cast.
//   k_msg_normalize NormalizeTimestamps (Utils.hpp:68-77) of uint32 stamps: divided by their maximum unless it is 0.
//   k_msg_pack     CreatePointCloud2Msg + FillPointCloud2XYZlRGB: packed Point4 rows into the 21-byte records the node
//                  publishes (include/sageicp.h, SAGEICP_MSG_*).
// The layouts have been validated by the caller (check_msg, capi_pipeline.hip); the pack is driven by capi_outputs.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sageicp.h"
#include "sageicp_types.h"

namespace sageicp {

// records of at most this many bytes are staged through LDS, a workgroup's 256 at a time, with 16-B loads; longer ones
// are read field by field, one lane per record
constexpr uint32_t kMsgStageStep = 64;
constexpr uint32_t kMsgMaxStep = 1024;

constexpr int kMsgLabelRange = 1;       // k_msg_pack, in its flag word: trunc(label) outside [0, 255]
constexpr int kMsgNoColor = 2;          // ... the colour table has no entry for the label

struct MsgUnpackArgs {
    const unsigned char *data;          // record i at data + i * point_step (device memory, any alignment)
    uint32_t point_step;
    uint32_t x_offset, y_offset, z_offset, label_offset, time_offset;
    int label_dtype;                    // SAGEICP_DTYPE_UINT8 / _FLOAT32
    int time_kind;                      // 0: not read; 1: uint32; 2: float64
    int n;
    double *ts_out;                     // [n] (time_kind != 0)
    uint32_t *ts_max;                   // device word, zeroed: the maximum of uint32 stamps (time_kind == 1)
    int *flags;                         // device word: kIngestBadTimestamp for a float64 stamp that is not finite
};
void launch_msg_unpack(const MsgUnpackArgs &a, Point4 *out, hipStream_t s);
// ts[i] = ts[i] / (double)*ts_max unless *ts_max == 0 (a true fp64 division)
void launch_msg_normalize(double *ts, int n, const uint32_t *ts_max, hipStream_t s);

// the colour of labels 0..255: value[l] is read only where bit l of `present` is set.  Passed by value (a kernel argument).
struct MsgColorTable {
    uint32_t value[256];
    uint32_t present[8];
};
// rows [0, n) of `in` as n * 21 bytes at `out` (device memory, any alignment); exactly those bytes are written
void launch_msg_pack(const Point4 *in, uint64_t n, const MsgColorTable &colors, unsigned char *out, int *flags,
                     hipStream_t s);

}  // namespace sageicp
