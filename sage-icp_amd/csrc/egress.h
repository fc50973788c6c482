// Rows of the library (Point4: fp64 x, y, z, label) written into a caller's device memory in the caller's layout
// (include/sageicp.h, sageicp_device_points): the inverse of ingest.hip.  The writers below are shared by k_egress
// (egress.hip: a packed array such as the pipeline's source cloud) and by the local map's gather kernels
// (map_update.hip), which write straight into the caller's layout instead of packing first.
//
// Conversions: float64 coordinates are written bit for bit, float32 ones through a plain (float) cast (round to
// nearest).  A float label is a plain cast; an integer label is static_cast<int64_t>(label) (the reference's cast),
// which must then fit the label's type — a label that does not raises kEgressLabelRange in *flags (a vector atomic)
// and the call is refused.  Only rows i < cap are written; nothing else of the destination is touched.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>
#include <type_traits>

#include "../../include/sageicp.h"
#include "sageicp_types.h"

namespace sageicp {

constexpr int kEgressLabelRange = 1;

struct EgressArgs {
    unsigned char *xyz;                 // row i at xyz + i * xyz_stride
    unsigned char *label;               // nullptr: column 3 of the rows (of the rows' type)
    unsigned long long xyz_stride, label_stride;     // bytes
    int xyz_dtype, label_dtype;         // SAGEICP_DTYPE_*
    unsigned long long cap;             // rows the destination holds: row i is written only if i < cap
    int *flags;                         // device word: kEgressLabelRange
};

// the label as the destination's type L
template <typename L>
__device__ __forceinline__ L egress_label(double l, int *flags) {
    if constexpr (std::is_floating_point<L>::value) {
        return static_cast<L>(l);
    } else {
        // [-2^63, 2^63): where the cast to int64 is defined; the labels are finite (non-finite input is refused)
        const bool in64 = l >= -9223372036854775808.0 && l < 9223372036854775808.0;
        const long long v = in64 ? static_cast<long long>(l) : 0;
        if (!in64 || v < static_cast<long long>(std::numeric_limits<L>::min()) ||
            v > static_cast<long long>(std::numeric_limits<L>::max()))
            atomicOr(flags, kEgressLabelRange);
        return static_cast<L>(v);
    }
}

// T: the coordinates' type; L: the separate label's type, void for column 3; Vec: base and stride are 16-B aligned,
// so that a float32 row with its label is one float4 store and a float64 row two double2 stores
template <typename T, typename L, bool Vec>
struct EgressWriter {
    EgressArgs a;
    __device__ __forceinline__ void operator()(size_t i, const Point4 &p) const {
        if (i >= a.cap) return;
        constexpr bool kColumn = std::is_void<L>::value;
        unsigned char *row = a.xyz + static_cast<unsigned long long>(i) * a.xyz_stride;
        if constexpr (std::is_same<T, float>::value) {
            float *r = reinterpret_cast<float *>(row);
            const float x = static_cast<float>(p.x), y = static_cast<float>(p.y), z = static_cast<float>(p.z);
            if constexpr (kColumn) {
                const float w = static_cast<float>(p.l);
                if constexpr (Vec) *reinterpret_cast<float4 *>(row) = make_float4(x, y, z, w);
                else { r[0] = x; r[1] = y; r[2] = z; r[3] = w; }
            } else {
                r[0] = x; r[1] = y; r[2] = z;
            }
        } else {
            double *r = reinterpret_cast<double *>(row);
            if constexpr (Vec) {
                *reinterpret_cast<double2 *>(row) = make_double2(p.x, p.y);
                if constexpr (kColumn) *reinterpret_cast<double2 *>(row + 16) = make_double2(p.z, p.l);
                else r[2] = p.z;
            } else {
                r[0] = p.x; r[1] = p.y; r[2] = p.z;
                if constexpr (kColumn) r[3] = p.l;
            }
        }
        if constexpr (!kColumn)
            *reinterpret_cast<L *>(a.label + static_cast<unsigned long long>(i) * a.label_stride) =
                egress_label<L>(p.l, a.flags);
    }
};

// the library's own packed rows (Pointcloud() into d_pc)
struct Point4Writer {
    Point4 *out;
    __device__ __forceinline__ void operator()(size_t i, const Point4 &p) const { out[i] = p; }
};
// where a gather of the local map writes (map_update.h): the library's packed rows, or a caller's layout
struct RowsOut {
    Point4 *packed;                     // nullptr: `caller`
    EgressArgs caller;
};

// f(EgressWriter<T, L, Vec>{a}) for the layout of `a` (validated by caller_mem.hip).  A float32 row without its label
// column has no 16-B store (12 B), so it always takes the element-wise form.
template <typename T, typename L, typename F>
inline void with_egress_vec(const EgressArgs &a, F &&f) {
    if constexpr (std::is_void<L>::value || std::is_same<T, double>::value) {
        if (reinterpret_cast<uintptr_t>(a.xyz) % 16 == 0 && a.xyz_stride % 16 == 0) {
            f(EgressWriter<T, L, true>{a});
            return;
        }
    }
    f(EgressWriter<T, L, false>{a});
}
template <typename T, typename F>
inline void with_egress_label(const EgressArgs &a, F &&f) {
    if (!a.label) with_egress_vec<T, void>(a, f);
    else if (a.label_dtype == SAGEICP_DTYPE_UINT8) with_egress_vec<T, uint8_t>(a, f);
    else if (a.label_dtype == SAGEICP_DTYPE_INT32) with_egress_vec<T, int32_t>(a, f);
    else if (a.label_dtype == SAGEICP_DTYPE_INT64) with_egress_vec<T, int64_t>(a, f);
    else if (a.label_dtype == SAGEICP_DTYPE_FLOAT32) with_egress_vec<T, float>(a, f);
    else with_egress_vec<T, double>(a, f);
}
template <typename F>
inline void with_egress_writer(const EgressArgs &a, F &&f) {
    if (a.xyz_dtype == SAGEICP_DTYPE_FLOAT32) with_egress_label<float>(a, f);
    else with_egress_label<double>(a, f);
}

// f(Point4Writer) or f(EgressWriter) for either output of a gather
template <typename F>
inline void with_writer(const RowsOut &out, F &&f) {
    if (out.packed) f(Point4Writer{out.packed});
    else with_egress_writer(out.caller, f);
}

// k_egress: rows [0, n) of `in` (n <= cap) into the caller's layout, one lane per row
void launch_egress(const EgressArgs &a, const Point4 *in, uint64_t n, hipStream_t s);

}  // namespace sageicp
