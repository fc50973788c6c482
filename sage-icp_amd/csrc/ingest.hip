// A raw frame from a caller's device memory (include/sageicp.h, sageicp_device_frame: a segmentation network's point
// and label tensors) into the library's Point4 rows, so that a frame that is already on the GPU does not cross PCIe
// twice.  One lane per point; every value becomes a double through a plain conversion (float -> double is exact,
// int64 -> double rounds to nearest like numpy's astype), nothing else: no mask, no label table.  Non-finite values
// pass through — the crop of preprocess.hip refuses them exactly as it does for host input.
// Rows whose layout allows it are read with 16-B loads (base and stride 16-B aligned): a float32 row as one float4, a
// float64 row as two double2.  A float32 row without its label column reads its fourth element only where the next
// row follows (the bytes lie inside the caller's extent); the last row reads its three elements one by one.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/sageicp.h"
#include "kernels.h"

namespace sageicp {

// element i of the separate label array (L: its element type)
template <typename L>
__device__ __forceinline__ double load_label(const IngestArgs &a, int i) {
    return static_cast<double>(*reinterpret_cast<const L *>(a.label + static_cast<unsigned long long>(i) * a.label_stride));
}

template <typename T, typename L, bool Vec>
__global__ __launch_bounds__(256) void k_ingest(IngestArgs a, Point4 *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    constexpr bool kColumn = std::is_void<L>::value;
    const unsigned char *row = a.xyz + static_cast<unsigned long long>(i) * a.xyz_stride;
    double x, y, z, l = 0.0;
    if constexpr (std::is_same<T, float>::value) {
        if (Vec && (kColumn || i + 1 < a.n)) {
            const float4 v = *reinterpret_cast<const float4 *>(row);
            x = v.x; y = v.y; z = v.z;
            if constexpr (kColumn) l = v.w;
        } else {
            const float *r = reinterpret_cast<const float *>(row);
            x = r[0]; y = r[1]; z = r[2];
            if constexpr (kColumn) l = r[3];
        }
    } else {
        const double *r = reinterpret_cast<const double *>(row);
        if (Vec) {
            const double2 v = *reinterpret_cast<const double2 *>(row);
            x = v.x; y = v.y;
            if constexpr (kColumn) {
                const double2 w = *reinterpret_cast<const double2 *>(row + 16);
                z = w.x; l = w.y;
            } else {
                z = r[2];
            }
        } else {
            x = r[0]; y = r[1]; z = r[2];
            if constexpr (kColumn) l = r[3];
        }
    }
    if constexpr (!kColumn) l = load_label<L>(a, i);
    out[i] = Point4{x, y, z, l};
    if (a.ts) {
        const double t = a.ts[i];
        a.ts_out[i] = t;
        if (!(fabs(t) <= 1.7976931348623157e308)) atomicOr(a.flags, kIngestBadTimestamp);
    }
}

template <typename T, typename L>
static void launch_typed(const IngestArgs &a, Point4 *out, hipStream_t s) {
    const dim3 grid((a.n + 255) / 256), block(256);
    const bool vec = (reinterpret_cast<uintptr_t>(a.xyz) % 16 == 0) && (a.xyz_stride % 16 == 0);
    if (vec) hipLaunchKernelGGL((k_ingest<T, L, true>), grid, block, 0, s, a, out);
    else hipLaunchKernelGGL((k_ingest<T, L, false>), grid, block, 0, s, a, out);
}

template <typename T>
static void launch_label(const IngestArgs &a, Point4 *out, hipStream_t s) {
    if (!a.label) launch_typed<T, void>(a, out, s);
    else if (a.label_dtype == SAGEICP_DTYPE_UINT8) launch_typed<T, uint8_t>(a, out, s);
    else if (a.label_dtype == SAGEICP_DTYPE_INT32) launch_typed<T, int32_t>(a, out, s);
    else launch_typed<T, int64_t>(a, out, s);
}

void launch_ingest(const IngestArgs &a, Point4 *out, hipStream_t s) {
    if (a.n <= 0) return;
    if (a.xyz_dtype == SAGEICP_DTYPE_FLOAT32) launch_label<float>(a, out, s);
    else launch_label<double>(a, out, s);
}

}  // namespace sageicp
