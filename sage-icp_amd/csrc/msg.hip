// sensor_msgs/PointCloud2 payloads unpacked and packed on the device (msg.h; include/sageicp.h, sageicp_msg_layout and
// SAGEICP_MSG_*): what ros/ros2/Utils.hpp:55-198 does in host loops at both ends of the reference's odometry node.
//
// k_msg_unpack.  A workgroup's 256 records are contiguous: 256 * point_step bytes.  Records of up to kMsgStageStep bytes
// are staged: the span, from its base aligned down to 16, goes into LDS with 16-B loads — every granule loaded holds at
// least one byte of the n * point_step extent, none lies wholly before or behind it — and each lane picks its fields out
// of LDS as the two aligned dwords around them, shifted.  Longer records are read field by field from global memory,
// dwords where the address allows and bytes where it does not.  Rows go out as two 16-B stores per lane.
// uint32 stamps: their maximum is exact in integers — reduced per wave, one atomicMax per workgroup — and
// k_msg_normalize divides by it afterwards (NormalizeTimestamps: not when it is below 1).
//
// k_msg_pack.  A workgroup builds its 256 * 21 = 5376 bytes in LDS and writes the span with 16-B stores: 5376 is a
// multiple of 16, so every span starts aligned when the destination does.  The last partial span ends in byte stores; a
// destination that is only 4-B aligned takes dword stores, any other byte stores.  Exactly n * 21 bytes are written.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "msg.h"

namespace sageicp {

namespace {

// the dword at byte offset `off` of an array of aligned dwords: the two around it, shifted
__device__ __forceinline__ uint32_t dword_at(const uint32_t *w, uint32_t off) {
    const uint32_t k = off >> 2, sh = (off & 3u) * 8u;
    const unsigned long long both = (static_cast<unsigned long long>(w[k + 1]) << 32) | w[k];
    return static_cast<uint32_t>(both >> sh);
}

// the same from global memory: one dword load where the address allows, else its four bytes
__device__ __forceinline__ uint32_t dword_at(const unsigned char *p) {
    if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) return *reinterpret_cast<const uint32_t *>(p);
    return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 |
           static_cast<uint32_t>(p[3]) << 24;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o, 64));
        v = other > v ? other : v;
    }
    return v;
}

constexpr uint32_t kStageGranules = (256 * kMsgStageStep + 15) / 16 + 2;     // the span from its aligned base, one to spare

}  // namespace

template <bool Staged>
__global__ __launch_bounds__(256) void k_msg_unpack(MsgUnpackArgs a, Point4 *out) {
    __shared__ uint32_t s_wave_max[4];
    const uint32_t tid = threadIdx.x;
    const unsigned long long first = static_cast<unsigned long long>(blockIdx.x) * 256;
    const unsigned long long i = first + tid;
    const bool live = i < static_cast<unsigned long long>(a.n);
    uint32_t fx = 0, fy = 0, fz = 0, fl = 0, t_lo = 0, t_hi = 0;
    const bool want_time = a.time_kind != 0;
    if constexpr (Staged) {
        __shared__ uint4 s_span[kStageGranules];
        const unsigned long long last = min(first + 256, static_cast<unsigned long long>(a.n));    // records [first, last)
        const uintptr_t begin = reinterpret_cast<uintptr_t>(a.data) + first * a.point_step;
        const uintptr_t end = reinterpret_cast<uintptr_t>(a.data) + last * a.point_step;
        const uintptr_t base = begin & ~static_cast<uintptr_t>(15);
        const uint32_t granules = static_cast<uint32_t>((end - base + 15) / 16);     // the last one starts before `end`
        for (uint32_t g = tid; g < granules; g += 256) s_span[g] = *reinterpret_cast<const uint4 *>(base + 16ull * g);
        __syncthreads();
        if (live) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(s_span);
            const uint32_t rec = static_cast<uint32_t>(begin - base) + tid * a.point_step;
            fx = dword_at(w, rec + a.x_offset);
            fy = dword_at(w, rec + a.y_offset);
            fz = dword_at(w, rec + a.z_offset);
            fl = dword_at(w, rec + a.label_offset);      // (a uint8 label: its byte and three that follow, inside s_span)
            if (want_time) {
                t_lo = dword_at(w, rec + a.time_offset);
                if (a.time_kind == 2) t_hi = dword_at(w, rec + a.time_offset + 4);
            }
        }
    } else {
        if (live) {
            const unsigned char *rec = a.data + i * a.point_step;
            fx = dword_at(rec + a.x_offset);
            fy = dword_at(rec + a.y_offset);
            fz = dword_at(rec + a.z_offset);
            fl = a.label_dtype == SAGEICP_DTYPE_UINT8 ? rec[a.label_offset] : dword_at(rec + a.label_offset);
            if (want_time) {
                t_lo = dword_at(rec + a.time_offset);
                if (a.time_kind == 2) t_hi = dword_at(rec + a.time_offset + 4);
            }
        }
    }
    if (live) {
        const double x = static_cast<double>(__uint_as_float(fx)), y = static_cast<double>(__uint_as_float(fy));
        const double z = static_cast<double>(__uint_as_float(fz));
        const double l = a.label_dtype == SAGEICP_DTYPE_UINT8 ? static_cast<double>(fl & 0xFFu)
                                                              : static_cast<double>(__uint_as_float(fl));
        double2 *row = reinterpret_cast<double2 *>(out + i);
        row[0] = make_double2(x, y);
        row[1] = make_double2(z, l);
        if (a.time_kind == 2) {
            const double t = __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(t_hi) << 32) | t_lo));
            a.ts_out[i] = t;
            if (!(fabs(t) <= 1.7976931348623157e308)) atomicOr(a.flags, kIngestBadTimestamp);
        } else if (a.time_kind == 1) {
            a.ts_out[i] = static_cast<double>(t_lo);
        }
    }
    if (a.time_kind == 1) {             // (uniform: every lane of the workgroup takes part, a dead one with 0)
        const uint32_t m = wave_max(live ? t_lo : 0u);
        if ((tid & 63u) == 0) s_wave_max[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) {
            uint32_t v = s_wave_max[0];
            for (int k = 1; k < 4; ++k) v = s_wave_max[k] > v ? s_wave_max[k] : v;
            if (v) atomicMax(a.ts_max, v);
        }
    }
}

__global__ __launch_bounds__(256) void k_msg_normalize(double *ts, int n, const uint32_t *ts_max) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double m = static_cast<double>(*ts_max);
    if (m < 1.0) return;                // Utils.hpp:71: already normalised
    ts[i] = ts[i] / m;
}

void launch_msg_unpack(const MsgUnpackArgs &a, Point4 *out, hipStream_t s) {
    if (a.n <= 0) return;
    const dim3 grid((a.n + 255) / 256), block(256);
    if (a.point_step <= kMsgStageStep) hipLaunchKernelGGL(k_msg_unpack<true>, grid, block, 0, s, a, out);
    else hipLaunchKernelGGL(k_msg_unpack<false>, grid, block, 0, s, a, out);
}

void launch_msg_normalize(double *ts, int n, const uint32_t *ts_max, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_msg_normalize, dim3((n + 255) / 256), dim3(256), 0, s, ts, n, ts_max);
}

namespace {

__device__ __forceinline__ void put_dword(unsigned char *p, uint32_t v) {
    p[0] = static_cast<unsigned char>(v);
    p[1] = static_cast<unsigned char>(v >> 8);
    p[2] = static_cast<unsigned char>(v >> 16);
    p[3] = static_cast<unsigned char>(v >> 24);
}

template <int W> struct StoreWord;
template <> struct StoreWord<16> { using type = uint4; };
template <> struct StoreWord<4> { using type = uint32_t; };
template <> struct StoreWord<1> { using type = unsigned char; };

}  // namespace

// W: bytes per store of a span's bulk, what the destination's alignment allows (16, 4 or 1)
template <int W>
__global__ __launch_bounds__(256) void k_msg_pack(const Point4 *in, unsigned long long n, MsgColorTable colors,
                                                  unsigned char *out, int *flags) {
    __shared__ __attribute__((aligned(16))) unsigned char s_rec[256 * SAGEICP_MSG_POINT_STEP];
    const uint32_t tid = threadIdx.x;
    const unsigned long long first = static_cast<unsigned long long>(blockIdx.x) * 256;
    const uint32_t rows = static_cast<uint32_t>(min(256ull, n - first));
    if (tid < rows) {
        const Point4 p = in[first + tid];
        // trunc(label) in [0, 255]: where static_cast<uint8_t> is defined, and all the colour table can hold
        const bool in_range = p.l > -1.0 && p.l < 256.0;
        const uint32_t label = in_range ? static_cast<uint32_t>(static_cast<int>(p.l)) : 0u;
        const bool has_color = (colors.present[label >> 5] >> (label & 31u)) & 1u;
        if (!in_range) atomicOr(flags, kMsgLabelRange);
        else if (!has_color) atomicOr(flags, kMsgNoColor);
        unsigned char *r = s_rec + tid * SAGEICP_MSG_POINT_STEP;
        put_dword(r + SAGEICP_MSG_X_OFFSET, __float_as_uint(static_cast<float>(p.x)));
        put_dword(r + SAGEICP_MSG_Y_OFFSET, __float_as_uint(static_cast<float>(p.y)));
        put_dword(r + SAGEICP_MSG_Z_OFFSET, __float_as_uint(static_cast<float>(p.z)));
        r[SAGEICP_MSG_LABEL_OFFSET] = static_cast<unsigned char>(label);
        put_dword(r + SAGEICP_MSG_RGB_OFFSET, has_color ? colors.value[label] : 0u);
        put_dword(r + SAGEICP_MSG_RGB_OFFSET + 4, 0u);          // the four bytes data.resize leaves
    }
    __syncthreads();
    using Word = typename StoreWord<W>::type;
    const uint32_t bytes = rows * SAGEICP_MSG_POINT_STEP;
    unsigned char *dst = out + first * SAGEICP_MSG_POINT_STEP;
    const uint32_t words = bytes / W;
    for (uint32_t k = tid; k < words; k += 256)
        reinterpret_cast<Word *>(dst)[k] = reinterpret_cast<const Word *>(s_rec)[k];
    for (uint32_t j = words * W + tid; j < bytes; j += 256) dst[j] = s_rec[j];
}

void launch_msg_pack(const Point4 *in, uint64_t n, const MsgColorTable &colors, unsigned char *out, int *flags,
                     hipStream_t s) {
    if (n == 0) return;
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    const uintptr_t at = reinterpret_cast<uintptr_t>(out);
    if (at % 16 == 0) hipLaunchKernelGGL(k_msg_pack<16>, grid, block, 0, s, in, n, colors, out, flags);
    else if (at % 4 == 0) hipLaunchKernelGGL(k_msg_pack<4>, grid, block, 0, s, in, n, colors, out, flags);
    else hipLaunchKernelGGL(k_msg_pack<1>, grid, block, 0, s, in, n, colors, out, flags);
}

}  // namespace sageicp
