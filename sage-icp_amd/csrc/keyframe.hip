// Key-frame selection by occupancy overlap (the odometry node's block at ros/ros2/OdometryServer.cpp:222-243, with
// EigenToGridMap and compute_occ_overlap of ros/ros2/Utils.hpp:221-260) on the device.
//
// A grid is the bird's-eye occupancy of a frame: a point inside the bounds (inclusive on every side) sets the cell
//     occ_x = int((x + bx_hi) / x_res),  occ_y = int((y + by_hi) / y_res)
// if 0 <= occ_x < W and 0 <= occ_y < H — the UPPER bound as the offset, and the cast truncating toward zero, as the
// reference does.  Everything is fp64 with a true division (the build's -ffp-contract=off keeps the sums plain); the
// range is tested on the double (v > -1 && v < W) before the cast, which is the reference's set wherever its cast is
// defined and has no undefined behaviour beyond.  Grids are packed bitmaps (kernels.h, OccGrid).
//
//   k_occ_keep    the raw frame copied aside before deskew and the dynamic filter rewrite it in place, every
//                 coordinate checked (a frame with one that is not finite is refused while selection is on)
//   k_occ_draw    one pass over the rows: the identity grid (the candidate for the next key grid) and the grid under
//                 rel = key_pose^-1 * pose (the point action of k_tf, bit for bit).  Grids that fit (two of them in
//                 32 KiB) are drawn in LDS with bitwise-OR atomics and only their non-zero words are OR-ed into
//                 memory; larger ones are OR-ed into memory directly.  OR is idempotent and commutative: both paths
//                 set the same bits in any order.
//   k_occ_decide  one workgroup: |key| and |key & cur| with integer atomics (exact, deterministic), the decision
//                 |key & cur| / |key| < th in fp64 (0 / 0 is NaN: no switch), and the candidate copied over the key
//                 grid when it is taken.  Only the two counts and the decision go to the host.
//   k_occ_unpack  a bitmap into H * W bytes for the caller.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "se3_math.h"

namespace sageicp {

namespace {
constexpr int kDrawThreads = 256;
constexpr uint32_t kLdsBytes = 32768;       // two grids of up to 131072 cells each
constexpr int kDecideThreads = 1024;

__device__ __forceinline__ bool finite3(const Point4 &p) {
    return fabs(p.x) <= 1.7976931348623157e308 && fabs(p.y) <= 1.7976931348623157e308 &&
           fabs(p.z) <= 1.7976931348623157e308;
}

// the cell (y * W + x) a point sets, or -1
__device__ __forceinline__ int occ_cell(double x, double y, double z, const OccGrid &g) {
    if (x < g.lo[0] || x > g.hi[0] || y < g.lo[1] || y > g.hi[1] || z < g.lo[2] || z > g.hi[2]) return -1;
    const double vx = (x + g.hi[0]) / g.x_res;
    const double vy = (y + g.hi[1]) / g.y_res;
    if (!(vx > -1.0 && vx < static_cast<double>(g.w) && vy > -1.0 && vy < static_cast<double>(g.h))) return -1;
    return static_cast<int>(vy) * g.w + static_cast<int>(vx);
}

__device__ __forceinline__ void set_bit(uint32_t *bits, int c) { atomicOr(bits + (c >> 5), 1u << (c & 31)); }
}  // namespace

__global__ __launch_bounds__(256) void k_occ_keep(const Point4 *in, Point4 *out, int n, int *flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Point4 p = in[i];
    out[i] = p;
    if (!finite3(p)) atomicOr(flags, kOccNonFinite);
}

template <bool Lds>
__global__ __launch_bounds__(kDrawThreads) void k_occ_draw(const Point4 *in, int n, OccGrid g, OccTransform tf,
                                                           uint32_t *id, uint32_t *cur, int *flags, uint32_t words) {
    extern __shared__ uint32_t s_bits[];        // Lds: [2 * words], the identity grid, then the transformed one
    if constexpr (Lds) {
        for (uint32_t w = threadIdx.x; w < 2 * words; w += kDrawThreads) s_bits[w] = 0;
        __syncthreads();
    }
    uint32_t *dst_id = Lds ? s_bits : id;
    uint32_t *dst_cur = Lds ? s_bits + words : cur;
    bool bad = false;
    for (int i = blockIdx.x * kDrawThreads + threadIdx.x; i < n; i += gridDim.x * kDrawThreads) {
        const Point4 p = in[i];
        if (!finite3(p)) {
            bad = true;
            continue;
        }
        if (id) {
            const int c = occ_cell(p.x, p.y, p.z, g);
            if (c >= 0) set_bit(dst_id, c);
        }
        if (cur) {
            const double v[3] = {p.x, p.y, p.z};
            double o[3];
            mat_apply(tf.R, tf.t, v, o);
            const int c = occ_cell(o[0], o[1], o[2], g);
            if (c >= 0) set_bit(dst_cur, c);
        }
    }
    if (bad && flags) atomicOr(flags, kOccNonFinite);
    if constexpr (Lds) {
        __syncthreads();
        for (uint32_t w = threadIdx.x; w < 2 * words; w += kDrawThreads) {
            const uint32_t v = s_bits[w];
            if (v) atomicOr(w < words ? id + w : cur + (w - words), v);
        }
    }
}

__global__ __launch_bounds__(kDecideThreads) void k_occ_decide(uint32_t *key, const uint32_t *cand, const uint32_t *cur,
                                                               uint32_t words, int force, double th, OccDecision *out) {
    __shared__ unsigned long long s_key, s_inter;
    if (threadIdx.x == 0) {
        s_key = 0;
        s_inter = 0;
    }
    __syncthreads();
    if (!force) {
        unsigned long long k = 0, x = 0;
        for (uint32_t w = threadIdx.x; w < words; w += kDecideThreads) {
            const uint32_t a = key[w];
            k += __popc(a);
            x += __popc(a & cur[w]);
        }
        if (k) atomicAdd(&s_key, k);
        if (x) atomicAdd(&s_inter, x);
    }
    __syncthreads();                            // (every read of `key` is done before it is overwritten)
    const unsigned long long kc = s_key, ic = s_inter;
    const bool take = force || static_cast<double>(ic) / static_cast<double>(kc) < th;
    if (threadIdx.x == 0) *out = OccDecision{kc, ic, take ? 1 : 0, 0};
    if (take)
        for (uint32_t w = threadIdx.x; w < words; w += kDecideThreads) key[w] = cand[w];
}

__global__ __launch_bounds__(256) void k_occ_unpack(const uint32_t *bits, unsigned n_cells, unsigned char *out) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cells) return;
    out[i] = static_cast<unsigned char>((bits[i >> 5] >> (i & 31)) & 1u);
}

void launch_occ_keep(const Point4 *in, Point4 *out, int n, int *flags, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_occ_keep, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n, flags);
}

void launch_occ_draw(const Point4 *in, int n, const OccGrid &g, const OccTransform *tf, uint32_t *id, uint32_t *cur,
                     int *flags, bool force_global, hipStream_t s) {
    if (n <= 0 || (!id && !cur)) return;
    const uint32_t words = occ_words(g);
    // four rows per lane at least; at most 512 workgroups, each zeroing and flushing its private grids once
    const unsigned blocks = static_cast<unsigned>(std::min<int>((n + 4 * kDrawThreads - 1) / (4 * kDrawThreads), 512));
    const OccTransform t = tf ? *tf : OccTransform{};
    const size_t lds = 2ull * words * sizeof(uint32_t);
    if (!force_global && lds <= kLdsBytes)
        hipLaunchKernelGGL(k_occ_draw<true>, dim3(blocks), dim3(kDrawThreads), lds, s, in, n, g, t, id,
                           tf ? cur : nullptr, flags, words);
    else
        hipLaunchKernelGGL(k_occ_draw<false>, dim3(blocks), dim3(kDrawThreads), 0, s, in, n, g, t, id,
                           tf ? cur : nullptr, flags, words);
}

void launch_occ_decide(uint32_t *key, const uint32_t *cand, const uint32_t *cur, uint32_t words, int force, double th,
                       OccDecision *out, hipStream_t s) {
    hipLaunchKernelGGL(k_occ_decide, dim3(1), dim3(kDecideThreads), 0, s, key, cand, cur, words, force, th, out);
}

void launch_occ_unpack(const uint32_t *bits, const OccGrid &g, unsigned char *out, hipStream_t s) {
    const unsigned cells = static_cast<unsigned>(g.h) * static_cast<unsigned>(g.w);
    if (cells) hipLaunchKernelGGL(k_occ_unpack, dim3((cells + 255) / 256), dim3(256), 0, s, bits, cells, out);
}

}  // namespace sageicp
