// The constant-velocity deskew of a frame on the device (core/Deskew.cpp:31-50, DeSkewScan): every point is moved by
// the motion its timestamp puts it at along the tangent `delta` of the last two poses,
//     p' = exp((t_i - 0.5) * delta) * p,   label and row order unchanged.
// One lane per point.  The exponential and the point action are se3_math.h's — the ones the ICP update uses
// (Registration.cpp:93,107) — so that the two paths cannot drift apart: se3_exp with the serial lane policy, then
// quat_to_mat and the operand order of mat_apply (as k_tf).  The build's -ffp-contract=off leaves the device's ocml
// sin / cos against the host's glibc ones as the only difference from a host evaluation (ulp level).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "se3_math.h"

namespace sageicp {

__global__ __launch_bounds__(256) void k_deskew(const Point4 *in, Point4 *out, const double *ts, int n,
                                                 DeskewTangent d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double s = ts[i] - 0.5;             // mid_pose_timestamp, Deskew.cpp:28
    double a[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] = s * d.v[j];
    double T[7], R[9];
    se3_exp(a, T);
    quat_to_mat(T, R);
    const Point4 p = in[i];
    const double v[3] = {p.x, p.y, p.z};
    double o[3];
    mat_apply(R, T + 4, v, o);
    out[i] = Point4{o[0], o[1], o[2], p.l};
}

void launch_deskew(const Point4 *in, Point4 *out, const double *ts, int n, const DeskewTangent &d, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_deskew, dim3((n + 255) / 256), dim3(256), 0, s, in, out, ts, n, d);
}

}  // namespace sageicp
