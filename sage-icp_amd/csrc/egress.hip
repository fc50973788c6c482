// The library's Point4 rows out into a caller's device memory (include/sageicp.h, sageicp_device_points): the pipeline's
// registered source cloud, and the local map when it is staged from the host copy (capi_outputs.hip drives both).  The inverse of k_ingest
// (ingest.hip): one lane per row, the conversions and 16-B stores of EgressWriter (egress.h).
#include <hip/hip_runtime.h>

#include "egress.h"

namespace sageicp {

template <typename W>
__global__ __launch_bounds__(256) void k_egress(const Point4 *in, unsigned long long n, W w) {
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    w(i, in[i]);
}

void launch_egress(const EgressArgs &a, const Point4 *in, uint64_t n, hipStream_t s) {
    if (n == 0) return;
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    with_egress_writer(a, [&](auto w) { hipLaunchKernelGGL(k_egress<decltype(w)>, grid, block, 0, s, in, n, w); });
}

}  // namespace sageicp
