// The acceptance radius of GetCorrespondences as a threshold on the squared distance.  Host only, no HIP, and a
// DEFINITION: included by exactly one translation unit of the library (capi_run.hip; the declaration the others see
// is capi_internal.h's) and by the g++-compiled shim of tests/test_accept_threshold_host.py.
#pragma once

#include <cmath>
#include <limits>

namespace sageicp_impl {

// largest r2 with sqrt(r2) < max_dist: the acceptance test (nn - p).norm() < max_dist
// (VoxelHashMap.cpp:111) without a device square root, exact for the IEEE sqrt the CPU evaluates
double accept_threshold(double max_dist) {
    if (!(max_dist > 0.0)) return -1.0;                       // nothing passes (also NaN)
    double x = max_dist * max_dist;
    if (std::isinf(x)) x = std::numeric_limits<double>::max();
    while (x > 0.0 && !(std::sqrt(x) < max_dist)) x = std::nextafter(x, 0.0);
    for (;;) {
        const double up = std::nextafter(x, std::numeric_limits<double>::infinity());
        if (std::isinf(up) || !(std::sqrt(up) < max_dist)) break;
        x = up;
    }
    return std::sqrt(x) < max_dist ? x : -1.0;
}

}  // namespace sageicp_impl
