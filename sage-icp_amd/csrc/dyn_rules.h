// The two scalar conversions of the dynamic vehicle filter (core/Preprocessing.cpp:95-172) whose C++ behaviour is
// undefined for some inputs, fixed here to what the reference's x86-64 build computes, host and device,
// and the order its clusters are emitted in (host).  Compiled on its own by tests/test_dynfilter_host.py.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "sageicp_types.h"

namespace sageicp {

// :107-111 — static_cast<uint32_t>(static_cast<long long>(label)).  cvttsd2si gives INT64_MIN, whose low 32 bits are
// 0, for |label| >= 2^63 (and NaN); on gfx950 the same cast reduces modulo 2^32 instead, so those labels are mapped
// to 0 explicitly.
SAGE_HD inline uint32_t label_code(double l) {
    return fabs(l) < 9223372036854775808.0 ? static_cast<uint32_t>(static_cast<long long>(l)) : 0u;
}

// static_cast<int>(v) as cvttsd2si computes it: INT_MIN for NaN and for any v outside the int range
SAGE_HD inline int x86_int_cast(double v) {
    return (v > -2147483649.0 && v < 2147483648.0) ? static_cast<int>(v) : INT_MIN;
}

// :141-158: a cluster is static iff the running count of its landmark neighbours ever exceeds
// static_cast<int>(dy_th * size) — i.e. count >= 1 and count > that threshold (the count only grows).  A threshold
// that overflows the int is INT_MIN: every cluster with a landmark neighbour is kept.
SAGE_HD inline bool cluster_is_static(uint64_t count, uint32_t size, double dy_th) {
    const int th = x86_int_cast(dy_th * static_cast<double>(size));
    return count >= 1 && (th < 0 || count > static_cast<uint64_t>(th));
}

// PCL's cluster order: EuclideanClusterExtraction finds the clusters in order of their smallest index, then
// std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters) orders them by size, largest first — not stably.
// std::sort permutes by comparisons only, so the same call on (size, index) records with the same comparator gives
// PCL's permutation under the same standard library (libstdc++).  order[j] = index of the j-th cluster emitted.
inline void cluster_emission_order(const uint32_t *sizes, size_t n, uint32_t *order) {
    struct Rec {
        uint32_t size, index;
    };
    std::vector<Rec> v(n);
    for (size_t k = 0; k < n; ++k) v[k] = Rec{sizes[k], static_cast<uint32_t>(k)};
    std::sort(v.rbegin(), v.rend(), [](const Rec &a, const Rec &b) { return a.size < b.size; });
    for (size_t k = 0; k < n; ++k) order[k] = v[k].index;
}

}  // namespace sageicp
