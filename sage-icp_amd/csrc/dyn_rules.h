// The two scalar conversions of the dynamic vehicle filter (core/Preprocessing.cpp:95-172) whose C++ behaviour is
// undefined for some inputs, fixed here to what the reference's x86-64 build computes.  Host and
// device; compiled on its own by tests/test_dynfilter_host.py.
#pragma once

#include <climits>
#include <cmath>
#include <cstdint>

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

}  // namespace sageicp
