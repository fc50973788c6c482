// A caller's device memory and stream, checked before anything is launched (caller_mem.hip): the extents of frames in
// (sageicp_device_frame, message payloads) and of destinations out (sageicp_device_points, records, grids).  Host,
// pinned and managed memory are refused, not copied.  Every check leaves its message in the error channel and returns a
// SAGEICP_* code.  Included by capi_internal.h; not part of the C ABI.
#pragma once

#include <cstdint>

#include "../../include/sageicp.h"

namespace sageicp_impl {

// the first and the last byte of an extent must be device memory of `device`
int check_extent(const void *p, uint64_t bytes, int device, const char *what);
// a caller's stream (NULL: the null stream) must be one of `device`
int check_stream(void *stream, int device);
// Strided rows, a frame's n or a destination's cap: the layout first (no device needed), then where the memory of the
// rows (and of the n timestamps `ts` that will be read, if given) lives, then the stream.  found: an entry without a
// handle works on the device xyz lives on (`device` is not read): it is looked up once the layout has passed, and
// stored there.
int check_device_frame(const sageicp_device_frame *f, const double *ts, void *stream, int device, int *found = nullptr);
int check_device_points(const sageicp_device_points *d, void *stream, int device);
// The layout part of the two checks above alone: no device is asked.  An entry that takes several layouts checks them
// all before it looks at where any of them points (sageicp_get_correspondences_device).
int check_frame_layout(const sageicp_device_frame *f);
int check_points_layout(const sageicp_device_points *d);
// the bytes [lo, hi) a destination of a valid layout spans — its rows and, if apart, its labels: `out` gets that many
// (0 for cap == 0), for comparing the extents of several destinations on the host
struct CallerExtent {
    const char *lo, *hi;
    bool overlaps(const CallerExtent &o) const { return lo < o.hi && o.lo < hi; }
};
int points_extents(const sageicp_device_points &d, CallerExtent out[2]);

}  // namespace sageicp_impl
