// The checks of a caller's device memory (caller_mem.h): rows in the caller's layout — frames in (ingest.hip), outputs
// out (egress.hip, egress.h) — and plain extents.  Host code only.
#include "capi_internal.h"

namespace sageicp_impl {
static size_t dtype_bytes(int32_t t) {
    switch (t) {
    case SAGEICP_DTYPE_FLOAT32: return 4;
    case SAGEICP_DTYPE_FLOAT64: return 8;
    case SAGEICP_DTYPE_UINT8: return 1;
    case SAGEICP_DTYPE_INT32: return 4;
    case SAGEICP_DTYPE_INT64: return 8;
    default: return 0;
    }
}

// the device whose memory p is, as this library's runtime sees it (false: not device memory — host, pinned or managed
// memory, or a pointer of another HIP runtime loaded into the process, which is unknown here)
static bool device_of(const void *p, int *device) {
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    (void)hipGetLastError();            // an unknown pointer leaves an error behind that the next call must not see
    if (e != hipSuccess || at.type != hipMemoryTypeDevice) return false;
    *device = at.device;
    return true;
}

int check_extent(const void *p, uint64_t bytes, int device, const char *what) {
    const char *ends[2] = {static_cast<const char *>(p), static_cast<const char *>(p) + bytes - 1};
    for (const char *q : ends) {
        int d = -1;
        if (!device_of(q, &d))
            return fail(SAGEICP_ERR_INVALID, std::string(what) + " is not device memory of this process's HIP runtime "
                                             "(host, pinned and managed memory are refused, not copied)");
        if (d != device)
            return fail(SAGEICP_ERR_INVALID, std::string(what) + " lives on device " + std::to_string(d) +
                                             ", the handle on device " + std::to_string(device));
    }
    return SAGEICP_OK;
}

int check_stream(void *stream, int device) {
    if (!stream) return SAGEICP_OK;
    int sd = -1;
    const hipError_t e = hipStreamGetDevice(static_cast<hipStream_t>(stream), &sd);
    (void)hipGetLastError();
    if (e != hipSuccess || sd != device) return fail(SAGEICP_ERR_INVALID, "stream is not a stream of the handle's device");
    return SAGEICP_OK;
}

// Strided rows in a caller's device memory: a frame's n (sageicp_device_frame) or a destination's cap
// (sageicp_device_points).  Host-side only: the kernels take IngestArgs / EgressArgs.
struct CallerRows {
    const void *xyz;
    uint64_t xyz_stride;
    int32_t xyz_dtype;
    const void *label;
    uint64_t label_stride;
    int32_t label_dtype;
    uint64_t rows;
};
// what differs between a frame and a destination
struct RowRules {
    const char *prefix;                 // of the messages
    unsigned label_dtypes;              // bit t: SAGEICP_DTYPE t is a valid label_dtype
    const char *label_dtypes_text;
    uint64_t max_rows;                  // (refused as a frame that is too large)
};
static const RowRules kFrameRows{
    "device frame: ", 1u << SAGEICP_DTYPE_UINT8 | 1u << SAGEICP_DTYPE_INT32 | 1u << SAGEICP_DTYPE_INT64,
    "SAGEICP_DTYPE_UINT8, _INT32 or _INT64", kMaxQueries};
static const RowRules kPointsRows{
    "device points: ", 1u << SAGEICP_DTYPE_UINT8 | 1u << SAGEICP_DTYPE_INT32 | 1u << SAGEICP_DTYPE_INT64 |
                       1u << SAGEICP_DTYPE_FLOAT32 | 1u << SAGEICP_DTYPE_FLOAT64,
    "SAGEICP_DTYPE_UINT8, _INT32, _INT64, _FLOAT32 or _FLOAT64", std::numeric_limits<uint64_t>::max()};

// the layout of caller rows: what can be known without a device.  *xyz_bytes, *label_bytes: what a row and a label occupy
static int check_layout(const CallerRows &r, const RowRules &k, size_t *xyz_bytes = nullptr, size_t *label_bytes = nullptr) {
    const std::string pre = k.prefix;
    if (r.rows && !r.xyz) return fail(SAGEICP_ERR_INVALID, pre + "xyz is NULL");
    const size_t ex = r.xyz_dtype == SAGEICP_DTYPE_FLOAT32 || r.xyz_dtype == SAGEICP_DTYPE_FLOAT64 ? dtype_bytes(r.xyz_dtype) : 0;
    if (!ex) return fail(SAGEICP_ERR_INVALID, pre + "xyz_dtype must be SAGEICP_DTYPE_FLOAT32 or _FLOAT64");
    const uint64_t cols = r.label ? 3 : 4;
    if (r.xyz_stride < cols * ex || r.xyz_stride % ex)
        return fail(SAGEICP_ERR_INVALID, pre + (r.label ? "xyz_stride must be a multiple of the element size and at least 3 "
                                                          "elements"
                                                        : "xyz_stride must be a multiple of the element size and at least 4 "
                                                          "elements (the label is column 3)"));
    size_t el = 0;
    if (r.label) {
        el = dtype_bytes(r.label_dtype) && ((k.label_dtypes >> r.label_dtype) & 1u) ? dtype_bytes(r.label_dtype) : 0;
        if (!el) return fail(SAGEICP_ERR_INVALID, pre + "label_dtype must be " + k.label_dtypes_text);
        if (r.label_stride < el || r.label_stride % el)
            return fail(SAGEICP_ERR_INVALID, pre + "label_stride must be a positive multiple of the label's size");
    }
    if (r.rows > k.max_rows) return fail(SAGEICP_ERR_INVALID, "frame too large (2^26 - 4 points max)");
    if (xyz_bytes) *xyz_bytes = cols * ex;
    if (label_bytes) *label_bytes = el;
    return SAGEICP_OK;
}

// everything about caller rows that can be known before the stream is touched or anything launched (caller_mem.h)
static int check_rows(const CallerRows &r, const RowRules &k, const double *ts, void *stream, int device,
                      int *found = nullptr) {
    const std::string pre = k.prefix;
    size_t row = 0, el = 0;
    int rc = check_layout(r, k, &row, &el);
    if (rc) return rc;
    if (!r.rows) return SAGEICP_OK;
    if ((rc = require_device())) return rc;
    if (found) {                        // (memory that is not device memory is refused just below)
        device = 0;
        (void)device_of(r.xyz, &device);
        *found = device;
    }
    rc = check_extent(r.xyz, (r.rows - 1) * r.xyz_stride + row, device, (pre + "xyz").c_str());
    if (!rc && r.label) rc = check_extent(r.label, (r.rows - 1) * r.label_stride + el, device, (pre + "label").c_str());
    if (!rc && ts) rc = check_extent(ts, r.rows * sizeof(double), device, "timestamps");
    return rc ? rc : check_stream(stream, device);
}

int check_device_frame(const sageicp_device_frame *f, const double *ts, void *stream, int device, int *found) {
    if (!f) return fail(SAGEICP_ERR_INVALID, "null device frame");
    return check_rows({f->xyz, f->xyz_stride, f->xyz_dtype, f->label, f->label_stride, f->label_dtype, f->n}, kFrameRows,
                      ts, stream, device, found);
}

static CallerRows rows_of(const sageicp_device_points &d) {
    return {d.xyz, d.xyz_stride, d.xyz_dtype, d.label, d.label_stride, d.label_dtype, d.cap};
}

int check_frame_layout(const sageicp_device_frame *f) {
    if (!f) return fail(SAGEICP_ERR_INVALID, "null device frame");
    return check_layout({f->xyz, f->xyz_stride, f->xyz_dtype, f->label, f->label_stride, f->label_dtype, f->n}, kFrameRows);
}

int check_points_layout(const sageicp_device_points *d) {
    if (!d) return fail(SAGEICP_ERR_INVALID, "null destination");
    return check_layout(rows_of(*d), kPointsRows);
}

int points_extents(const sageicp_device_points &d, CallerExtent out[2]) {
    size_t row = 0, el = 0;
    if (check_layout(rows_of(d), kPointsRows, &row, &el) || !d.cap) return 0;
    const char *xyz = static_cast<const char *>(d.xyz);
    int k = 0;
    out[k++] = {xyz, xyz + (d.cap - 1) * d.xyz_stride + row};
    if (d.label) {
        const char *l = static_cast<const char *>(d.label);
        out[k++] = {l, l + (d.cap - 1) * d.label_stride + el};
    }
    return k;
}

int check_device_points(const sageicp_device_points *d, void *stream, int device) {
    if (!d) return fail(SAGEICP_ERR_INVALID, "null destination");
    return check_rows({d->xyz, d->xyz_stride, d->xyz_dtype, d->label, d->label_stride, d->label_dtype, d->cap},
                      kPointsRows, nullptr, stream, device);
}
}  // namespace sageicp_impl
