// The way out (capi_outputs.hip): the rows of a cloud — the pipeline's registered source, a map — leave as rows or as
// sensor_msgs/PointCloud2 records, into host memory or into a caller's device memory, through one driver; occupancy
// grids leave as bytes.  A RowSource says where the rows come from, a RowSink where they go, and export_rows does what
// every export does, once.  Declarations only; host code.  Included by capi_internal.h before the handles, which hold
// an OutputBuffers each; not part of the C ABI.
#pragma once

namespace sageicp_impl {

// What the exports of one handle work in.  Work on the owner's streams (a map's Scratch, a pipeline's Preps) and on
// callers' streams touches these buffers, and every export is synchronous, so nothing touches them once it has
// returned; the owner still has its streams waited for before this member goes (sageicp_map: in its destructor's body;
// sageicp_pipeline: by declaring it before the Preps).
struct OutputBuffers {
    DevBuf<Point4> d_pc;                // a map's rows, packed, before they cross PCIe or change layout
    DevBuf<unsigned char> d_msg;        // the 21-byte records before they cross PCIe
    DevBuf<int> d_flag;                 // the word the kernels raise their refusals in (flagged section, capi_outputs.hip)
    OwnedEvent ev_caller;               // orders a caller's stream before the owner's (created with the first use)
};

// Where the rows of an export come from, and on which stream they are there.
struct RowSource {
    // (a) n packed rows already on the device, valid on `stream`: the pipeline's d_src on its Prep's stream.  Into a
    // caller's device memory they are read on the caller's stream itself.
    const Point4 *d_rows = nullptr;
    uint64_t n = 0;
    hipStream_t stream = nullptr;
    // (b) a map, in sageicp_map_pointcloud's order, on the map's own stream, which a caller's stream is ordered before.
    // Resident: the gather, fused into a caller's layout or packed into d_pc (SAGEICP_EGRESS_TWO_PASS=1: always
    // packed); in reference-order mode the listed gather, synchronous.  Not resident: the host copy, staged and
    // uploaded — or, for host rows, copied on the host with no device at all.
    sageicp_map *map = nullptr;

    static RowSource packed(const Point4 *d_rows, uint64_t n, hipStream_t stream) {
        RowSource s;
        s.d_rows = d_rows; s.n = n; s.stream = stream;
        return s;
    }
    static RowSource of_map(sageicp_map &m) {
        RowSource s;
        s.map = &m;
        return s;
    }
};

// Where they go: `cap` rows or records of room, validated by the entry.
struct RowSink {
    enum Kind { kHostRows, kDeviceRows, kHostRecords, kDeviceRecords } kind;
    void *out = nullptr;                            // host rows (fp64 x, y, z, label); records, host or device
    const sageicp_device_points *dst = nullptr;     // kDeviceRows
    const MsgColorTable *colors = nullptr;          // records
    uint64_t cap = 0;
    hipStream_t caller = nullptr;                   // the device sinks: the caller's stream

    bool on_device() const { return kind == kDeviceRows || kind == kDeviceRecords; }
    static RowSink host_rows(double *out, uint64_t cap) {
        RowSink k{kHostRows};
        k.out = out; k.cap = out ? cap : 0;
        return k;
    }
    static RowSink device_rows(const sageicp_device_points *dst, void *stream) {
        RowSink k{kDeviceRows};
        k.dst = dst; k.cap = dst->cap; k.caller = static_cast<hipStream_t>(stream);
        return k;
    }
    static RowSink records_out(void *out, uint64_t cap, const MsgColorTable &colors, bool on_device, void *stream) {
        RowSink k{on_device ? kDeviceRecords : kHostRecords};
        k.out = out; k.cap = cap; k.colors = &colors; k.caller = static_cast<hipStream_t>(stream);
        return k;
    }
};

// The driver: *n_out = the rows the source has, min(cap, that) of them written; synchronous.  A label that the sink
// cannot hold, or that has no colour, refuses the call (whatever was written below cap stays written).
int export_rows(OutputBuffers &ob, int device, const RowSource &src, const RowSink &sink, uint64_t *n_out);

// A map's rows in sageicp_map_pointcloud's order, packed in its d_pc on s (source (b) above, for an export that puts them
// behind other rows: the session's map, capi_archive.hip).  `staged` lives until s has been waited for.
int map_packed_rows(sageicp_map &m, hipStream_t s, std::vector<double> &staged, const Point4 **rows);

// a validated destination as the writers of egress.h take it; flags: the device word a label that does not fit is raised in
EgressArgs egress_args(const sageicp_device_points &d, int *flags);

// what the record entries check first: the node's color_list as the 256-entry table the label rule leaves room for (keys
// outside 0..255 can never match), and a caller's destination of cap records in device memory with its stream
int color_table(const sageicp_msg_colors *c, MsgColorTable &t);
int check_records_out(const void *out, uint64_t cap, void *stream, int device);

// ---- occupancy grids (keyframe.hip) ----------------------------------------------------------------------------------
// the grid of validated params (include/sageicp.h: what is refused)
int occ_grid_from(const sageicp_occupancy_params *prm, OccGrid &g);
OccTransform occ_transform(const double pose[7]);
// the bits of a grid on the device as H * W bytes: in host memory (a blocking copy), or in a caller's device memory on
// its stream, synchronous (d_bits == nullptr: an empty grid)
int occ_bytes_to_host(const uint32_t *d_bits, const OccGrid &g, uint8_t *out);
int occ_bytes_to_device(const uint32_t *d_bits, const OccGrid &g, uint8_t *out, hipStream_t s);

}  // namespace sageicp_impl
