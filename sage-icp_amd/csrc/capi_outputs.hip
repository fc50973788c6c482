// The way out of libsageicp_hip.so (outputs.h): a cloud's rows as rows or as sensor_msgs/PointCloud2 records, into host
// memory or a caller's device memory, and occupancy grids as bytes.  One driver (export_rows) does what every export
// does — the count, the early return, the device, the order of the streams, the buffers, the flagged section, the copy
// to the host; the entries validate what only they validate, say where the rows come from and where they go, and call
// it.  The map's export entries and the stand-alone occupancy entries are here; the pipeline's are with its handle
// (capi_pipeline.hip).  The kernels are egress.hip's, msg.hip's, map_update.hip's and keyframe.hip's.  Host code only.
#include "capi_internal.h"
#include "replay_pool.h"

#include <mutex>

#include <sys/mman.h>

namespace sageicp_impl {

// ---- the flagged section ---------------------------------------------------------------------------------------------
// what a bit that the kernels raised in the flag word refuses the call with; the first that matches speaks
struct FlagText {
    int bit;
    const char *text;
};
static const FlagText kRowFlags[] = {
    {kEgressLabelRange, "a label does not fit the destination's label type (static_cast<int64_t>(label) out of its range)"}};
static const FlagText kRecordFlags[] = {
    {kMsgLabelRange, "a label does not fit the record's uint8 (trunc(label) outside [0, 255])"},
    {kMsgNoColor, "the colour table has no colour for a label"}};
static const FlagText kGridFlags[] = {{kOccNonFinite, "a coordinate is not finite (NaN / Inf)"}};

// What enqueue(word) puts on s behind a zeroed flag word: waited for, then the bits it may have raised read and turned
// into a refusal.  Synchronous also when enqueue fails part-way: nothing this call enqueued runs on once it has returned.
template <size_t N, typename Enqueue>
static int flagged(DevBuf<int> &flag, hipStream_t s, const FlagText (&texts)[N], Enqueue &&enqueue) {
    if (!flag) HIPCHK(flag.reserve(1));
    HIPCHK(hipMemsetAsync(flag.data(), 0, sizeof(int), s));
    int flags = 0;
    const int rc = enqueue(flag.data());
    hipError_t e = rc ? hipSuccess : hipGetLastError();
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(&flags, flag.data(), sizeof(int), hipMemcpyDeviceToHost, s);
    const hipError_t w = hipStreamSynchronize(s);
    if (rc) return rc;
    HIPCHK(e);
    HIPCHK(w);
    for (const FlagText &t : texts)
        if (flags & t.bit) return fail(SAGEICP_ERR_INVALID, t.text);
    return SAGEICP_OK;
}

// ---- host rows: the pages of a fresh destination -------------------------------------------------------------------
// Make the pages of [p, p + bytes) exist — the range is about to be overwritten as a whole — from
// SAGEICP_TOUCH_THREADS (default 4; 0: off) parked threads, each a contiguous share populated with
// one madvise(MADV_POPULATE_WRITE) call (Linux 5.14) or, where that is refused, by a byte written
// into every page.  (Measured and not kept: asking for huge pages first — no better; the copy cut
// in pieces running behind the populating threads — slower than populate-then-copy, 3.1 vs 2.2 ms.)
static void pretouch(void *p, size_t bytes) {
    const Knobs &kn = knobs();
    const int threads = std::min(kn.touch_threads.get(), ReplayPool::kMaxThreads);
    constexpr size_t kPage = 4096;
    if (threads <= 0 || bytes < (size_t{4} << 20)) return;
    static ReplayPool pool;
    static std::mutex one_at_a_time;
    std::lock_guard<std::mutex> lk(one_at_a_time);
    char *base = static_cast<char *>(p);
    // whole pages inside the range go through madvise; the ragged ends are touched
    char *lo_al = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(base) + kPage - 1) & ~(kPage - 1));
    char *hi_al = reinterpret_cast<char *>(reinterpret_cast<uintptr_t>(base + bytes) & ~(kPage - 1));
    *static_cast<volatile char *>(base) = 0;
    *static_cast<volatile char *>(base + bytes - 1) = 0;
    if (hi_al <= lo_al) return;
#ifdef MADV_HUGEPAGE
    // where the kernel hands out transparent huge pages on request (.../transparent_hugepage/enabled = madvise, the
    // usual setting), the 2-MB-aligned inside of the range is faulted in as ~20 huge pages instead of ~11,000 small
    // ones: 2.95 against 3.11 ms per LocalMap() of 46 MB (SAGEICP_HUGEPAGES=0: off)
    if (kn.hugepages.get()) {
        constexpr uintptr_t kHuge = uintptr_t{2} << 20;
        const uintptr_t h0 = (reinterpret_cast<uintptr_t>(lo_al) + kHuge - 1) & ~(kHuge - 1);
        const uintptr_t h1 = reinterpret_cast<uintptr_t>(hi_al) & ~(kHuge - 1);
        if (h1 > h0) (void)madvise(reinterpret_cast<void *>(h0), h1 - h0, MADV_HUGEPAGE);
    }
#endif
    const size_t pages = static_cast<size_t>(hi_al - lo_al) / kPage, share = (pages + threads - 1) / threads;
    pool.run(static_cast<size_t>(threads), [&](size_t t) {
        const size_t lo = t * share, hi = std::min(pages, lo + share);
        if (lo >= hi) return;
#ifdef MADV_POPULATE_WRITE
        if (madvise(lo_al + lo * kPage, (hi - lo) * kPage, MADV_POPULATE_WRITE) == 0) return;
#endif
        for (size_t i = lo; i < hi; ++i) *static_cast<volatile char *>(lo_al + i * kPage) = 0;
    }, static_cast<size_t>(threads));
}

// ---- a map's rows -----------------------------------------------------------------------------------------------------
// Pointcloud() while the HBM copy is the authority: packed on the device (block counts -> prefix
// sum -> gather, block-pool order like the host's), only size() x 32 B cross PCIe, and the map
// stays where it is — the node's per-frame LocalMap() (ros/ros2/OdometryServer.cpp:211-220 under
// publish_frame, the launch files' default) costs the copy of the live points and nothing else:
// no table rebuild, no re-upload before the next RegisterFrame.
// The live points of a resident map gathered on stream s in sageicp_map_pointcloud's order into `out`: packed, or
// straight into a caller's layout (egress.h; the rows at and beyond its cap are not written).  Synchronous only in
// reference-order mode.
static int gather_resident(sageicp_map &m, const RowsOut &out, hipStream_t s) {
    const uint32_t blocks_hi = m.dev.ctr.blocks_hi;
    MapDevice::GatherScratch g;
    int rc = m.dev.gather_scratch(static_cast<size_t>(blocks_hi) + 1, &g);
    if (rc) return rc;
    const DevMap dm = m.dev.view(m.host);
    if (!m.host.track_order) {
        HIPCHK(map_pointcloud_device(dm, blocks_hi, g.flag, g.sel, g.temp, g.temp_bytes, out, s));
        return SAGEICP_OK;
    }
    // reference-order mode: the voxels in the bucket order of the host's array (VoxelHashMap.cpp:132-142), their points
    // gathered on the device in that order
    std::vector<uint32_t> list;
    list.reserve(m.host.order.size());
    m.host.order.for_each([&](uint32_t b) { list.push_back(b); });
    if ((rc = m.dev.gather_scratch(list.size() + 1, &g))) return rc;
    if (!list.empty()) HIPCHK(hipMemcpyAsync(g.list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(map_pointcloud_listed(dm, g.list, static_cast<uint32_t>(list.size()), g.flag, g.sel, g.temp, g.temp_bytes, out, s));
    HIPCHK(hipStreamSynchronize(s));                                             // (`list` is pageable and leaves scope)
    return SAGEICP_OK;
}

// *rows: the n packed rows of a source, there on s.  Its own; or a map's in d_pc: gathered from the HBM copy, or staged
// from the host copy and uploaded (`staged` must live until s has been waited for).
static int packed_rows(const RowSource &src, uint64_t n, DevBuf<Point4> &d_pc, std::vector<double> &staged, hipStream_t s,
                       const Point4 **rows) {
    *rows = src.d_rows;
    sageicp_map *m = src.map;
    if (!m) return SAGEICP_OK;
    if (n > d_pc.capacity()) HIPCHK(d_pc.reserve(n + n / 4 + 1024));
    *rows = d_pc.data();
    if (m->resident()) return gather_resident(*m, RowsOut{d_pc.data(), {}}, s);
    staged.resize(4 * n);
    m->host.pointcloud(staged.data(), n);
    HIPCHK(hipMemcpyAsync(d_pc.data(), staged.data(), n * sizeof(Point4), hipMemcpyHostToDevice, s));
    return SAGEICP_OK;
}

int map_packed_rows(sageicp_map &m, hipStream_t s, std::vector<double> &staged, const Point4 **rows) {
    return packed_rows(RowSource::of_map(m), m.counts().points, m.out.d_pc, staged, s, rows);
}

EgressArgs egress_args(const sageicp_device_points &d, int *flags) {
    EgressArgs a{};
    a.xyz = static_cast<unsigned char *>(d.xyz);
    a.xyz_stride = d.xyz_stride;
    a.xyz_dtype = d.xyz_dtype;
    a.label = static_cast<unsigned char *>(d.label);
    a.label_stride = d.label_stride;
    a.label_dtype = d.label_dtype;
    a.cap = d.cap;
    a.flags = flags;
    return a;
}

// ---- the driver -------------------------------------------------------------------------------------------------------
int export_rows(OutputBuffers &ob, int device, const RowSource &src, const RowSink &sink, uint64_t *n_out) {
    sageicp_map *m = src.map;
    const uint64_t n = m ? m->counts().points : src.n;
    *n_out = n;
    const uint64_t want = std::min(sink.cap, n);
    if (!want) return SAGEICP_OK;
    // Host rows are the caller's pageable buffer, and under the reference's interface a FRESH one every call
    // (`std::vector<Eigen::Vector4d> Pointcloud()` returns by value: tens of MB straight from mmap).  The runtime's
    // staged copy moves 63 MB in 1.2 ms into pages that exist — and in 3.4 ms into pages that do not: two thirds of
    // the call were first-touch faults taken one by one inside the copy (profiles/pointcloud_probe.py).  So a map's
    // pages are made to exist first, by a few parked host threads side by side (while the device gathers the rows).
    if (m && !m->resident() && sink.kind == RowSink::kHostRows) {        // host to host: no device
        pretouch(sink.out, want * sizeof(Point4));
        m->host.pointcloud(static_cast<double *>(sink.out), sink.cap);
        return SAGEICP_OK;
    }
    int rc = m ? m->sc.init(device) : SAGEICP_OK;
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    // The stream.  A map works on its own, which waits for the work the caller enqueued before this call (it may still
    // use the destination); packed rows go into a caller's memory on the caller's stream itself, behind that work.
    hipStream_t s = m ? m->sc.stream.get() : src.stream;
    if (sink.on_device()) {
        if (!m) s = sink.caller;
        else if ((rc = stream_after_caller(ob.ev_caller, sink.caller, s))) return rc;
    }
    std::vector<double> staged;                 // (read by a copy on s: every path below waits for s)
    const Point4 *rows = nullptr;
    if (sink.kind == RowSink::kHostRows) {
        if (!m) {
            HIPCHK(hipMemcpy(sink.out, src.d_rows, want * sizeof(Point4), hipMemcpyDeviceToHost));
            return SAGEICP_OK;
        }
        if ((rc = packed_rows(src, n, ob.d_pc, staged, s, &rows))) return rc;
        pretouch(sink.out, want * sizeof(Point4));
        HIPCHK(hipMemcpyAsync(sink.out, rows, want * sizeof(Point4), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return SAGEICP_OK;
    }
    if (sink.kind == RowSink::kDeviceRows)
        return flagged(ob.d_flag, s, kRowFlags, [&](int *word) -> int {
            const EgressArgs e = egress_args(*sink.dst, word);
            if (m && m->resident() && !knobs().egress_two_pass.get())
                return gather_resident(*m, RowsOut{nullptr, e}, s);      // the gather writes the caller's layout itself
            // two passes: the rows packed, then k_egress
            if (int r = packed_rows(src, n, ob.d_pc, staged, s, &rows)) return r;
            launch_egress(e, rows, want, s);
            return SAGEICP_OK;
        });
    // records: packed on the device into the caller's memory, or into d_msg, from where they follow to the host
    const size_t bytes = static_cast<size_t>(want) * SAGEICP_MSG_POINT_STEP;
    if (!sink.on_device() && bytes > ob.d_msg.capacity()) HIPCHK(ob.d_msg.reserve(bytes + bytes / 4 + 4096));
    unsigned char *d_out = sink.on_device() ? static_cast<unsigned char *>(sink.out) : ob.d_msg.data();
    return flagged(ob.d_flag, s, kRecordFlags, [&](int *word) -> int {
        if (int r = packed_rows(src, n, ob.d_pc, staged, s, &rows)) return r;
        launch_msg_pack(rows, want, *sink.colors, d_out, word, s);
        if (sink.on_device()) return SAGEICP_OK;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(sink.out, d_out, bytes, hipMemcpyDeviceToHost, s));
        return SAGEICP_OK;
    });
}

int color_table(const sageicp_msg_colors *c, MsgColorTable &t) {
    std::memset(&t, 0, sizeof(t));
    if (!c || !c->n) return SAGEICP_OK;
    if (!c->keys || !c->values) return fail(SAGEICP_ERR_INVALID, "colour table: n > 0 with a NULL array");
    for (uint32_t i = 0; i < c->n; ++i) {
        const int32_t k = c->keys[i];
        if (k < 0 || k > 255) continue;
        t.value[k] = static_cast<uint32_t>(c->values[i]);
        t.present[k >> 5] |= 1u << (k & 31);
    }
    return SAGEICP_OK;
}
int check_records_out(const void *out, uint64_t cap, void *stream, int device) {
    if (!cap) return SAGEICP_OK;
    if (!out) return fail(SAGEICP_ERR_INVALID, "null argument");
    int rc = require_device();
    if (rc) return rc;
    if ((rc = check_extent(out, cap * SAGEICP_MSG_POINT_STEP, device, "message records: out"))) return rc;
    return check_stream(stream, device);
}

// ---- occupancy grids (keyframe.hip) --------------------------------------------------------------------------------
int occ_grid_from(const sageicp_occupancy_params *prm, OccGrid &g) {
    if (!prm) return fail(SAGEICP_ERR_INVALID, "null occupancy params");
    for (int a = 0; a < 3; ++a) {
        const double lo = prm->bounds[a][0], hi = prm->bounds[a][1];
        if (!std::isfinite(lo) || !std::isfinite(hi)) return fail(SAGEICP_ERR_INVALID, "occupancy bounds are not finite");
        if (!(lo < hi)) return fail(SAGEICP_ERR_INVALID, "occupancy bounds: lo >= hi on an axis");
        g.lo[a] = lo;
        g.hi[a] = hi;
    }
    if (prm->occ_h < 1 || prm->occ_h > kOccMaxSide || prm->occ_w < 1 || prm->occ_w > kOccMaxSide)
        return fail(SAGEICP_ERR_INVALID, "occupancy size: occ_h and occ_w must lie in [1, 4096]");
    if (!std::isfinite(prm->overlap_th)) return fail(SAGEICP_ERR_INVALID, "the overlap threshold is not finite");
    g.h = prm->occ_h;
    g.w = prm->occ_w;
    // Utils.hpp:224-225: (bounds[0][1] - bounds[0][0]) / occ_size[1], (bounds[1][1] - bounds[1][0]) / occ_size[0]
    g.x_res = (g.hi[0] - g.lo[0]) / static_cast<double>(g.w);
    g.y_res = (g.hi[1] - g.lo[1]) / static_cast<double>(g.h);
    return SAGEICP_OK;
}
OccTransform occ_transform(const double pose[7]) {
    OccTransform t;
    quat_to_mat(pose, t.R);                 // as fill_state does for k_tf
    for (int i = 0; i < 3; ++i) t.t[i] = pose[4 + i];
    return t;
}
// bits of a grid into H * W bytes
static void occ_unpack_host(const uint32_t *bits, const OccGrid &g, uint8_t *out) {
    const uint64_t cells = static_cast<uint64_t>(g.h) * g.w;
    for (uint64_t i = 0; i < cells; ++i) out[i] = static_cast<uint8_t>((bits[i >> 5] >> (i & 31)) & 1u);
}
int occ_bytes_to_host(const uint32_t *d_bits, const OccGrid &g, uint8_t *out) {
    std::vector<uint32_t> bits(occ_words(g));
    HIPCHK(hipMemcpy(bits.data(), d_bits, bits.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    occ_unpack_host(bits.data(), g, out);
    return SAGEICP_OK;
}
int occ_bytes_to_device(const uint32_t *d_bits, const OccGrid &g, uint8_t *out, hipStream_t s) {
    if (d_bits) launch_occ_unpack(d_bits, g, out, s);
    else HIPCHK(hipMemsetAsync(out, 0, static_cast<uint64_t>(g.h) * g.w, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return SAGEICP_OK;
}

// the grid of n rows already on the device (d_pts), moved by pose (or not), into host bytes; a coordinate that is not
// finite refuses the call.  On stream s, which is synchronised.
static int occupancy_on_device(const Point4 *d_pts, uint64_t n, const double *pose, const OccGrid &g, uint8_t *grid_out,
                               hipStream_t s) {
    const uint32_t words = occ_words(g);
    DevBuf<uint32_t> d_bits;
    DevBuf<int> d_flag;
    HIPCHK(d_bits.reserve(words));
    std::vector<uint32_t> bits(words);
    const int rc = flagged(d_flag, s, kGridFlags, [&](int *word) -> int {
        HIPCHK(hipMemsetAsync(d_bits.data(), 0, words * sizeof(uint32_t), s));
        const OccTransform tf = pose ? occ_transform(pose) : OccTransform{};
        launch_occ_draw(d_pts, static_cast<int>(n), g, pose ? &tf : nullptr, pose ? nullptr : d_bits.data(),
                        pose ? d_bits.data() : nullptr, word, knobs().occ_global.get() != 0, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(bits.data(), d_bits.data(), words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        return SAGEICP_OK;
    });
    if (rc) return rc;
    occ_unpack_host(bits.data(), g, grid_out);
    return SAGEICP_OK;
}
}  // namespace sageicp_impl

// =============================================================================================
static int export_map(sageicp_map &m, const RowSink &sink, uint64_t *n_out) {
    return export_rows(m.out, m.device, RowSource::of_map(m), sink, n_out);
}

extern "C" {

// ---- a map's live points out ---------------------------------------------------------------------------------------
uint64_t sageicp_map_pointcloud(const sageicp_map *m, double *out, uint64_t cap) {
    uint64_t n = 0;
    if (!m || export_map(internal(m), RowSink::host_rows(out, cap), &n)) return 0;
    return n;
}
int sageicp_map_pointcloud_device(const sageicp_map *m, const sageicp_device_points *dst, void *stream, uint64_t *n_out) {
    if (!m || !n_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (int rc = check_device_points(dst, stream, m->device)) return rc;
    return export_map(internal(m), RowSink::device_rows(dst, stream), n_out);
}
static int map_msg(const sageicp_map *m, const sageicp_msg_colors *colors, void *out, uint64_t cap, bool on_device,
                   void *stream, uint64_t *n_out) {
    if (!m || !n_out || (cap && !out)) return fail(SAGEICP_ERR_INVALID, "null argument");
    MsgColorTable t;
    int rc = color_table(colors, t);
    if (rc) return rc;
    if (on_device && (rc = check_records_out(out, cap, stream, m->device))) return rc;
    return export_map(internal(m), RowSink::records_out(out, cap, t, on_device, stream), n_out);
}
int sageicp_map_pointcloud_msg(const sageicp_map *m, const sageicp_msg_colors *colors, void *out, uint64_t cap,
                               uint64_t *n_out) {
    return map_msg(m, colors, out, cap, false, nullptr, n_out);
}
int sageicp_map_pointcloud_msg_device(const sageicp_map *m, const sageicp_msg_colors *colors, void *out, uint64_t cap,
                                      void *stream, uint64_t *n_out) {
    return map_msg(m, colors, out, cap, true, stream, n_out);
}

// ---- occupancy grids of a frame ------------------------------------------------------------------------------------
int sageicp_occupancy_grid(const double *xyzl, uint64_t n, const double pose[7], const sageicp_occupancy_params *params,
                           uint8_t *grid_out, int device) {
    if ((n && !xyzl) || !grid_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    OccGrid g{};
    int rc = occ_grid_from(params, g);
    if (rc) return rc;
    if (n > kMaxQueries) return fail(SAGEICP_ERR_INVALID, "frame too large (2^26 - 4 points max)");
    if (pose && !finite_n(pose, 7)) return fail(SAGEICP_ERR_INVALID, "the pose is not finite");
    for (uint64_t i = 0; i < n; ++i)
        if (!finite_n(xyzl + 4 * i, 3)) return fail(SAGEICP_ERR_INVALID, "a coordinate is not finite (NaN / Inf)");
    if (int rc = require_device(device)) return rc;
    if (n == 0) {
        std::memset(grid_out, 0, static_cast<size_t>(g.h) * g.w);
        return SAGEICP_OK;
    }
    HIPCHK(hipSetDevice(device));
    DevBuf<Point4> d_p;
    OwnedStream s;                      // (after the buffer: waited for before it is freed)
    HIPCHK(s.create());
    HIPCHK(d_p.reserve(n));
    HIPCHK(hipMemcpyAsync(d_p.data(), xyzl, n * sizeof(Point4), hipMemcpyHostToDevice, s.get()));
    return occupancy_on_device(d_p.data(), n, pose, g, grid_out, s.get());
}
int sageicp_occupancy_grid_device(const sageicp_device_frame *frame, const double pose[7],
                                  const sageicp_occupancy_params *params, uint8_t *grid_out, void *stream) {
    if (!frame || !grid_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    OccGrid g{};
    int rc = occ_grid_from(params, g);
    if (rc) return rc;
    if (pose && !finite_n(pose, 7)) return fail(SAGEICP_ERR_INVALID, "the pose is not finite");
    // no handle: the work runs on the device the frame's memory lives on, looked up once its layout has passed
    int device = 0;
    rc = check_device_frame(frame, nullptr, stream, device, &device);
    if (rc) return rc;
    if (frame->n == 0) {
        std::memset(grid_out, 0, static_cast<size_t>(g.h) * g.w);
        return SAGEICP_OK;
    }
    HIPCHK(hipSetDevice(device));
    // on the caller's stream, behind the work that wrote the frame; synchronous
    const hipStream_t s = static_cast<hipStream_t>(stream);
    DevBuf<Point4> d_p;
    HIPCHK(d_p.reserve(frame->n));
    launch_ingest(ingest_args(*frame), d_p.data(), s);
    HIPCHK(hipGetLastError());
    rc = occupancy_on_device(d_p.data(), frame->n, pose, g, grid_out, s);
    (void)hipStreamSynchronize(s);          // (d_p leaves scope)
    return rc;
}

}  // extern "C"
