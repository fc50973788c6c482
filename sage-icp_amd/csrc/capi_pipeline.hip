// The pipeline handle of the C ABI (include/sageicp.h, sageicp_pipeline_*): sageICP::RegisterFrame for a stream of scans
// around the device stages.  A register entry validates its arguments into one FrameSource (prep.h) — host rows, a
// device frame, a message — and pipeline_register runs Pipeline::register_frame (pipeline.hpp) over a backend that
// holds it: Prep (prep.hip) prepares the frame, or hands over the one the prefetch worker prepared (prefetch.h); the
// registration and the map update are capi.hip's and capi_run.hip's.  Then the key-frame step, the exported source
// cloud (through outputs.h's driver) and the switches.  Host code only.  Part of libsageicp_hip.so's host side: capi_internal.h.
#include "capi_internal.h"
#include "query.h"

extern "C" {

// ---- pipeline counterpart -----------------------------------------------------------------------
struct sageicp_pipeline {
    Pipeline impl;
    // Preprocess() + Voxelize() depend on the raw frame only (not on the pose, not on the map), so
    // the next frame's can run while this one registers (sageicp_pipeline_prefetch): two sets of
    // buffers and streams (prep[2], below), `cur` the one the frame being registered lives in; `pf` (last member) says
    // what the other holds.  (Not with deskew on: a deskewed frame depends on the poses of the two frames before it, so
    // prefetch is refused then.)
    int cur = 0;
    int device;
    // Preprocess()'s dynamic vehicle filter (sageicp_pipeline_set_dynamic_vehicle_filter): off by default
    bool dyn_on = false;
    DynFilterConfig dyn_cfg;
    // sageConfig::deskew (sageicp_pipeline_set_deskew): off by default; read by the timestamped entry only
    bool deskew_on = false;
    // the source cloud of the last successful register call (sageicp_pipeline_source*): src_n rows of
    // prep[src_buf].d_src, 0 when there is none.  Nothing writes that buffer before the next register call: the
    // prefetch worker fills the other one, and the registration reads d_src without reordering it.
    uint64_t src_n = 0;
    int src_buf = 0;
    mutable OutputBuffers out;                     // sageicp_pipeline_source*: the exports work in these (outputs.h)
    // key-frame selection (sageicp_pipeline_set_key_frames, keyframe.hip): off by default.  The key grid lives on the
    // device (d_key); the host holds the key pose and what the last frame's step decided.
    struct KeyFrames {
        bool on = false;
        sageicp_occupancy_params prm{};
        OccGrid g{};
        bool has_key = false;
        Pose7 key_pose;
        sageicp_key_frame_info info{};
        DevBuf<uint32_t> d_key, d_cand, d_cur;     // bitmaps (allocated with the first frame)
        DevBuf<OccDecision> d_dec;
        PinnedBuf<OccDecision> h_dec;
        // "no key frame"
        void clear() {
            has_key = false;
            key_pose = Pose7();
            info = sageicp_key_frame_info{};
            info.enabled = on ? 1 : 0;
            info.overlap = std::numeric_limits<double>::quiet_NaN();
            for (int i = 0; i < 7; ++i) info.key_pose[i] = key_pose.v[i];
        }
        KeyFrames() { clear(); }
    } kf;
    // place recognition (sageicp_pipeline_set_places, place.hip): off by default.  The database of the key frames'
    // descriptors (capi_place.hip) and what the last frame's step found in it.
    struct Places {
        struct Destroy {
            void operator()(sageicp_place_db *d) const { sageicp_place_db_destroy(d); }
        };
        bool on = false;
        sageicp_place_query query{};
        std::unique_ptr<sageicp_place_db, Destroy> db;
        sageicp_place_info info{};
        // what every register call starts from
        void no_frame() {
            info.described = 0;
            info.n_matches = 0;
        }
        void clear() {
            if (db) place_db_clear(*db);
            info = sageicp_place_info{};
            info.enabled = on ? 1 : 0;
        }
        void off() {
            on = false;
            db.reset();
            clear();
        }
    } places;
    // the registration quality report (sageicp_pipeline_set_quality, quality.hip): off by default; `quality` is the last
    // register call's, valid = 0 when there is none
    bool quality_on = false;
    sageicp_quality quality{};
    // (after the buffers that work on their streams touches — out, kf's: the Preps wait and go first)
    Prep prep[2];
    // (after the Preps: its worker runs voxelize_into on prep[cur ^ 1], and is joined before either goes)
    Prefetch pf;
    explicit sageicp_pipeline(const sageicp_pipeline_config &c) : impl(c), device(c.device) {}
    int voxelize_into(Prep &pr, const FrameSource &src, const DeskewTangent *deskew = nullptr) {
        int rc = pr.init(device);
        if (rc) return rc;
        std::vector<int> counts, labels;
        std::vector<double> vs;
        impl.group_tables(counts, labels, vs);
        PrepJob job;
        job.max_range = impl.max_range_(); job.min_range = impl.min_range_(); job.label_max_range = impl.label_max_range_();
        job.n_groups = static_cast<int>(counts.size());
        job.group_counts = counts.data(); job.group_labels = labels.data(); job.group_voxel_size = vs.data();
        job.n_levels = 2;
        job.levels[0] = {/*crop*/ 1, /*scale*/ 0.5};
        job.levels[1] = {/*crop*/ 0, /*scale*/ 1.5};
        job.dyn = dyn_on ? &dyn_cfg : nullptr; job.deskew = deskew;
        // level 0 (frame_downsample: it goes into the map, AddPoints depends on arrival order)
        // keeps the reference's emission order; level 1 (the registered source) does not need it
        pr.arrival_order_levels = knobs().source_reference_order.get() ? 0u : 2u;
        pr.keep_raw = kf.on;
        return pr.run(src, job);
    }
};

sageicp_pipeline *sageicp_pipeline_create(const sageicp_pipeline_config *c) {
    if (!c || c->n_groups < 0 || (c->n_groups && (!c->group_label_counts || !c->group_voxel_size))) {
        fail(SAGEICP_ERR_INVALID, "sageicp_pipeline_create: bad config");
        return nullptr;
    }
    // (both levels' scales, 0.5 and 1.5, are positive constants: the sizes decide)
    for (int g = 0; g < c->n_groups; ++g)
        if (!(std::isfinite(c->group_voxel_size[g]) && c->group_voxel_size[g] > 0.0)) {
            fail(SAGEICP_ERR_INVALID, "sageicp_pipeline_create: a label group's voxel size is not finite or not above 0");
            return nullptr;
        }
    sageicp_pipeline *p = new sageicp_pipeline(*c);
    if (!p->impl.ok()) {
        delete p;
        return nullptr;
    }
    return p;
}
void sageicp_pipeline_destroy(sageicp_pipeline *p) { delete p; }

// OdometryServer.cpp:222-243 for the frame just registered (its raw rows in prep[cur].d_raw, its pose the last one
// pushed): the identity grid (the candidate) and, with a key frame, the grid under key_pose^-1 * pose in one pass, then
// the counts, the decision and the swap on the device.  The host state changes only once the decision is back.
static int key_frame_step(sageicp_pipeline *p, uint64_t n) {
    auto &k = p->kf;
    Prep &pr = p->prep[p->cur];
    const hipStream_t s = pr.stream.get();
    const uint32_t words = occ_words(k.g);
    HIPCHK(hipSetDevice(p->device));
    if (!k.d_key) {
        HIPCHK(k.d_cand.reserve(words));
        HIPCHK(k.d_cur.reserve(words));
        HIPCHK(k.d_dec.reserve(1));
        HIPCHK(k.h_dec.reserve(1));
        HIPCHK(k.d_key.reserve(words));
    }
    const Pose7 pose = p->impl.poses.back();
    OccTransform tf{};
    if (k.has_key) {                         // sageICP::TransformToLastFrame, pipeline/sageICP.cpp:123-129
        Pose7 inv, rel;
        se3_inv(k.key_pose.v, inv.v);
        se3_mul(inv.v, pose.v, rel.v);
        tf = occ_transform(rel.v);
    }
    HIPCHK(hipMemsetAsync(k.d_cand.data(), 0, words * sizeof(uint32_t), s));
    if (k.has_key) HIPCHK(hipMemsetAsync(k.d_cur.data(), 0, words * sizeof(uint32_t), s));
    launch_occ_draw(pr.d_raw.data(), static_cast<int>(n), k.g, k.has_key ? &tf : nullptr, k.d_cand.data(), k.d_cur.data(),
                    nullptr, knobs().occ_global.get() != 0, s);
    HIPCHK(hipGetLastError());
    launch_occ_decide(k.d_key.data(), k.d_cand.data(), k.d_cur.data(), words, k.has_key ? 0 : 1, k.prm.overlap_th,
                      k.d_dec.data(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(k.h_dec.data(), k.d_dec.data(), sizeof(OccDecision), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const OccDecision d = *k.h_dec.data();
    sageicp_key_frame_info &info = k.info;
    info.is_key_frame = d.take;
    info.key_occupied = k.has_key ? d.key : 0;
    info.intersect = k.has_key ? d.inter : 0;
    // Utils.hpp:257: static_cast<double>(overlap) / total — NaN for 0 / 0, as the device's decision saw it
    info.overlap = k.has_key ? static_cast<double>(d.inter) / static_cast<double>(d.key)
                             : std::numeric_limits<double>::quiet_NaN();
    if (d.take) {
        k.has_key = true;
        k.key_pose = pose;
        info.key_frame_index = p->impl.poses.size() - 1;
        ++info.key_frames;
        for (int i = 0; i < 7; ++i) info.key_pose[i] = pose.v[i];
        // the key frame's place: described from the raw rows, matched against the places before it, then added
        auto &pl = p->places;
        if (pl.on) {
            if (int rc = place_db_step(*pl.db, pr.d_raw.data(), n, pl.query, info.key_frame_index, pose.v, s,
                                       pl.info.matches, &pl.info.n_matches))
                return rc;
            pl.info.described = 1;
            pl.info.entries = sageicp_place_db_size(pl.db.get());
        }
    }
    return SAGEICP_OK;
}

// RegisterFrame of the frame at `src`, deskewed first when the call reads its stamps and the pipeline decides so.
static int pipeline_register(sageicp_pipeline *p, const FrameSource &src, double pose_out[7], double *icp_s,
                             double *total_s, uint64_t *n_source, sageicp_stats *stats) {
    // Deskew (deskew.hip) on the uploaded frame when the pipeline decides so, then Preprocess + Voxelize on the
    // device (preprocess.hip): crop + scale 0.5, then scale 1.5.
    // Neither cloud comes back to the host: the source is registered and the down-sampled frame
    // inserted into the map from where the kernels left them (only a host-side map update
    // downloads its points).
    struct Backend {
        sageicp_pipeline *p;
        const FrameSource &src;
        int voxelize(uint64_t &n_src, const double *delta) {
            Prefetch &pf = p->pf;
            pf.join();
            if (src.empty_message()) {           // no rows, no device work (an announcement is dropped)
                Prep &pr = p->prep[p->cur];
                pr.kept_levels[0] = pr.kept_levels[1] = 0;
                pr.dyn_ran = false;
                pr.dyn.info = sageicp_dynfilter_info{};
                pf.drop_all();
                n_src = 0;
                return SAGEICP_OK;
            }
            int r;
            if (!delta && src.kind == FrameSource::kHostRows && pf.prepared_is(src.rows, src.n)) {
                r = pf.rc ? fail(pf.rc, pf.err) : SAGEICP_OK;       // prepared while the last frame registered
                p->cur ^= 1;
            } else {
                // not prepared ahead: a deskewed frame (it depends on the last two poses), a device frame, a message,
                // another frame or a refilled buffer
                DeskewTangent tangent{};
                for (int k = 0; delta && k < 6; ++k) tangent.v[k] = delta[k];
                r = p->voxelize_into(p->prep[p->cur], src, delta ? &tangent : nullptr);
            }
            pf.drop_prepared();
            n_src = p->prep[p->cur].kept_levels[1];
            // the frame after this one: its Preprocess() + Voxelize() run on the other set of
            // buffers (own stream, own host thread) under this frame's ICP loop and map update
            if (r == SAGEICP_OK)
                pf.promote_and_start([q = p, dst = &p->prep[p->cur ^ 1]](const double *f, uint64_t m) {
                    (void)hipSetDevice(q->device);
                    const int rc = q->voxelize_into(*dst, FrameSource::host_rows(f, m));
                    if (rc) q->pf.err = g_err;                       // the error text is per thread
                    return rc;
                });
            pf.drop_announced();     // consumed by this call, also when it failed
            return r;
        }
        int register_source(const double guess[7], double max_dist, double kernel, double sem_th,
                            double pose[7], sageicp_stats *stats) {
            // the source cloud in the Prep buffers
            return register_resident(*p->impl.map, p->prep[p->cur].d_src.data(), p->prep[p->cur].kept_levels[1],
                                     p->device, guess, max_dist, kernel, sem_th, nullptr, pose, stats);
        }
        // the quality of the new pose against the map before Update(): the source rows copied into the map handle's
        // frame buffer (on a multi-device map: rank 0's) and evaluated there as the stand-alone entry evaluates them
        int evaluate_quality(const double pose[7], double max_dist, double kernel, double sem_th) {
            if (!p->quality_on) return SAGEICP_OK;
            sageicp_map &m = *p->impl.map;
            const uint64_t n = p->prep[p->cur].kept_levels[1];
            if (n == 0 || m.empty()) return SAGEICP_OK;            // (valid stays 0)
            if (!(std::isfinite(kernel) && kernel > 0.0) || !finite_n(pose, 7)) return SAGEICP_OK;
            int rc = refresh_mirror(m);
            if (rc) return rc;
            sageicp_quality q;
            if ((rc = quality_of_device_rows(m, p->prep[p->cur].d_src.data(), n, pose, max_dist, kernel, sem_th, &q)))
                return rc;
            p->quality = q;
            return SAGEICP_OK;
        }
        int update_map(const double pose[7]) {
            const Prep &pr = p->prep[p->cur];
            const uint64_t n_fd = pr.kept_levels[0];
            if (src.kind == FrameSource::kMessage && !n_fd && p->impl.map->empty())
                return SAGEICP_OK;               // nothing into nothing
            if (p->impl.map_update_on_device_())
                return device_update_all(*p->impl.map, nullptr, n_fd, pose, pr.d_fd.data());
            std::vector<double> fd(4 * n_fd);
            if (n_fd) {
                HIPCHK(hipSetDevice(p->device));
                HIPCHK(hipMemcpy(fd.data(), pr.d_fd.data(), n_fd * sizeof(Point4), hipMemcpyDeviceToHost));
            }
            return sageicp_map_update_pose(p->impl.map, fd.data(), n_fd, pose);
        }
    };
    // (voxelize is register_frame's first step: whatever was announced is consumed by this call, also when it fails)
    int rc = p->impl.register_frame(src.read_stamps, pose_out, icp_s, total_s, n_source, stats, Backend{p, src});
    p->src_buf = p->cur;
    p->src_n = rc == SAGEICP_OK ? p->prep[p->cur].kept_levels[1] : 0;
    // the node's key-frame block runs after RegisterFrame has returned (outside the times reported above)
    if (rc == SAGEICP_OK && p->kf.on && !src.empty_message()) rc = key_frame_step(p, src.n);
    return rc;
}
// Every register entry drops the last source first: a call that is refused before it reaches pipeline_register (a bad
// argument, a device frame or timestamps that fail their checks) leaves 0 rows, as one that fails later does.
static void drop_source(sageicp_pipeline *p) {
    if (!p) return;
    p->src_n = 0;
    p->quality = sageicp_quality{};          // ... and no report
    p->places.no_frame();
}
int sageicp_pipeline_register_frame(sageicp_pipeline *p, const double *frame, uint64_t n,
                                    double pose_out[7], double *icp_s, double *total_s,
                                    uint64_t *n_source, sageicp_stats *stats) {
    drop_source(p);
    if (!p || !pose_out || (n && !frame)) return fail(SAGEICP_ERR_INVALID, "null argument");
    return pipeline_register(p, FrameSource::host_rows(frame, n), pose_out, icp_s, total_s, n_source, stats);
}
int sageicp_pipeline_register_frame_timestamps(sageicp_pipeline *p, const double *frame, const double *timestamps,
                                               uint64_t n, double pose_out[7], double *icp_s, double *total_s,
                                               uint64_t *n_source, sageicp_stats *stats) {
    drop_source(p);
    if (!p || !pose_out || (n && !frame)) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (!p->deskew_on)          // config_.deskew false: the frame passes through, the timestamps are not read
        return pipeline_register(p, FrameSource::host_rows(frame, n), pose_out, icp_s, total_s, n_source, stats);
    // checked on every frame, also before the third pose exists, so that a bad stream fails on its first frame
    if (n && !timestamps) return fail(SAGEICP_ERR_INVALID, "deskew is on and timestamps is NULL");
    for (uint64_t i = 0; i < n; ++i)
        if (!std::isfinite(timestamps[i])) return fail(SAGEICP_ERR_INVALID, "deskew is on and a timestamp is not finite");
    return pipeline_register(p, FrameSource::host_rows(frame, n, /*read_stamps*/ true, timestamps), pose_out, icp_s,
                             total_s, n_source, stats);
}
int sageicp_pipeline_register_frame_device(sageicp_pipeline *p, const sageicp_device_frame *frame,
                                           const double *timestamps, void *stream, double pose_out[7], double *icp_s,
                                           double *total_s, uint64_t *n_source, sageicp_stats *stats) {
    drop_source(p);
    if (!p || !pose_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    // without timestamps the one-argument RegisterFrame (never deskews); with deskew off they are not read (not even
    // checked), as in sageicp_pipeline_register_frame_timestamps
    const double *ts = p->deskew_on ? timestamps : nullptr;
    int rc = check_device_frame(frame, ts, stream, p->device);
    if (rc) return rc;
    return pipeline_register(p, FrameSource::device_frame(frame, ts, static_cast<hipStream_t>(stream)), pose_out,
                             icp_s, total_s, n_source, stats);
}

// ---- sensor_msgs/PointCloud2 payloads (msg.hip) ---------------------------------------------------------------------
// everything about a message that can be known without a device (include/sageicp.h: what is refused)
static int check_msg(const sageicp_msg_layout *l, const void *data, uint64_t data_bytes, uint64_t n) {
    if (!l) return fail(SAGEICP_ERR_INVALID, "message: null layout");
    if (l->point_step == 0 || l->point_step > kMsgMaxStep)
        return fail(SAGEICP_ERR_INVALID, "message: point_step must lie in [1, 1024]");
    const auto ends_within = [&](uint32_t off, uint32_t size) { return static_cast<uint64_t>(off) + size <= l->point_step; };
    if (!ends_within(l->x_offset, 4)) return fail(SAGEICP_ERR_INVALID, "message: field x ends beyond point_step");
    if (!ends_within(l->y_offset, 4)) return fail(SAGEICP_ERR_INVALID, "message: field y ends beyond point_step");
    if (!ends_within(l->z_offset, 4)) return fail(SAGEICP_ERR_INVALID, "message: field z ends beyond point_step");
    if (l->label_dtype != SAGEICP_DTYPE_UINT8 && l->label_dtype != SAGEICP_DTYPE_FLOAT32)
        return fail(SAGEICP_ERR_INVALID, "message: label_dtype must be SAGEICP_DTYPE_UINT8 or _FLOAT32");
    if (!ends_within(l->label_offset, l->label_dtype == SAGEICP_DTYPE_UINT8 ? 1 : 4))
        return fail(SAGEICP_ERR_INVALID, "message: field label ends beyond point_step");
    if (l->time_kind < 0 || l->time_kind > 2)
        return fail(SAGEICP_ERR_INVALID, "message: time_kind must be 0 (none), 1 (uint32) or 2 (float64)");
    if (l->time_kind && !ends_within(l->time_offset, l->time_kind == 1 ? 4 : 8))
        return fail(SAGEICP_ERR_INVALID, "message: the time field ends beyond point_step");
    if (n > kMaxQueries) return fail(SAGEICP_ERR_INVALID, "frame too large (2^26 - 4 points max)");
    if (data_bytes < n * l->point_step)
        return fail(SAGEICP_ERR_INVALID, "message: data holds fewer than n * point_step bytes");
    if (n && !data) return fail(SAGEICP_ERR_INVALID, "message: data is NULL");
    return SAGEICP_OK;
}
static int register_msg(sageicp_pipeline *p, const void *data, uint64_t data_bytes, uint64_t n,
                        const sageicp_msg_layout *layout, bool on_device, void *stream, double pose_out[7], double *icp_s,
                        double *total_s, uint64_t *n_source, sageicp_stats *stats) {
    drop_source(p);
    if (!p || !pose_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    int rc = check_msg(layout, data, data_bytes, n);
    if (rc) return rc;
    // deskew off: the time field is never read, whatever the layout says (OdometryServer.cpp:161-164)
    const bool read_stamps = p->deskew_on;
    if (read_stamps && layout->time_kind == 0)
        return fail(SAGEICP_ERR_INVALID, "deskew is on and the message has no time field (time_kind 0)");
    if (n && on_device) {
        if ((rc = require_device())) return rc;
        if ((rc = check_extent(data, n * layout->point_step, p->device, "message data"))) return rc;
        if ((rc = check_stream(stream, p->device))) return rc;
    }
    const FrameSource src = FrameSource::message(data, on_device, n, *layout, read_stamps, static_cast<hipStream_t>(stream));
    return pipeline_register(p, src, pose_out, icp_s, total_s, n_source, stats);
}
int sageicp_pipeline_register_frame_msg(sageicp_pipeline *p, const void *data, uint64_t data_bytes, uint64_t n,
                                        const sageicp_msg_layout *layout, double pose_out[7], double *icp_s,
                                        double *total_s, uint64_t *n_source, sageicp_stats *stats) {
    return register_msg(p, data, data_bytes, n, layout, false, nullptr, pose_out, icp_s, total_s, n_source, stats);
}
int sageicp_pipeline_register_frame_msg_device(sageicp_pipeline *p, const void *data, uint64_t data_bytes, uint64_t n,
                                               const sageicp_msg_layout *layout, void *stream, double pose_out[7],
                                               double *icp_s, double *total_s, uint64_t *n_source, sageicp_stats *stats) {
    return register_msg(p, data, data_bytes, n, layout, true, stream, pose_out, icp_s, total_s, n_source, stats);
}

// ---- the registered source cloud out (outputs.h) --------------------------------------------------------------------
// src_n rows of prep[src_buf].d_src, there on that Prep's stream
static RowSource source_rows(const sageicp_pipeline *p) {
    const Prep &pr = p->prep[p->src_buf];
    return RowSource::packed(pr.d_src.data(), p->src_n, pr.stream.get());
}
static int source_msg(const sageicp_pipeline *p, const sageicp_msg_colors *colors, void *out, uint64_t cap, bool on_device,
                      void *stream, uint64_t *n_out) {
    if (!p || !n_out || (!on_device && cap && !out)) return fail(SAGEICP_ERR_INVALID, "null argument");
    MsgColorTable t;
    int rc = color_table(colors, t);
    if (rc) return rc;
    if (on_device && (rc = check_records_out(out, cap, stream, p->device))) return rc;
    return export_rows(p->out, p->device, source_rows(p), RowSink::records_out(out, cap, t, on_device, stream), n_out);
}
int sageicp_pipeline_source_msg(const sageicp_pipeline *p, const sageicp_msg_colors *colors, void *out, uint64_t cap,
                                uint64_t *n_out) {
    return source_msg(p, colors, out, cap, false, nullptr, n_out);
}
int sageicp_pipeline_source_msg_device(const sageicp_pipeline *p, const sageicp_msg_colors *colors, void *out,
                                       uint64_t cap, void *stream, uint64_t *n_out) {
    return source_msg(p, colors, out, cap, true, stream, n_out);
}
int sageicp_pipeline_source(const sageicp_pipeline *p, double *out, uint64_t cap, uint64_t *n_out) {
    if (!p || !n_out || (cap && !out)) return fail(SAGEICP_ERR_INVALID, "null argument");
    return export_rows(p->out, p->device, source_rows(p), RowSink::host_rows(out, cap), n_out);
}
int sageicp_pipeline_source_device(const sageicp_pipeline *p, const sageicp_device_points *dst, void *stream,
                                   uint64_t *n_out) {
    if (!p || !n_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (int rc = check_device_points(dst, stream, p->device)) return rc;
    return export_rows(p->out, p->device, source_rows(p), RowSink::device_rows(dst, stream), n_out);
}
int sageicp_pipeline_set_deskew(sageicp_pipeline *p, int enable) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    p->pf.drop_all();                   // an announced or prepared frame is dropped
    p->deskew_on = enable != 0;
    return SAGEICP_OK;
}
int sageicp_pipeline_deskew_info(const sageicp_pipeline *p, int *applied, double delta_out[6]) {
    if (!p || !applied || !delta_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    *applied = p->impl.deskew_applied ? 1 : 0;
    for (int k = 0; k < 6; ++k) delta_out[k] = p->impl.deskew_delta[k];
    return SAGEICP_OK;
}
int sageicp_pipeline_prefetch(sageicp_pipeline *p, const double *frame, uint64_t n) {
    if (!p || (n && !frame)) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (p->deskew_on)
        return fail(SAGEICP_ERR_INVALID, "sageicp_pipeline_prefetch: deskew is on: a deskewed frame's Preprocess() needs "
                                         "the pose of the frame registered before it, so it cannot be prepared ahead");
    p->pf.announce(frame, n);
    return SAGEICP_OK;
}
int sageicp_pipeline_prefetch_wait(sageicp_pipeline *p) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    p->pf.join();                       // what it prepared stays
    return SAGEICP_OK;
}
int sageicp_pipeline_prefetch_cancel(sageicp_pipeline *p) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    p->pf.drop_all();                   // nothing reads an announced buffer after this
    return SAGEICP_OK;
}
int sageicp_pipeline_set_dynamic_vehicle_filter(sageicp_pipeline *p, int enable, double dy_th,
                                                int voxid, const int *landmark_labels, int n_landmark) {
    if (!p || n_landmark < 0 || (n_landmark && !landmark_labels) || !std::isfinite(dy_th))
        return fail(SAGEICP_ERR_INVALID, "bad argument");
    std::vector<int> counts, labels;
    std::vector<double> vs;
    p->impl.group_tables(counts, labels, vs);
    if (voxid < 0 || voxid >= static_cast<int>(counts.size()))
        return fail(SAGEICP_ERR_INVALID, "dynamic_vehicle_voxid is not a label group of the config");
    p->pf.drop_prepared();              // a frame prepared under the old setting
    int off = 0;
    for (int g = 0; g < voxid; ++g) off += counts[g];
    p->dyn_on = enable != 0;
    p->dyn_cfg.dy_th = dy_th;
    p->dyn_cfg.dynamic_labels.assign(labels.begin() + off, labels.begin() + off + counts[voxid]);
    p->dyn_cfg.landmark_labels.assign(landmark_labels, landmark_labels + n_landmark);
    return SAGEICP_OK;
}
int sageicp_pipeline_dynamic_filter_info(const sageicp_pipeline *p, sageicp_dynfilter_info *info) {
    if (!p || !info) return fail(SAGEICP_ERR_INVALID, "null argument");
    const Prep &pr = p->prep[p->cur];
    *info = pr.dyn_ran ? pr.dyn.info : sageicp_dynfilter_info{};
    return SAGEICP_OK;
}
int sageicp_pipeline_reinitialize(sageicp_pipeline *p) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    p->impl.reinitialize();
    p->src_n = 0;
    p->quality = sageicp_quality{};
    return SAGEICP_OK;
}
uint64_t sageicp_pipeline_num_poses(const sageicp_pipeline *p) { return p ? p->impl.poses.size() : 0; }
int sageicp_pipeline_pose(const sageicp_pipeline *p, uint64_t i, double out[7]) {
    if (!p || !out || i >= p->impl.poses.size()) return fail(SAGEICP_ERR_INVALID, "bad pose index");
    for (int k = 0; k < 7; ++k) out[k] = p->impl.poses[i].v[k];
    return SAGEICP_OK;
}
const sageicp_map *sageicp_pipeline_local_map(const sageicp_pipeline *p) {
    return p ? p->impl.map : nullptr;
}

int sageicp_pipeline_set_quality(sageicp_pipeline *p, int enable) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    p->quality_on = enable != 0;
    p->quality = sageicp_quality{};
    return SAGEICP_OK;
}
int sageicp_pipeline_quality(const sageicp_pipeline *p, sageicp_quality *out) {
    if (!p || !out) return fail(SAGEICP_ERR_INVALID, "null argument");
    *out = p->quality;
    return SAGEICP_OK;
}

int sageicp_pipeline_set_key_frames(sageicp_pipeline *p, int enable, const sageicp_occupancy_params *params) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    OccGrid g{};
    if (enable) {
        int rc = occ_grid_from(params, g);
        if (rc) return rc;
    }
    p->pf.drop_prepared();              // a frame prepared under the old setting
    auto &k = p->kf;
    k.on = enable != 0;
    if (k.on) {
        k.prm = *params;
        k.g = g;
    }
    // the bitmaps are sized for the grid at the next frame; off, nothing of the selection stays allocated
    k.d_key.reset();
    k.d_cand.reset();
    k.d_cur.reset();
    if (!k.on) {
        k.d_dec.reset();
        k.h_dec.reset();
        (void)hipSetDevice(p->device);
        p->prep[0].d_raw.reset();
        p->prep[1].d_raw.reset();
    }
    k.clear();
    (void)hipSetDevice(p->device);
    p->places.off();                    // (places describe key frames: a new selection starts without them)
    return SAGEICP_OK;
}
int sageicp_pipeline_key_frame_reset(sageicp_pipeline *p) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    p->kf.clear();
    p->places.clear();
    return SAGEICP_OK;
}
int sageicp_pipeline_set_places(sageicp_pipeline *p, int enable, const sageicp_place_params *params,
                                const sageicp_place_query *query) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    auto &pl = p->places;
    if (!enable) {
        (void)hipSetDevice(p->device);
        pl.off();
        return SAGEICP_OK;
    }
    if (!p->kf.on) return fail(SAGEICP_ERR_INVALID, "sageicp_pipeline_set_places: key-frame selection is off");
    if (int rc = place_check_params(params)) return rc;
    if (int rc = place_check_query(query)) return rc;
    if (int rc = require_device(p->device)) return rc;
    sageicp_place_db *db = place_db_new(*params, p->device);
    if (!db) return SAGEICP_ERR_HIP;    // (the message is the failing call's)
    pl.off();
    pl.db.reset(db);
    pl.on = true;
    pl.query = *query;
    pl.clear();
    return SAGEICP_OK;
}
int sageicp_pipeline_place_info(const sageicp_pipeline *p, sageicp_place_info *out) {
    if (!p || !out) return fail(SAGEICP_ERR_INVALID, "null argument");
    *out = p->places.info;
    return SAGEICP_OK;
}
const sageicp_place_db *sageicp_pipeline_place_db(const sageicp_pipeline *p) { return p ? p->places.db.get() : nullptr; }
int sageicp_pipeline_place_reset(sageicp_pipeline *p) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    p->places.clear();
    return SAGEICP_OK;
}
int sageicp_pipeline_key_frame_info(const sageicp_pipeline *p, sageicp_key_frame_info *info) {
    if (!p || !info) return fail(SAGEICP_ERR_INVALID, "null argument");
    *info = p->kf.info;
    return SAGEICP_OK;
}
// what both key-grid entries check first: the selection is on and `cap` bytes hold the grid's *cells
static int key_grid_cells(const sageicp_pipeline *p, const uint8_t *out, uint64_t cap, uint64_t *cells) {
    if (!p || !out) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (!p->kf.on) return fail(SAGEICP_ERR_INVALID, "key-frame selection is off");
    *cells = static_cast<uint64_t>(p->kf.g.h) * p->kf.g.w;
    if (cap < *cells) return fail(SAGEICP_ERR_INVALID, "the key grid needs occ_h * occ_w bytes");
    return SAGEICP_OK;
}
int sageicp_pipeline_key_frame_grid(const sageicp_pipeline *p, uint8_t *out, uint64_t cap) {
    uint64_t cells = 0;
    if (int rc = key_grid_cells(p, out, cap, &cells)) return rc;
    const auto &k = p->kf;
    if (!k.has_key) {
        std::memset(out, 0, cells);
        return SAGEICP_OK;
    }
    HIPCHK(hipSetDevice(p->device));
    return occ_bytes_to_host(k.d_key.data(), k.g, out);
}
int sageicp_pipeline_key_frame_grid_device(const sageicp_pipeline *p, uint8_t *out, uint64_t cap, void *stream) {
    uint64_t cells = 0;
    int rc = key_grid_cells(p, out, cap, &cells);
    if (!rc) rc = require_device();
    if (!rc) rc = check_extent(out, cells, p->device, "key-frame grid");
    if (!rc) rc = check_stream(stream, p->device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(p->device));
    // on the caller's stream, behind the work it enqueued before this call; synchronous
    const auto &k = p->kf;
    return occ_bytes_to_device(k.has_key ? k.d_key.data() : nullptr, k.g, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
