// C ABI of libsageicp_hip.so (include/sageicp.h): host side of the SAGE-ICP registration hot
// path on MI355X.  Owns the host-authoritative map, its HBM mirror, the per-map stream and
// scratch, the ICP launch loop (no host round trip per iteration: kernels early-exit on a
// device-resident `done` flag and the host polls it once per chunk of iterations) and the
// optional RCCL exchange of the Gauss-Newton sums for query-sharded multi-GPU runs.
//
// Reference call sites this file stands in for (cpp/sage_icp/):
//   core/Registration.cpp:113-141   RegisterFrame        -> run_icp()
//   core/VoxelHashMap.cpp:144-184   Update/AddPoints/... -> HostMap (host_map.hpp)
// There is no CPU fallback: without a HIP device the compute entries fail with
// SAGEICP_ERR_NO_DEVICE.
#include "capi_internal.h"

namespace sageicp {
thread_local std::string g_err;
std::atomic<int> g_profiling{0};
std::atomic<int> g_counting{1};
std::atomic<int> g_reference_order{1};
}  // namespace sageicp

namespace sageicp_impl {
// RegisterFrame of n points already on `device` (an uploaded frame, or the pipeline's source cloud)
int register_resident(sageicp_map &m, const Point4 *d_frame, uint64_t n, int device, const double init[7],
                      double max_dist, double kernel, double sem_th, sageicp_comm *comm, double pose_out[7],
                      sageicp_stats *stats) {
    if (!init || !pose_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (device != m.device) return fail(SAGEICP_ERR_INVALID, "frame and map live on different devices");
    if (comm && comm->device != m.device) return fail(SAGEICP_ERR_INVALID, "comm and map live on different devices");
    const double t0 = now_us();
    if (m.empty()) {
        std::memcpy(pose_out, init, 56);
        if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->n_queries = n; }
        return SAGEICP_OK;
    }
    if (!m.replicas.empty()) {
        if (comm) return fail(SAGEICP_ERR_INVALID, "a map that spans several devices shards the frame itself");
        return register_sharded(m, nullptr, d_frame, n, init, max_dist, kernel, sem_th, pose_out, stats, t0);
    }
    int rc = refresh_mirror(m);
    if (rc) return rc;
    const double us_upload = now_us() - t0;
    return run_icp(m, d_frame, n, init, max_dist, kernel, sem_th, comm, pose_out, stats, us_upload, t0);
}

}  // namespace sageicp_impl

// =============================================================================================
extern "C" {

int sageicp_abi_version(void) { return SAGEICP_ABI_VERSION; }
const char *sageicp_last_error(void) { return g_err.c_str(); }
int sageicp_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}
void sageicp_set_profiling(int level) { g_profiling = level; }
void sageicp_set_counting(int on) { g_counting = on ? 1 : 0; }
void sageicp_reload_env(void) { (void)sageicp::reload_knobs(); }
void sageicp_set_downsample_order(int reference_order) { g_reference_order = reference_order ? 1 : 0; }
int sageicp_robin_iteration_order(const int32_t *vox_xyz, uint64_t n, uint32_t *order_out) {
    if (n && (!vox_xyz || !order_out)) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (n >= (1ull << 27)) return fail(SAGEICP_ERR_INVALID, "too many voxels (2^27 max)");
    std::vector<uint32_t> h(n), order;
    for (uint64_t i = 0; i < n; ++i) h[i] = reference_voxel_hash(vox_xyz[3 * i], vox_xyz[3 * i + 1], vox_xyz[3 * i + 2]);
    order.reserve(n);
    static thread_local RobinScratch scratch;      // (exercises the reuse of the bucket arrays across calls)
    uint32_t max_probe = 0;
    if (!RobinOrderReplay::iteration_order(h.data(), n, 0u, order, &scratch, &max_probe))
        return fail(SAGEICP_ERR_CAPACITY, "a probe distance of " + std::to_string(max_probe) + " or more: beyond it "
                    "tsl::robin_map forces a growth this replay does not model (the reference's 20-bit hash: at "
                    "the latest from ~2^19 voxels)");
    std::memcpy(order_out, order.data(), n * sizeof(uint32_t));
    return SAGEICP_OK;
}

// ---- map ----------------------------------------------------------------------------------
int sageicp_robin_sweep(const int32_t *vox_xyz, uint64_t n, const uint8_t *far, int listed, uint32_t *erased_out,
                        uint64_t *n_erased, uint32_t *order_after, uint64_t *n_after) {
    if (n && (!vox_xyz || !far || !erased_out || !order_after)) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (!n_erased || !n_after) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (n >= (1ull << 27)) return fail(SAGEICP_ERR_INVALID, "too many voxels (2^27 max)");
    sageicp::RobinTable t;
    std::vector<uint32_t> h(n);
    for (uint64_t i = 0; i < n; ++i) {
        h[i] = reference_voxel_hash(vox_xyz[3 * i], vox_xyz[3 * i + 1], vox_xyz[3 * i + 2]);
        t.insert(h[i], static_cast<uint32_t>(i));
    }
    uint64_t k = 0;
    if (listed) {
        std::vector<std::pair<uint32_t, uint32_t>> lst;
        for (uint64_t i = n; i-- > 0;)          // (any order: here the reverse of arrival)
            if (far[i]) lst.emplace_back(h[i], static_cast<uint32_t>(i));
        t.sweep_erase_listed(std::move(lst), [&](uint32_t v) { erased_out[k++] = v; });
    } else {
        t.sweep_erase([&](uint32_t v) { return far[v] != 0; }, [&](uint32_t v) { erased_out[k++] = v; });
    }
    *n_erased = k;
    uint64_t a = 0;
    t.for_each([&](uint32_t v) { order_after[a++] = v; });
    *n_after = a;
    return t.valid() ? SAGEICP_OK : fail(SAGEICP_ERR_CAPACITY, "a probe distance the replay does not model");
}

sageicp_map *sageicp_map_create(double voxel_size, double max_distance, int basic, int critical,
                                const int *labels, int n_labels, int device) {
    if (!(voxel_size > 0.0) || basic < 0 || critical < 0 || basic + critical < 1 ||
        basic + critical > kMaxCap || n_labels < 0 || (n_labels > 0 && !labels)) {
        fail(SAGEICP_ERR_INVALID, "sageicp_map_create: invalid parameters (need voxel_size > 0, "
                                  "1 <= basic+critical <= 255)");
        return nullptr;
    }
    const Knobs &kn = knobs();               // (the knobs of a map's creation: read here, not per call)
    sageicp_map *m = new sageicp_map;
    m->host.configure(voxel_size, max_distance, basic, critical, labels, n_labels, kn.size_classes);
    m->device = device;
    // SAGEICP_DEVICES=0,1,2,3: every map of this process spans these devices (the knob for callers
    // that cannot be changed, e.g. the ROS node behind the header shim); the first is rank 0
    if (kn.n_devices > 1 && sageicp_map_set_devices(m, kn.devices, kn.n_devices)) {
        sageicp_map_destroy(m);
        return nullptr;
    }
    // SAGEICP_MAP_REFERENCE_ORDER=1: every map of this process is created in reference-order mode (the
    // knob for callers behind the header shim; sageicp_map_set_reference_order for everyone else)
    if (kn.map_reference_order.get()) (void)sageicp_map_set_reference_order(m, 1);
    // SAGEICP_MAP_ARCHIVE=1: every map of this process keeps what it evicts (sageicp_map_set_archive), at most
    // SAGEICP_MAP_ARCHIVE_MAX_ROWS rows of it (0 / unset: no limit)
    if (kn.map_archive.get()) (void)sageicp_map_set_archive(m, 1, kn.map_archive_max_rows);      // (64 bits: 2^31 rows are only 64 GiB)
    return m;
}

int sageicp_map_set_reference_order(sageicp_map *m, int on) {
    if (!m) return fail(SAGEICP_ERR_INVALID, "null map");
    if (!m->empty() || m->resident())
        return fail(SAGEICP_ERR_INVALID, "sageicp_map_set_reference_order: the map must be empty (the bucket order "
                                         "records every insertion since construction)");
    m->host.track_order = on != 0;
    m->host.order = sageicp::RobinTable();          // zero buckets, like a default-constructed robin_map
    for (sageicp_map *r : m->replicas)
        if (int rc = sageicp_map_set_reference_order(r, on)) return rc;
    return SAGEICP_OK;
}
int sageicp_map_reference_order(const sageicp_map *m) {
    if (!m || !m->host.track_order) return 0;
    return m->host.order.valid() ? 1 : -1;
}

int sageicp_map_set_devices(sageicp_map *m, const int *devices, int n) {
    if (!m || !devices || n < 1 || n > kMaxRanks)
        return fail(SAGEICP_ERR_INVALID, "sageicp_map_set_devices: 1..8 devices");
    if (m->sc.stream && devices[0] != m->device)
        return fail(SAGEICP_ERR_INVALID, "sageicp_map_set_devices: the map already lives on another first device");
    const int count = sageicp_device_count();
    for (int k = 0; k < n; ++k)
        if (count > 0 && (devices[k] < 0 || devices[k] >= count))
            return fail(SAGEICP_ERR_INVALID, "sageicp_map_set_devices: device ordinal out of range");
    if (int rc = ensure_host(*m)) return rc;
    for (sageicp_map *r : m->replicas) sageicp_map_destroy(r);
    m->replicas.clear();
    for (sageicp_comm *c : m->ranks) sageicp_comm_destroy(c);
    m->ranks.clear();
    m->device = devices[0];
    for (int k = 1; k < n; ++k) {
        sageicp_map *r = new sageicp_map;
        r->device = devices[k];
        r->host = m->host;                 // the same map, mirrored on its own device at first use (a new handle: nothing valid in HBM)
        m->replicas.push_back(r);
    }
    return SAGEICP_OK;
}
int sageicp_map_num_devices(const sageicp_map *m) { return m ? 1 + static_cast<int>(m->replicas.size()) : 0; }

void sageicp_map_destroy(sageicp_map *m) {
    if (!m) return;
    for (sageicp_comm *c : m->ranks) sageicp_comm_destroy(c);
    m->ranks.clear();
    for (sageicp_map *r : m->replicas) sageicp_map_destroy(r);
    m->replicas.clear();
    delete m;
}

// copy of a map whose authority is the HBM copy: device-to-device, the (stale) host side is not
// touched on either map
static int clone_on_device(const sageicp_map &src, sageicp_map *m) {
    const HostMap &h = src.host;
    m->host.configure(h.voxel_size, h.max_distance, h.basic, h.critical, h.basic_labels.data(),
                      static_cast<int>(h.basic_labels.size()), true);
    m->host.n_classes = h.n_classes;                    // (the source's size classes, whatever the knob says now)
    for (int k = 0; k < kMaxClasses; ++k) m->host.class_points[k] = h.class_points[k];
    // (a map in reference-order mode: the bucket array lives on the host whoever holds the points — "a copy has the same array")
    m->host.track_order = h.track_order;
    m->host.order = h.order;
    int rc = m->sc.init(m->device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipStreamSynchronize(src.sc.stream.get()));
    return m->dev.copy_from(src.dev, m->host, m->sc.stream.get());
}

static sageicp_map *clone_one(const sageicp_map &src) {
    sageicp_map *m = new sageicp_map;       // (nothing valid in HBM: a copy of a host map builds its own mirror on first use)
    m->device = src.device;
    if (src.resident()) {
        if (clone_on_device(src, m)) {
            sageicp_map_destroy(m);
            return nullptr;
        }
        return m;
    }
    m->host = src.host;
    return m;
}

// the archive's setting and contents (a deep copy: the device part device to device)
static int clone_archive(const sageicp_map &src, sageicp_map *m) {
    if (src.arc.dev_vox) {
        if (int rc = m->sc.init(m->device)) return rc;
        HIPCHK(hipSetDevice(m->device));
        HIPCHK(hipStreamSynchronize(src.sc.stream.get()));
    }
    return m->arc.copy_from(src.arc, m->sc.stream.get());
}

sageicp_map *sageicp_map_clone(const sageicp_map *src) {
    if (!src) return nullptr;
    sageicp_map *m = clone_one(*src);
    if (!m) return nullptr;
    if (clone_archive(*src, m)) {
        sageicp_map_destroy(m);
        return nullptr;
    }
    for (const sageicp_map *r : src->replicas) {
        sageicp_map *c = clone_one(*r);
        if (!c) {
            sageicp_map_destroy(m);
            return nullptr;
        }
        m->replicas.push_back(c);
    }
    return m;
}

int sageicp_map_clear(sageicp_map *m) {
    if (!m) return fail(SAGEICP_ERR_INVALID, "null map");
    m->dev.invalidate();      // whatever the device holds is dropped with the rest
    m->host.clear();
    for (sageicp_map *r : m->replicas) sageicp_map_clear(r);
    m->replicas_diverged = false;         // every copy is empty again
    return SAGEICP_OK;
}
int sageicp_map_empty(const sageicp_map *m) { return (!m || m->empty()) ? 1 : 0; }
uint64_t sageicp_map_size(const sageicp_map *m) { return m ? m->counts().points : 0; }
uint64_t sageicp_map_num_voxels(const sageicp_map *m) { return m ? m->counts().voxels : 0; }

int sageicp_map_add_points(sageicp_map *m, const double *xyzl, uint64_t n) {
    if (!m || (n && !xyzl)) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (m->replicas_diverged)
        return fail(SAGEICP_ERR_INVALID, "the copies of this multi-device map diverged in an earlier failed update: Clear() it");
    if (!all_finite(xyzl, n))
        return fail(SAGEICP_ERR_INVALID, "AddPoints: a coordinate or label is not finite (NaN / Inf); nothing was inserted");
    if (int rc = ensure_host(*m)) return rc;
    // A voxel index out of range is found by a dry pass: nothing is inserted then (like non-finite input
    // above).  Only the storage limits (2^24 voxels / 2^24 units of 4 points: 67 M point slots, DESIGN.md
    // section 1) can still stop a call part-way — before the point that does not fit, the points before it
    // in, the map consistent: which point that is depends on the retention policy's decisions on every
    // point before it.
    {
        const double vs = m->host.voxel_size;
        // (the range is tested on the quotient in double: casting a value beyond int32 is the undefined
        // behaviour D5 refuses to rely on; truncation toward zero keeps |index| < 2^20 exactly when |q| < 2^20)
        constexpr double kLim = 1048576.0;
        for (uint64_t i = 0; i < n; ++i) {
            const double qx = xyzl[4 * i] / vs, qy = xyzl[4 * i + 1] / vs, qz = xyzl[4 * i + 2] / vs;
            if (!(std::fabs(qx) < kLim && std::fabs(qy) < kLim && std::fabs(qz) < kLim))
                return fail(SAGEICP_ERR_CAPACITY, "AddPoints: voxel index beyond +-2^20 at point " + std::to_string(i) +
                                                      "; nothing was inserted");
        }
    }
    uint64_t at = 0;
    const int why = m->host.add_points(xyzl, n, &at);     // limits are checked before a point is taken
    // every copy of a multi-device map takes exactly the points rank 0 took: all of them, or the
    // prefix before the point a limit stopped at
    const uint64_t took = why ? at : n;
    for (sageicp_map *r : m->replicas)
        if (int rc = sageicp_map_add_points(r, xyzl, took)) {
            m->replicas_diverged = true;
            const std::string w2 = g_err;
            return fail(rc, "AddPoints reached only some devices of the map (" + w2 + "); the map must be cleared");
        }
    if (why == 1)
        return fail(SAGEICP_ERR_CAPACITY, "map full (2^24 voxels / 2^24 storage units of 4 points): stopped before point " +
                                              std::to_string(at) + ", the points before it are in");
    if (why == 2)
        return fail(SAGEICP_ERR_CAPACITY, "voxel index beyond +-2^20: stopped before point " +
                                              std::to_string(at) + ", the points before it are in");
    return SAGEICP_OK;
}

int sageicp_map_remove_far(sageicp_map *m, const double origin[3]) {
    if (!m || !origin) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (int rc = ensure_host(*m)) return rc;
    host_remove_far(*m, origin);          // (the evicted voxels into the handle's archive while it is on)
    for (sageicp_map *r : m->replicas)
        if (int rc = sageicp_map_remove_far(r, origin)) return rc;
    return SAGEICP_OK;
}

int sageicp_map_update(sageicp_map *m, const double *xyzl, uint64_t n, const double origin[3]) {
    int rc = sageicp_map_add_points(m, xyzl, n);
    if (rc) return rc;
    return sageicp_map_remove_far(m, origin);
}

int sageicp_map_update_pose(sageicp_map *m, const double *xyzl, uint64_t n, const double pose[7]) {
    if (!m || (n && !xyzl) || !pose) return fail(SAGEICP_ERR_INVALID, "null argument");
    // Update(points, pose): transform into the map frame, origin = pose.translation()
    double R[9];
    quat_to_mat(pose, R);
    std::vector<double> w(4 * n);
    for (uint64_t i = 0; i < n; ++i) {
        mat_apply(R, pose + 4, xyzl + 4 * i, &w[4 * i]);
        w[4 * i + 3] = xyzl[4 * i + 3];
    }
    return sageicp_map_update(m, w.data(), n, pose + 4);
}

int sageicp_map_update_pose_device(sageicp_map *m, const double *xyzl, uint64_t n, const double pose[7]) {
    if (!m || (n && !xyzl) || !pose) return fail(SAGEICP_ERR_INVALID, "null argument");
    return device_update_all(*m, xyzl, n, pose, nullptr);
}

int sageicp_map_resident(const sageicp_map *m) { return (m && m->resident()) ? 1 : 0; }

uint64_t sageicp_map_point_slots(const sageicp_map *m) {
    if (!m) return 0;
    return static_cast<uint64_t>(m->counts().units_hi) * kUnitPoints;
}

// ---- for tests: the slot hash, and the state of the authoritative slot table (host-side words only) ----
uint32_t sageicp_voxel_hash(int32_t x, int32_t y, int32_t z) { return sageicp::voxel_hash(x, y, z); }

int sageicp_map_table_stats(const sageicp_map *m, uint64_t out[3]) {
    if (!m || !out) return fail(SAGEICP_ERR_INVALID, "null argument");
    const MapCounts c = m->counts();    // (resident: the counters of the last device pass, kept on the host with the handle)
    out[0] = c.table_capacity;
    out[1] = c.used_slots;
    out[2] = c.voxels;
    return SAGEICP_OK;
}

int sageicp_map_sync(const sageicp_map *m) {
    if (!m) return fail(SAGEICP_ERR_INVALID, "null map");
    if (int rc = refresh_mirror(internal(m))) return rc;
    for (sageicp_map *r : m->replicas)
        if (int rc = refresh_mirror(*r)) return rc;
    return SAGEICP_OK;
}

// ---- AlignClouds ------------------------------------------------------------------------------
int sageicp_align_clouds(const double *src, const double *tgt, uint64_t n, double kernel,
                         double pose_out[7], double *JTJ_out, double *JTr_out, int device) {
    if (!pose_out || (n && (!src || !tgt))) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (n > 0x7FFFFFFFull) return fail(SAGEICP_ERR_INVALID, "too many pairs");
    Scratch sc;
    int rc = sc.init(device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    if ((rc = sc.reserve_frame(n))) return rc;
    if ((rc = sc.reserve_tgt(n))) return rc;
    hipStream_t s = sc.stream.get();
    if (n) {
        HIPCHK(hipMemcpyAsync(sc.d_frame.data(), src, n * sizeof(Point4), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sc.d_tgt.data(), tgt, n * sizeof(Point4), hipMemcpyHostToDevice, s));
    }
    double I[7];
    identity_pose(I);
    fill_state(sc.h_state.data(), I);
    HIPCHK(hipMemcpyAsync(sc.d_state.data(), sc.h_state.data(), sizeof(IcpState), hipMemcpyHostToDevice, s));
    if ((rc = sc.reserve_partials(128))) return rc;
    GnParams gp{sc.d_frame.data(), sc.d_tgt.data(), static_cast<int>(n), kernel, sc.d_partials.data()};
    FinParams fp{};
    fp.st = sc.d_state.data();
    fp.partials = sc.d_partials.data();
    fp.nparts = launch_gn(gp, s);
    fp.mode = 0;
    fp.standalone = 1;
    launch_fin(fp, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sc.h_state.data(), sc.d_state.data(), sizeof(IcpState), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // one step from identity: T_icp == est
    for (int i = 0; i < 7; ++i) pose_out[i] = sc.h_state.data()->T_icp[i];
    if (JTJ_out || JTr_out) {
        double JTJ[36], JTr[6];
        assemble_normal_equations(sc.h_state.data()->sums, JTJ, JTr);
        if (JTJ_out) std::memcpy(JTJ_out, JTJ, sizeof(JTJ));
        if (JTr_out) std::memcpy(JTr_out, JTr, sizeof(JTr));
    }
    return SAGEICP_OK;
}

// ---- TransformPoints --------------------------------------------------------------------------
int sageicp_transform_points(const double pose[7], double *xyzl, uint64_t n, int device) {
    if (!pose || (n && !xyzl)) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (n > 0x7FFFFFFFull) return fail(SAGEICP_ERR_INVALID, "too many points");
    Scratch sc;
    int rc = sc.init(device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    if ((rc = sc.reserve_frame(n))) return rc;
    hipStream_t s = sc.stream.get();
    fill_state(sc.h_state.data(), pose);
    HIPCHK(hipMemcpyAsync(sc.d_state.data(), sc.h_state.data(), sizeof(IcpState), hipMemcpyHostToDevice, s));
    if (n) {
        HIPCHK(hipMemcpyAsync(sc.d_frame.data(), xyzl, n * sizeof(Point4), hipMemcpyHostToDevice, s));
        launch_tf(sc.d_frame.data(), static_cast<int>(n), sc.d_state.data(), s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(xyzl, sc.d_frame.data(), n * sizeof(Point4), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return SAGEICP_OK;
}

// ---- RegisterFrame ----------------------------------------------------------------------------
int sageicp_register_frame(const sageicp_map *map, const double *frame, uint64_t n,
                           const double init[7], double max_dist, double kernel, double sem_th,
                           double pose_out[7], sageicp_stats *stats) {
    if (!map || !init || !pose_out || (n && !frame)) return fail(SAGEICP_ERR_INVALID, "null argument");
    sageicp_map &m = internal(map);
    const double t0 = now_us();
    if (m.empty()) {   // Registration.cpp:119
        std::memcpy(pose_out, init, 56);
        if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->n_queries = n; }
        return SAGEICP_OK;
    }
    if (!m.replicas.empty())
        return register_sharded(m, frame, nullptr, n, init, max_dist, kernel, sem_th, pose_out, stats, t0);
    int rc = refresh_mirror(m);
    if (rc) return rc;
    Scratch &sc = m.sc;
    if ((rc = sc.reserve_frame(n))) return rc;
    if (n) HIPCHK(hipMemcpyAsync(sc.d_frame.data(), frame, n * sizeof(Point4), hipMemcpyHostToDevice,
                                 sc.stream.get()));
    const double us_upload = now_us() - t0;
    return run_icp(m, sc.d_frame.data(), n, init, max_dist, kernel, sem_th, nullptr, pose_out, stats,
                   us_upload, t0);
}

int sageicp_map_loop_status(const sageicp_map *m, sageicp_loop_status *out) {
    if (!m || !out) return fail(SAGEICP_ERR_INVALID, "null argument");
    const Scratch &sc = m->sc;
    out->calls_single_launch = sc.calls_single_launch;
    out->calls_per_iteration = sc.calls_per_iteration;
    out->calls_chained = sc.calls_chained;
    out->timeouts = sc.loop_timeouts;
    out->cooldown_calls = static_cast<uint32_t>(std::max(0, sc.loop_cooldown));
    out->derate_workgroups = 32u * static_cast<uint32_t>(std::max(0, sc.loop_derate));
    out->last_fallback = sc.last_fallback;
    return SAGEICP_OK;
}

// a frame of n rows on the map's device, its memory allocated (the first step of both frame entries; nullptr: failed)
static std::unique_ptr<sageicp_frame> new_frame(sageicp_map &m, uint64_t n) {
    if (m.sc.init(m.device)) return nullptr;
    if (hipSetDevice(m.device) != hipSuccess) { fail(SAGEICP_ERR_HIP, "hipSetDevice"); return nullptr; }
    auto f = std::make_unique<sageicp_frame>();
    f->device = m.device;
    f->n = n;
    if (f->d.reserve(std::max<uint64_t>(n, 1)) != hipSuccess) { fail(SAGEICP_ERR_HIP, "hipMalloc(frame)"); return nullptr; }
    return f;
}

sageicp_frame *sageicp_frame_upload(const sageicp_map *m, const double *frame, uint64_t n) {
    if (!m || (n && !frame)) { fail(SAGEICP_ERR_INVALID, "null argument"); return nullptr; }
    std::unique_ptr<sageicp_frame> f = new_frame(internal(m), n);
    if (!f) return nullptr;
    if (n && hipMemcpy(f->d.data(), frame, n * sizeof(Point4), hipMemcpyHostToDevice) != hipSuccess) {
        fail(SAGEICP_ERR_HIP, "hipMemcpy(frame)");
        return nullptr;
    }
    return f.release();
}

void sageicp_frame_destroy(sageicp_frame *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    delete f;
}

sageicp_frame *sageicp_frame_from_device(const sageicp_map *m, const sageicp_device_frame *fr, void *stream) {
    if (!m) { fail(SAGEICP_ERR_INVALID, "null argument"); return nullptr; }
    if (check_device_frame(fr, nullptr, stream, m->device)) return nullptr;
    std::unique_ptr<sageicp_frame> f = new_frame(internal(m), fr->n);
    if (!f) return nullptr;
    // on the caller's stream, behind the work that wrote the buffers; synchronous: afterwards nothing reads them
    const hipStream_t s = static_cast<hipStream_t>(stream);
    launch_ingest(ingest_args(*fr), f->d.data(), s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        fail(SAGEICP_ERR_HIP, std::string("ingest of a device frame: ") + hipGetErrorString(e));
        return nullptr;
    }
    return f.release();
}

int sageicp_register_frame_resident(const sageicp_map *m, const sageicp_frame *f,
                                    const double init[7], double max_dist, double kernel,
                                    double sem_th, sageicp_comm *comm, double pose_out[7],
                                    sageicp_stats *stats) {
    if (!f || !m) return fail(SAGEICP_ERR_INVALID, "null argument");
    return register_resident(internal(m), f->d.data(), f->n, f->device, init, max_dist, kernel, sem_th, comm, pose_out, stats);
}

// ---- RCCL communicator ------------------------------------------------------------------------
int sageicp_comm_unique_id(uint8_t id_out[SAGEICP_UNIQUE_ID_BYTES]) {
    if (!id_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    int rc = load_rccl();
    if (rc) return rc;
    static_assert(sizeof(ncclUniqueId) == SAGEICP_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) return fail(SAGEICP_ERR_RCCL, "ncclGetUniqueId failed");
    std::memcpy(id_out, &id, sizeof(id));
    return SAGEICP_OK;
}

sageicp_comm *sageicp_comm_create(const uint8_t id_in[SAGEICP_UNIQUE_ID_BYTES], int rank,
                                  int nranks, int device) {
    if (!id_in || nranks < 1 || rank < 0 || rank >= nranks) {
        fail(SAGEICP_ERR_INVALID, "sageicp_comm_create: bad rank/nranks");
        return nullptr;
    }
    if (load_rccl()) return nullptr;
    if (hipSetDevice(device) != hipSuccess) { fail(SAGEICP_ERR_HIP, "hipSetDevice"); return nullptr; }
    ncclUniqueId id;
    std::memcpy(&id, id_in, sizeof(id));
    sageicp_comm *c = new sageicp_comm;
    c->rank = rank; c->nranks = nranks; c->device = device;
    ncclResult_t r = g_rccl.CommInitRank(&c->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        fail(SAGEICP_ERR_RCCL, std::string("ncclCommInitRank: ") +
                                   (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?"));
        delete c;
        return nullptr;
    }
    return c;
}

sageicp_comm *sageicp_comm_create_local(int rank, int nranks, int device) {
    if (nranks < 1 || nranks > kMaxRanks || rank < 0 || rank >= nranks) {
        fail(SAGEICP_ERR_INVALID, "sageicp_comm_create_local: bad rank/nranks (at most 8 ranks)");
        return nullptr;
    }
    sageicp_comm *c = new sageicp_comm;
    c->rank = rank; c->nranks = nranks; c->device = device;
    return c;
}

int sageicp_comm_p2p_export(sageicp_comm *c, uint8_t handle_out[SAGEICP_P2P_HANDLE_BYTES]) {
    if (!c || !handle_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (c->nranks > kMaxRanks) return fail(SAGEICP_ERR_INVALID, "direct exchange: at most 8 ranks");
    static_assert(sizeof(hipIpcMemHandle_t) == SAGEICP_P2P_HANDLE_BYTES, "hipIpcMemHandle_t size");
    HIPCHK(hipSetDevice(c->device));
    if (!c->my_block) {
        // fine-grained: peers' stores and this rank's polling loads bypass the non-coherent caches
        HIPCHK(hipExtMallocWithFlags(reinterpret_cast<void **>(&c->my_block), sizeof(P2pBlock),
                                     hipDeviceMallocFinegrained));
        HIPCHK(hipMemset(c->my_block, 0, sizeof(P2pBlock)));
        HIPCHK(c->d_exchanges.reserve(1));
        HIPCHK(hipMemset(c->d_exchanges.data(), 0, sizeof(unsigned long long)));
        HIPCHK(hipDeviceSynchronize());
    }
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, c->my_block));
    std::memcpy(handle_out, &h, sizeof(h));
    return SAGEICP_OK;
}

int sageicp_comm_p2p_connect(sageicp_comm *c, const uint8_t *handles) {
    if (!c || !handles) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (!c->my_block) return fail(SAGEICP_ERR_INVALID, "sageicp_comm_p2p_export first");
    HIPCHK(hipSetDevice(c->device));
    for (int r = 0; r < c->nranks; ++r) {
        if (r == c->rank) { c->blocks[r] = c->my_block; continue; }
        if (c->blocks[r]) continue;
        hipIpcMemHandle_t h;
        std::memcpy(&h, handles + static_cast<size_t>(r) * SAGEICP_P2P_HANDLE_BYTES, sizeof(h));
        void *p = nullptr;
        HIPCHK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
        c->blocks[r] = static_cast<P2pBlock *>(p);
    }
    c->p2p = true;
    return SAGEICP_OK;
}

int sageicp_comm_p2p_enable(sageicp_comm *c, int on) {
    if (!c) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (on) {
        if (c->poisoned)
            return fail(SAGEICP_ERR_INVALID, "direct exchange failed earlier on this communicator: "
                                             "create a new communicator and connect it");
        for (int r = 0; r < c->nranks; ++r)
            if (!c->blocks[r]) return fail(SAGEICP_ERR_INVALID, "direct exchange is not connected");
    }
    c->p2p = on != 0;
    return SAGEICP_OK;
}

int sageicp_comm_p2p_enabled(const sageicp_comm *c) { return c && c->p2p ? 1 : 0; }

int sageicp_comm_describe(const sageicp_comm *c, sageicp_comm_info *out) {
    if (!c || !out) return fail(SAGEICP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    out->rank = c->rank;
    out->nranks = c->nranks;
    out->device = c->device;
    out->rccl_ranks = out->rccl_rank = -1;
    if (c->comm) {
        out->has_rccl = 1;
        int v = -1;
        if (g_rccl.CommCount && g_rccl.CommCount(c->comm, &v) == ncclSuccess) out->rccl_ranks = v;
        v = -1;
        if (g_rccl.CommUserRank && g_rccl.CommUserRank(c->comm, &v) == ncclSuccess) out->rccl_rank = v;
    }
    out->p2p_connected = 1;
    for (int r = 0; r < c->nranks && r < kMaxRanks; ++r)
        if (!c->blocks[r]) out->p2p_connected = 0;
    if (c->nranks > kMaxRanks) out->p2p_connected = 0;
    out->p2p_enabled = c->p2p ? 1 : 0;
    out->p2p_poisoned = c->poisoned ? 1 : 0;
    return SAGEICP_OK;
}

void sageicp_comm_destroy(sageicp_comm *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (int r = 0; r < c->nranks && r < kMaxRanks; ++r)
        if (r != c->rank && c->blocks[r] && !c->peer_mapped) (void)hipIpcCloseMemHandle(c->blocks[r]);
    if (c->my_block) (void)hipFree(c->my_block);
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    delete c;
}

// ---- Preprocess / VoxelDownsample on the device --------------------------------------------------
// The one level of `job` on a Prep of its own on `device`, its cloud copied to out; info: the dynamic filter's, with
// job.dyn
static int prep_one_level(int device, const double *frame, uint64_t n, const PrepJob &job, double *out, uint64_t *n_out,
                          sageicp_dynfilter_info *info) {
    Prep pr;
    int rc = pr.init(device);
    if (rc) return rc;
    if ((rc = pr.run(FrameSource::host_rows(frame, n), job))) return rc;
    *n_out = pr.kept_levels[0];
    if ((rc = pr.fetch(0, out))) return rc;
    if (info) *info = pr.dyn.info;
    return SAGEICP_OK;
}

int sageicp_preprocess(const double *frame, uint64_t n, double max_range, double min_range,
                       double label_max_range, double *out, uint64_t *n_out, int device) {
    if (!n_out || (n && (!frame || !out))) return fail(SAGEICP_ERR_INVALID, "null argument");
    PrepJob job;
    job.max_range = max_range; job.min_range = min_range; job.label_max_range = label_max_range;
    job.n_levels = 1;
    job.levels[0] = {/*crop*/ 1, /*scale*/ 0.0};         // crop only
    return prep_one_level(device, frame, n, job, out, n_out, nullptr);
}

int sageicp_voxel_downsample(const double *frame, uint64_t n, int n_groups,
                             const int *group_label_counts, const int *group_labels,
                             const double *group_voxel_size, double vox_scale, double *out,
                             uint64_t *n_out, int device) {
    if (!n_out || (n && (!frame || !out)) || n_groups < 0 ||
        (n_groups && (!group_label_counts || !group_labels || !group_voxel_size)) || !(vox_scale > 0.0))
        return fail(SAGEICP_ERR_INVALID, "bad argument");
    // (p / vs of a NaN size is NaN and its cast to int undefined; a size of 0 puts every index beyond the key range)
    for (int g = 0; g < n_groups; ++g) {
        const double vs = group_voxel_size[g] * vox_scale;
        if (!(std::isfinite(vs) && vs > 0.0))
            return fail(SAGEICP_ERR_INVALID, "a label group's voxel size times vox_scale is not finite or not above 0");
    }
    PrepJob job;
    job.n_groups = n_groups;
    job.group_counts = group_label_counts; job.group_labels = group_labels; job.group_voxel_size = group_voxel_size;
    job.n_levels = 1;
    job.levels[0] = {/*crop*/ 0, vox_scale};
    return prep_one_level(device, frame, n, job, out, n_out, nullptr);
}

int sageicp_preprocess_dynamic(const double *frame, uint64_t n, double max_range, double min_range,
                               double label_max_range, double dy_th, const int *dynamic_labels, int n_dynamic,
                               const int *landmark_labels, int n_landmark, double *out, uint64_t *n_out,
                               sageicp_dynfilter_info *info, int device) {
    if (!n_out || (n && (!frame || !out)) || n_dynamic < 0 || n_landmark < 0 || (n_dynamic && !dynamic_labels) ||
        (n_landmark && !landmark_labels) || !std::isfinite(dy_th))
        return fail(SAGEICP_ERR_INVALID, "bad argument");
    if (info) *info = sageicp_dynfilter_info{};
    DynFilterConfig cfg;
    cfg.dy_th = dy_th;
    cfg.dynamic_labels.assign(dynamic_labels, dynamic_labels + n_dynamic);
    cfg.landmark_labels.assign(landmark_labels, landmark_labels + n_landmark);
    PrepJob job;
    job.max_range = max_range; job.min_range = min_range; job.label_max_range = label_max_range;
    job.dyn = &cfg;
    job.n_levels = 1;
    job.levels[0] = {/*crop*/ 0, /*scale*/ 0.0};         // a pass-through level: the filtered cloud, downloaded
    return prep_one_level(device, frame, n, job, out, n_out, info);
}

int sageicp_cluster_emission_order(const uint32_t *sizes, uint64_t n, uint32_t *order_out) {
    if (n && (!sizes || !order_out)) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (n >= (1ull << 32)) return fail(SAGEICP_ERR_INVALID, "too many clusters");
    cluster_emission_order(sizes, static_cast<size_t>(n), order_out);
    return SAGEICP_OK;
}

// ---- DeSkewScan on the device (deskew.hip) -----------------------------------------------------------
int sageicp_deskew_scan(const double *frame, const double *timestamps, uint64_t n, const double start_pose[7],
                        const double finish_pose[7], double *out, int device) {
    if (!start_pose || !finish_pose || (n && (!frame || !timestamps || !out)))
        return fail(SAGEICP_ERR_INVALID, "null argument");
    if (n > kMaxQueries) return fail(SAGEICP_ERR_INVALID, "frame too large (2^26 - 4 points max)");
    if (!finite_n(start_pose, 7) || !finite_n(finish_pose, 7)) return fail(SAGEICP_ERR_INVALID, "a pose is not finite");
    if (!finite_n(timestamps, n)) return fail(SAGEICP_ERR_INVALID, "a timestamp is not finite (NaN / Inf)");
    if (!finite_n(frame, 4 * n)) return fail(SAGEICP_ERR_INVALID, "a point is not finite (NaN / Inf)");
    // Deskew.cpp:36: delta_pose = (start_pose.inverse() * finish_pose).log(), once per frame on the host
    double inv[7], rel[7];
    DeskewTangent delta;
    se3_inv(start_pose, inv);
    se3_mul(inv, finish_pose, rel);
    se3_log(rel, delta.v);
    if (n == 0) return SAGEICP_OK;
    int rc = require_device(device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    DevBuf<Point4> d_p;
    DevBuf<double> d_t;
    OwnedStream s;                      // (after the buffers: waited for before they are freed)
    HIPCHK(s.create());
    HIPCHK(d_p.reserve(n));
    HIPCHK(d_t.reserve(n));
    HIPCHK(hipMemcpyAsync(d_p.data(), frame, n * sizeof(Point4), hipMemcpyHostToDevice, s.get()));
    HIPCHK(hipMemcpyAsync(d_t.data(), timestamps, n * sizeof(double), hipMemcpyHostToDevice, s.get()));
    launch_deskew(d_p.data(), d_p.data(), d_t.data(), static_cast<int>(n), delta, s.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_p.data(), n * sizeof(Point4), hipMemcpyDeviceToHost, s.get()));
    HIPCHK(hipStreamSynchronize(s.get()));
    return SAGEICP_OK;
}

uint32_t sageicp_msg_output_fields(sageicp_msg_field *out, uint32_t cap) {
    static const sageicp_msg_field kFields[5] = {          // CreatePointCloud2Msg, Utils.hpp:109-113
        {"x", SAGEICP_MSG_X_OFFSET, SAGEICP_MSG_FIELD_FLOAT32, 1},
        {"y", SAGEICP_MSG_Y_OFFSET, SAGEICP_MSG_FIELD_FLOAT32, 1},
        {"z", SAGEICP_MSG_Z_OFFSET, SAGEICP_MSG_FIELD_FLOAT32, 1},
        {"label", SAGEICP_MSG_LABEL_OFFSET, SAGEICP_MSG_FIELD_UINT8, 1},
        {"rgb", SAGEICP_MSG_RGB_OFFSET, SAGEICP_MSG_FIELD_UINT32, 1}};
    for (uint32_t i = 0; out && i < std::min<uint32_t>(cap, 5); ++i) out[i] = kFields[i];
    return 5;
}

// ---- KITTI trajectory metrics (metrics/Metrics.cpp) ------------------------------------------------
static std::vector<sageicp::metrics::M4> to_m4(const double *p, uint64_t n) {
    std::vector<sageicp::metrics::M4> v(n);
    for (uint64_t i = 0; i < n; ++i) std::memcpy(v[i].m, p + 16 * i, 16 * sizeof(double));
    return v;
}
int sageicp_metrics_seq_error(const double *poses_gt, const double *poses_result, uint64_t n,
                              float *avg_trans_error, float *avg_rot_error) {
    if (!avg_trans_error || !avg_rot_error || (n && (!poses_gt || !poses_result)))
        return fail(SAGEICP_ERR_INVALID, "null argument");
    sageicp::metrics::seq_error(to_m4(poses_gt, n), to_m4(poses_result, n), avg_trans_error, avg_rot_error);
    return SAGEICP_OK;
}
int sageicp_metrics_absolute_trajectory_error(const double *poses_gt, const double *poses_result,
                                              uint64_t n, float *ate_rot, float *ate_trans) {
    if (!ate_rot || !ate_trans || !n || !poses_gt || !poses_result)
        return fail(SAGEICP_ERR_INVALID, "null argument or empty trajectory");
    sageicp::metrics::absolute_trajectory_error(to_m4(poses_gt, n), to_m4(poses_result, n), ate_rot, ate_trans);
    return SAGEICP_OK;
}

}  // extern "C"

// probes: the loop state the last RegisterFrame of this map left on the host (pose T[7], T_icp[7], the last
// reduced sums [20], iterations, last step)
extern "C" int sageicp_debug_last_state(const sageicp_map *m, double *out36) {
    if (!m || !m->sc.h_state.data()) return SAGEICP_ERR_INVALID;
    const sageicp::IcpState &st = *m->sc.h_state.data();
    for (int i = 0; i < 7; ++i) out36[i] = st.T[i];
    for (int i = 0; i < 7; ++i) out36[7 + i] = st.T_icp[i];
    for (int i = 0; i < sageicp::kNumSums; ++i) out36[14 + i] = st.sums[i];
    out36[34] = st.iter;
    out36[35] = st.last_step_norm;
    return SAGEICP_OK;
}

#ifdef SAGE_NN_TIMING
// probe: map points handed to every query in the last iteration (sorted order)
extern "C" int sageicp_debug_work(const sageicp_map *m, uint32_t *out, size_t n) {
    if (!m || !m->sc.d_work.data()) return SAGEICP_ERR_INVALID;
    return hipMemcpy(out, m->sc.d_work.data(), n * 4, hipMemcpyDeviceToHost) == hipSuccess ? SAGEICP_OK : SAGEICP_ERR_HIP;
}
#endif
