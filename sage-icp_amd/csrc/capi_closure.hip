// A loop closure on the host side of libsageicp_hip.so (closure.h): the corrections of a trajectory (fp64,
// host arithmetic of se3_math.h, no device), and the C entries that tie every voxel of a session's map to a pose (the
// stays) and export the session's map re-posed — the selection and the walk are closure.hip's, the session's two parts
// capi_recall.hip's, the way out export_rows (outputs.h).  Host code only.
#include "capi_internal.h"
#include "closure.h"

namespace sageicp_impl {
namespace {

constexpr double kMaxClosureAngle = 3.14159265358979323846 - 1e-6;

inline double dist3(const double *a, const double *b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return std::sqrt((dx * dx + dy * dy) + dz * dz);
}

bool zero_quaternion(const double *T) { return T[0] == 0.0 && T[1] == 0.0 && T[2] == 0.0 && T[3] == 0.0; }

int corrections(const double *poses, uint64_t n, uint64_t i, uint64_t j, const double closed[7], double *corr_out, double *poses_out,
                sageicp_closure_info *info) {
    if (!poses || !closed || !corr_out) return fail(SAGEICP_ERR_INVALID, "closure: null argument");
    if (n == 0 || i >= j || j >= n) return fail(SAGEICP_ERR_INVALID, "closure: needs i < j < n");
    if (!finite_n(poses, 7 * n) || !finite_n(closed, 7)) return fail(SAGEICP_ERR_INVALID, "closure: a pose is not finite");
    if (zero_quaternion(closed)) return fail(SAGEICP_ERR_INVALID, "closure: a quaternion of norm 0");
    for (uint64_t k = 0; k < n; ++k)
        if (zero_quaternion(poses + 7 * k)) return fail(SAGEICP_ERR_INVALID, "closure: a quaternion of norm 0");
    const double *Pj = poses + 7 * j, *c = Pj + 4;
    double inv[7], delta[7];
    se3_inv(Pj, inv);
    se3_mul(closed, inv, delta);
    // D = Tr(-c) delta Tr(c): delta's rotation, and where delta takes the pivot, relative to it
    double R[9], u[3], D[7], a[6];
    quat_to_mat(delta, R);
    mat_apply(R, delta + 4, c, u);
    for (int m = 0; m < 4; ++m) D[m] = delta[m];
    for (int m = 0; m < 3; ++m) D[4 + m] = u[m] - c[m];
    se3_log(D, a);
    const double angle = std::sqrt((a[3] * a[3] + a[4] * a[4]) + a[5] * a[5]);
    if (!finite_n(delta, 7) || !finite_n(a, 6) || !(angle <= kMaxClosureAngle))
        return fail(SAGEICP_ERR_INVALID, "closure: delta turns by more than pi - 1e-6 (that is not drift)");
    double path = 0.0;
    for (uint64_t m = i + 1; m <= j; ++m) path += dist3(poses + 7 * m + 4, poses + 7 * (m - 1) + 4);
    if (!std::isfinite(path)) return fail(SAGEICP_ERR_INVALID, "closure: the path length is not finite");
    // ---- nothing is refused from here on ----
    const double I[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    const double negc[3] = {-c[0], -c[1], -c[2]};
    double run = 0.0;
    for (uint64_t k = 0; k < n; ++k) {
        double *C = corr_out + 7 * k;
        const double *Pk = poses + 7 * k;
        if (k <= i) {                                // the two ends do not pass through log or exp
            std::memcpy(C, I, sizeof(I));
            if (poses_out && poses_out != poses) std::memmove(poses_out + 7 * k, Pk, 7 * sizeof(double));
            continue;
        }
        if (k >= j) {
            std::memcpy(C, delta, sizeof(delta));
        } else {
            run += dist3(Pk + 4, Pk - 7 + 4);
            const double alpha = path > 0.0 ? run / path : static_cast<double>(k - i) / static_cast<double>(j - i);
            double sa[6], E[7], RE[9], v[3];
            for (int m = 0; m < 6; ++m) sa[m] = alpha * a[m];
            se3_exp(sa, E);
            quat_to_mat(E, RE);
            mat_apply(RE, E + 4, negc, v);           // C_k = Tr(c) E Tr(-c)
            for (int m = 0; m < 4; ++m) C[m] = E[m];
            for (int m = 0; m < 3; ++m) C[4 + m] = v[m] + c[m];
        }
        if (poses_out) {
            double O[7];
            se3_mul(C, Pk, O);
            std::memcpy(poses_out + 7 * k, O, sizeof(O));
        }
    }
    if (info) {
        sageicp_closure_info o{};
        std::memcpy(o.delta, delta, sizeof(delta));
        o.angle = angle;
        o.shift = std::sqrt((D[4] * D[4] + D[5] * D[5]) + D[6] * D[6]);
        o.path = path;
        o.i = i;
        o.j = j;
        *info = o;
    }
    return SAGEICP_OK;
}

// ---- the stays and the re-posed export ------------------------------------------------------------------------------------
struct PartScratch {
    DevBuf<uint32_t> flag, sel, n_sel, cnt, off, stay;
    int reserve(ClosurePart &c) {
        const size_t n = c.P.n_cand;
        if (!n) return SAGEICP_OK;
        HIPCHK(flag.reserve(n)); HIPCHK(sel.reserve(n)); HIPCHK(n_sel.reserve(1));
        HIPCHK(cnt.reserve(n + 1)); HIPCHK(off.reserve(n + 1)); HIPCHK(stay.reserve(n));
        c.P.flag = flag.data(); c.P.sel = sel.data(); c.P.n_sel = n_sel.data();
        c.cnt = cnt.data(); c.off = off.data(); c.stay = stay.data();
        return SAGEICP_OK;
    }
};

struct ClosureJob {
    sageicp_map &m;
    int which;
    ClosureJob(sageicp_map &map, int w) : m(map), which(w) {}
    hipStream_t s = nullptr;         // the map's: its archive and its HBM copy are used on it
    SessionParts sp;
    PartScratch ps[2];
    ClosurePart part[2]{};
    DevBuf<double> d_pos, d_corr;
    DevBuf<unsigned char> temp;
    uint32_t voxels[2] = {0, 0}, rows[2] = {0, 0};   // what the one wait brings back
};

}  // namespace

// (capi_internal.h: the rebuild's entries make the same checks)
int check_selection(const sageicp_map *m, int which, const double *positions, uint64_t n, const uint64_t *n_out, const char *who) {
    const std::string w(who);
    if (!m || !positions || !n_out) return fail(SAGEICP_ERR_INVALID, w + ": null argument");
    if (which != SAGEICP_ARCHIVE_ALL && which != SAGEICP_ARCHIVE_LATEST && which != SAGEICP_SESSION)
        return fail(SAGEICP_ERR_INVALID, w + ": which is SAGEICP_ARCHIVE_ALL, SAGEICP_ARCHIVE_LATEST or SAGEICP_SESSION");
    if (n == 0 || n > 0xFFFFFFFFull) return fail(SAGEICP_ERR_INVALID, w + ": n is 0 or beyond 2^32 - 1 positions");
    if (!finite_n(positions, 3 * n)) return fail(SAGEICP_ERR_INVALID, w + ": a position is not finite");
    return SAGEICP_OK;
}

namespace {

// the selection of `which`, every voxel's stay, and the one wait for the totals
int stays(ClosureJob &j, const double *positions, uint64_t n) {
    sageicp_map &m = j.m;
    int rc = require_device(m.device);
    if (rc) return rc;
    if ((rc = m.sc.init(m.device))) return rc;
    HIPCHK(hipSetDevice(m.device));
    j.s = m.sc.stream.get();
    const bool latest = j.which != SAGEICP_ARCHIVE_ALL;
    if ((rc = session_archive_part(m, j.s, latest, j.sp))) return rc;
    if (j.which == SAGEICP_SESSION && (rc = session_live_part(m, j.s, j.sp))) return rc;
    // (the scans count rows in 32 bits, as LATEST's and recall's do)
    if (m.arc.dev_rows + m.counts().points >= 0xFFFFFFFFull) return fail(SAGEICP_ERR_CAPACITY, "closure: more than 2^32 - 2 rows");
    HIPCHK(j.d_pos.reserve(3 * n));
    HIPCHK(hipMemcpyAsync(j.d_pos.data(), positions, 3 * n * sizeof(double), hipMemcpyHostToDevice, j.s));
    HIPCHK(j.temp.reserve(std::max(closure_temp_bytes(j.sp.part[0].n_cand), closure_temp_bytes(j.sp.part[1].n_cand))));
    const double max_dist2 = m.host.max_distance * m.host.max_distance;      // formed once, as the update's is
    for (int k = 0; k < 2; ++k) {
        ClosurePart &c = j.part[k];
        c.P = j.sp.part[k];
        if (!c.P.n_cand) continue;
        if ((rc = j.ps[k].reserve(c))) return rc;
        HIPCHK(closure_select(c, j.temp.data(), j.temp.capacity(), j.s));
        HIPCHK(closure_stays(c, j.d_pos.data(), static_cast<uint32_t>(n), max_dist2, j.s));
        HIPCHK(hipMemcpyAsync(&j.voxels[k], c.P.n_sel, sizeof(uint32_t), hipMemcpyDeviceToHost, j.s));
        HIPCHK(hipMemcpyAsync(&j.rows[k], c.off + c.P.n_cand, sizeof(uint32_t), hipMemcpyDeviceToHost, j.s));
    }
    HIPCHK(hipStreamSynchronize(j.s));
    return SAGEICP_OK;
}

int session_stays(sageicp_map &m, int which, uint64_t first, const double *positions, uint64_t n, uint32_t *out, uint64_t cap,
                  uint64_t *n_out) {
    *n_out = 0;
    ClosureJob j(m, which);
    int rc = stays(j, positions, n);
    if (rc) {
        if (j.s) (void)hipStreamSynchronize(j.s);
        return rc;
    }
    const uint64_t total = static_cast<uint64_t>(j.voxels[0]) + j.voxels[1];
    *n_out = total;
    if (!out || first >= total) return SAGEICP_OK;
    const uint64_t last = first + std::min(cap, total - first);
    uint64_t base = 0;
    for (int k = 0; k < 2; ++k) {
        const uint64_t a = std::max(first, base), b = std::min<uint64_t>(last, base + j.voxels[k]);
        if (a < b) HIPCHK(hipMemcpy(out + (a - first), j.part[k].stay + (a - base), (b - a) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        base += j.voxels[k];
    }
    return SAGEICP_OK;
}

int session_corrected(sageicp_map &m, int which, uint64_t first, const double *positions, const double *corr, uint64_t n,
                      const RowSink &sink, uint64_t *n_out) {
    *n_out = 0;
    ClosureJob j(m, which);
    DevBuf<Point4> buf;              // (declared before anything runs into it; the stream is waited for on every path)
    auto run = [&]() -> int {
        if (int rc = stays(j, positions, n)) return rc;
        const uint64_t total = static_cast<uint64_t>(j.rows[0]) + j.rows[1];
        *n_out = total;
        if (first >= total) return SAGEICP_OK;
        const uint64_t want = std::min(sink.cap, total - first);
        if (!want) return SAGEICP_OK;
        const uint64_t last = first + want;
        HIPCHK(j.d_corr.reserve(7 * n));
        HIPCHK(hipMemcpyAsync(j.d_corr.data(), corr, 7 * n * sizeof(double), hipMemcpyHostToDevice, j.s));
        HIPCHK(buf.reserve(want));
        uint64_t base = 0;
        for (int k = 0; k < 2; ++k) {
            const uint64_t a = std::max(first, base), b = std::min<uint64_t>(last, base + j.rows[k]);
            if (a < b)
                HIPCHK(closure_move(j.part[k], j.d_corr.data(), static_cast<uint32_t>(a - base), static_cast<uint32_t>(b - base),
                                    buf.data() + (a - first), j.s));
            base += j.rows[k];
        }
        HIPCHK(hipStreamSynchronize(j.s));
        uint64_t n_packed = 0;
        return export_rows(m.out, m.device, RowSource::packed(buf.data(), want, j.s), sink, &n_packed);
    };
    const int rc = run();
    if (rc && j.s) (void)hipStreamSynchronize(j.s);
    return rc;
}

}  // namespace

int check_corrections(const double *corr, uint64_t n, const char *who) {
    if (!corr) return fail(SAGEICP_ERR_INVALID, std::string(who) + ": null argument");
    if (!finite_n(corr, 7 * n)) return fail(SAGEICP_ERR_INVALID, std::string(who) + ": a correction is not finite");
    return SAGEICP_OK;
}

// serial s of the archive is pose s only if the archive was on from the first frame and nothing interrupted the count
int pipeline_positions(const sageicp_pipeline *p, const char *who, std::vector<double> &pos, std::vector<double> *poses) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    sageicp_archive_info ai{};
    if (int rc = sageicp_map_archive_info(sageicp_pipeline_local_map(p), &ai)) return rc;
    const uint64_t n = sageicp_pipeline_num_poses(p);
    if (n == 0 || ai.updates != n)
        return fail(SAGEICP_ERR_INVALID, std::string(who) + ": the archive's updates differ from the pipeline's poses (it was not on from "
                                                            "the first frame, or the count was interrupted)");
    pos.resize(3 * n);
    if (poses) poses->resize(7 * n);
    for (uint64_t k = 0; k < n; ++k) {
        double T[7];
        if (int rc = sageicp_pipeline_pose(p, k, T)) return rc;
        for (int m = 0; m < 3; ++m) pos[3 * k + m] = T[4 + m];
        if (poses) std::memcpy(poses->data() + 7 * k, T, sizeof(T));
    }
    return SAGEICP_OK;
}

}  // namespace sageicp_impl

extern "C" {

int sageicp_closure_corrections(const double *poses, uint64_t n, uint64_t i, uint64_t j, const double closed[7],
                                double *corrections_out, double *poses_out, sageicp_closure_info *info) {
    return corrections(poses, n, i, j, closed, corrections_out, poses_out, info);
}

int sageicp_map_session_stays(const sageicp_map *m, int which, uint64_t first, const double *positions, uint64_t n,
                              uint32_t *stay_out, uint64_t cap, uint64_t *n_out) {
    if (int rc = check_selection(m, which, positions, n, n_out, "sageicp_map_session_stays")) return rc;
    return session_stays(internal(m), which, first, positions, n, stay_out, stay_out ? cap : 0, n_out);
}

int sageicp_map_session_corrected(const sageicp_map *m, int which, uint64_t first, const double *positions,
                                  const double *corrections, uint64_t n, double *out_xyzl, uint64_t cap, uint64_t *n_out) {
    if (int rc = check_selection(m, which, positions, n, n_out, "sageicp_map_session_corrected")) return rc;
    if (int rc = check_corrections(corrections, n, "sageicp_map_session_corrected")) return rc;
    return session_corrected(internal(m), which, first, positions, corrections, n, RowSink::host_rows(out_xyzl, cap), n_out);
}

int sageicp_map_session_corrected_device(const sageicp_map *m, int which, uint64_t first, const double *positions,
                                         const double *corrections, uint64_t n, const sageicp_device_points *dst, void *stream,
                                         uint64_t *n_out) {
    if (int rc = check_selection(m, which, positions, n, n_out, "sageicp_map_session_corrected_device")) return rc;
    if (int rc = check_corrections(corrections, n, "sageicp_map_session_corrected_device")) return rc;
    if (int rc = check_device_points(dst, stream, m->device)) return rc;
    return session_corrected(internal(m), which, first, positions, corrections, n, RowSink::device_rows(dst, stream), n_out);
}

int sageicp_pipeline_closure(const sageicp_pipeline *p, uint64_t i, const double closed[7], double *corrections_out,
                             double *poses_out, sageicp_closure_info *info) {
    std::vector<double> pos, poses;
    if (int rc = pipeline_positions(p, "sageicp_pipeline_closure", pos, &poses)) return rc;
    const uint64_t n = poses.size() / 7;
    return corrections(poses.data(), n, i, n - 1, closed, corrections_out, poses_out, info);
}

int sageicp_pipeline_session_corrected(const sageicp_pipeline *p, int which, uint64_t first, const double *corrections, uint64_t n,
                                       double *out_xyzl, uint64_t cap, uint64_t *n_out) {
    std::vector<double> pos;
    if (int rc = pipeline_positions(p, "sageicp_pipeline_session_corrected", pos, nullptr)) return rc;
    if (n != pos.size() / 3) return fail(SAGEICP_ERR_INVALID, "sageicp_pipeline_session_corrected: n is not the pipeline's number of poses");
    return sageicp_map_session_corrected(sageicp_pipeline_local_map(p), which, first, pos.data(), corrections, n, out_xyzl, cap, n_out);
}

int sageicp_pipeline_session_corrected_device(const sageicp_pipeline *p, int which, uint64_t first, const double *corrections,
                                              uint64_t n, const sageicp_device_points *dst, void *stream, uint64_t *n_out) {
    std::vector<double> pos;
    if (int rc = pipeline_positions(p, "sageicp_pipeline_session_corrected_device", pos, nullptr)) return rc;
    if (n != pos.size() / 3)
        return fail(SAGEICP_ERR_INVALID, "sageicp_pipeline_session_corrected_device: n is not the pipeline's number of poses");
    return sageicp_map_session_corrected_device(sageicp_pipeline_local_map(p), which, first, pos.data(), corrections, n, dst, stream,
                                                n_out);
}

}  // extern "C"
