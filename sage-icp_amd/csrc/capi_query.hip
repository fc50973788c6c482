// The query entries' shared path (query.h) and the entries built directly on it: GetCorrespondences and
// RegistrationQuality, on host rows and on a frame in device memory, with the host side of the quality report
// (quality_solve, quality_finish).  Host code only: the kernels are kernels.hip's, sort.hip's, ingest.hip's,
// correspond.hip's and quality.hip's.
//
// Reference call site this file stands in for (cpp/sage_icp/):
//   core/VoxelHashMap.cpp:48-130    GetCorrespondences   -> sageicp_get_correspondences(), and on a frame in device
//                                                           memory sageicp_get_correspondences_device() (correspond.hip)
#include "query.h"

namespace sageicp_impl {

// ---- the path -----------------------------------------------------------------------------------------------------------
int QueryCall::stage(const FrameSource &src, Point4 *d_dst) {
    if (src.kind == FrameSource::kHostRows) {
        HIPCHK(hipMemcpyAsync(d_dst, src.rows, src.n * sizeof(Point4), hipMemcpyHostToDevice, stream()));
        return SAGEICP_OK;
    }
    if (src.kind != FrameSource::kDeviceFrame)
        return fail(SAGEICP_ERR_INVALID, std::string(who_) + ": host rows or a device frame");
    // the work that wrote the frame, and may still use an entry's destinations, goes first
    if (int rc = stream_after_caller(m.out.ev_caller, src.stream, stream())) return rc;
    launch_ingest(ingest_args(*src.frame), d_dst, stream());
    HIPCHK(hipGetLastError());
    return SAGEICP_OK;
}

int QueryCall::stage(const Point4 *d_rows, uint64_t n, Point4 *d_dst) {
    HIPCHK(hipMemcpyAsync(d_dst, d_rows, n * sizeof(Point4), hipMemcpyDeviceToDevice, stream()));
    return SAGEICP_OK;
}

int QueryCall::move(Point4 *d_rows, uint64_t n, const double *pose) {
    double I[7];
    identity_pose(I);
    fill_state(sc.h_state.data(), pose ? pose : I);
    HIPCHK(hipMemcpyAsync(sc.d_state.data(), sc.h_state.data(), sizeof(IcpState), hipMemcpyHostToDevice, stream()));
    if (pose) launch_tf(d_rows, static_cast<int>(n), sc.d_state.data(), stream());
    HIPCHK(hipGetLastError());
    return SAGEICP_OK;
}

int QueryCall::sort_and_search(const Point4 *d_rows, uint64_t n, double sem_th, bool read_verdict) {
    // the same pipeline as the ICP loop at the identity: sort, rows, search; an entry maps the answers back to the
    // caller's order through the sort's permutation
    HIPCHK(sort_frame(d_rows, sc.d_sorted.data(), static_cast<int>(n), sc.d_state.data(), false, false,
                      m.host.voxel_size, sc.d_keys.data(), sc.d_vals.data(), sc.d_sort_temp.data(),
                      sc.d_sort_temp.capacity(), stream()));
    if (read_verdict) {
        HIPCHK(hipMemcpyAsync(sc.h_state.data(), sc.d_state.data(), sizeof(IcpState), hipMemcpyDeviceToHost, stream()));
        if (int rc = wait()) return rc;
        if (sc.h_state.data()->bad_input) return refuse_non_finite(who_, noun_);
    }
    const Knobs &kn = knobs();
    const int lw = icp_lw(kn, n, sparse_voxels(m));
    if (int rc = m.dev.ensure_cand(wants_filter(kn, m, n, sem_th), stream())) return rc;
    const IcpParams ip = icp_params(kn, m, sc.d_sorted.data(), n, sem_th, lw, 0);      // identity pose, no loop state
    launch_rows(ip, stream());
    launch_icp(ip, lw, false, stream());
    HIPCHK(hipGetLastError());
    return SAGEICP_OK;
}

CorrespondArgs QueryCall::answers(uint64_t n, double max_dist, int32_t *d_by_query) const {
    CorrespondArgs a{};
    a.n = static_cast<int>(n);
    a.sorted = sc.d_sorted.data();
    a.perm = sc.d_vals.data() + n;
    a.nn = sc.d_nn.data();
    a.pts = m.dev.search_view().pts;
    a.accept_r2 = accept_threshold(max_dist);
    a.by_query = d_by_query;
    return a;
}

int QueryCall::accept(uint64_t n, double max_dist, int32_t *d_by_query) {
    launch_corr_flag(answers(n, max_dist, d_by_query), stream());
    HIPCHK(hipGetLastError());
    return SAGEICP_OK;
}

int refuse_non_finite(const char *who, const char *noun) {
    return fail(SAGEICP_ERR_INVALID,
                std::string(who) + ": a coordinate or label of a " + noun + " is not finite (NaN / Inf)");
}

int check_host_rows(const char *who, const double *xyzl, uint64_t n) {
    if (n && !xyzl) return fail(SAGEICP_ERR_INVALID, std::string(who) + ": xyzl is NULL");
    if (n > kMaxQueries) return fail(SAGEICP_ERR_INVALID, std::string(who) + ": too many rows (2^26 - 4 max)");
    if (!all_finite(xyzl, n)) return refuse_non_finite(who, "row");
    return SAGEICP_OK;
}

int check_device_source(const char *who, const sageicp_map *map, const sageicp_device_frame *frame, void *stream) {
    if (!frame) return fail(SAGEICP_ERR_INVALID, std::string(who) + ": frame is NULL");
    if (int rc = check_frame_layout(frame)) return rc;
    // where the memory lives, and the stream
    if (int rc = check_device_frame(frame, nullptr, stream, map->device)) return rc;
    return check_stream(stream, map->device);
}

// ---- registration quality (quality.h) ---------------------------------------------------------------------------------
static_assert(sizeof(sageicp_quality) == 5464, "sageicp_quality: doubles first, no padding (include/sageicp.h)");
static_assert(kQualClasses == 256, "the class tables of sageicp_quality");

// A pivot of the Cholesky factorisation counts as positive above this share of its diagonal entry.  Its rounding error
// is a few u of that entry: at the bound it keeps about half of fp64's digits, far below it is the rounding of a zero
// (collinear pairs).  A 30 m scene at UTM coordinates (|s| ~ 5.5e6 m) has pivots of ~2^-40: no covariance there.
constexpr double kQualPivotBound = 1.0 / 67108864.0;                // 2^-26

// The Gauss-Newton step still left and JTJ^-1 from the assembled system, by Cholesky: false — nothing written that
// counts — with fewer than three pairs, a pivot at or below the bound, or a result that is not finite.  The one solve
// behind sageicp_quality and sageicp_pose_score (derive_shared, query.h).
bool quality_solve(const double JTJ[36], const double JTr[6], double sum_w_r2, uint64_t n_pairs, QualitySolve *o) {
    if (n_pairs < 3) return false;
    const double np = static_cast<double>(n_pairs);
    // JTJ = L L^T; the pivots are the squares of L's diagonal
    double L[6][6] = {};
    for (int j = 0; j < 6; ++j) {
        double d = JTJ[j * 6 + j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > kQualPivotBound * JTJ[j * 6 + j]) || !std::isfinite(d)) return false;
        L[j][j] = std::sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double v = JTJ[i * 6 + j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double Li[6][6] = {};                     // L^-1, lower triangular
    for (int j = 0; j < 6; ++j) {
        Li[j][j] = 1.0 / L[j][j];
        for (int i = j + 1; i < 6; ++i) {
            double v = 0.0;
            for (int k = j; k < i; ++k) v -= L[i][k] * Li[k][j];
            Li[i][j] = v / L[i][i];
        }
    }
    for (int i = 0; i < 6; ++i)               // JTJ^-1 = L^-T L^-1
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int k = i; k < 6; ++k) v += Li[k][i] * Li[k][j];
            o->inv[i][j] = o->inv[j][i] = v;
        }
    double y[6], x[6], norm2 = 0.0;           // step = -L^-T (L^-1 JTr)
    for (int i = 0; i < 6; ++i) {
        double v = -JTr[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    o->s2 = sum_w_r2 / (3.0 * np - 6.0);
    bool finite = std::isfinite(o->s2);
    for (int i = 0; i < 6; ++i) {
        finite = finite && std::isfinite(x[i]);
        for (int j = 0; j < 6; ++j) finite = finite && std::isfinite(o->inv[i][j]);
    }
    if (!finite) return false;
    for (int i = 0; i < 6; ++i) {
        o->step[i] = x[i];
        norm2 += x[i] * x[i];
    }
    o->step_norm = std::sqrt(norm2);
    return true;
}

// the report from what the kernels left: everything derived, on the host in fp64 (include/sageicp.h)
static void quality_finish(const QualityRaw &r, uint64_t n, const double *pose, sageicp_quality *q) {
    QualitySolve sol;
    const bool solved = derive_shared(r, n, q, &sol);
    q->other_queries = r.counts[kQOtherQueries];
    q->other_pairs = r.counts[kQOtherPairs];
    for (int c = 0; c < kQualClasses; ++c) {
        q->class_queries[c] = static_cast<uint32_t>(r.class_queries[c]);
        q->class_pairs[c] = static_cast<uint32_t>(r.class_pairs[c]);
        q->class_sum_r2[c] = r.class_r2[c];
    }
    q->other_sum_r2 = r.class_r2[kQualClasses];
    {
        // sum J^T J without weights: the same assembly over n_pairs, sum s, sum s s^T
        double S[kNumSums] = {}, unused[6];
        S[kW] = static_cast<double>(q->n_pairs);
        S[kWsx] = r.real[kQSx]; S[kWsy] = r.real[kQSy]; S[kWsz] = r.real[kQSz];
        S[kWxx] = r.real[kQSxx]; S[kWxy] = r.real[kQSxy]; S[kWxz] = r.real[kQSxz];
        S[kWyy] = r.real[kQSyy]; S[kWyz] = r.real[kQSyz]; S[kWzz] = r.real[kQSzz];
        assemble_normal_equations(S, q->info, unused);
    }
    if (!solved) return;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) q->covariance[i * 6 + j] = sol.s2 * sol.inv[i][j];
    // G C G^T, G = [[I, -hat(t)], [0, I]]: rows 0..2 of G hold two more entries each, rows 3..5 none
    const double t[3] = {pose ? pose[4] : 0.0, pose ? pose[5] : 0.0, pose ? pose[6] : 0.0};
    const double G[3][3] = {{0.0, t[2], -t[1]}, {-t[2], 0.0, t[0]}, {t[1], -t[0], 0.0}};      // -hat(t)
    double M[6][6];                           // G C
    for (int a = 0; a < 6; ++a)
        for (int j = 0; j < 6; ++j) {
            double v = q->covariance[a * 6 + j];
            if (a < 3)
                for (int k = 0; k < 3; ++k)
                    if (k != a) v += G[a][k] * q->covariance[(3 + k) * 6 + j];
            M[a][j] = v;
        }
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            double v = M[a][b];
            if (b < 3)
                for (int k = 0; k < 3; ++k)
                    if (k != b) v += M[a][3 + k] * G[b][k];
            q->covariance_pose[a * 6 + b] = v;
        }
    q->covariance_valid = 1;
}

// the quality report of the n rows staged in d_frame, not yet moved by `pose`
static int quality_of_staged_rows(QueryCall &c, uint64_t n, const double *pose, double max_dist, double kernel,
                                  double sem_th, sageicp_quality *out) {
    Scratch &sc = c.sc;
    int rc;
    if ((rc = sc.reserve_nn(n))) return rc;
    if ((rc = sc.reserve_sort(n))) return rc;
    if ((rc = sc.reserve_quality(n))) return rc;
    if ((rc = c.move(sc.d_frame.data(), n, pose))) return rc;
    if ((rc = c.sort_and_search(sc.d_frame.data(), n, sem_th))) return rc;
    if ((rc = c.accept(n, max_dist, sc.d_by_query.data()))) return rc;
    // the pass
    HIPCHK(hipMemsetAsync(sc.d_qual_raw.data(), 0, sizeof(QualityRaw), c.stream()));
    QualityArgs a{};
    a.n = static_cast<int>(n);
    a.frame = sc.d_frame.data();
    a.by_query = sc.d_by_query.data();
    a.pts = c.m.dev.search_view().pts;
    a.kernel = kernel;
    a.slabs = sc.d_qual_slabs.data();
    a.out = sc.d_qual_raw.data();
    launch_quality(a, c.stream());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sc.h_qual_raw.data(), sc.d_qual_raw.data(), sizeof(QualityRaw), hipMemcpyDeviceToHost,
                          c.stream()));
    if ((rc = c.wait())) return rc;
    quality_finish(*sc.h_qual_raw.data(), n, pose, out);
    return SAGEICP_OK;
}

int quality_of_device_rows(sageicp_map &m, const Point4 *d_rows, uint64_t n, const double *pose, double max_dist,
                           double kernel, double sem_th, sageicp_quality *out) {
    QueryCall c(m, "RegistrationQuality");
    if (int rc = c.sc.reserve_frame(n)) return rc;
    if (int rc = c.stage(d_rows, n, c.sc.d_frame.data())) return rc;
    return quality_of_staged_rows(c, n, pose, max_dist, kernel, sem_th, out);
}

// what both quality entries refuse before they look at the rows
static int check_quality_args(const sageicp_map *map, const double *pose, double kernel, const sageicp_quality *out) {
    if (!map) return fail(SAGEICP_ERR_INVALID, "RegistrationQuality: map is NULL");
    if (!out) return fail(SAGEICP_ERR_INVALID, "RegistrationQuality: out is NULL");
    if (pose && !finite_n(pose, 7)) return fail(SAGEICP_ERR_INVALID, "RegistrationQuality: the pose is not finite");
    if (!(std::isfinite(kernel) && kernel > 0.0))
        return fail(SAGEICP_ERR_INVALID, "RegistrationQuality: kernel must be finite and above 0");
    return SAGEICP_OK;
}

// both quality entries behind their argument checks
static int registration_quality(const sageicp_map *map, const FrameSource &src, const double *pose, double max_dist,
                                double kernel, double sem_th, sageicp_quality *out) {
    std::memset(out, 0, sizeof(*out));
    sageicp_map &m = internal(map);
    if (src.n == 0 || m.empty()) return SAGEICP_OK;
    int rc = refresh_mirror(m);          // (makes the device current; a resident map stays resident)
    if (rc) return rc;
    QueryCall c(m, "RegistrationQuality");
    if ((rc = m.sc.reserve_frame(src.n))) return rc;
    if ((rc = c.stage(src, m.sc.d_frame.data()))) return rc;
    return quality_of_staged_rows(c, src.n, pose, max_dist, kernel, sem_th, out);
}

}  // namespace sageicp_impl

extern "C" {

// ---- search ---------------------------------------------------------------------------------
int sageicp_get_correspondences(const sageicp_map *map, const double *q, uint64_t n, double max_dist,
                                double sem_th, double *src_out, double *tgt_out, uint64_t *n_out,
                                int64_t *query_idx_out) {
    if (!map || !n_out || (n && (!q || !src_out || !tgt_out)))
        return fail(SAGEICP_ERR_INVALID, "null argument");
    if (n > kMaxQueries) return fail(SAGEICP_ERR_INVALID, "too many queries (2^26 - 4 max)");
    *n_out = 0;
    if (!all_finite(q, n)) return refuse_non_finite("GetCorrespondences", "query");
    sageicp_map &m = internal(map);
    int rc = ensure_host(m);      // the returned target points are read from the host copy
    if (rc) return rc;
    if ((rc = refresh_mirror(m))) return rc;
    if (n == 0 || m.empty()) return SAGEICP_OK;
    QueryCall c(m, "GetCorrespondences", "query");
    Scratch &sc = m.sc;
    if ((rc = sc.reserve_frame(n))) return rc;
    if ((rc = sc.reserve_nn(n))) return rc;
    if ((rc = sc.reserve_sort(n))) return rc;
    if ((rc = c.stage(FrameSource::host_rows(q, n), sc.d_frame.data()))) return rc;
    if ((rc = c.move(sc.d_frame.data(), n, nullptr))) return rc;
    // (the rows were checked above and are not moved: the sort's verdict is not read)
    if ((rc = c.sort_and_search(sc.d_frame.data(), n, sem_th, /*read_verdict*/ false))) return rc;
    std::vector<int32_t> idx(n);
    std::vector<uint32_t> perm(n);
    HIPCHK(hipMemcpyAsync(idx.data(), sc.d_nn.data(), n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream()));
    HIPCHK(hipMemcpyAsync(perm.data(), sc.d_vals.data() + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream()));
    if ((rc = c.wait())) return rc;
    std::vector<int32_t> by_query(n);
    for (uint64_t i = 0; i < n; ++i) by_query[perm[i]] = idx[i];
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; ++i) {     // pairs in query order (VoxelHashMap.cpp:119-127)
        if (by_query[i] < 0) continue;
        // acceptance on the unscaled distance: (nn - point).norm() < max (VoxelHashMap.cpp:111)
        const Point4 &t = m.host.pts[by_query[i]];
        const double dx = t.x - q[4 * i], dy = t.y - q[4 * i + 1], dz = t.z - q[4 * i + 2];
        if (!(std::sqrt(SAGE_SQNORM3_ACCEPT(dx * dx, dy * dy, dz * dz)) < max_dist)) continue;
        std::memcpy(src_out + 4 * k, q + 4 * i, 32);
        std::memcpy(tgt_out + 4 * k, &t, 32);
        if (query_idx_out) query_idx_out[k] = static_cast<int64_t>(i);
        ++k;
    }
    *n_out = k;
    return SAGEICP_OK;
}

// GetCorrespondences of a frame in device memory, answered into device memory: the same search, and behind it the
// acceptance, the compaction in query order and the gather of the target rows on the device (correspond.hip).  The
// target rows come from the HBM copy, which is valid as a mirror and as the authority alike: refresh_mirror() only,
// never ensure_host() — a resident map stays resident.
int sageicp_get_correspondences_device(const sageicp_map *map, const sageicp_device_frame *frame, const double pose[7],
                                       double max_dist, double sem_th, const sageicp_device_points *src_out,
                                       const sageicp_device_points *tgt_out, int64_t *query_idx_out, uint64_t idx_cap,
                                       void *stream, uint64_t *n_out) {
    if (!map || !frame || !n_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    // what needs no device: the three layouts, the pose, the caps, the index array's alignment, destinations that overlap
    int rc = check_frame_layout(frame);
    if (!rc && src_out) rc = check_points_layout(src_out);
    if (!rc && tgt_out) rc = check_points_layout(tgt_out);
    if (rc) return rc;
    if (pose && !finite_n(pose, 7)) return fail(SAGEICP_ERR_INVALID, "GetCorrespondences: the pose is not finite");
    {
        const uint64_t caps[3] = {src_out ? src_out->cap : 0, tgt_out ? tgt_out->cap : 0, idx_cap};
        const bool given[3] = {src_out != nullptr, tgt_out != nullptr, query_idx_out != nullptr};
        for (int a = 0; a < 3; ++a)
            for (int b = a + 1; b < 3; ++b)
                if (given[a] && given[b] && caps[a] != caps[b])
                    return fail(SAGEICP_ERR_INVALID, "GetCorrespondences: src_out->cap, tgt_out->cap and idx_cap of the "
                                                     "destinations given must be equal");
    }
    if (reinterpret_cast<uintptr_t>(query_idx_out) % 8)
        return fail(SAGEICP_ERR_INVALID, "GetCorrespondences: query_idx_out must be 8-byte aligned");
    CallerExtent ext[5];
    int n_ext = 0;
    int first_of_tgt = 0, first_of_idx = 0;
    if (src_out) n_ext += points_extents(*src_out, ext + n_ext);
    first_of_tgt = n_ext;
    if (tgt_out) n_ext += points_extents(*tgt_out, ext + n_ext);
    first_of_idx = n_ext;
    if (query_idx_out && idx_cap) {
        const char *p = reinterpret_cast<const char *>(query_idx_out);
        ext[n_ext++] = {p, p + idx_cap * sizeof(int64_t)};
    }
    for (int a = 0; a < n_ext; ++a)
        for (int b = a + 1; b < n_ext; ++b) {
            // (a destination's own rows and labels are its caller's business, as everywhere)
            const bool same = (b < first_of_tgt) || (a >= first_of_tgt && b < first_of_idx);
            if (!same && ext[a].overlaps(ext[b]))
                return fail(SAGEICP_ERR_INVALID, "GetCorrespondences: src_out, tgt_out and query_idx_out must not overlap "
                                                 "each other");
        }
    // where the memory lives, and the stream
    if ((rc = check_device_frame(frame, nullptr, stream, map->device))) return rc;
    if (src_out && (rc = check_device_points(src_out, stream, map->device))) return rc;
    if (tgt_out && (rc = check_device_points(tgt_out, stream, map->device))) return rc;
    if (query_idx_out && idx_cap) {
        if ((rc = require_device())) return rc;
        if ((rc = check_extent(query_idx_out, idx_cap * sizeof(int64_t), map->device, "GetCorrespondences: query_idx_out")))
            return rc;
    }
    if ((rc = check_stream(stream, map->device))) return rc;
    sageicp_map &m = internal(map);
    const uint64_t n = frame->n;
    if (n == 0 || m.empty()) {
        *n_out = 0;
        return SAGEICP_OK;
    }
    if ((rc = refresh_mirror(m))) return rc;          // (makes the device current)
    QueryCall c(m, "GetCorrespondences", "query");
    Scratch &sc = m.sc;
    if ((rc = sc.reserve_frame(n))) return rc;
    if ((rc = sc.reserve_nn(n))) return rc;
    if ((rc = sc.reserve_sort(n))) return rc;
    if ((rc = sc.reserve_correspond(n))) return rc;
    if ((rc = c.stage(FrameSource::device_frame(frame, nullptr, static_cast<hipStream_t>(stream)), sc.d_frame.data())))
        return rc;
    if ((rc = c.move(sc.d_frame.data(), n, pose))) return rc;
    if ((rc = c.sort_and_search(sc.d_frame.data(), n, sem_th))) return rc;
    // correspond.hip on what the search left
    HIPCHK(hipMemsetAsync(sc.d_corr_words.data(), 0, 2 * sizeof(unsigned long long), c.stream()));
    int *flags = reinterpret_cast<int *>(sc.d_corr_words.data() + 1);
    CorrespondArgs a = c.answers(n, max_dist, sc.d_by_query.data());
    a.frame = sc.d_frame.data();
    a.counts = sc.d_corr_counts.data();
    a.total = sc.d_corr_words.data();
    a.has_src = src_out != nullptr;
    a.has_tgt = tgt_out != nullptr;
    if (src_out) a.src = egress_args(*src_out, flags);
    if (tgt_out) a.tgt = egress_args(*tgt_out, flags);
    a.idx = reinterpret_cast<long long *>(query_idx_out);
    a.idx_cap = idx_cap;
    launch_correspond(a, c.stream());
    HIPCHK(hipGetLastError());
    unsigned long long *h_words = sc.h_corr_words.data();
    HIPCHK(hipMemcpyAsync(h_words, sc.d_corr_words.data(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          c.stream()));
    if ((rc = c.wait())) return rc;
    if (static_cast<int>(h_words[1]) & kEgressLabelRange)
        return fail(SAGEICP_ERR_INVALID, "GetCorrespondences: a label does not fit the destination's label type "
                                         "(static_cast<int64_t>(label) out of its range)");
    *n_out = h_words[0];
    return SAGEICP_OK;
}

// ---- registration quality (quality.hip) --------------------------------------------------------------------------------
int sageicp_registration_quality(const sageicp_map *map, const double *xyzl, uint64_t n, const double pose[7],
                                 double max_dist, double kernel, double sem_th, sageicp_quality *out) {
    int rc = check_quality_args(map, pose, kernel, out);
    if (rc) return rc;
    if ((rc = check_host_rows("RegistrationQuality", xyzl, n))) return rc;
    return registration_quality(map, FrameSource::host_rows(xyzl, n), pose, max_dist, kernel, sem_th, out);
}

int sageicp_registration_quality_device(const sageicp_map *map, const sageicp_device_frame *frame, const double pose[7],
                                        double max_dist, double kernel, double sem_th, void *stream,
                                        sageicp_quality *out) {
    int rc = check_quality_args(map, pose, kernel, out);
    if (rc) return rc;
    if ((rc = check_device_source("RegistrationQuality", map, frame, stream))) return rc;
    return registration_quality(map, FrameSource::device_frame(frame, nullptr, static_cast<hipStream_t>(stream)), pose,
                                max_dist, kernel, sem_th, out);
}

}  // extern "C"
