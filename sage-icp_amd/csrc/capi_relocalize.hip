// A batch of candidate poses scored in one pass, and Relocalize on top of it (include/sageicp.h; score.h; DESIGN.md
// D14): the host side.  The frame's pristine rows live in Scratch::d_score_frame for the whole call — uploaded or
// ingested once —; the candidates are taken in chunks of max(1, chunk_rows / n), each chunk moved (k_score_move),
// searched and accepted by the steps the quality report uses (QueryCall, query.h) and summed (k_score,
// k_score_reduce); score_finish derives what sageicp_registration_quality derives, through the same code.
#include "query.h"

#include <algorithm>

namespace sageicp_impl {

static_assert(sizeof(sageicp_pose_score) == 488, "sageicp_pose_score: doubles first, no padding (include/sageicp.h)");
static_assert(sizeof(sageicp_relocalize_params) == 80 && sizeof(sageicp_relocalize_info) == 64, "include/sageicp.h");

constexpr uint64_t kMaxCandidates = 1ull << 20;
constexpr uint32_t kMaxRefine = 16;

// one candidate's fields from what the kernels left
static void score_finish(const ScoreRaw &r, uint64_t n, sageicp_pose_score *q) {
    QualitySolve sol;
    q->step_valid = derive_shared(r, n, q, &sol) ? 1 : 0;
    q->score = q->sum_w;
}

// what every scoring entry refuses before any device is asked (k > 0)
static int check_score_args(const char *who, const sageicp_map *map, const double *poses, uint64_t k, double kernel,
                            const void *out) {
    const std::string w(who);
    if (!map) return fail(SAGEICP_ERR_INVALID, w + ": map is NULL");
    if (!out) return fail(SAGEICP_ERR_INVALID, w + ": out is NULL");
    if (!poses) return fail(SAGEICP_ERR_INVALID, w + ": poses is NULL");
    if (k > kMaxCandidates) return fail(SAGEICP_ERR_INVALID, w + ": too many candidates (2^20 max)");
    if (!(std::isfinite(kernel) && kernel > 0.0)) return fail(SAGEICP_ERR_INVALID, w + ": kernel must be finite and above 0");
    for (uint64_t c = 0; c < k; ++c)
        if (!finite_n(poses + 7 * c, 7))
            return fail(SAGEICP_ERR_INVALID, w + ": pose " + std::to_string(c) + " of " + std::to_string(k) + " is not finite");
    return SAGEICP_OK;
}

// The scores of k candidates for the n pristine rows in m.sc.d_score_frame (n > 0, a map that is not empty, the mirror
// current): staged in `out`, which the caller copies out once everything has succeeded.
static int score_staged(QueryCall &c, uint64_t n, const double *poses, uint64_t k, double max_dist, double kernel,
                        double sem_th, sageicp_pose_score *out) {
    Scratch &sc = c.sc;
    uint64_t chunk_rows = static_cast<uint64_t>(knobs().score_chunk_rows.get());
    chunk_rows = std::min<uint64_t>(chunk_rows, kMaxQueries);
    const uint64_t per_chunk = std::max<uint64_t>(1, chunk_rows / n);
    int rc;
    for (uint64_t c0 = 0; c0 < k; c0 += per_chunk) {
        const uint64_t kc = std::min(per_chunk, k - c0), rows = kc * n;          // rows <= kMaxQueries
        if ((rc = sc.reserve_nn(rows))) return rc;
        if ((rc = sc.reserve_sort(rows))) return rc;
        if ((rc = sc.reserve_score(n, kc))) return rc;
        ScorePose *hp = sc.h_score_poses.data();
        for (uint64_t i = 0; i < kc; ++i) {
            const double *p = poses + 7 * (c0 + i);
            quat_to_mat(p, hp[i].R);
            hp[i].t[0] = p[4]; hp[i].t[1] = p[5]; hp[i].t[2] = p[6];
        }
        HIPCHK(hipMemcpyAsync(sc.d_score_poses.data(), hp, kc * sizeof(ScorePose), hipMemcpyHostToDevice, c.stream()));
        // (the search's state: the rows are moved by their candidates, k_score_move, not by it)
        if ((rc = c.move(sc.d_score_rows.data(), rows, nullptr))) return rc;
        HIPCHK(hipMemsetAsync(sc.d_score_raw.data(), 0, kc * sizeof(ScoreRaw), c.stream()));
        ScoreArgs a{};
        a.n = static_cast<int>(n);
        a.kc = static_cast<uint32_t>(kc);
        a.frame = sc.d_score_frame.data();
        a.poses = sc.d_score_poses.data();
        a.rows = sc.d_score_rows.data();
        a.by_query = sc.d_score_by_query.data();
        a.kernel = kernel;
        a.slabs = sc.d_score_slabs.data();
        a.out = sc.d_score_raw.data();
        launch_score_move(a, c.stream());
        HIPCHK(hipGetLastError());
        // one search over the chunk's rows
        if ((rc = c.sort_and_search(sc.d_score_rows.data(), rows, sem_th))) return rc;
        if ((rc = c.accept(rows, max_dist, sc.d_score_by_query.data()))) return rc;
        a.pts = c.m.dev.search_view().pts;
        launch_score(a, c.stream());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(sc.h_score_raw.data(), sc.d_score_raw.data(), kc * sizeof(ScoreRaw), hipMemcpyDeviceToHost,
                              c.stream()));
        if ((rc = c.wait())) return rc;
        for (uint64_t i = 0; i < kc; ++i) score_finish(sc.h_score_raw.data()[i], n, out + c0 + i);
    }
    return SAGEICP_OK;
}

// the frame of a scoring entry, whole, into d_score_frame, where it stays pristine for the whole call
static int stage_score_frame(QueryCall &c, const FrameSource &src) {
    if (int rc = c.sc.reserve_score_frame(src.n)) return rc;
    return c.stage(src, c.sc.d_score_frame.data());
}

// ---- candidates ---------------------------------------------------------------------------------------------------------
// the largest integer m >= 0 with m * step <= extent in fp64 (0 when step <= 0 or extent < step); false: beyond 2^20
static bool axis_steps(double extent, double step, uint64_t *m_out) {
    *m_out = 0;
    if (!(step > 0.0) || extent < step) return true;
    const double q = extent / step;
    if (!(q < 2097152.0)) return false;
    uint64_t m = static_cast<uint64_t>(q);
    while (static_cast<double>(m + 1) * step <= extent) ++m;
    while (m > 0 && static_cast<double>(m) * step > extent) --m;
    *m_out = m;
    return m <= kMaxCandidates;
}

struct CandidateGrid {
    uint64_t m_yaw = 0, m_xy = 0, m_z = 0, count = 0;
};

static int candidate_grid(const double prior[7], const sageicp_relocalize_params *p, CandidateGrid *g) {
    if (!prior || !p) return fail(SAGEICP_ERR_INVALID, "Relocalize: null argument");
    if (!finite_n(prior, 7)) return fail(SAGEICP_ERR_INVALID, "Relocalize: the prior is not finite");
    const double v[9] = {p->xy_extent, p->xy_step, p->z_extent, p->z_step, p->yaw_extent, p->yaw_step,
                         p->max_correspondence_distance, p->kernel, p->sem_th};
    if (!finite_n(v, 9)) return fail(SAGEICP_ERR_INVALID, "Relocalize: a parameter is not finite");
    if (p->refine_top > kMaxRefine) return fail(SAGEICP_ERR_INVALID, "Relocalize: refine_top above 16");
    const bool ok = axis_steps(p->yaw_extent, p->yaw_step, &g->m_yaw) && axis_steps(p->xy_extent, p->xy_step, &g->m_xy) &&
                    axis_steps(p->z_extent, p->z_step, &g->m_z);
    // (every factor is at most 2^21 + 1: the running product is tested before it can leave 64 bits)
    uint64_t count = ok ? 2 * g->m_yaw + 1 : 0;
    const uint64_t factors[3] = {2 * g->m_xy + 1, 2 * g->m_xy + 1, 2 * g->m_z + 1};
    for (int a = 0; a < 3 && count && count <= kMaxCandidates; ++a) count *= factors[a];
    if (!ok || count > kMaxCandidates)
        return fail(SAGEICP_ERR_INVALID, "Relocalize: more than 2^20 candidates: widen the steps or narrow the extents");
    g->count = count;
    return SAGEICP_OK;
}

// candidates [0, min(cap, count)) of the grid, in order: yaw outermost, then x, then y, z innermost, each ascending
static void write_candidates(const double prior[7], const sageicp_relocalize_params &p, const CandidateGrid &g,
                             double *out, uint64_t cap) {
    const int64_t my = static_cast<int64_t>(g.m_yaw), mx = static_cast<int64_t>(g.m_xy), mz = static_cast<int64_t>(g.m_z);
    uint64_t at = 0;
    for (int64_t a = -my; a <= my && at < cap; ++a) {
        double q[4] = {prior[0], prior[1], prior[2], prior[3]};
        if (a != 0) {
            // q_z(theta) (x) q_prior, q_z = (0, 0, s, c): the Hamilton product with its zero terms left out
            const double theta = static_cast<double>(a) * p.yaw_step;
            const double s = std::sin(theta / 2.0), c = std::cos(theta / 2.0);
            q[0] = c * prior[0] - s * prior[1];
            q[1] = c * prior[1] + s * prior[0];
            q[2] = c * prior[2] + s * prior[3];
            q[3] = c * prior[3] - s * prior[2];
        }
        for (int64_t i = -mx; i <= mx && at < cap; ++i)
            for (int64_t j = -mx; j <= mx && at < cap; ++j)
                for (int64_t l = -mz; l <= mz && at < cap; ++l, ++at) {
                    double *o = out + 7 * at;
                    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
                    o[4] = i ? prior[4] + static_cast<double>(i) * p.xy_step : prior[4];
                    o[5] = j ? prior[5] + static_cast<double>(j) * p.xy_step : prior[5];
                    o[6] = l ? prior[6] + static_cast<double>(l) * p.z_step : prior[6];
                }
    }
}

// ---- Relocalize ---------------------------------------------------------------------------------------------------------
// steps 2-5 of sageicp_relocalize on the n rows in m.sc.d_score_frame (n > 0, a map that is not empty, mirror current)
static int relocalize_staged(QueryCall &c, uint64_t n, const std::vector<double> &cands,
                             const sageicp_relocalize_params &p, double pose_out[7], sageicp_quality *quality_out,
                             sageicp_relocalize_info *info) {
    sageicp_map &m = c.m;
    const Point4 *d_rows = m.sc.d_score_frame.data();
    // the quality report of the pristine rows at `pose`
    auto quality_at = [&](const double *pose, sageicp_quality *q) {
        return quality_of_device_rows(m, d_rows, n, pose, p.max_correspondence_distance, p.kernel, p.sem_th, q);
    };
    const uint64_t K = cands.size() / 7;
    const double t0 = now_us();
    std::vector<sageicp_pose_score> scores(K);
    int rc = score_staged(c, n, cands.data(), K, p.max_correspondence_distance, p.kernel, p.sem_th, scores.data());
    if (rc) return rc;
    const double t1 = now_us();
    // the ranking: score descending, ties to the lower index; only the first few are needed
    const uint32_t top = static_cast<uint32_t>(std::min<uint64_t>(std::max<uint32_t>(p.refine_top, 1u), K));
    std::vector<uint64_t> ranked;
    std::vector<char> taken(K, 0);
    for (uint32_t r = 0; r < top; ++r) {
        uint64_t best = K;
        for (uint64_t i = 0; i < K; ++i)
            if (!taken[i] && (best == K || scores[i].score > scores[best].score)) best = i;
        taken[best] = 1;
        ranked.push_back(best);
    }
    double pose[7] = {};
    sageicp_quality quality{};
    sageicp_relocalize_info I{};
    I.candidates = K;
    if (p.refine_top == 0) {
        std::memcpy(pose, cands.data() + 7 * ranked[0], 56);
        if ((rc = quality_at(pose, &quality))) return rc;
        I.best_candidate = ranked[0];
        I.best_candidate_score = scores[ranked[0]].score;
    } else {
        bool have = false;
        for (uint32_t r = 0; r < top; ++r) {
            double refined[7];
            sageicp_stats st;
            sageicp_quality q;
            if ((rc = register_resident(m, d_rows, n, m.device, cands.data() + 7 * ranked[r],
                                        p.max_correspondence_distance, p.kernel, p.sem_th, nullptr, refined, &st))) {
                (void)c.stream();              // (an ICP loop that failed may have left work on it)
                return rc;
            }
            if ((rc = quality_at(refined, &q))) return rc;
            ++I.refined;
            if (!have || q.sum_w > quality.sum_w) {
                have = true;
                std::memcpy(pose, refined, 56);
                quality = q;
                I.best_candidate = ranked[r];
                I.best_candidate_score = scores[ranked[r]].score;
                I.winner_rank = r;
                I.iterations = st.iterations;
                I.converged = st.converged;
            }
        }
    }
    const double t2 = now_us();
    I.us_score = t1 - t0;
    I.us_refine = t2 - t1;
    I.us_wall = t2 - t0;
    std::memcpy(pose_out, pose, 56);
    if (quality_out) *quality_out = quality;
    if (info) *info = I;
    return SAGEICP_OK;
}

// the answer for an empty map or an empty frame: the prior, as RegisterFrame returns its initial guess
static int relocalize_nothing(const double prior[7], uint64_t K, double pose_out[7], sageicp_quality *quality_out,
                              sageicp_relocalize_info *info) {
    std::memcpy(pose_out, prior, 56);
    if (quality_out) std::memset(quality_out, 0, sizeof(*quality_out));
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->candidates = K;
    }
    return SAGEICP_OK;
}

// both ScorePoses entries behind their argument checks
static int score_poses(const sageicp_map *map, const FrameSource &src, const double *poses, uint64_t k, double max_dist,
                       double kernel, double sem_th, sageicp_pose_score *out) {
    sageicp_map &m = internal(map);
    if (src.n == 0 || m.empty()) {
        std::memset(out, 0, k * sizeof(*out));
        return SAGEICP_OK;
    }
    int rc = refresh_mirror(m);          // (makes the device current; a resident map stays resident)
    if (rc) return rc;
    QueryCall c(m, "ScorePoses");
    if ((rc = stage_score_frame(c, src))) return rc;
    std::vector<sageicp_pose_score> staged(k);
    if ((rc = score_staged(c, src.n, poses, k, max_dist, kernel, sem_th, staged.data()))) return rc;
    std::memcpy(out, staged.data(), k * sizeof(*out));
    return SAGEICP_OK;
}

// both Relocalize entries behind their argument checks
static int relocalize(const sageicp_map *map, const FrameSource &src, const double prior[7],
                      const sageicp_relocalize_params &p, const CandidateGrid &g, double pose_out[7],
                      sageicp_quality *quality_out, sageicp_relocalize_info *info) {
    sageicp_map &m = internal(map);
    if (src.n == 0 || m.empty()) return relocalize_nothing(prior, g.count, pose_out, quality_out, info);
    std::vector<double> cands(7 * g.count);
    write_candidates(prior, p, g, cands.data(), g.count);
    int rc = refresh_mirror(m);
    if (rc) return rc;
    QueryCall c(m, "Relocalize");
    if ((rc = stage_score_frame(c, src))) return rc;
    return relocalize_staged(c, src.n, cands, p, pose_out, quality_out, info);
}

}  // namespace sageicp_impl

extern "C" {

int sageicp_score_poses(const sageicp_map *map, const double *xyzl, uint64_t n, const double *poses, uint64_t k,
                        double max_dist, double kernel, double sem_th, sageicp_pose_score *out) {
    if (k == 0) return SAGEICP_OK;
    int rc = check_score_args("ScorePoses", map, poses, k, kernel, out);
    if (rc) return rc;
    if ((rc = check_host_rows("ScorePoses", xyzl, n))) return rc;
    return score_poses(map, FrameSource::host_rows(xyzl, n), poses, k, max_dist, kernel, sem_th, out);
}

int sageicp_score_poses_device(const sageicp_map *map, const sageicp_device_frame *frame, const double *poses, uint64_t k,
                               double max_dist, double kernel, double sem_th, void *stream, sageicp_pose_score *out) {
    if (k == 0) return SAGEICP_OK;
    int rc = check_score_args("ScorePoses", map, poses, k, kernel, out);
    if (rc) return rc;
    if ((rc = check_device_source("ScorePoses", map, frame, stream))) return rc;
    return score_poses(map, FrameSource::device_frame(frame, nullptr, static_cast<hipStream_t>(stream)), poses, k,
                       max_dist, kernel, sem_th, out);
}

int sageicp_relocalize_candidates(const double prior[7], const sageicp_relocalize_params *params, double *poses_out,
                                  uint64_t cap, uint64_t *k_out) {
    if (!k_out || (cap && !poses_out)) return fail(SAGEICP_ERR_INVALID, "Relocalize: null argument");
    CandidateGrid g;
    if (int rc = candidate_grid(prior, params, &g)) return rc;
    *k_out = g.count;
    write_candidates(prior, *params, g, poses_out, std::min(cap, g.count));
    return SAGEICP_OK;
}

int sageicp_relocalize(const sageicp_map *map, const double *xyzl, uint64_t n, const double prior[7],
                       const sageicp_relocalize_params *params, double pose_out[7], sageicp_quality *quality_out,
                       sageicp_relocalize_info *info) {
    if (!map || !pose_out || (n && !xyzl)) return fail(SAGEICP_ERR_INVALID, "Relocalize: null argument");
    CandidateGrid g;
    int rc = candidate_grid(prior, params, &g);
    if (rc) return rc;
    if (n > kMaxQueries) return fail(SAGEICP_ERR_INVALID, "Relocalize: too many rows (2^26 - 4 max)");
    if (!(params->kernel > 0.0)) return fail(SAGEICP_ERR_INVALID, "Relocalize: kernel must be finite and above 0");
    if (!all_finite(xyzl, n)) return refuse_non_finite("Relocalize", "row");
    return relocalize(map, FrameSource::host_rows(xyzl, n), prior, *params, g, pose_out, quality_out, info);
}

int sageicp_relocalize_device(const sageicp_map *map, const sageicp_device_frame *frame, const double prior[7],
                              const sageicp_relocalize_params *params, void *stream, double pose_out[7],
                              sageicp_quality *quality_out, sageicp_relocalize_info *info) {
    if (!map || !pose_out || !frame) return fail(SAGEICP_ERR_INVALID, "Relocalize: null argument");
    CandidateGrid g;
    int rc = candidate_grid(prior, params, &g);
    if (rc) return rc;
    if (!(params->kernel > 0.0)) return fail(SAGEICP_ERR_INVALID, "Relocalize: kernel must be finite and above 0");
    if ((rc = check_device_source("Relocalize", map, frame, stream))) return rc;
    return relocalize(map, FrameSource::device_frame(frame, nullptr, static_cast<hipStream_t>(stream)), prior, *params, g,
                      pose_out, quality_out, info);
}

}  // extern "C"
