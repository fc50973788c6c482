// The one path behind the entries that ask the map about a frame (capi_query.hip): GetCorrespondences,
// RegistrationQuality, ScorePoses, Relocalize — on host rows and on a frame in device memory — and the pipeline's
// quality report.  All of them bring the frame into the handle's scratch (stage), move it by a pose (move), sort it and
// search it once against the map (sort_and_search), and sum or compact what the search found (accept, then a pass of
// their own).  Every step exists once, as a member of QueryCall.  Included by the units that use the path
// (capi_query.hip, capi_relocalize.hip, capi_pipeline.hip); not part of the C ABI.
#pragma once

#include "capi_internal.h"

namespace sageicp_impl {

// One entry's use of the handle's stream, from its first enqueue to its return.  The rule it owns: when the entry
// returns, on any path, nothing it enqueued is running and nothing reads or writes the caller's memory.  Whoever
// enqueues asks stream() for the stream, which marks work in flight; wait() clears the mark, and the destructor waits
// when it is still set — that is: on the paths that fail between an enqueue and the success path's own last wait().
class QueryCall {
public:
    sageicp_map &m;
    Scratch &sc;

    // who, noun: the refusal of non-finite rows is worded "<who>: a coordinate or label of a <noun> is not finite"
    QueryCall(sageicp_map &map, const char *who, const char *noun = "row")
        : m(map), sc(map.sc), s_(map.sc.stream.get()), who_(who), noun_(noun) {}
    ~QueryCall() {
        if (in_flight_) (void)hipStreamSynchronize(s_);
    }
    QueryCall(const QueryCall &) = delete;
    QueryCall &operator=(const QueryCall &) = delete;

    hipStream_t stream() {
        in_flight_ = true;
        return s_;
    }
    // The stream idle, and a wait that failed reported: the last step of every success path, before the host reads what
    // the device left.
    int wait() {
        in_flight_ = false;
        HIPCHK(hipStreamSynchronize(s_));
        return SAGEICP_OK;
    }

    // The frame's n rows into d_dst (reserved by the entry): host rows by one upload; a caller's device frame by the
    // ingest kernel behind the work the caller enqueued on its stream — from there on the caller's frame is not read
    // again, so a destination may alias it.  Not waited for: the next wait() covers it, or the destructor.
    int stage(const FrameSource &src, Point4 *d_dst);
    // ... and rows the library already holds on the device (the pipeline's source cloud, d_score_frame): a copy
    int stage(const Point4 *d_rows, uint64_t n, Point4 *d_dst);
    // The state for `pose`, or for the identity without one, uploaded; the rows moved in place when a pose was given
    // (k_tf: sageicp_transform_points' point action).
    int move(Point4 *d_rows, uint64_t n, const double *pose);
    // The n moved rows sorted and searched (rows, k_icp search-only: the ready-made queries, no pose applied): the
    // answers in sorted order in d_nn, the permutation in d_vals + n.  The sort's first pass refuses non-finite rows as
    // it does for every frame; with read_verdict its verdict is read — one wait — before anything is searched or
    // written.  Only an entry that checked its rows on the host and did not move them (a finite row stays finite under
    // no pose) may pass false: host GetCorrespondences, whose many parity tests are spared the round trip.
    // Needs reserve_nn(n) and reserve_sort(n).
    int sort_and_search(const Point4 *d_rows, uint64_t n, double sem_th, bool read_verdict = true);
    // the acceptance by query (k_corr_flag) into d_by_query
    int accept(uint64_t n, double max_dist, int32_t *d_by_query);
    // what sort_and_search left, as correspond.hip reads it
    CorrespondArgs answers(uint64_t n, double max_dist, int32_t *d_by_query) const;

private:
    const hipStream_t s_;
    const char *who_, *noun_;
    bool in_flight_ = false;
};

// the refusal of a frame with a NaN or an Inf in it, on the host and from the sort's verdict alike
int refuse_non_finite(const char *who, const char *noun);
// what an entry on host rows checks of them: NULL, too many, not finite
int check_host_rows(const char *who, const double *xyzl, uint64_t n);
// what an entry on a device frame checks of it: NULL, the layout, where the memory lives, the stream
int check_device_source(const char *who, const sageicp_map *map, const sageicp_device_frame *frame, void *stream);

// the Gauss-Newton step still left and JTJ^-1 (false: none — too few pairs, a pivot below the bound, not finite)
struct QualitySolve {
    double step[6], step_norm, inv[6][6], s2;
};
bool quality_solve(const double JTJ[36], const double JTr[6], double sum_w_r2, uint64_t n_pairs, QualitySolve *o);

// What sageicp_quality and sageicp_pose_score derive alike from the sums both passes leave (QualityRaw, ScoreRaw: the
// four pair counts and the first kQWR2 + 1 real sums): the report zeroed, then counts, sum_r2, sum_w, sum_w_r2, JTJ, JTr,
// fitness, rmse, and step and step_norm when the system can be solved (the return value; *sol is written then).
template <typename Report, typename Raw>
bool derive_shared(const Raw &r, uint64_t n, Report *q, QualitySolve *sol) {
    std::memset(q, 0, sizeof(*q));
    q->valid = 1;
    q->n_queries = n;
    q->n_pairs = r.counts[kQPairs];
    q->pairs_same_label = r.counts[kQSame];
    q->pairs_unlabelled = r.counts[kQUnlabelled];
    q->pairs_cross_label = r.counts[kQCross];
    q->sum_r2 = r.real[kQR2];
    q->sum_w = r.real[kW];
    q->sum_w_r2 = r.real[kQWR2];
    assemble_normal_equations(r.real, q->JTJ, q->JTr);        // (reads the 16 sums of sageicp_types.h's Sum only)
    const double np = static_cast<double>(q->n_pairs);
    q->fitness = np / static_cast<double>(n);
    q->rmse = q->n_pairs ? std::sqrt(q->sum_r2 / np) : 0.0;
    if (!quality_solve(q->JTJ, q->JTr, q->sum_w_r2, q->n_pairs, sol)) return false;
    for (int i = 0; i < 6; ++i) q->step[i] = sol->step[i];
    q->step_norm = sol->step_norm;
    return true;
}

// The quality report of n rows the library holds on the device (the pipeline's source cloud, d_score_frame), not yet
// moved by `pose`: a call of its own, worded as RegistrationQuality's; staged into d_frame, where the report moves them.
// The mirror is current.
int quality_of_device_rows(sageicp_map &m, const Point4 *d_rows, uint64_t n, const double *pose, double max_dist,
                           double kernel, double sem_th, sageicp_quality *out);

}  // namespace sageicp_impl
