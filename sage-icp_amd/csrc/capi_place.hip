// Place recognition behind the C ABI (include/sageicp.h, sageicp_place_*): the parameter checks and the two host-made
// tables, the stand-alone describe entries, the database handle and its matcher, and the step the pipeline runs for a
// key frame (capi_pipeline.hip).  The kernels are place.hip's.  Host code only.  Part of libsageicp_hip.so's host side:
// capi_internal.h.
#include "capi_internal.h"

namespace sageicp_impl {

int place_check_params(const sageicp_place_params *p) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null place params");
    if (!std::isfinite(p->min_range) || !std::isfinite(p->max_range) || !std::isfinite(p->z_lo) || !std::isfinite(p->z_hi))
        return fail(SAGEICP_ERR_INVALID, "place params: a range or a height is not finite");
    if (!(p->min_range > 0.0) || !(p->min_range < p->max_range))
        return fail(SAGEICP_ERR_INVALID, "place params: 0 < min_range < max_range does not hold");
    if (!(p->z_lo < p->z_hi)) return fail(SAGEICP_ERR_INVALID, "place params: z_lo >= z_hi");
    if (p->rings < 1 || p->rings > kPlaceMaxRings) return fail(SAGEICP_ERR_INVALID, "place params: rings must lie in [1, 64]");
    if (p->sectors < kPlaceMinSectors || p->sectors > kPlaceMaxSectors)
        return fail(SAGEICP_ERR_INVALID, "place params: sectors must lie in [3, 360]");
    if (static_cast<uint32_t>(p->rings) * static_cast<uint32_t>(p->sectors) > kPlaceMaxCells)
        return fail(SAGEICP_ERR_INVALID, "place params: rings * sectors must not exceed 16384");
    return SAGEICP_OK;
}

int place_check_query(const sageicp_place_query *q) {
    if (!q) return fail(SAGEICP_ERR_INVALID, "null place query");
    if (q->top_k < 1 || q->top_k > kPlaceMaxTop) return fail(SAGEICP_ERR_INVALID, "place query: top_k must lie in [1, 16]");
    if (q->h_tol > 255) return fail(SAGEICP_ERR_INVALID, "place query: h_tol must lie in [0, 255]");
    if (!std::isfinite(q->min_similarity)) return fail(SAGEICP_ERR_INVALID, "place query: min_similarity is not finite");
    return SAGEICP_OK;
}

static void place_tables(const sageicp_place_params &p, double *edge2, double *dir) {
    const double width = (p.max_range - p.min_range) / static_cast<double>(p.rings);
    for (int k = 0; k <= p.rings; ++k) {
        const double e = p.min_range + static_cast<double>(k) * width;
        edge2[k] = e * e;
    }
    for (int s = 0; s < p.sectors; ++s) {
        const double a = (2.0 * M_PI * static_cast<double>(s)) / static_cast<double>(p.sectors);
        dir[2 * s] = std::cos(a);
        dir[2 * s + 1] = std::sin(a);
    }
}

// a parameter set on a device: the tables, and the planes a descriptor is drawn in
struct PlaceDevice {
    sageicp_place_params prm{};
    uint32_t cells = 0;
    DevBuf<double> d_edge2, d_dir;
    DevBuf<uint8_t> d_rank;
    DevBuf<uint32_t> d_planes;
    PlaceGrid grid{};
    // (the device is current; the uploads are waited for)
    int init(const sageicp_place_params &p) {
        prm = p;
        cells = static_cast<uint32_t>(p.rings) * static_cast<uint32_t>(p.sectors);
        std::vector<double> edge2(p.rings + 1), dir(2 * static_cast<size_t>(p.sectors));
        place_tables(p, edge2.data(), dir.data());
        HIPCHK(d_edge2.reserve(edge2.size()));
        HIPCHK(d_dir.reserve(dir.size()));
        HIPCHK(d_rank.reserve(256));
        HIPCHK(d_planes.reserve(2 * static_cast<size_t>(cells)));
        HIPCHK(hipMemcpy(d_edge2.data(), edge2.data(), edge2.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_dir.data(), dir.data(), dir.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_rank.data(), p.rank, 256, hipMemcpyHostToDevice));
        grid = PlaceGrid{p.z_lo, p.z_hi, p.rings, p.sectors, d_edge2.data(), d_dir.data(), d_rank.data()};
        return SAGEICP_OK;
    }
    uint32_t bytes() const { return 2 * cells; }
    // enqueues on s: the descriptor of n rows into d_desc (device memory, bytes() of them)
    int describe(const Point4 *d_rows, uint64_t n, uint8_t *d_desc, int *d_flag, hipStream_t s) {
        HIPCHK(hipMemsetAsync(d_planes.data(), 0, 2 * static_cast<size_t>(cells) * sizeof(uint32_t), s));
        launch_place_draw(d_rows, static_cast<int>(n), grid, d_planes.data(), d_flag, s);
        HIPCHK(hipGetLastError());
        launch_place_pack(d_planes.data(), cells, d_desc, s);
        HIPCHK(hipGetLastError());
        return SAGEICP_OK;
    }
};

// n rows on the device into host bytes, on s, which is waited for; a coordinate that is not finite refuses the call
static int describe_to_host(const sageicp_place_params &prm, const Point4 *d_rows, uint64_t n, uint8_t *desc_out,
                            hipStream_t s) {
    PlaceDevice pd;
    DevBuf<uint8_t> d_desc;
    DevBuf<int> d_flag;
    int rc = pd.init(prm);
    if (rc) return rc;
    HIPCHK(d_desc.reserve(pd.bytes()));
    HIPCHK(d_flag.reserve(1));
    HIPCHK(hipMemsetAsync(d_flag.data(), 0, sizeof(int), s));
    int flags = 0;
    rc = pd.describe(d_rows, n, d_desc.data(), d_flag.data(), s);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(&flags, d_flag.data(), sizeof(int), hipMemcpyDeviceToHost, s);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(desc_out, d_desc.data(), pd.bytes(), hipMemcpyDeviceToHost, s);
    const hipError_t w = hipStreamSynchronize(s);       // (nothing this call enqueued runs on once it has returned)
    if (rc) return rc;
    HIPCHK(e);
    HIPCHK(w);
    if (flags & kOccNonFinite) {
        std::memset(desc_out, 0, pd.bytes());
        return fail(SAGEICP_ERR_INVALID, "a coordinate is not finite (NaN / Inf)");
    }
    return SAGEICP_OK;
}

static void place_prior(const double pose[7], uint32_t shift, int32_t sectors, double *yaw_out, double prior[7]) {
    const double w = 2.0 * M_PI / static_cast<double>(sectors);
    const uint32_t S = static_cast<uint32_t>(sectors);
    const double yaw = shift <= S / 2 ? static_cast<double>(shift) * w
                                      : static_cast<double>(static_cast<int64_t>(shift) - static_cast<int64_t>(S)) * w;
    if (yaw_out) *yaw_out = yaw;
    if (!prior) return;
    for (int i = 0; i < 7; ++i) prior[i] = pose[i];
    if (shift == 0) return;
    // q_entry (x) q_z(yaw), q_z = (0, 0, s, c): the Hamilton product with its zero terms left out
    const double s = std::sin(yaw / 2.0), c = std::cos(yaw / 2.0);
    prior[0] = c * pose[0] + s * pose[1];
    prior[1] = c * pose[1] - s * pose[0];
    prior[2] = c * pose[2] + s * pose[3];
    prior[3] = c * pose[3] - s * pose[2];
}

}  // namespace sageicp_impl

struct sageicp_place_db {
    int device = 0;
    PlaceDevice pd;
    uint64_t size = 0;
    std::vector<uint64_t> tags;
    std::vector<std::array<double, 7>> poses;
    DevBuf<uint8_t> d_desc;             // [capacity][bytes]
    uint64_t capacity = 0;              // entries
    DevBuf<uint8_t> d_query;            // the descriptor being matched (and, in the pipeline, appended)
    DevBuf<PlaceQueryCell> d_cells;
    DevBuf<uint32_t> d_nq;
    DevBuf<PlaceScore> d_scores;        // [capacity]
    DevBuf<PlaceTop> d_top;
    PinnedBuf<PlaceTop> h_top;
    OwnedStream stream;                 // (after the buffers: waited for before they go)

    int init(const sageicp_place_params &p, int dev) {
        device = dev;
        HIPCHK(hipSetDevice(device));
        if (int rc = pd.init(p)) return rc;
        HIPCHK(d_query.reserve(pd.bytes()));
        HIPCHK(d_cells.reserve(pd.cells));
        HIPCHK(d_nq.reserve(1));
        HIPCHK(d_top.reserve(1));
        HIPCHK(h_top.reserve(1));
        HIPCHK(stream.create());
        return SAGEICP_OK;
    }
    // room for one more entry; growth by doubling, the entries copied over on s (which is waited for)
    int reserve_one(hipStream_t s) {
        if (size >= kPlaceMaxEntries) return fail(SAGEICP_ERR_CAPACITY, "the place database holds 2^20 entries");
        if (size < capacity) return SAGEICP_OK;
        const uint64_t cap = capacity ? 2 * capacity : 64;
        HIPCHK(d_desc.grow(cap * pd.bytes(), size * pd.bytes(), s));
        capacity = cap;
        d_scores.reset();                // (sized with the next match)
        return SAGEICP_OK;
    }
    void push_host(uint64_t tag, const double *pose) {
        std::array<double, 7> ps{0, 0, 0, 1, 0, 0, 0};
        if (pose) std::copy(pose, pose + 7, ps.begin());
        tags.push_back(tag);
        poses.push_back(ps);
        ++size;
    }
    // Enqueues on s the match of d_query against entries [0, considered): compile, score, select, the download of the
    // records.  The caller waits for s, then reads them with finish_match.
    int enqueue_match(const sageicp_place_query &q, uint64_t considered, hipStream_t s) {
        if (!d_scores || d_scores.capacity() < capacity) HIPCHK(d_scores.reserve(capacity));
        HIPCHK(hipMemsetAsync(d_nq.data(), 0, sizeof(uint32_t), s));
        launch_place_compile(d_query.data(), pd.prm.rings, pd.prm.sectors, q.h_tol, d_cells.data(), d_nq.data(), s);
        HIPCHK(hipGetLastError());
        launch_place_score(d_desc.data(), static_cast<uint32_t>(considered), pd.prm.rings, pd.prm.sectors, d_cells.data(),
                           d_nq.data(), d_scores.data(), knobs().place_doubled.get() == 0, s);
        HIPCHK(hipGetLastError());
        launch_place_select(d_scores.data(), static_cast<uint32_t>(considered), d_nq.data(), q.top_k, d_top.data(), s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_top.data(), d_top.data(), sizeof(PlaceTop), hipMemcpyDeviceToHost, s));
        return SAGEICP_OK;
    }
    void finish_match(const sageicp_place_query &q, sageicp_place_match *out, uint32_t *n_out) const {
        const PlaceTop &t = *h_top.data();
        uint32_t n = 0;
        for (uint32_t i = 0; i < t.count && i < q.top_k; ++i) {
            const PlaceTop::Rec &r = t.rec[i];
            const uint32_t m = std::max(t.n_query, r.n_entry);
            const double sim = m ? static_cast<double>(r.agree) / static_cast<double>(m) : 0.0;
            if (sim < q.min_similarity) break;          // (the ranking is by this ratio: the rest lie below too)
            sageicp_place_match &o = out[n++];
            o = sageicp_place_match{};
            o.similarity = sim;
            o.index = r.index;
            o.tag = tags[r.index];
            o.agree = r.agree;
            o.n_query = t.n_query;
            o.n_entry = r.n_entry;
            o.shift = r.shift;
            for (int k = 0; k < 7; ++k) o.pose[k] = poses[r.index][k];
            place_prior(o.pose, r.shift, pd.prm.sectors, &o.yaw, o.prior);
        }
        *n_out = n;
    }
    ~sageicp_place_db() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream.get());
    }
};

namespace sageicp_impl {

sageicp_place_db *place_db_new(const sageicp_place_params &p, int device) {
    std::unique_ptr<sageicp_place_db> db(new sageicp_place_db);
    if (db->init(p, device)) return nullptr;
    return db.release();
}
void place_db_clear(sageicp_place_db &db) {
    db.size = 0;
    db.tags.clear();
    db.poses.clear();
}

// The pipeline's step for a key frame, on s: the descriptor of the n raw rows, its match against the database as it is,
// then the descriptor appended.  One wait, for the download of the records.
int place_db_step(sageicp_place_db &db, const Point4 *d_rows, uint64_t n, const sageicp_place_query &q, uint64_t tag,
                  const double pose[7], hipStream_t s, sageicp_place_match *out, uint32_t *n_out) {
    *n_out = 0;
    HIPCHK(hipSetDevice(db.device));
    if (int rc = db.reserve_one(s)) return rc;
    if (int rc = db.pd.describe(d_rows, n, db.d_query.data(), nullptr, s)) return rc;
    // (the slot is not an entry until the host counts it: the match below considers [0, size - exclude_last))
    HIPCHK(hipMemcpyAsync(db.d_desc.data() + db.size * db.pd.bytes(), db.d_query.data(), db.pd.bytes(),
                          hipMemcpyDeviceToDevice, s));
    const uint64_t considered = q.exclude_last >= db.size ? 0 : db.size - q.exclude_last;
    if (considered)
        if (int rc = db.enqueue_match(q, considered, s)) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
    HIPCHK(hipStreamSynchronize(s));
    if (considered) db.finish_match(q, out, n_out);
    db.push_host(tag, pose);
    return SAGEICP_OK;
}

}  // namespace sageicp_impl

extern "C" {

int sageicp_place_tables(const sageicp_place_params *params, double *edge2_out, double *dir_out) {
    if (int rc = place_check_params(params)) return rc;
    if (!edge2_out || !dir_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    place_tables(*params, edge2_out, dir_out);
    return SAGEICP_OK;
}

int sageicp_place_prior(const double pose[7], uint32_t shift, int32_t sectors, double *yaw_out, double prior_out[7]) {
    if (!pose || (!yaw_out && !prior_out)) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (sectors < kPlaceMinSectors || sectors > kPlaceMaxSectors || shift >= static_cast<uint32_t>(sectors))
        return fail(SAGEICP_ERR_INVALID, "sectors must lie in [3, 360] and shift below it");
    place_prior(pose, shift, sectors, yaw_out, prior_out);
    return SAGEICP_OK;
}

int sageicp_place_describe(const double *xyzl, uint64_t n, const sageicp_place_params *params, uint8_t *desc_out,
                           int device) {
    if ((n && !xyzl) || !desc_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (int rc = place_check_params(params)) return rc;
    if (n > kMaxQueries) return fail(SAGEICP_ERR_INVALID, "frame too large (2^26 - 4 points max)");
    for (uint64_t i = 0; i < n; ++i)
        if (!finite_n(xyzl + 4 * i, 3)) return fail(SAGEICP_ERR_INVALID, "a coordinate is not finite (NaN / Inf)");
    if (int rc = require_device(device)) return rc;
    const size_t bytes = 2 * static_cast<size_t>(params->rings) * params->sectors;
    if (n == 0) {
        std::memset(desc_out, 0, bytes);
        return SAGEICP_OK;
    }
    HIPCHK(hipSetDevice(device));
    DevBuf<Point4> d_p;
    OwnedStream s;                      // (after the buffer: waited for before it is freed)
    HIPCHK(s.create());
    HIPCHK(d_p.reserve(n));
    HIPCHK(hipMemcpyAsync(d_p.data(), xyzl, n * sizeof(Point4), hipMemcpyHostToDevice, s.get()));
    return describe_to_host(*params, d_p.data(), n, desc_out, s.get());
}

int sageicp_place_describe_device(const sageicp_device_frame *frame, const sageicp_place_params *params,
                                  uint8_t *desc_out, void *stream) {
    if (!frame || !desc_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (int rc = place_check_params(params)) return rc;
    // no handle: the work runs on the device the frame's memory lives on, looked up once its layout has passed
    int device = 0;
    if (int rc = check_device_frame(frame, nullptr, stream, device, &device)) return rc;
    const size_t bytes = 2 * static_cast<size_t>(params->rings) * params->sectors;
    if (frame->n == 0) {
        std::memset(desc_out, 0, bytes);
        return SAGEICP_OK;
    }
    HIPCHK(hipSetDevice(device));
    // on the caller's stream, behind the work that wrote the frame; synchronous
    const hipStream_t s = static_cast<hipStream_t>(stream);
    DevBuf<Point4> d_p;
    HIPCHK(d_p.reserve(frame->n));
    launch_ingest(ingest_args(*frame), d_p.data(), s);
    HIPCHK(hipGetLastError());
    const int rc = describe_to_host(*params, d_p.data(), frame->n, desc_out, s);
    (void)hipStreamSynchronize(s);          // (d_p leaves scope)
    return rc;
}

sageicp_place_db *sageicp_place_db_create(const sageicp_place_params *params, int device) {
    if (place_check_params(params)) return nullptr;
    if (require_device(device)) return nullptr;
    return place_db_new(*params, device);
}
void sageicp_place_db_destroy(sageicp_place_db *db) { delete db; }
uint64_t sageicp_place_db_size(const sageicp_place_db *db) { return db ? db->size : 0; }
int sageicp_place_db_clear(sageicp_place_db *db) {
    if (!db) return fail(SAGEICP_ERR_INVALID, "null place database");
    place_db_clear(*db);
    return SAGEICP_OK;
}
int sageicp_place_db_add(sageicp_place_db *db, const uint8_t *desc, uint64_t tag, const double pose[7],
                         uint64_t *index_out) {
    if (!db || !desc) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (pose && !finite_n(pose, 7)) return fail(SAGEICP_ERR_INVALID, "the pose is not finite");
    HIPCHK(hipSetDevice(db->device));
    const hipStream_t s = db->stream.get();
    if (int rc = db->reserve_one(s)) return rc;
    HIPCHK(hipMemcpyAsync(db->d_desc.data() + db->size * db->pd.bytes(), desc, db->pd.bytes(), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (index_out) *index_out = db->size;
    db->push_host(tag, pose);
    return SAGEICP_OK;
}
int sageicp_place_db_read(const sageicp_place_db *db, uint64_t first, uint64_t count, uint8_t *desc_out,
                          uint64_t *tags_out, double *poses_out) {
    if (!db) return fail(SAGEICP_ERR_INVALID, "null place database");
    if (first > db->size || count > db->size - first) return fail(SAGEICP_ERR_INVALID, "entries beyond the database's size");
    if (!count) return SAGEICP_OK;
    for (uint64_t i = 0; i < count; ++i) {
        if (tags_out) tags_out[i] = db->tags[first + i];
        if (poses_out) std::copy(db->poses[first + i].begin(), db->poses[first + i].end(), poses_out + 7 * i);
    }
    if (desc_out) {
        HIPCHK(hipSetDevice(db->device));
        const hipStream_t s = db->stream.get();
        HIPCHK(hipMemcpyAsync(desc_out, db->d_desc.data() + first * db->pd.bytes(), count * db->pd.bytes(),
                              hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return SAGEICP_OK;
}
int sageicp_place_db_match(const sageicp_place_db *cdb, const uint8_t *desc, const sageicp_place_query *query,
                           sageicp_place_match *out, uint32_t *n_out) {
    if (!cdb || !desc || !out || !n_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (int rc = place_check_query(query)) return rc;
    // (the entries are unchanged by a match; its work buffers and stream are the handle's)
    sageicp_place_db &db = *const_cast<sageicp_place_db *>(cdb);
    *n_out = 0;
    if (query->exclude_last >= db.size) return SAGEICP_OK;
    const uint64_t considered = db.size - query->exclude_last;
    HIPCHK(hipSetDevice(db.device));
    const hipStream_t s = db.stream.get();
    HIPCHK(hipMemcpyAsync(db.d_query.data(), desc, db.pd.bytes(), hipMemcpyHostToDevice, s));
    const int rc = db.enqueue_match(*query, considered, s);
    const hipError_t w = hipStreamSynchronize(s);
    if (rc) return rc;
    HIPCHK(w);
    db.finish_match(*query, out, n_out);
    return SAGEICP_OK;
}

}  // extern "C"
