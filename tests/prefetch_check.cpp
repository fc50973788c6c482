// csrc/prefetch.h on the CPU: the pipeline's announce / prepare state driven the way the entries of capi_pipeline.hip
// drive it, with a stand-in for the worker's job that records which (pointer, n, side) it was given and returns a
// chosen rc.  Its own main; no HIP.  tests/test_prefetch_host.py builds and runs it plain, with the address and
// undefined-behaviour sanitizers, and with the thread sanitizer.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "prefetch.h"

using sageicp::Prefetch;

static long g_checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) {                                                               \
            std::printf("prefetch_check: FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

// The entries' use of Prefetch, without the device: two sides, `cur` the one the frame being registered lives in.
struct Model {
    struct Given {
        const double *frame;
        uint64_t n;
        int side;
    };
    std::vector<Given> worker_got;      // written by the worker: read after a join only
    int worker_rc = 0;                  // what the next worker job returns
    int prepared_here = 0;              // register calls that prepared their own frame (in side `cur`)
    int cur = 0;
    Prefetch pf;                        // (last: joined before what its worker writes goes)

    enum Kind { kHostRows, kDeviceFrame, kMessage };
    struct Result {
        int rc;
        std::string err;
        bool took_prepared;
    };
    // Backend::voxelize; prepare_rc: what preparing this frame in this call gives, if it comes to that
    Result register_frame(const double *rows, uint64_t n, Kind kind = kHostRows, bool deskewed = false, int prepare_rc = 0) {
        pf.join();
        if (kind == kMessage && n == 0) {
            pf.drop_all();
            return {0, "", false};
        }
        Result r{0, "", false};
        if (!deskewed && kind == kHostRows && pf.prepared_is(rows, n)) {
            r = {pf.rc, pf.rc ? pf.err : "", true};
            cur ^= 1;
        } else {
            r.rc = prepare_rc;
            ++prepared_here;
        }
        pf.drop_prepared();
        const int side = cur ^ 1;
        const int rc = worker_rc;
        if (r.rc == 0)
            pf.promote_and_start([this, side, rc](const double *f, uint64_t m) {
                worker_got.push_back({f, m, side});
                if (rc) pf.err = "the worker's job failed";
                return rc;
            });
        pf.drop_announced();
        return r;
    }
    void prefetch(const double *rows, uint64_t n) { pf.announce(rows, n); }
    void wait() { pf.join(); }
    void cancel() { pf.drop_all(); }
    void set_deskew() { pf.drop_all(); }
    void set_dynamic_filter() { pf.drop_prepared(); }
};

static std::vector<double> frame_of(uint64_t n, double seed) {
    std::vector<double> f(4 * n);
    for (uint64_t i = 0; i < 4 * n; ++i) f[i] = seed + 0.25 * static_cast<double>(i);
    return f;
}

// announce b, register a: the worker is started with b; register b: the prepared frame is taken, the side flips
static void announce_then_register(uint64_t n) {
    std::vector<double> a = frame_of(n, 1.0), b = frame_of(n, 2.0);
    Model m;
    m.prefetch(b.data(), n);
    Model::Result r = m.register_frame(a.data(), n);
    CHECK(r.rc == 0 && !r.took_prepared && m.prepared_here == 1 && m.cur == 0);
    m.wait();
    CHECK(m.worker_got.size() == 1 && m.worker_got[0].frame == b.data() && m.worker_got[0].n == n && m.worker_got[0].side == 1);
    r = m.register_frame(b.data(), n);
    CHECK(r.rc == 0 && r.took_prepared && m.prepared_here == 1 && m.cur == 1);
    // taken once: the same buffer again is prepared in its own call
    r = m.register_frame(b.data(), n);
    CHECK(r.rc == 0 && !r.took_prepared && m.prepared_here == 2 && m.cur == 1 && m.worker_got.size() == 1);
}

// the announced buffer with one sampled row rewritten before it is registered is another frame
static void refilled_buffer(uint64_t n) {
    const uint64_t step = n / 64 ? n / 64 : 1;
    const uint64_t rows[3] = {0, n - 1, step * ((n / 2) / step)};
    for (uint64_t row : rows) {
        std::vector<double> a = frame_of(n, 1.0), b = frame_of(n, 2.0);
        Model m;
        m.prefetch(b.data(), n);
        CHECK(m.register_frame(a.data(), n).rc == 0);
        m.wait();
        b[4 * row + 1] += 1.0;
        const Model::Result r = m.register_frame(b.data(), n);
        CHECK(r.rc == 0 && !r.took_prepared && m.prepared_here == 2 && m.cur == 0);
    }
    if (step > 1) {     // what the fingerprint is: a row it does not sample can change unseen
        std::vector<double> a = frame_of(n, 1.0), b = frame_of(n, 2.0);
        Model m;
        m.prefetch(b.data(), n);
        CHECK(m.register_frame(a.data(), n).rc == 0);
        m.wait();
        b[4 * 1] += 1.0;
        CHECK(m.register_frame(b.data(), n).took_prepared);
    }
}

static void another_n_or_kind(uint64_t n) {
    std::vector<double> a = frame_of(n, 1.0), b = frame_of(n + 1, 2.0);
    {   // the same pointer with another n
        Model m;
        m.prefetch(b.data(), n + 1);
        CHECK(m.register_frame(a.data(), n).rc == 0);
        const Model::Result r = m.register_frame(b.data(), n);
        CHECK(!r.took_prepared && m.prepared_here == 2 && m.cur == 0);
    }
    // a device frame, a message and a deskewed frame are never the prepared frame; each consumes the announcement
    const Model::Kind kinds[3] = {Model::kDeviceFrame, Model::kMessage, Model::kHostRows};
    for (int k = 0; k < 3; ++k) {
        Model m;
        m.prefetch(b.data(), n + 1);
        CHECK(m.register_frame(a.data(), n).rc == 0);
        m.prefetch(a.data(), n);
        const Model::Result r = m.register_frame(b.data(), n + 1, kinds[k], /*deskewed*/ k == 2);
        CHECK(!r.took_prepared && m.prepared_here == 2 && m.cur == 0);
        m.wait();
        CHECK(m.worker_got.size() == 2 && m.worker_got[1].frame == a.data() && m.worker_got[1].side == 1);
        CHECK(m.register_frame(a.data(), n).took_prepared);
    }
    {   // an empty message drops the prepared frame and the announcement, and starts nothing
        Model m;
        m.prefetch(b.data(), n + 1);
        CHECK(m.register_frame(a.data(), n).rc == 0);
        m.prefetch(a.data(), n);
        CHECK(m.register_frame(nullptr, 0, Model::kMessage).rc == 0);
        CHECK(!m.pf.has_announcement() && m.worker_got.size() == 1);
        CHECK(!m.register_frame(b.data(), n + 1).took_prepared);
        CHECK(m.worker_got.size() == 1);
    }
}

// a failing worker's rc and text come back from the register call that consumes its frame, not earlier
static void failing_worker(uint64_t n) {
    std::vector<double> a = frame_of(n, 1.0), b = frame_of(n, 2.0);
    Model m;
    m.worker_rc = -7;
    m.prefetch(b.data(), n);
    Model::Result r = m.register_frame(a.data(), n);
    CHECK(r.rc == 0 && r.err.empty());
    m.wait();
    m.worker_rc = 0;
    m.prefetch(a.data(), n);
    r = m.register_frame(b.data(), n);
    CHECK(r.rc == -7 && r.err == "the worker's job failed" && r.took_prepared && m.cur == 1);
    // ... and a register call that fails still consumes the announcement: nothing was started for it
    CHECK(!m.pf.has_announcement() && m.worker_got.size() == 1);
    CHECK(!m.register_frame(a.data(), n).took_prepared);
    // the same when the frame fails in its own call
    m.prefetch(b.data(), n);
    r = m.register_frame(a.data(), n, Model::kHostRows, false, /*prepare_rc*/ -3);
    CHECK(r.rc == -3 && !m.pf.has_announcement() && m.worker_got.size() == 1);
    CHECK(!m.register_frame(b.data(), n).took_prepared);
}

static void switches(uint64_t n) {
    std::vector<double> a = frame_of(n, 1.0), b = frame_of(n, 2.0), c = frame_of(n, 3.0);
    for (int which = 0; which < 2; ++which) {   // cancel and the deskew switch drop both records
        Model m;
        m.prefetch(b.data(), n);
        CHECK(m.register_frame(a.data(), n).rc == 0);
        m.prefetch(c.data(), n);
        if (which) m.set_deskew(); else m.cancel();
        CHECK(!m.pf.has_announcement());
        CHECK(!m.register_frame(b.data(), n).took_prepared);
        m.wait();
        CHECK(m.worker_got.size() == 1);        // c was never promoted
        CHECK(!m.register_frame(c.data(), n).took_prepared);
    }
    {   // the dynamic-filter switch drops the prepared frame and leaves the announcement, which the next register promotes
        Model m;
        m.prefetch(b.data(), n);
        CHECK(m.register_frame(a.data(), n).rc == 0);
        m.prefetch(c.data(), n);
        m.set_dynamic_filter();
        CHECK(m.pf.has_announcement());
        CHECK(!m.register_frame(b.data(), n).took_prepared && m.cur == 0);
        m.wait();
        CHECK(m.worker_got.size() == 2 && m.worker_got[1].frame == c.data() && m.worker_got[1].side == 1);
        CHECK(m.register_frame(c.data(), n).took_prepared && m.cur == 1);
    }
    {   // wait keeps the prepared frame; a later announcement overwrites an earlier one
        Model m;
        m.prefetch(c.data(), n);
        m.prefetch(b.data(), n);
        CHECK(m.register_frame(a.data(), n).rc == 0);
        m.wait();
        m.wait();
        CHECK(m.worker_got.size() == 1 && m.worker_got[0].frame == b.data());
        CHECK(m.register_frame(b.data(), n).took_prepared);
    }
}

// destruction with a worker in flight joins it
static void destruction_joins() {
    std::atomic<bool> leaving{false}, done{false};
    std::vector<double> a = frame_of(8, 1.0);
    {
        Prefetch pf;
        pf.announce(a.data(), 8);
        pf.promote_and_start([&](const double *, uint64_t) {
            while (!leaving.load()) std::this_thread::yield();
            for (int i = 0; i < 1000; ++i) std::this_thread::yield();
            done.store(true);
            return 0;
        });
        leaving.store(true);
    }
    CHECK(done.load());
}

int main() {
    // step = max(1, n / 64) is 1 below 128 rows
    for (uint64_t n : {uint64_t{1}, uint64_t{63}, uint64_t{64}, uint64_t{65}, uint64_t{200}}) {
        announce_then_register(n);
        refilled_buffer(n);
        another_n_or_kind(n);
        failing_worker(n);
        switches(n);
    }
    // the fingerprint of nothing is defined (an empty announcement is legal)
    CHECK(Prefetch::fingerprint(nullptr, 0) == Prefetch::fingerprint(nullptr, 0));
    destruction_joins();
    std::printf("prefetch_check: OK %ld\n", g_checks);
    return 0;
}
