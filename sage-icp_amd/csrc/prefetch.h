// The pipeline's announce / prepare state (sageicp_pipeline_prefetch): Preprocess() + Voxelize() depend on the raw frame
// only, so the frame after the one being registered can be prepared on a host thread of its own meanwhile.  Two records
// — the frame the caller ANNOUNCED, and the frame the worker PREPARED (or is preparing) — and the worker's result.
// No HIP in here: what the worker runs is the caller's (capi_pipeline.hip); tests/prefetch_check.cpp drives it alone.
//
// One host thread calls in.  The worker writes rc (and, through the caller's job, err) only; both are read after a
// join.  Every operation that touches the prepared record joins first, so no caller has to.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <thread>

namespace sageicp {

class Prefetch {
public:
    int rc = 0;                         // of the prepared frame's job, and its error text (the text is per thread: the
    std::string err;                    // job copies it here)

    // FNV-1a over n and 64 rows spread over the frame: cheap, and enough to tell a buffer that was
    // refilled since it was announced from the frame that was announced
    static uint64_t fingerprint(const double *f, uint64_t m) {
        uint64_t h = 1469598103934665603ull ^ m;
        if (!f || !m) return h;
        const uint64_t step = m / 64 ? m / 64 : 1;
        for (uint64_t i = 0; i < m; i += step) {
            uint64_t w[4];
            std::memcpy(w, f + 4 * i, 32);
            for (uint64_t x : w) { h ^= x; h *= 1099511628211ull; }
        }
        uint64_t w[4];
        std::memcpy(w, f + 4 * (m - 1), 32);
        for (uint64_t x : w) { h ^= x; h *= 1099511628211ull; }
        return h;
    }

    ~Prefetch() { join(); }
    void join() { if (worker.joinable()) worker.join(); }
    // the frame that follows the next one registered (a later announcement overwrites an earlier one)
    void announce(const double *frame, uint64_t n) {
        announced = true;
        an = {frame, n, fingerprint(frame, n)};
    }
    bool has_announcement() const { return announced; }
    // these rows are the prepared frame: the same buffer, the same n, and not refilled since they were announced
    bool prepared_is(const double *frame, uint64_t n) {
        join();
        return ready && pf.frame == frame && pf.n == n && pf.print == fingerprint(frame, n);
    }
    void drop_prepared() { join(); ready = false; }
    void drop_announced() { announced = false; }
    void drop_all() { drop_prepared(); drop_announced(); }
    // The announcement, if there is one, becomes the prepared frame and job(frame, n) -> rc runs on the worker.
    template <typename Job>
    void promote_and_start(Job job) {
        if (!announced) return;
        drop_prepared();
        announced = false;
        ready = true;
        rc = 0;
        err.clear();
        const Record r = pf = an;
        worker = std::thread([this, job, r] { rc = job(r.frame, r.n); });
    }

private:
    struct Record {
        const double *frame = nullptr;
        uint64_t n = 0;
        uint64_t print = 0;             // content fingerprint (a buffer re-used for other data is another frame)
    };
    std::thread worker;
    bool announced = false, ready = false;    // ready: the worker holds, or is filling, pf
    Record an, pf;
};

}  // namespace sageicp
