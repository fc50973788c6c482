// ReplayPool: a few parked host threads that run the indices of one small job side by side.  Used by Prep's order
// replays (prep.hip) and by the pre-touch of a fresh host destination (capi_outputs.hip).
#pragma once

#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace sageicp {

// A few parked host threads for the order replays of one Prep (one per label group at most): a
// replay of a few thousand keys costs no more than starting a thread does, and the replays of a
// level are the critical path of a streamed frame.  run(count, f) executes f(0..count-1), each index
// once, on the workers and the calling thread; indices are handed out in order (largest job first
// if the caller sorted them so).
class ReplayPool {
public:
    static constexpr int kMaxThreads = 64;     // what a caller that takes the count from outside asks for at most
    ~ReplayPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    void run(size_t count, const std::function<void(size_t)> &f, size_t want_threads) {
        if (count <= 1 || want_threads <= 1) {
            for (size_t i = 0; i < count; ++i) f(i);
            return;
        }
        while (th_.size() + 1 < std::min(want_threads, count)) th_.emplace_back([this] { worker(); });
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &f;
            total_ = count;
            next_ = 0;
            pending_ = count;
            ++epoch_;
        }
        cv_.notify_all();
        drain();
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
        job_ = nullptr;
        total_ = next_ = 0;
    }

private:
    void drain() {
        for (;;) {
            size_t i;
            const std::function<void(size_t)> *job;
            {   // (a handful of jobs per level: the lock is not contended, and a worker still between
                // two jobs when the next run() starts sees that run's state consistently)
                std::lock_guard<std::mutex> lk(mu_);
                if (next_ >= total_) return;
                i = next_++;
                job = job_;
            }
            (*job)(i);
            std::lock_guard<std::mutex> lk(mu_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    void worker() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || (epoch_ != seen && job_); });
                if (stop_) return;
                seen = epoch_;
            }
            drain();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t)> *job_ = nullptr;
    size_t total_ = 0, pending_ = 0, next_ = 0;
    uint64_t epoch_ = 0;
    bool stop_ = false;
};

}  // namespace sageicp
