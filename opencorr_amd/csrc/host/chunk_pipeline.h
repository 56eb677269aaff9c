// chunk_pipeline.h -- the host logic of the chunked host-queue pipeline (capi_host.hip), without the engine: how a queue is
// cut into chunks, and how the thread that feeds chunks in tells the thread that copies them out how far it has got.
// Standard headers only (tests/cpp/chunk_pipeline_check.cpp runs both on a CPU).
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <mutex>
#include <utility>
#include <vector>

namespace ochip_host {

// Chunk schedule: (first POI, POIs) per chunk, contiguous from 0.  What a pipeline cannot hide is the copy-in of its FIRST
// chunk and the copy-out of its LAST one, and every extra chunk costs a launch tail (the ICGN kernels' last workgroups run on
// a half-empty chip) plus an inter-stream hand-over.  So: small chunks at both ends (half of "host_chunk"), few large ones
// (three times "host_chunk") in between, whose copies hide behind the neighbours' kernels.  Measured on config B (250 000
// POIs, chain of FFTCC2D + ICGN2D1): uniform chunks of 65 536: 4.76 ms, one piece: 5.36 ms, this schedule: see DESIGN 4.4.
// host_chunk = 0: the whole queue at once.
inline std::vector<std::pair<size_t, size_t>> chunk_schedule(size_t count, int host_chunk, bool transfer_bound) {
    std::vector<std::pair<size_t, size_t>> sched;
    const size_t unit = host_chunk > 0 ? (size_t)host_chunk : count;
    // A lone FFTCC engine (the first call of the reference's unmodified `fftcc->compute(q); icgn->compute(q);`) is
    // TRANSFER bound: 0.44 ms of kernel between 0.5 ms in and 0.5 ms out on config B.  There the copies of the two
    // directions should overlap each other (PCIe is full duplex): uniform chunks of half a unit -- with the edge / middle
    // schedule below the big middle chunk's copy-in, kernel and copy-out run one after the other (round 6: two-call
    // sequence 5.0 -> see DESIGN 4.6).
    if (transfer_bound && host_chunk > 0 && count >= unit) {
        const size_t piece = std::max<size_t>(unit / 2, 1), np = (count + piece - 1) / piece;
        size_t at = 0;
        for (size_t i = 0; i < np; i++) {
            const size_t n = count / np + (i < count % np ? 1 : 0);
            sched.emplace_back(at, n);
            at += n;
        }
    } else if (count < 2 * unit) {
        sched.emplace_back(0, count);  // not worth a pipeline
    } else {
        const size_t edge = std::max<size_t>(unit / 2, 1), mid_max = 3 * unit;
        sched.emplace_back(0, edge);
        size_t at = edge;
        const size_t mid_total = count - 2 * edge;
        const size_t nmid = (mid_total + mid_max - 1) / mid_max;
        for (size_t i = 0; i < nmid; i++) {
            const size_t n = mid_total / nmid + (i < mid_total % nmid ? 1 : 0);
            sched.emplace_back(at, n);
            at += n;
        }
        sched.emplace_back(at, count - at);
    }
    return sched;
}

// The feeding thread enqueues chunk c's kernels and the event behind them, then hands the chunk over; the copy-out thread
// must not wait on that event earlier (it would see the event of an earlier call), so it sleeps here until the hand-over.
// One feeder, one consumer per reset().
class ChunkHandoff {
public:
    void reset() {
        std::lock_guard<std::mutex> lk(mu_);
        fed_ = 0;
    }
    // chunks 0 .. n-1 are enqueued
    void hand_over(size_t n) { publish(n); }
    // the feeder gives up: no further chunk will come
    void fail() { publish(kFailed); }
    // sleeps until chunk c has been handed over; false once the feeder has failed
    bool wait_for(size_t c) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return fed_ > c; });
        return fed_ != kFailed;
    }

private:
    static constexpr size_t kFailed = (size_t)-1;
    void publish(size_t fed) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            fed_ = fed;
        }
        cv_.notify_one();
    }
    std::mutex mu_;
    std::condition_variable cv_;
    size_t fed_ = 0;  // chunks whose kernels (and event) are enqueued
};

}  // namespace ochip_host
