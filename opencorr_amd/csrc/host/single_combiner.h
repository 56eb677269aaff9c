// single_combiner.h -- the combining front end of compute(POI*), without the engine: concurrent callers hand in one request
// each, one of them (the leader) serves everything that is queued as ONE batch.  Standard headers only, so that the protocol
// runs on a CPU under a thread sanitizer (tests/cpp/single_combiner_stress.cpp).
//
// The reference's single-POI form is called from the CALLER's own OpenMP loops (src/oc_epipolar_search.cpp:184-188).  T
// threads then cost one launch per ~T POIs instead of T serialised launches.
//
// submit(req, serve): queue the request.  Whoever finds no leader becomes one: it takes everything that is queued as ONE
// batch, serves it, publishes the served requests' state, wakes sleeping owners and goes on with what has arrived meanwhile --
// back to back, so the GPU never waits for a thread to wake up.  Its own request sits in its first batch; after
// `extra_batches` further batches it promotes the owner of a queued request to leader and returns (no caller serves the
// others for ever).  Owners spin (a batch in flight is usually ~50 us from done: cheaper than a futex round trip per served
// thread), then poll politely -- yielding the core between looks, so that 60 waiting threads do not crowd out the leader and
// the HIP runtime's own threads --, then sleep.
//
// Invariants
//  1. Who may touch a request.  Its owner builds it and reads it again only after submit returns.  Between the push onto
//     `pending_` and the store that makes `state` non-zero it belongs to the leader that took it in a batch (a queued request
//     belongs to whoever holds `mu_`).  That store is the leader's LAST access: the owner may return at once and the request,
//     which lives in the owner's stack frame, is gone.  A leader never stores to its own request's state.
//  2. No wake-up is lost.  The leader stores `state`, fences, then reads `sleepers_`; an owner registers in `sleepers_`
//     (under `sleep_mu_`), fences, then re-reads `state`.  Both fences are seq_cst and therefore totally ordered.  Leader's
//     fence first: the owner's re-read sees the new state and it does not sleep.  Owner's fence first: the leader sees the
//     registration and takes `sleep_mu_` -- which the owner holds from before its registration until it is inside wait() --
//     before it notifies.  Release / acquire alone does not give this: the leader's load may pass its own store (a store
//     buffer does exactly that), both sides read the old value and the owner sleeps with nobody left to wake it.  One fence
//     per batch on the leader's side, one per sleep on the owner's.
//  3. The promoted request stays queued.  Promotion (state 2) hands over leadership, not a result: `leader_` stays true,
//     the request stays in `pending_` and its owner, as the new leader, serves it in its own first batch.  The fence of 2
//     covers this store as well: a promoted owner that sleeps through it would leave `leader_` set with nobody leading.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace ochip_host {

// Payload: what `serve` reads and writes per request (the engine: record, centre offset, status, error text).
template <class Payload>
class SingleCombiner {
public:
    struct Request : Payload {
        using Payload::Payload;

    private:
        friend class SingleCombiner;
        std::atomic<int> state{0};   // 0 = queued, 1 = served, 2 = promoted to leader while still queued
    };

    explicit SingleCombiner(int spins = 1500, std::chrono::microseconds yield_window = std::chrono::microseconds(400), int extra_batches = 32)
        : spins_(spins), yield_window_(yield_window), extra_batches_(extra_batches) {}

    // Returns once `req` has been served.  serve(std::vector<Request*>& batch) is called by one thread at a time.
    template <class Serve>
    void submit(Request& req, Serve&& serve) {
        bool lead;
        {
            std::lock_guard<std::mutex> lk(mu_);
            pending_.push_back(&req);
            lead = !leader_;
            if (lead) leader_ = true;
        }
        if (!lead) lead = wait_as_owner(req);
        if (!lead) return;
        std::vector<Request*> batch;
        bool own_done = false;
        for (int served = 0;; served++) {
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (pending_.empty()) {
                    leader_ = false;   // (its own request was queued before this thread became leader: it is done)
                    break;
                }
                if (own_done && served > extra_batches_) {
                    pending_.front()->state.store(2, std::memory_order_release);   // its owner takes over (invariant 3)
                    promotions_.fetch_add(1, std::memory_order_relaxed);
                    wake_sleepers();
                    break;
                }
                batch.clear();
                batch.swap(pending_);
            }
            serve(batch);
            for (Request* r : batch) {
                if (r == &req) own_done = true;
                else r->state.store(1, std::memory_order_release);
            }
            wake_sleepers();
        }
    }

    // owners that went to sleep / leaders that handed over, so far (tests, diagnostics)
    unsigned long long sleeps() const { return sleeps_.load(std::memory_order_relaxed); }
    unsigned long long promotions() const { return promotions_.load(std::memory_order_relaxed); }
    // no leader and nothing queued: what every quiescent combiner must show
    bool idle() {
        std::lock_guard<std::mutex> lk(mu_);
        return !leader_ && pending_.empty();
    }

private:
    // after the stores to `state` (invariant 2)
    void wake_sleepers() {
        std::atomic_thread_fence(std::memory_order_seq_cst);
        if (sleepers_.load(std::memory_order_relaxed) > 0) {
            std::lock_guard<std::mutex> ls(sleep_mu_);
            sleep_cv_.notify_all();
        }
    }

    // true: promoted while still queued, this thread leads now
    bool wait_as_owner(Request& req) {
        for (int spin = 0; spin < spins_ && req.state.load(std::memory_order_acquire) == 0; spin++) __builtin_ia32_pause();
        if (req.state.load(std::memory_order_acquire) == 0) {
            const auto t0 = std::chrono::steady_clock::now();
            while (req.state.load(std::memory_order_acquire) == 0 && std::chrono::steady_clock::now() - t0 < yield_window_)
                std::this_thread::yield();
        }
        if (req.state.load(std::memory_order_acquire) == 0) {
            std::unique_lock<std::mutex> ls(sleep_mu_);
            sleepers_.fetch_add(1, std::memory_order_relaxed);
            std::atomic_thread_fence(std::memory_order_seq_cst);
            if (req.state.load(std::memory_order_acquire) == 0) {
                sleeps_.fetch_add(1, std::memory_order_relaxed);
                sleep_cv_.wait(ls, [&] { return req.state.load(std::memory_order_acquire) != 0; });
            }
            sleepers_.fetch_sub(1, std::memory_order_relaxed);
        }
        return req.state.load(std::memory_order_acquire) == 2;
    }

    const int spins_;
    const std::chrono::microseconds yield_window_;
    const int extra_batches_;
    std::mutex mu_;                  // guards pending_ and leader_
    std::vector<Request*> pending_;
    bool leader_ = false;
    std::mutex sleep_mu_;            // sleepers: owners whose spin and yield budgets ran out
    std::condition_variable sleep_cv_;
    std::atomic<int> sleepers_{0};
    std::atomic<unsigned long long> sleeps_{0}, promotions_{0};
};

}  // namespace ochip_host
