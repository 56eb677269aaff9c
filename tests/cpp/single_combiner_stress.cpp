// The combining front end of compute(POI*) (opencorr_amd/csrc/host/single_combiner.h) on the CPU, with a fake `serve`:
//
//   single_combiner_stress <mode> <threads> <rounds>
//
//   free       every thread submits <rounds> requests as fast as it can; serve busy-waits a few microseconds (a launch);
//              the component's default spin / yield / extra-batch parameters
//   barrier    rounds: every thread submits ONE request, then all meet at a barrier -- so every round ends in a last batch
//              with nothing behind it, and an owner whose wake-up is lost sleeps for ever (no later batch's notify rescues
//              it).  Spin and yield budgets are 0: every owner that is not served at once takes the sleep path.
//   promote    `barrier` with the extra-batch limit at 2: leaders hand over often
//
// Exit status 0 only if every request was served exactly once with the value derived from its payload, the component ends
// with no leader and nothing pending, and the paths under test were actually taken: sleeps in barrier / promote, promotions
// in free / promote (a promotion needs four requests in flight: with fewer than 4 threads it is not demanded).  A lost
// wake-up shows as a hang: the caller sets the time limit.
#include "../../opencorr_amd/csrc/host/single_combiner.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

struct Job {
    unsigned long long in;
    unsigned long long out = 0;
    int served = 0;
    explicit Job(unsigned long long v) : in(v) {}
};
using Combiner = ochip_host::SingleCombiner<Job>;

static unsigned long long expected(unsigned long long in) { return in * 0x9E3779B97F4A7C15ull + 1; }

// sense-reversing barrier (C++17 has none); yields, so that more threads than cores still make progress
struct Barrier {
    const int n;
    std::atomic<int> waiting{0};
    std::atomic<unsigned> phase{0};
    explicit Barrier(int threads) : n(threads) {}
    void wait() {
        const unsigned p = phase.load(std::memory_order_acquire);
        if (waiting.fetch_add(1, std::memory_order_acq_rel) + 1 == n) {
            waiting.store(0, std::memory_order_relaxed);
            phase.store(p + 1, std::memory_order_release);
        } else {
            while (phase.load(std::memory_order_acquire) == p) std::this_thread::yield();
        }
    }
};

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: single_combiner_stress free|barrier|promote <threads> <rounds>\n");
        return 2;
    }
    const bool free_running = !strcmp(argv[1], "free"), promote = !strcmp(argv[1], "promote");
    if (!free_running && !promote && strcmp(argv[1], "barrier")) return 2;
    const int threads = atoi(argv[2]);
    const long rounds = atol(argv[3]);
    if (threads < 1 || rounds < 1) return 2;

    Combiner defaults, no_budget(0, std::chrono::microseconds(0), promote ? 2 : 32);
    Combiner& combiner = free_running ? defaults : no_budget;
    std::atomic<unsigned long long> batches{0}, served_total{0};
    auto serve = [&](std::vector<Combiner::Request*>& batch) {
        if (free_running) {
            const auto t0 = std::chrono::steady_clock::now();
            while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(3)) {
            }
        }
        for (Combiner::Request* r : batch) {
            r->out = expected(r->in);
            r->served++;
        }
        batches.fetch_add(1, std::memory_order_relaxed);
        served_total.fetch_add(batch.size(), std::memory_order_relaxed);
    };

    Barrier barrier(threads);
    std::atomic<unsigned long long> wrong{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            for (long i = 0; i < rounds; i++) {
                Combiner::Request req((unsigned long long)t * (unsigned long long)rounds + (unsigned long long)i);
                combiner.submit(req, serve);
                if (req.served != 1 || req.out != expected(req.in)) wrong.fetch_add(1, std::memory_order_relaxed);
                if (!free_running) barrier.wait();
            }
        });
    for (auto& th : pool) th.join();

    const unsigned long long requests = (unsigned long long)threads * (unsigned long long)rounds;
    printf("%s threads %d rounds %ld requests %llu served %llu batches %llu sleeps %llu promotions %llu wrong %llu idle %d\n", argv[1], threads,
           rounds, requests, served_total.load(), batches.load(), combiner.sleeps(), combiner.promotions(), wrong.load(), (int)combiner.idle());
    bool ok = wrong.load() == 0 && served_total.load() == requests && combiner.idle();
    if (!free_running && threads > 1 && combiner.sleeps() == 0) ok = false;
    if ((free_running || promote) && threads >= 4 && combiner.promotions() == 0) ok = false;
    if (!ok) fprintf(stderr, "single_combiner_stress: FAILED\n");
    return ok ? 0 : 1;
}
