// opencorr_amd/csrc/host/chunk_pipeline.h on the CPU: the chunk schedule of the host-queue pipeline pinned to the values the
// inline expressions of capi_host.hip gave before they moved, its invariants over a sweep, and the feeder / copy-out
// hand-off driven by two threads (the caller builds this with a thread sanitizer).  Prints one line per check; exit status 0
// only if all pass.
#include "../../opencorr_amd/csrc/host/chunk_pipeline.h"

#include <atomic>
#include <cstdio>
#include <thread>

using Sched = std::vector<std::pair<size_t, size_t>>;
using ochip_host::chunk_schedule;

static int failures = 0;

static void check(bool ok, const char* what) {
    printf("%-60s %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) failures++;
}

static Sched from_lengths(std::initializer_list<size_t> lengths) {
    Sched s;
    size_t at = 0;
    for (size_t n : lengths) {
        s.emplace_back(at, n);
        at += n;
    }
    return s;
}

static bool well_formed(const Sched& s, size_t count) {
    size_t at = 0;
    for (const auto& c : s) {
        if (c.first != at || c.second == 0) return false;
        at += c.second;
    }
    return !s.empty() && at == count;
}

// the consumer's loop of capi_host.hip: take chunks in order until the feeder fails; returns how many it took
static size_t drain(ochip_host::ChunkHandoff& h, size_t nchunk, std::atomic<size_t>& taken) {
    size_t c = 0;
    for (; c < nchunk; c++) {
        if (!h.wait_for(c)) break;
        taken.store(c + 1, std::memory_order_release);
    }
    return c;
}

int main() {
    const int unit = 65536;
    check(chunk_schedule(250000, unit, false) == Sched{{0, 32768}, {32768, 184464}, {217232, 32768}}, "250000 / 65536: edge, middle, edge");
    check(chunk_schedule(131071, unit, false) == Sched{{0, 131071}}, "131071 / 65536: one piece");
    check(chunk_schedule(131072, unit, false) == from_lengths({32768, 65536, 32768}), "131072 / 65536: 32768, 65536, 32768");
    check(chunk_schedule(1000000, unit, false) == from_lengths({32768, 186893, 186893, 186893, 186893, 186892, 32768}),
          "1000000 / 65536: edges of 32768 around 4 x 186893 + 186892");
    check(chunk_schedule(250000, unit, true) == from_lengths({31250, 31250, 31250, 31250, 31250, 31250, 31250, 31250}),
          "250000 / 65536, transfer bound: 8 x 31250");
    check(chunk_schedule(100001, unit, true) == from_lengths({25001, 25000, 25000, 25000}), "100001 / 65536, transfer bound: 25001 + 3 x 25000");
    check(chunk_schedule(65535, unit, true) == Sched{{0, 65535}}, "65535 / 65536, transfer bound: one piece");
    bool whole = true, formed = true;
    const size_t counts[] = {1, 2, 3, 63, 64, 16383, 16384, 32767, 32768, 32769, 65535, 65536, 65537, 98304, 131071, 131072, 131073,
                             196608, 250000, 262143, 262144, 999999, 1000000, 1048577, 5000001};
    const int units[] = {0, 16384, 16385, 65536, 100000, 1 << 20};
    for (int tb = 0; tb < 2; tb++) {
        for (size_t count : counts) {
            whole = whole && chunk_schedule(count, 0, tb != 0) == Sched{{0, count}};
            for (int u : units) formed = formed && well_formed(chunk_schedule(count, u, tb != 0), count);
        }
        // every branch and rounding case at sizes where the pieces are a few POIs
        for (size_t count = 1; count <= 200; count++)
            for (int u = 0; u <= 12; u++) formed = formed && well_formed(chunk_schedule(count, u, tb != 0), count);
    }
    check(whole, "host_chunk 0: one piece, any count");
    check(formed, "sweep: contiguous from 0, positive lengths, sum = count");

    ochip_host::ChunkHandoff h;
    {   // success: the feeder hands over 1 ... n, the consumer takes all n
        const size_t n = 5000;
        std::atomic<size_t> taken{0};
        size_t got = 0;
        h.reset();
        std::thread consumer([&] { got = drain(h, n, taken); });
        for (size_t c = 0; c < n; c++) h.hand_over(c + 1);
        consumer.join();
        check(got == n, "hand-off: every chunk handed over is taken");
    }
    {   // failure once the consumer has taken k chunks: it takes exactly k and stops
        const size_t n = 64, k = 23;
        std::atomic<size_t> taken{0};
        size_t got = 0;
        h.reset();
        std::thread consumer([&] { got = drain(h, n, taken); });
        for (size_t c = 0; c < k; c++) h.hand_over(c + 1);
        while (taken.load(std::memory_order_acquire) < k) std::this_thread::yield();
        h.fail();
        consumer.join();
        check(got == k && !h.wait_for(0) && !h.wait_for(n), "hand-off: fail() after k chunks: the consumer takes k and stops");
    }
    {   // failure at any moment: the consumer stops, with no more than was handed over; reset() makes the object usable again
        bool ok = true;
        for (int rep = 0; rep < 400 && ok; rep++) {
            const size_t n = 16, k = (size_t)rep % 16;
            std::atomic<size_t> taken{0};
            size_t got = 0;
            h.reset();
            std::thread consumer([&] { got = drain(h, n, taken); });
            for (size_t c = 0; c < k; c++) h.hand_over(c + 1);
            h.fail();
            consumer.join();
            ok = got <= k;
        }
        check(ok, "hand-off: fail() at any moment stops the consumer");
    }
    return failures ? 1 : 0;
}
