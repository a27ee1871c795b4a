// Host-only driver of the counter shifts of ragged launches in same::ResetLedger (sameold_amd/csrc/same_resets.h), for
// tests/test_ragged_calls_cpu.py under ASan + UBSan.  A synthesised stream of launches (each giving every channel its own
// number of rows), per-channel resets between them and harvests (at most two launches in flight, harvested oldest first, at
// random moments, the way same_batch.cpp makes and collects them) is checked against a straightforward per-channel model:
// every channel knows the batch position where its own stream restarted and how many batch rows it has skipped since.
//   - an event of channel c at device sample t of launch L is queued as t - (the model's base of c when L was queued);
//   - same_batch_channel_input_sample_counter(c), i.e. batch counter - api_base[c], is the channel's own sample count.
// Prints "OK" on success; exits non-zero on the first mismatch.
#include "../../sameold_amd/csrc/same_resets.h"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <vector>

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

using same::ResetLedger;

struct Launch {
    int slot;
    uint64_t start, n;
    std::vector<uint32_t> got;          // rows each channel consumed
    std::vector<uint64_t> base;         // the model's base of each channel while the launch runs
};

static void fixed_cases()
{
    ResetLedger L;
    L.init(4);
    const uint32_t by[4] = {0, 5, 0, 100};
    L.shift(by, 1000, 0);                       // launch [0, 1000) in slot 0: channel 1 got 995 rows, channel 3 900
    CHECK(L.api_base[1] == 5 && L.api_base[3] == 100 && L.api_base[0] == 0);
    CHECK(L.rec_base[1] == 0 && L.rec_base[3] == 0);          // its own records keep the old base
    CHECK(L.pending_shift(0, 1) == 5 && L.pending_shift(0, 2) == 0 && L.pending_shift(0, 3) == 100);
    CHECK(L.rebase(3, 900) == 900);
    const ResetLedger::SlotShift &h = L.shift_due(0);
    CHECK(h.channels.size() == 2 && h.pos == 1000);
    L.done_shift(0);
    CHECK(L.rec_base[1] == 5 && L.rec_base[3] == 100);
    CHECK(L.rebase(3, 1500) == 1400);
    CHECK(L.pending_shift(0, 3) == 0);
    // a reset at the same position as a shift of the launch in flight: the reset wins
    std::vector<uint32_t> now;
    L.shift(by, 2000, 1);
    L.request({3}, 2000, 1, now);
    CHECK(now.empty() && L.api_base[3] == 2000);
    L.shift_due(1); L.done_shift(1);
    L.host_due(1); L.done_host(1);
    CHECK(L.rec_base[3] == 2000 && L.rec_base[1] == 10);
    L.clear();
    CHECK(L.api_base[1] == 0 && L.rec_base[1] == 0 && L.pending_shift(1, 1) == 0);
}

static void random_stream(uint32_t seed)
{
    std::mt19937_64 rng(seed);
    const uint32_t C = 1 + (uint32_t)(rng() % 40);
    ResetLedger L;
    L.init(C);
    std::vector<uint64_t> base(C, 0);            // model: batch position - own position, for the channel's next sample
    std::vector<uint64_t> own(C, 0);             // model: own samples since the last reset
    std::deque<Launch> flight;
    std::vector<uint32_t> now, by(C);
    uint64_t counter = 0, seq = 0;
    auto harvest_one = [&]() {
        Launch &l = flight.front();
        // the launch's records: every sample a channel consumed may carry an event
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t t = 0; t < l.got[c]; t += 1 + (uint32_t)(rng() % 7)) {
                const uint64_t dev = l.start + t + 1;
                CHECK(L.rebase(c, dev) == dev - l.base[c]);
            }
        L.shift_due(l.slot); L.done_shift(l.slot);
        L.host_due(l.slot); L.done_host(l.slot);
        flight.pop_front();
    };
    for (int step = 0; step < 400; ++step) {
        const int what = (int)(rng() % 10);
        if (what < 6) {
            // queue a launch: harvest its slot's previous launch first (same_batch.cpp's order)
            const int slot = (int)(seq & 1);
            while (flight.size() >= 2) harvest_one();
            if (!flight.empty() && flight.front().slot == slot) harvest_one();
            Launch l;
            l.slot = slot;
            l.start = counter;
            l.n = 1 + rng() % 5000;
            l.got.resize(C);
            l.base = base;
            const bool ragged = rng() % 4 != 0;
            for (uint32_t c = 0; c < C; ++c) {
                uint32_t g = (uint32_t)l.n;
                if (ragged) { const int r = (int)(rng() % 4); g = r == 0 ? 0u : (r == 1 ? (uint32_t)l.n : (uint32_t)(rng() % (l.n + 1))); }
                l.got[c] = g;
                by[c] = (uint32_t)l.n - g;
            }
            L.take_device(now);
            L.shift(by.data(), counter + l.n, slot);
            for (uint32_t c = 0; c < C; ++c) { base[c] += by[c]; own[c] += l.got[c]; }
            counter += l.n;
            ++seq;
            flight.push_back(std::move(l));
        } else if (what < 8) {
            // reset some channels at the current stream position
            std::vector<uint32_t> chans;
            for (uint32_t c = 0; c < C; ++c) if (rng() % 3 == 0) chans.push_back(c);
            const int newest = flight.empty() ? -1 : flight.back().slot;
            L.request(chans, counter, newest, now);
            if (newest < 0) CHECK(now == chans);
            for (uint32_t c : chans) { base[c] = counter; own[c] = 0; }
        } else if (!flight.empty()) {
            harvest_one();
        }
        for (uint32_t c = 0; c < C; ++c) CHECK(counter - L.api_base[c] == own[c]);
    }
    while (!flight.empty()) harvest_one();
    for (uint32_t c = 0; c < C; ++c) CHECK(L.rec_base[c] == L.api_base[c] && L.api_base[c] == base[c]);
}

// same::ragged_launch_split, the per-launch arithmetic of a ragged call as same_batch.cpp runs it: random calls (counts in
// [0, n_rows], their smallest m and largest M) are cut into launches the way the batch host cuts them -- rows [0, M) in pieces
// of at most `limit` rows, limits of 1 and limits beyond M among them, a fresh limit now and then within a call (the upload
// slab, the transpose slab and the launch length nest) -- and every launch's shifts go through the ledger.  The model walks the
// launch's rows one by one: a channel consumes call row r iff r < counts[c], every channel does iff r < m.
static void split_fixed_cases()
{
    const uint32_t counts[5] = {0, 7, 10, 11, 25};
    uint32_t by[5];
    CHECK(same::ragged_launch_split(counts, 5, 0, 0, 10, by) == 0);
    CHECK(by[0] == 10 && by[1] == 3 && by[2] == 0 && by[3] == 0 && by[4] == 0);
    CHECK(same::ragged_launch_split(counts, 5, 0, 10, 10, by) == 0);
    CHECK(by[0] == 10 && by[1] == 10 && by[2] == 10 && by[3] == 9 && by[4] == 0);
    CHECK(same::ragged_launch_split(counts, 5, 0, 20, 5, by) == 0);
    CHECK(by[0] == 5 && by[3] == 5 && by[4] == 0);
    const uint32_t k2[3] = {12, 30, 12};
    CHECK(same::ragged_launch_split(k2, 3, 12, 0, 10, by) == 10 && by[0] == 0 && by[1] == 0);     // a launch inside the prefix
    CHECK(same::ragged_launch_split(k2, 3, 12, 10, 10, by) == 2 && by[0] == 8 && by[1] == 0 && by[2] == 8);
    CHECK(same::ragged_launch_split(k2, 3, 12, 12, 10, by) == 0 && by[0] == 10);                  // m == row0
    CHECK(same::ragged_launch_split(k2, 3, 12, 20, 10, by) == 0 && by[0] == 10 && by[1] == 0);
    // beyond 2^31: nothing wraps
    const uint32_t big[2] = {0xfffffff0u, 0x80000001u};
    CHECK(same::ragged_launch_split(big, 2, 0x80000001u, 0x80000000u, 0x1000, by) == 1 && by[0] == 0 && by[1] == 0xfff);
}

static void random_calls(uint32_t seed)
{
    std::mt19937_64 rng(seed);
    const uint32_t C = 1 + (uint32_t)(rng() % 40);
    ResetLedger L;
    L.init(C);
    std::vector<uint64_t> base(C, 0), own(C, 0);
    std::deque<Launch> flight;
    std::vector<uint32_t> now, by(C), counts(C);
    std::vector<uint64_t> by_sum(C);
    uint64_t counter = 0, seq = 0;
    auto harvest_one = [&]() {
        Launch &l = flight.front();
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t t = 0; t < l.got[c]; t += 1 + (uint32_t)(rng() % 7)) {
                const uint64_t dev = l.start + t + 1;
                CHECK(L.rebase(c, dev) == dev - l.base[c]);
            }
        L.shift_due(l.slot); L.done_shift(l.slot);
        L.host_due(l.slot); L.done_host(l.slot);
        flight.pop_front();
    };
    for (int call = 0; call < 25; ++call) {
        const uint32_t n_rows = 1 + (uint32_t)(rng() % (call % 5 == 0 ? 20 : 800));
        uint32_t m = UINT32_MAX, M = 0;
        const int shape = (int)(rng() % 4);
        for (uint32_t c = 0; c < C; ++c) {
            const int r = (int)(rng() % 4);
            uint32_t k = r == 0 ? 0u : (r == 1 ? n_rows : (uint32_t)(rng() % (n_rows + 1)));
            if (shape == 1) k = n_rows / 2 + (uint32_t)(rng() % (n_rows - n_rows / 2 + 1));     // a common prefix
            if (shape == 2) k = std::min(n_rows, k + n_rows / 3);
            counts[c] = k;
            m = std::min(m, k); M = std::max(M, k);
        }
        if (m == M) continue;                                 // (a plain call of M rows: no ragged launch)
        std::fill(by_sum.begin(), by_sum.end(), 0);
        uint64_t lock_sum = 0;
        // the chunk limit: 1, tiny, about the call, beyond M
        auto draw_limit = [&]() -> size_t {
            switch ((int)(rng() % 5)) {
            case 0: return 1;
            case 1: return 1 + (size_t)(rng() % 17);
            case 2: return 1 + (size_t)(rng() % (M + 1));
            case 3: return (size_t)M + 1 + (size_t)(rng() % 1000);
            default: return 1 + (size_t)(rng() % (2 * (size_t)n_rows));
            }
        };
        size_t limit = draw_limit();
        if (limit == 1 && M > 400) limit = 1 + (size_t)(rng() % 3);     // (keeps the run short: limits of 1 on the short calls)
        for (size_t row0 = 0; row0 < M;) {
            const size_t n = std::min(limit, (size_t)M - row0);
            const int slot = (int)(seq & 1);
            while (flight.size() >= 2) harvest_one();
            if (!flight.empty() && flight.front().slot == slot) harvest_one();
            const size_t n_lock = same::ragged_launch_split(counts.data(), C, m, row0, n, by.data());
            Launch l;
            l.slot = slot; l.start = counter; l.n = n; l.got.resize(C); l.base = base;
            size_t lock_model = 0;
            for (size_t r = row0; r < row0 + n; ++r) lock_model += r < m;
            CHECK(n_lock == lock_model && n_lock <= n);
            for (uint32_t c = 0; c < C; ++c) {
                uint32_t got = 0;
                for (size_t r = row0; r < row0 + n; ++r) got += r < counts[c];
                CHECK(by[c] == n - got);
                CHECK(got >= n_lock);
                l.got[c] = got;
                by_sum[c] += by[c];
            }
            lock_sum += n_lock;
            L.take_device(now);
            L.shift(by.data(), counter + n, slot);
            for (uint32_t c = 0; c < C; ++c) { base[c] += by[c]; own[c] += l.got[c]; }
            counter += n;
            ++seq;
            flight.push_back(std::move(l));
            row0 += n;
            if (rng() % 3 == 0) harvest_one();
            if (rng() % 6 == 0) limit = draw_limit();
            for (uint32_t c = 0; c < C; ++c) CHECK(counter - L.api_base[c] == own[c]);
        }
        CHECK(lock_sum == m);
        for (uint32_t c = 0; c < C; ++c) CHECK(by_sum[c] == (uint64_t)M - counts[c]);
        if (rng() % 4 == 0) {
            std::vector<uint32_t> chans;
            for (uint32_t c = 0; c < C; ++c) if (rng() % 5 == 0) chans.push_back(c);
            L.request(chans, counter, flight.empty() ? -1 : flight.back().slot, now);
            for (uint32_t c : chans) { base[c] = counter; own[c] = 0; }
        }
    }
    while (!flight.empty()) harvest_one();
    for (uint32_t c = 0; c < C; ++c) CHECK(L.rec_base[c] == L.api_base[c] && L.api_base[c] == base[c]);
}

int main()
{
    fixed_cases();
    split_fixed_cases();
    for (uint32_t s = 1; s <= 300; ++s) random_stream(s);
    for (uint32_t s = 1; s <= 80; ++s) random_calls(1000 + s);
    std::printf("OK\n");
    return 0;
}
