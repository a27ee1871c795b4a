// Host-only driver of same::ResetLedger (sameold_amd/csrc/same_resets.h), the bookkeeping of same_batch_reset_channels,
// for tests/test_reset_channels_cpu.py under ASan + UBSan.  A synthesised stream of launches, harvests and per-channel resets
// (at most two launches in flight, harvested oldest first, the way same_batch.cpp makes and collects them) is checked against
// a plain model: an event of channel c at device sample t must be queued as t - (position of c's last reset at or before the
// start of t's launch), a launch must re-initialise exactly the channels reset since the launch before it, and the host half
// of a reset must come due when the harvest has replayed the launch in front of it -- never earlier, never later.
// Prints "OK" on success; exits non-zero on the first mismatch.
#include "../../sameold_amd/csrc/same_resets.h"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <set>
#include <vector>

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

using same::ResetLedger;

static void fixed_cases()
{
    ResetLedger L;
    L.init(8);
    std::vector<uint32_t> out{42}, now;
    const uint32_t bad[] = {1, 8};
    CHECK(!ResetLedger::normalise(bad, 2, 8, out));
    CHECK(out.size() == 1 && out[0] == 42);                      // untouched on error
    const uint32_t dup[] = {5, 1, 5, 3, 1};
    CHECK(ResetLedger::normalise(dup, 5, 8, out));
    CHECK((out == std::vector<uint32_t>{1, 3, 5}));
    CHECK(ResetLedger::normalise(nullptr, 0, 8, out) && out.empty());

    // a reset behind a launch still in flight (slot 0): nothing of the host half is due yet
    L.request({1, 3}, 100, 0, now);
    CHECK(now.empty());
    CHECK(L.api_base[1] == 100 && L.rec_base[1] == 0);
    CHECK(L.rebase(1, 150) == 150);                              // records of the launch before the reset keep their numbering
    L.request({3, 6}, 100, 0, now);                              // a second call at the same position merges
    std::vector<uint32_t> dev;
    L.take_device(dev);
    CHECK((dev == std::vector<uint32_t>{1, 3, 6}) && L.device.empty());
    const std::vector<uint32_t> due = L.host_due(0);
    CHECK((due == std::vector<uint32_t>{1, 3, 6}));
    L.done_host(0);
    CHECK(L.slot[0].channels.empty());
    CHECK(L.rebase(1, 150) == 50 && L.rebase(2, 150) == 150 && L.rebase(6, 100) == 0);
    // nothing in flight: the host half is due at once
    L.request({2}, 300, -1, now);
    CHECK((now == std::vector<uint32_t>{2}) && L.rec_base[2] == 300 && L.api_base[2] == 300);
    L.clear();
    for (uint32_t c = 0; c < 8; ++c) CHECK(L.api_base[c] == 0 && L.rec_base[c] == 0);
    CHECK(L.device.empty() && L.slot[0].channels.empty() && L.slot[1].channels.empty());
}

struct Launch { uint64_t a, b; int slot; };

static void random_stream(uint32_t seed)
{
    std::mt19937 rng(seed);
    const uint32_t C = 1 + rng() % 40;
    ResetLedger L;
    L.init(C);
    std::vector<std::vector<uint64_t>> resets(C, std::vector<uint64_t>{0});   // model: every channel's reset positions
    std::set<uint32_t> since_launch;                                           // model: channels reset since the last launch
    std::vector<uint64_t> host_reset_at(C, 0);                                 // when the host half last came due, per channel
    std::deque<Launch> flight;
    uint64_t counter = 0, seq = 0;
    std::vector<uint32_t> list, norm, now, dev;
    auto harvest_one = [&]() {
        const Launch l = flight.front();
        flight.pop_front();
        // the replay of this launch's records
        for (int k = 0; k < 20; ++k) {
            const uint32_t c = rng() % C;
            const uint64_t t = l.a + rng() % (l.b - l.a);
            uint64_t base = 0;
            for (uint64_t p : resets[c]) if (p <= l.a) base = p;
            CHECK(L.rebase(c, t) == t - base);
        }
        for (uint32_t c : L.host_due(l.slot)) {
            CHECK(L.rec_pos(l.slot) == l.b);                       // due exactly behind the launch before the position
            host_reset_at[c] = l.b;
        }
        L.done_host(l.slot);
    };
    for (int step = 0; step < 400; ++step) {
        const uint32_t op = rng() % 4;
        if (op <= 1) {
            // a process call: a launch into the slot of its sequence number (harvested first if still in flight), then the
            // launch before it is harvested while this one runs
            const int s = (int)(seq & 1);
            while (!flight.empty() && flight.front().slot == s) harvest_one();
            L.take_device(dev);
            CHECK((std::set<uint32_t>(dev.begin(), dev.end()) == since_launch) && dev.size() == since_launch.size());
            since_launch.clear();
            const uint64_t n = 1 + rng() % 5000;
            flight.push_back(Launch{counter, counter + n, s});
            ++seq;
            counter += n;
            if (flight.size() > 1) harvest_one();
        } else if (op == 2) {
            // same_batch_reset_channels with duplicates, sometimes out of range
            list.clear();
            const uint32_t k = rng() % 6;
            for (uint32_t i = 0; i < k; ++i) list.push_back(rng() % (C + (rng() % 8 == 0 ? 3 : 0)));
            bool ok = true;
            for (uint32_t c : list) ok &= c < C;
            CHECK(ResetLedger::normalise(list.data(), list.size(), C, norm) == ok);
            if (!ok) continue;
            const int newest = flight.empty() ? -1 : flight.back().slot;
            L.request(norm, counter, newest, now);
            for (uint32_t c : norm) { resets[c].push_back(counter); since_launch.insert(c); CHECK(L.api_base[c] == counter); }
            if (newest < 0) {
                CHECK(now == norm);
                for (uint32_t c : now) host_reset_at[c] = counter;
            } else {
                CHECK(now.empty());
            }
        } else {
            // same_batch_sync: everything in flight harvested
            while (!flight.empty()) harvest_one();
            for (uint32_t c = 0; c < C; ++c) CHECK(host_reset_at[c] == resets[c].back());
        }
    }
}

int main()
{
    fixed_cases();
    for (uint32_t seed = 1; seed <= 300; ++seed) random_stream(seed);
    std::printf("OK\n");
    return 0;
}
