// Host-only driver of the tone family's host unit (sameold_amd/csrc/same_tone_queue.h) for tests/test_tone_queue_cpu.py under
// ASan + UBSan: the chunk log in both instantiations -- the float capture's record and the delivery form's -- on plain memory
// that counts its allocations, and the event queue.  It emulates the library's three slots: a slot's "device pool" is a plain
// array, a call goes to slot (call index mod 3) and is harvested at once, and before that the slot is taken the way
// same_tones.hip takes it: the log fetches the block that still waits for the slot's samples, then the whole pool is overwritten
// with -1 and the new call's samples are written.  A read that comes after the reuse therefore shows -1 or the later call's
// samples.  The record buffers are laid out by tq::Layout with the channels' slot regions in a shuffled order and spare slots
// between them, a call's samples are placed from the pool's used end downwards, and every word the mode must not read (the
// other header word, a span's own n and off in delivery mode) holds a value that would show.
//
//     tone_queue_main audio|delivery SEED
//         stdout, phase "script" (seeded operations, then stated ones) and phase "freelist" (a fresh log):
//         "call INDEX SLOT fetches F" (F: fetch requests of the reuse), its inputs in the buffers' order "ev CHANNEL KIND EDGE
//         COUNTER DURATION" and "in CHANNEL I FLAGS KIND RATE COUNTER OUT_INDEX N TONE_START : SAMPLES" (I: the chunk's index in its
//         channel); "peek FAIL_AT rc RC n N fetches F" (FAIL_AT: which fetch request of this peek fails, 0: none) and the view
//         "out CHANNEL FLAGS KIND RATE COUNTER OUT_INDEX N TONE_START null|ptr : SAMPLES" read through the `samples` pointers;
//         "review N" and the last view read again, behind three further calls; "drop K rc RC"; "poll CAP n N left L" and
//         "pev CHANNEL KIND EDGE COUNTER DURATION"; "stat allocs A free F"; "OK".  (RATE and OUT_INDEX of the float record: its
//         reserved word, and 0.)
#include "../../sameold_amd/csrc/same_tone_queue.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace tn = same::tn;
namespace td = same::td;
namespace tq = same::tq;

constexpr uint32_t kChannels = 5;
constexpr size_t kPool = 64;                                 // samples of a slot's pool: 5 channels x 3 chunks x 4 samples fit
constexpr uint32_t kOutRate = 4000;

// plain memory that counts its allocations
template <typename S>
struct Block {
    static int allocs;
    S *p = nullptr;
    size_t n = 0;
    Block() = default;
    Block(const Block &) = delete;
    Block &operator=(const Block &) = delete;
    Block(Block &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    Block &operator=(Block &&o) noexcept
    {
        if (this != &o) { delete[] p; p = std::exchange(o.p, nullptr); n = std::exchange(o.n, 0); }
        return *this;
    }
    ~Block() { delete[] p; }
    S *get() const { return p; }
    size_t size() const { return n; }
    void ensure(size_t k)
    {
        if (k <= n) return;
        delete[] p;
        p = new S[k];
        n = k;
        ++allocs;
    }
};
template <typename S> int Block<S>::allocs = 0;

static void print_record(const char *tag, const same_tone_audio_chunk &c)
{
    std::printf("%s %u %u %u %u %llu 0 %llu %llu", tag, c.channel, c.flags, c.kind, c.reserved, (unsigned long long)c.sample_counter,
                (unsigned long long)c.n_samples, (unsigned long long)c.tone_start);
}
static void print_record(const char *tag, const same_tone_delivery_chunk &c)
{
    std::printf("%s %u %u %u %u %llu %llu %llu %llu", tag, c.channel, c.flags, c.kind, c.rate, (unsigned long long)c.sample_counter,
                (unsigned long long)c.out_index, (unsigned long long)c.n_samples, (unsigned long long)c.tone_start);
}
static void print_event(const char *tag, const same_tone_event &e)
{
    std::printf("%s %u %u %u %llu %llu\n", tag, e.channel, e.kind, e.edge, (unsigned long long)e.sample_counter, (unsigned long long)e.duration);
}

template <typename Chunk, typename S>
struct Driver {
    static constexpr bool kDelivery = std::is_same<Chunk, same_tone_delivery_chunk>::value;
    tq::ChunkLog<Chunk, S, Block<S>> log{kDelivery ? (size_t)tq::kSlots + 1 : 0};
    tq::EventQueue events;
    std::vector<S> pool[tq::kSlots];
    std::mt19937 rng;
    uint32_t calls = 0;
    int requests = 0, fail_at = 0;                           // this operation's fetch requests; the fail_at-th fails
    const Chunk *view = nullptr;
    size_t n_view = 0;                                       // the last peek's view, and how much of it has not been dropped
    bool view_ok = true;

    explicit Driver(uint32_t seed) : rng(seed) { Block<S>::allocs = 0; }

    int fetch(int slot, uint64_t used, Block<S> &mem)
    {
        if (++requests == fail_at) return SAME_EHIP;
        CHECK(used > 0 && used <= kPool);
        mem.ensure((size_t)used);
        std::memcpy(mem.get(), pool[slot].data(), (size_t)used * sizeof(S));
        return SAME_OK;
    }

    // one call: channel c has sizes[c].size() chunks of these sample counts
    void call(const std::vector<std::vector<uint32_t>> &sizes)
    {
        const int slot = (int)(calls % tq::kSlots);
        requests = 0;
        fail_at = 0;
        CHECK(log.fetch_slot(slot, [this](int s, uint64_t used, Block<S> &mem) { return fetch(s, used, mem); }) == SAME_OK);
        std::printf("call %u %d fetches %d\n", calls, slot, requests);
        pool[slot].assign(kPool, (S)-1);
        // the channels' regions of event slots and chunk slots: in a shuffled order, some with a spare slot behind them
        uint32_t order[kChannels];
        for (uint32_t c = 0; c < kChannels; ++c) order[c] = c;
        for (uint32_t c = kChannels - 1; c > 0; --c) std::swap(order[c], order[rng() % (c + 1)]);
        std::vector<tn::Desc> desc(kChannels, tn::Desc{});
        std::vector<uint32_t> span_off(kChannels), n_ev(kChannels);
        uint64_t ev_slots = 0, chunk_slots = 0, used = 0;
        for (uint32_t k = 0; k < kChannels; ++k) {
            const uint32_t c = order[k];
            n_ev[c] = rng() % 3;
            desc[c].ev_off = (uint32_t)ev_slots;
            ev_slots += n_ev[c] + rng() % 2;
            span_off[c] = (uint32_t)chunk_slots;
            chunk_slots += sizes[c].size() + rng() % 2;
            for (uint32_t n : sizes[c]) used += n;
        }
        CHECK(used <= kPool);
        tq::Layout at;
        CHECK(at.set_events(kChannels, ev_slots) == SAME_OK && at.set_capture(kChannels, chunk_slots, kDelivery) == SAME_OK);
        std::vector<uint8_t> out((size_t)at.out_bytes, 0xee), cap_out((size_t)at.cap_bytes, 0xee);
        const uint64_t header[4] = {12345, kDelivery ? 4242 : used, kDelivery ? used : 4242, 777};
        std::memcpy(cap_out.data(), header, sizeof(header));
        uint64_t cursor = used;
        for (uint32_t k = 0; k < kChannels; ++k) {
            const uint32_t c = order[k], n_chunks = (uint32_t)sizes[c].size();
            std::memcpy(out.data() + (size_t)c * 4, &n_ev[c], 4);
            std::memcpy(cap_out.data() + same::kCapHeaderBytes + (size_t)c * 4, &n_chunks, 4);
            for (uint32_t i = 0; i < n_ev[c]; ++i) {
                const same_tone_event e{c, 1 + (calls + i) % 2, 1 + i % 2, 0, (uint64_t)calls * 1000 + c * 10 + i, (uint64_t)(rng() % 50)};
                std::memcpy(out.data() + at.events_at + ((size_t)desc[c].ev_off + i) * sizeof(e), &e, sizeof(e));
                print_event("ev", e);
            }
            for (uint32_t i = 0; i < n_chunks; ++i) {
                const uint64_t n = sizes[c][i];
                cursor -= n;
                Chunk ch{};
                ch.channel = c;
                ch.flags = rng() % 16;
                ch.kind = 1 + rng() % 2;
                ch.sample_counter = (uint64_t)calls * 100000 + c * 1000 + i;
                ch.n_samples = n;
                ch.tone_start = rng() % 100000;
                tn::Span sp{c, ch.flags, ch.kind, 3, ch.sample_counter, n, ch.tone_start, cursor};
                if constexpr (kDelivery) {
                    ch.rate = kOutRate;
                    ch.out_index = rng() % 100000;
                    sp.n = 9000 + n;                         // (the placed rows and their place in the staging pool: not the log's business)
                    sp.off = 7000;
                    const td::Out o{5, ch.out_index, n, cursor};
                    std::memcpy(cap_out.data() + at.outs_at + ((size_t)span_off[c] + i) * sizeof(o), &o, sizeof(o));
                }
                std::memcpy(cap_out.data() + at.spans_at + ((size_t)span_off[c] + i) * sizeof(sp), &sp, sizeof(sp));
                std::printf("in %u %u %u %u %u %llu %llu %llu %llu :", c, i, ch.flags, ch.kind, kDelivery ? kOutRate : 0u, (unsigned long long)ch.sample_counter,
                            (unsigned long long)out_index_of(ch), (unsigned long long)n, (unsigned long long)ch.tone_start);
                for (uint64_t j = 0; j < n; ++j) {
                    const S v = (S)((calls * 131 + (cursor + j) * 7 + 1) % 30000);
                    pool[slot][(size_t)(cursor + j)] = v;
                    std::printf(" %ld", (long)v);
                }
                std::printf("\n");
            }
        }
        CHECK(cursor == 0);
        const tq::Records r{kChannels, desc.data(), span_off.data(), out.data(), cap_out.data(), kOutRate};
        events.harvest(at, r);
        log.harvest(at, r, slot);
        ++calls;
    }
    static uint64_t out_index_of(const same_tone_audio_chunk &) { return 0; }
    static uint64_t out_index_of(const same_tone_delivery_chunk &c) { return c.out_index; }

    std::vector<std::vector<uint32_t>> random_sizes()
    {
        std::vector<std::vector<uint32_t>> sizes(kChannels);
        const uint32_t shape = rng() % 8;                    // 0: no chunk at all; 1: chunks, all of them empty
        for (uint32_t c = 0; c < kChannels && shape; ++c)
            for (uint32_t i = rng() % 4; i > 0; --i) sizes[c].push_back(shape == 1 || rng() % 4 == 0 ? 0 : 1 + rng() % 4);
        return sizes;
    }
    void call_even(uint32_t chunks, uint32_t n) { call(std::vector<std::vector<uint32_t>>(kChannels, std::vector<uint32_t>(chunks, n))); }

    void print_view(const Chunk *v, size_t n) const
    {
        for (size_t i = 0; i < n; ++i) {
            print_record("out", v[i]);
            std::printf(" %s :", v[i].samples ? "ptr" : "null");
            for (uint64_t j = 0; j < v[i].n_samples; ++j) std::printf(" %ld", (long)v[i].samples[j]);
            std::printf("\n");
        }
    }
    void peek(int fail)
    {
        requests = 0;
        fail_at = fail;
        const Chunk *v = nullptr;
        size_t n = 0;
        const int rc = log.publish([this](int s, uint64_t used, Block<S> &mem) { return fetch(s, used, mem); }, &v, &n);
        std::printf("peek %d rc %d n %zu fetches %d\n", fail, rc, n, requests);
        CHECK(rc == SAME_OK || (n == 0 && v == nullptr));
        print_view(v, n);
        view = v;
        n_view = n;
        view_ok = rc == SAME_OK;
    }
    // the view of the peek just made, read again behind three further calls
    void review()
    {
        for (int i = 0; i < 3; ++i) call(random_sizes());
        std::printf("review %zu\n", n_view);
        print_view(view, n_view);
    }
    void drop(size_t k)
    {
        const int rc = log.drop(k);
        std::printf("drop %zu rc %d\n", k, rc);
        if (rc == SAME_OK) { view += k; n_view -= k; }
    }
    void poll(size_t cap)
    {
        std::vector<same_tone_event> got(cap);
        size_t left = 0;
        const size_t n = events.take(got.data(), cap, &left);
        std::printf("poll %zu n %zu left %zu\n", cap, n, left);
        for (size_t i = 0; i < n; ++i) print_event("pev", got[i]);
    }
    void stat() const { std::printf("stat allocs %d free %zu\n", Block<S>::allocs, log.n_free()); }

    void script()
    {
        std::printf("phase script\n");
        for (int step = 0; step < 150; ++step) {
            const uint32_t op = rng() % 12;
            if (op < 5) call(random_sizes());
            else if (op < 7) peek(0);
            else if (op == 7) { if (view_ok) drop(rng() % (n_view + 1)); }
            else if (op == 8) { if (view_ok) drop(n_view + 1); }
            else if (op == 9) peek(1 + (int)(rng() % 3));
            else if (op == 10) { peek(0); review(); }
            else poll(rng() % 6);
        }
        // stated: four calls nobody peeks between; a drop that ends on a block's boundary, a call behind it, a drop that ends inside a block
        peek(0);
        drop(n_view);
        call_even(2, 0);                                     // (only empty chunks: its slot is free for the third call behind it)
        for (int i = 0; i < 4; ++i) call_even(2, 3);
        peek(0);
        drop(2 * kChannels);
        call_even(1, 1);
        peek(0);
        drop(3);
        peek(0);
        drop(n_view + 1);
        drop(n_view);
        // stated: a fetch that fails at the second of three unpublished blocks
        for (int i = 0; i < 3; ++i) call_even(1, 2 + i);
        peek(2);
        peek(0);
        drop(n_view);
        poll(3);
        call(random_sizes());
        poll(1000);
        stat();
    }
    void freelist()
    {
        std::printf("phase freelist\n");
        for (int i = 0; i < 8; ++i) {
            call_even(2, 4);
            peek(0);
            drop(n_view);
            stat();
        }
        // six calls published and none dropped, then all of them at once
        for (int i = 0; i < 3; ++i) { call_even(1, 3 + i); peek(0); }
        for (int i = 0; i < 3; ++i) call_even(3, 1 + i);
        peek(0);
        stat();
        drop(n_view);
        stat();
    }
};

int main(int argc, char **argv)
{
    CHECK(argc == 3);
    const std::string kind = argv[1];
    const uint32_t seed = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    CHECK(kind == "audio" || kind == "delivery");
    if (kind == "audio") {
        { Driver<same_tone_audio_chunk, float> d(seed); d.script(); }
        { Driver<same_tone_audio_chunk, float> d(seed + 1); d.freelist(); }
    } else {
        { Driver<same_tone_delivery_chunk, int16_t> d(seed); d.script(); }
        { Driver<same_tone_delivery_chunk, int16_t> d(seed + 1); d.freelist(); }
    }
    std::printf("OK\n");
    return 0;
}
