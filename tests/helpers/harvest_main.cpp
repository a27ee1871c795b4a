// Host-only driver of the host half of a harvest (sameold_amd/csrc/same_harvest.h) for tests/test_harvest_cpu.py, under
// ASan + UBSan and, in a second build, under TSan.  Three modes:
//
//   harvest_main digest NAME RECORD THREADS REPS
//       replays a recorded launch (profiles/harvest/*.bin.xz, unpacked) REPS times on THREADS replay threads the way
//       same_debug_harvest_replay does, and prints one digest line per repetition: the number of queue records, of burst-index
//       entries and of re-arm channels, and an FNV-1a-64 over the records in queue order (kind, channel, sample_counter,
//       symbol_count, len, aux, aux2, n_bytes, then the payload bytes; not the payload's offset) and the re-arm list.
//       tests/golden/harvest_digest.txt holds these lines as the code printed them before it moved into this unit.
//   harvest_main eventlog
//       a fixed-seed sequence of appends, polls, peeks, drops and burst packs on same::EventLog against a plain
//       std::vector model that materialises every record when it is appended.
//   harvest_main audiolog
//       a handful of operations on same::AudioLog against the same kind of model.
//
// The last two print "OK" on success; every mode exits non-zero on the first mismatch.
#include "../../sameold_amd/csrc/same_capture_dev.h"
#include "../../sameold_amd/csrc/same_harvest.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

using same::AudioLog;
using same::EventLog;
using same::HarvestPart;
using same::QEvent;
using same::ResetLedger;
using same::WorkerPool;

// ---- digest ----------------------------------------------------------------------------------------------------------

static int run_digest(const char *name, const char *path, int threads, int reps)
{
    std::vector<double> ms((size_t)reps);
    const same::HarvestSeen each = [&](int rep, const same::Replay &rp, const EventLog &log, const std::vector<uint32_t> &rearm) {
        uint64_t fnv = 0xcbf29ce484222325ull;
        auto mix = [&](const void *p, size_t n) {
            const uint8_t *b = static_cast<const uint8_t *>(p);
            for (size_t i = 0; i < n; ++i) { fnv ^= b[i]; fnv *= 0x100000001b3ull; }
        };
        size_t n_idx = 0;
        for (const HarvestPart &p : rp.parts) n_idx += p.bursts.size();
        const QEvent *q = log.records();
        for (size_t i = 0; i < log.pending(); ++i) {
            mix(&q[i].kind, 4); mix(&q[i].channel, 4); mix(&q[i].sample_counter, 8); mix(&q[i].symbol_count, 8);
            mix(&q[i].len, 4); mix(&q[i].aux, 4); mix(&q[i].aux2, 4); mix(&q[i].n_bytes, 4);
            if (q[i].n_bytes) mix(log.payload_of(q[i]), q[i].n_bytes);
        }
        for (uint32_t c : rearm) mix(&c, 4);
        std::printf("%s rep %d: records %zu burst_index %zu rearm %zu fnv1a64 %016" PRIx64 "\n", name, rep, log.pending(), n_idx, rearm.size(), fnv);
        std::fflush(stdout);
    };
    const long n = same::replay_harvest_file(path, threads, reps, ms.data(), &each);
    if (n < 0) { std::fprintf(stderr, "replay failed (%ld): %s\n", n, same::last_error()); return 1; }
    return 0;
}

// ---- EventLog against a model ------------------------------------------------------------------------------------------

struct ModelEvent { same_rx_event ev; uint32_t n_bytes; bool burst; };

struct EventLogTest {
    EventLog log;
    WorkerPool pool;
    std::vector<ModelEvent> model;                 // what is pending, oldest first
    std::mt19937_64 rng{20261019u};
    uint64_t clock = 1;
    size_t n_moved_views = 0, n_views_read_after_drop = 0, n_parallel = 0;

    uint64_t pick(uint64_t n) { return rng() % n; }

    // one random record: its queue form (payload relative to `bytes`) and what a consumer must see of it
    ModelEvent make(QEvent &q, std::vector<uint8_t> &bytes)
    {
        ModelEvent m;
        std::memset(&m, 0, sizeof(m));
        static const uint32_t lens[] = {0u, 1u, SAME_EVENT_MAX_BYTES, SAME_EVENT_MAX_BYTES + 7u};
        const uint64_t what = pick(10);
        m.burst = what < 4;
        const bool header = what == 4;
        uint32_t len = 0;
        if (m.burst || header) len = pick(3) ? lens[pick(4)] : (uint32_t)pick(SAME_EVENT_MAX_BYTES + 1u);
        m.ev.kind = m.burst ? SAME_LINK_BURST : (header ? SAME_TRANSPORT_MSG_START : (uint32_t)pick(SAME_LINK_BURST));
        m.ev.channel = (uint32_t)pick(97); m.ev.sample_counter = clock += 1 + pick(1000); m.ev.symbol_count = clock / 42u;
        m.ev.len = len; m.ev.aux = (uint32_t)pick(300); m.ev.aux2 = (uint32_t)pick(8);
        m.n_bytes = len < SAME_EVENT_MAX_BYTES ? len : SAME_EVENT_MAX_BYTES;
        for (uint32_t i = 0; i < m.n_bytes; ++i) m.ev.bytes[i] = (uint8_t)rng();
        q = QEvent{};
        q.kind = m.ev.kind; q.channel = m.ev.channel; q.sample_counter = m.ev.sample_counter; q.symbol_count = m.ev.symbol_count;
        q.len = m.ev.len; q.aux = m.ev.aux; q.aux2 = m.ev.aux2; q.n_bytes = m.n_bytes;
        q.payload = bytes.size();
        bytes.insert(bytes.end(), m.ev.bytes, m.ev.bytes + m.n_bytes);
        return m;
    }
    // a harvest's slices, the way the replay threads leave them (some of them empty)
    void append_parts(size_t n_records)
    {
        std::vector<HarvestPart> parts(1 + pick(5));
        for (size_t i = 0, t = 0; i < n_records; ++i) {
            while (t + 1 < parts.size() && pick(n_records / parts.size() + 1) == 0) ++t;
            HarvestPart &p = parts[t];
            QEvent q;
            const ModelEvent m = make(q, p.bytes);
            if (m.burst) p.bursts.push_back((uint32_t)p.out.size());
            p.out.push_back(q);
            model.push_back(m);
        }
        CHECK(log.append_parts(pool, parts) == SAME_OK);
    }
    // a message log's records, written in place (none of them is a burst)
    void append_in_place(size_t n_records)
    {
        std::vector<QEvent> qs(n_records);
        std::vector<uint8_t> bytes;
        for (size_t i = 0; i < n_records; ++i) {
            const size_t mark = bytes.size();
            ModelEvent m = make(qs[i], bytes);
            while (m.burst) { bytes.resize(mark); m = make(qs[i], bytes); }
            model.push_back(m);
        }
        QEvent *dst = nullptr;
        uint8_t *bdst = nullptr;
        size_t byte0 = 0;
        CHECK(log.begin_append(n_records, bytes.size(), &dst, &bdst, &byte0) == SAME_OK);
        for (size_t i = 0; i < n_records; ++i) { dst[i] = qs[i]; dst[i].payload += byte0; }
        if (!bytes.empty()) std::memcpy(bdst, bytes.data(), bytes.size());
    }
    void check_view(const same_rx_event *view, size_t n, size_t model_from = 0)
    {
        CHECK(n == model.size() - model_from);
        CHECK((n == 0) == (view == nullptr));
        for (size_t i = 0; i < n; ++i) CHECK(std::memcmp(&view[i], &model[model_from + i].ev, sizeof(same_rx_event)) == 0);
    }
    void poll(size_t cap)
    {
        std::vector<same_rx_event> out(cap);         // (exactly `cap`: a record too many is a heap overflow)
        size_t n = 0, left = 0;
        CHECK(log.poll(pool, cap ? out.data() : nullptr, cap, &n, &left) == SAME_OK);
        CHECK(n == std::min(cap, model.size()) && left == model.size() - n);
        for (size_t i = 0; i < n; ++i) CHECK(std::memcmp(&out[i], &model[i].ev, sizeof(same_rx_event)) == 0);
        model.erase(model.begin(), model.begin() + (std::ptrdiff_t)n);
        CHECK(log.pending() == model.size());
        n_parallel += n >= 4096;
    }
    void drop(size_t n)
    {
        CHECK(log.drop(n) == SAME_OK);
        model.erase(model.begin(), model.begin() + (std::ptrdiff_t)n);
        CHECK(log.pending() == model.size());
    }
    void pack(size_t cap_kind)
    {
        std::vector<const ModelEvent *> bursts;
        for (const ModelEvent &m : model) if (m.burst) bursts.push_back(&m);
        const size_t cap = cap_kind == 0 ? 0 : (cap_kind == 1 ? bursts.size() / 2 : (cap_kind == 2 ? bursts.size() : bursts.size() + 5));
        const size_t n_copy = std::min(cap, bursts.size());
        std::vector<uint8_t> out(n_copy * SAME_BURST_RECORD_BYTES, 0xa5);
        const uint32_t first_channel = (uint32_t)pick(1000);
        size_t n = ~(size_t)0;
        CHECK(log.pack_bursts(pool, first_channel, n_copy ? out.data() : nullptr, cap, &n) == SAME_OK);
        CHECK(n == bursts.size());
        for (size_t i = 0; i < n_copy; ++i) {
            uint8_t want[SAME_BURST_RECORD_BYTES];
            std::memset(want, 0, sizeof(want));
            const uint32_t ch = bursts[i]->ev.channel + first_channel, len = bursts[i]->n_bytes;
            std::memcpy(want, &ch, 4); std::memcpy(want + 4, &bursts[i]->ev.sample_counter, 8); std::memcpy(want + 12, &len, 4);
            std::memcpy(want + 16, bursts[i]->ev.bytes, len);
            CHECK(std::memcmp(out.data() + i * SAME_BURST_RECORD_BYTES, want, sizeof(want)) == 0);
        }
    }
    void run()
    {
        const same_rx_event *view = nullptr;
        size_t n = 0;
        CHECK(log.peek(pool, &view, &n) == SAME_OK);
        check_view(view, n);                                              // an empty queue
        CHECK(log.drop(1) == SAME_EINVAL);
        for (int it = 0; it < 4000; ++it) {
            if (it % 1000 == 500) {
                // now and then past the 4 096 events / 8 192 bursts from which the copies run side by side
                append_parts(24000 + pick(500));
                pack(2);
                if (it == 1500) { CHECK(log.peek(pool, &view, &n) == SAME_OK); check_view(view, n); }
                poll(model.size());
            }
            switch (pick(9)) {
            case 0: case 1:
                append_parts(pick(70));
                break;
            case 2:
                append_in_place(pick(12));
                break;
            case 3: {
                const size_t p = model.size();
                const size_t caps[] = {p ? p - 1 : 0, p, p + 3, (size_t)pick(40), p / 2 + 1};
                poll(caps[pick(5)]);
                break;
            }
            case 4: {
                // peek twice in a row: the same view
                CHECK(log.peek(pool, &view, &n) == SAME_OK);
                check_view(view, n);
                const same_rx_event *again = nullptr;
                size_t n2 = 0;
                CHECK(log.peek(pool, &again, &n2) == SAME_OK);
                CHECK(again == view && n2 == n);
                check_view(again, n2);
                break;
            }
            case 5: {
                // peek, drop some, peek again: the view moves up
                CHECK(log.peek(pool, &view, &n) == SAME_OK);
                check_view(view, n);
                if (n < 2) break;
                drop(1 + pick(n - 1));
                check_view(view + (n - model.size()), model.size());       // (still readable across the drop)
                CHECK(log.peek(pool, &view, &n) == SAME_OK);
                check_view(view, n);
                ++n_moved_views;
                break;
            }
            case 6: {
                // peek, drop everything, read the view before the next call: the header's promise
                CHECK(log.peek(pool, &view, &n) == SAME_OK);
                check_view(view, n);
                if (!n) break;
                const std::vector<ModelEvent> before = model;
                drop(n);
                for (size_t i = 0; i < n; ++i) CHECK(std::memcmp(&view[i], &before[i].ev, sizeof(same_rx_event)) == 0);
                ++n_views_read_after_drop;
                break;
            }
            case 7:
                pack(pick(4));
                break;
            case 8:
                if (!model.empty()) drop(pick(model.size() + 1));
                else if (it % 7 == 0) { log.clear(); model.clear(); }
                break;
            }
            CHECK(log.pending() == model.size());
        }
        pack(2);
        poll(model.size() + 1);
        CHECK(log.pending() == 0);
        // the sequence has to have been where the queue and the burst index reclaim what was consumed
        CHECK(log.n_queue_reclaims >= 1);
        CHECK(log.n_index_trims >= 1);
        CHECK(n_moved_views >= 1 && n_views_read_after_drop >= 1 && n_parallel >= 1);
    }
};

// ---- AudioLog against a model ------------------------------------------------------------------------------------------

struct ModelChunk { uint32_t channel, flags; uint64_t counter; std::vector<float> samples; };

static void check_audio(AudioLog &A, const std::vector<ModelChunk> &model)
{
    const same_audio_chunk *v = nullptr;
    size_t n = 0;
    CHECK(A.peek(&v, &n) == SAME_OK);
    CHECK(n == model.size() && (n == 0) == (v == nullptr));
    for (size_t i = 0; i < n; ++i) {
        CHECK(v[i].channel == model[i].channel && v[i].flags == model[i].flags && v[i].sample_counter == model[i].counter);
        CHECK(v[i].n_samples == model[i].samples.size());
        for (size_t k = 0; k < v[i].n_samples; ++k) CHECK(v[i].samples[k] == model[i].samples[k]);
    }
}

static void run_audiolog()
{
    using same::cap::Span;
    AudioLog A;
    ResetLedger resets;
    resets.init(8);
    std::vector<ModelChunk> model;
    // capture is off: a reset ends nothing
    CHECK(A.end_reset({1, 2}, 100, resets) == SAME_OK);
    check_audio(A, model);
    A.open.assign(8, 0);
    std::vector<uint32_t> now;
    resets.request({5}, 1000, -1, now);                     // channel 5 counts from 1000
    std::vector<float> pool(64);
    for (size_t i = 0; i < pool.size(); ++i) pool[i] = (float)i + 0.5f;
    uint64_t n_reclaims_seen = 0;
    for (int round = 0; round < 6; ++round) {
        const uint64_t t0 = 2000 + 500 * (uint64_t)round;
        // spans as the lanes list them: out of channel order; one overruns the used part of the pool
        const size_t used = 40;
        const Span spans[] = {
            {5, SAME_AUDIO_FIRST, t0, 0, 0, 10},                               // opens channel 5
            {2, SAME_AUDIO_FIRST | SAME_AUDIO_END_MESSAGE, t0 + 3, 10, 3, 7},  // opens and closes channel 2
            {5, 0u, t0 + 10, 17, 10, 5},                                       // channel 5, second in emission order
            {3, SAME_AUDIO_FIRST, t0 + 1, 36, 1, 9},                           // 36 + 9 > used: truncated, no samples
            {7, SAME_AUDIO_FIRST, t0, 22, 0, 6},
        };
        size_t n_samples = 0;
        CHECK(A.append_spans(spans, 5, pool.data(), used, resets, &n_samples) == SAME_OK);
        CHECK(n_samples == 10 + 7 + 5 + 6);
        auto chunk = [&](const Span &s, uint32_t flags, bool keep) {
            ModelChunk m{s.channel, flags, resets.rebase(s.channel, s.counter), {}};
            if (keep) m.samples.assign(pool.begin() + (std::ptrdiff_t)s.off, pool.begin() + (std::ptrdiff_t)(s.off + s.n));
            model.push_back(m);
        };
        chunk(spans[1], spans[1].flags, true);
        chunk(spans[3], spans[3].flags | SAME_AUDIO_TRUNCATED, false);
        chunk(spans[0], spans[0].flags, true);
        chunk(spans[2], spans[2].flags, true);
        chunk(spans[4], spans[4].flags, true);
        CHECK(model[model.size() - 3].counter == t0 - 1000);                   // (channel 5 is rebased)
        CHECK(A.open[5] == 1 && A.open[2] == 0 && A.open[3] == 1 && A.open[7] == 1);
        check_audio(A, model);
        // a reset of an open, a closed and another open channel: END_RESET chunks for the open ones only
        CHECK(A.end_reset({2, 3, 5}, t0 + 100, resets) == SAME_OK);
        model.push_back(ModelChunk{3, SAME_AUDIO_END_RESET, t0 + 100, {}});
        model.push_back(ModelChunk{5, SAME_AUDIO_END_RESET, t0 + 100 - 1000, {}});
        CHECK(A.open[3] == 0 && A.open[5] == 0 && A.open[7] == 1);
        check_audio(A, model);
        CHECK(A.end_reset({2, 3, 5}, t0 + 101, resets) == SAME_OK);           // nothing open: nothing queued
        check_audio(A, model);
        // the consumer keeps a chunk with samples and the two behind it, or nothing; what it dropped is reclaimed by the next append
        CHECK(A.drop(model.size() + 1) == SAME_EINVAL);
        const size_t n_drop = round % 2 ? model.size() : model.size() - 3;
        CHECK(A.drop(n_drop) == SAME_OK);
        model.erase(model.begin(), model.begin() + (std::ptrdiff_t)n_drop);
        check_audio(A, model);
        n_reclaims_seen = A.n_reclaims;
    }
    CHECK(n_reclaims_seen >= 2);
    A.clear();
    model.clear();
    check_audio(A, model);
    CHECK(A.open[7] == 0);
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "digest" && argc == 6) return run_digest(argv[2], argv[3], std::atoi(argv[4]), std::atoi(argv[5]));
    if (mode == "eventlog") { EventLogTest t; t.run(); std::printf("OK\n"); return 0; }
    if (mode == "audiolog") { run_audiolog(); std::printf("OK\n"); return 0; }
    std::fprintf(stderr, "usage: harvest_main digest NAME RECORD THREADS REPS | eventlog | audiolog\n");
    return 2;
}
