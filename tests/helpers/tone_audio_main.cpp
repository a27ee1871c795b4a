// Host-only driver of tone-alert audio's plan (sameold_amd/csrc/same_tone_audio_plan.h, same_tones_plan.h) and device core
// (same_tone_audio_dev.h, same_tones_dev.h), for tests/test_tone_audio_cpu.py under ASan + UBSan.  It runs calls the way
// same_tones.hip and same_tone_audio.hip do -- describe, the chunk slots, every (channel, block) item, run_capture per channel
// over the call's qualify bits, an exclusive prefix over the channels' captured counts, span_place, a plain C++ copy out of the
// call's buffer into the call's pool -- on buffers of exactly the size the library provides: the input with NaN (f32) or 32767
// (int16) behind every channel's count, the two record buffers of exactly the layout's bytes (same_tone_queue.h), a pool of
// exactly samples_per_call floats.  Behind a call comes the library's own harvest: the unit's event queue and chunk log take the
// call's records, the log fetches the pool's used part with a memcpy, and what is printed is what the queue and the published
// view hold.  Layouts alternate from call to call.
//
//     tone_audio_main streams IN_FILE f32|i16 RATE CHANNELS CUT KINDS TAIL_BLOCKS MAX_BLOCKS POOL RESET_CHANNEL RESET_AFTER OUT_FILE
//         IN_FILE: [CHANNELS x samples] channel-major, little-endian f32 or int16.  CUT: "fixed" -- plain calls of 1, 319, 320,
//         321, 1000 rows and the rest -- or a seed: random ragged calls.  RESET_CHANNEL (-1: none) is reset between two calls
//         once it has consumed RESET_AFTER samples.
//         stdout: "reset CHANNEL POSITION", "call INDEX K_0 .. K_C-1" (the counts), "event CALL CHANNEL KIND EDGE COUNTER
//         DURATION", "chunk CALL CHANNEL FLAGS KIND COUNTER N_SAMPLES TONE_START AT" in queue order (AT: the first sample's
//         index in OUT_FILE, f32), "OK".
//     tone_audio_main bound
//         stdout: "bound N CHUNKS LIMIT" for N = 0 .. 200: the chunks of a channel that completes N blocks on the adversarial
//         pattern of same_tone_audio_dev.h, and chunk_bound(N); "OK".
#include "../../sameold_amd/csrc/same_tone_audio_plan.h"
#include "../../sameold_amd/csrc/same_tone_queue.h"
#include "../../sameold_amd/csrc/same_tones_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace tn = same::tn;
namespace tq = same::tq;
using same::ToneAudioPlan;
using same::TonesPlan;

static float blank(float) { return std::numeric_limits<float>::quiet_NaN(); }
static int16_t blank(int16_t) { return 0x7fff; }

template <typename T>
static std::vector<T> read_file(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    CHECK(f != nullptr);
    CHECK(std::fseek(f, 0, SEEK_END) == 0);
    const long bytes = std::ftell(f);
    CHECK(bytes >= 0 && bytes % (long)sizeof(T) == 0);
    CHECK(std::fseek(f, 0, SEEK_SET) == 0);
    std::vector<T> v((size_t)bytes / sizeof(T));
    CHECK(std::fread(v.data(), sizeof(T), v.size(), f) == v.size());
    CHECK(std::fclose(f) == 0);
    return v;
}

// A handle with capture on: the plans and the device's memory
struct Runner {
    TonesPlan plan;
    ToneAudioPlan audio;
    std::vector<float> acc;
    std::vector<tn::Sm> sm;
    std::vector<tn::Cap> cap;
    tq::EventQueue events;
    tq::ChunkLog<same_tone_audio_chunk, float, std::vector<float>> log{0};
    std::vector<float> captured;                         // every queued chunk's samples, in queue order
    uint32_t calls = 0;

    Runner(uint32_t C, uint32_t rate, uint32_t kinds, uint32_t tail, uint32_t maxb, uint64_t pool)
    {
        CHECK(plan.init(C, rate) == SAME_OK);
        CHECK(audio.set(0, tail, maxb, pool) == SAME_EINVAL && audio.set(4, tail, maxb, pool) == SAME_EINVAL);
        CHECK(audio.set(kinds, tail, 0, pool) == SAME_EINVAL && !audio.on());
        CHECK(audio.set(kinds, tail, maxb, pool) == SAME_OK && audio.on());
        // (garbage: the first call that runs makes the state machines and the capture state idle)
        acc.assign((size_t)2 * tn::kAccWords * C, std::numeric_limits<float>::quiet_NaN());
        tn::Sm junk;
        std::memset(&junk, 0x5a, sizeof(junk));
        sm.assign((size_t)2 * C, junk);
        tn::Cap cjunk;
        std::memset(&cjunk, 0x5a, sizeof(cjunk));
        cap.assign(C, cjunk);
    }

    template <typename SampleT>
    void call(const SampleT *x, size_t n_rows, const uint32_t *counts, int layout)
    {
        const uint32_t C = plan.n_channels(), N = plan.coef.N;
        std::vector<tn::Desc> desc(C);
        const TonesPlan::Shape shape = plan.describe(counts, n_rows, desc.data());
        if (!shape.any_samples) return;
        std::vector<uint32_t> span_off(C);
        const uint64_t slots = ToneAudioPlan::describe(desc.data(), C, span_off.data());
        std::printf("call %u", calls);
        for (uint32_t c = 0; c < C; ++c) std::printf(" %u", desc[c].count);
        std::printf("\n");
        std::vector<uint8_t> qual((size_t)(shape.max_complete ? shape.max_complete : 1) * C, 0xff);
        // the call's two record buffers, as the device writes them
        tq::Layout at;
        CHECK(at.set_events(C, shape.event_slots) == SAME_OK && at.set_capture(C, slots, false) == SAME_OK);
        std::vector<uint8_t> out((size_t)at.out_bytes, 0xee), cap_out((size_t)at.cap_bytes, 0xee);
        same_tone_event *ev = (same_tone_event *)(out.data() + at.events_at);
        tn::Span *spans = (tn::Span *)(cap_out.data() + at.spans_at);
        const size_t bank_words = (size_t)tn::kAccWords * C;
        for (uint32_t c = 0; c < C; ++c) {
            const tn::Desc &d = desc[c];
            const float *bank_in = acc.data() + ((d.flags & tn::kDescBank) ? bank_words : 0);
            float *bank_out = acc.data() + ((d.flags & tn::kDescBank) ? 0 : bank_words);
            for (uint32_t j = d.n_touch; j-- > 0;) {
                uint32_t r0, r1;
                tn::block_rows(d, N, j, r0, r1);
                tn::Acc a = tn::block_continues(d, j) ? tn::acc_load(bank_in, C, c) : tn::acc_zero();
                if (layout == SAME_LAYOUT_TIME_MAJOR) tn::run_rows(a, plan.coef, x + c, C, r0, r1);
                else tn::run_rows(a, plan.coef, x + (size_t)c * n_rows, 1, r0, r1);
                tn::block_end(d, plan.coef, j, a, c, C, nullptr, qual.data(), bank_out);
            }
        }
        // the state-machine kernel: lane = channel
        std::vector<uint32_t> n_ev(C, 0), n_spans(C, 0);
        std::vector<uint64_t> count(C, 0);
        for (uint32_t c = 0; c < C; ++c) {
            // (spans + offset, not &spans[offset]: a channel with no slot may sit at the end)
            count[c] = tn::run_capture(desc[c], N, c, C, qual.data(), &sm[2 * (size_t)c], cap[c], audio.params, ev, &n_ev[c],
                                       spans + span_off[c], &n_spans[c]);
            CHECK(n_ev[c] <= tn::events_bound(desc[c].n_complete) && n_spans[c] <= tn::chunk_bound(desc[c].n_complete));
            uint64_t sum = 0;
            for (uint32_t i = 0; i < n_spans[c]; ++i) {
                const tn::Span &s = spans[span_off[c] + i];
                CHECK(s.channel == c && s.n > 0 && s.off == sum && (uint64_t)s.row0 + s.n <= desc[c].count);
                CHECK(i == 0 || s.row0 >= spans[span_off[c] + i - 1].row0 + spans[span_off[c] + i - 1].n + N);    // a block apart
                sum += s.n;
            }
            CHECK(sum == count[c]);
        }
        // the prefix kernel: exclusive sums in channel order, then every span's room
        uint64_t base = 0;
        for (uint32_t c = 0; c < C; ++c) {
            for (uint32_t i = 0; i < n_spans[c]; ++i) tn::span_place(spans[span_off[c] + i], base, audio.pool_cap);
            base += count[c];
        }
        const uint64_t used = base < audio.pool_cap ? base : audio.pool_cap;
        const uint64_t header[2] = {base, used};
        std::memcpy(cap_out.data(), header, sizeof(header));
        std::memcpy(out.data(), n_ev.data(), (size_t)C * sizeof(uint32_t));
        std::memcpy(cap_out.data() + same::kCapHeaderBytes, n_spans.data(), (size_t)C * sizeof(uint32_t));
        // the copy kernel, into a pool of exactly the capacity
        std::vector<float> pool((size_t)audio.pool_cap, -12345.5f);
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t i = 0; i < n_spans[c]; ++i) {
                const tn::Span &s = spans[span_off[c] + i];
                for (uint64_t t = 0; t < s.n; ++t) {
                    const size_t row = (size_t)s.row0 + t;
                    pool[(size_t)(s.off + t)] = (float)(layout == SAME_LAYOUT_TIME_MAJOR ? x[row * C + c] : x[(size_t)c * n_rows + row]);
                }
            }
        // the pool is filled without a gap
        uint64_t seen = 0;
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t i = 0; i < n_spans[c]; ++i) {
                const tn::Span &s = spans[span_off[c] + i];
                CHECK(s.n == 0 || (s.off == seen && s.off + s.n <= used));
                seen += s.n;
            }
        CHECK(seen == used);
        // the harvest: the unit's, into the slot the library would use; then what the queue and the view hold, and all of it leaves
        const tq::Records r{C, desc.data(), span_off.data(), out.data(), cap_out.data(), 0};
        events.harvest(at, r);
        log.harvest(at, r, (int)(calls % tq::kSlots));
        std::vector<same_tone_event> got(events.queue.size() - events.head);
        size_t left = 1;
        CHECK(events.take(got.data(), got.size(), &left) == got.size() && left == 0);
        for (const same_tone_event &e : got)
            std::printf("event %u %u %u %u %llu %llu\n", calls, e.channel, e.kind, e.edge, (unsigned long long)e.sample_counter,
                        (unsigned long long)e.duration);
        const same_tone_audio_chunk *view = nullptr;
        size_t n_view = 0;
        const auto fetch = [&](int, uint64_t n, std::vector<float> &mem) {
            mem.resize((size_t)n);
            std::memcpy(mem.data(), pool.data(), (size_t)n * sizeof(float));
            return (int)SAME_OK;
        };
        CHECK(log.publish(fetch, &view, &n_view) == SAME_OK);
        for (size_t i = 0; i < n_view; ++i) {
            const same_tone_audio_chunk &ch = view[i];
            CHECK(ch.reserved == 0 && (ch.samples != nullptr) == (ch.n_samples != 0));
            std::printf("chunk %u %u %u %u %llu %llu %llu %zu\n", calls, ch.channel, ch.flags, ch.kind, (unsigned long long)ch.sample_counter,
                        (unsigned long long)ch.n_samples, (unsigned long long)ch.tone_start, captured.size());
            captured.insert(captured.end(), ch.samples, ch.samples + ch.n_samples);
        }
        CHECK(log.drop(n_view + 1) == SAME_EINVAL && log.drop(n_view) == SAME_OK);
        plan.commit(desc.data());
        ++calls;
    }
};

template <typename SampleT>
static void streams(const char *in_file, uint32_t rate, uint32_t C, const std::string &cut, uint32_t kinds, uint32_t tail, uint32_t maxb,
                    uint64_t pool, int reset_channel, uint64_t reset_after, const char *out_file)
{
    const std::vector<SampleT> all = read_file<SampleT>(in_file);
    CHECK(all.size() % C == 0);
    const size_t total = all.size() / C;
    Runner run(C, rate, kinds, tail, maxb, pool);
    const uint32_t N = run.plan.coef.N;
    const bool fixed = cut == "fixed";
    std::mt19937 rng(fixed ? 0u : (uint32_t)std::strtoul(cut.c_str(), nullptr, 10));
    const size_t fixed_rows[5] = {1, 319, 320, 321, 1000};
    size_t fixed_at = 0;
    std::vector<size_t> done(C, 0);
    const uint32_t special[5] = {0, 1, N - 1, N, N + 1};
    bool was_reset = reset_channel < 0;
    for (;;) {
        bool any = false;
        for (uint32_t c = 0; c < C; ++c) any |= done[c] < total;
        if (!any) break;
        if (!was_reset && done[(size_t)reset_channel] >= reset_after) {
            const uint32_t ch = (uint32_t)reset_channel;
            CHECK(run.plan.reset(&ch, 1) == SAME_OK);
            std::printf("reset %u %zu\n", ch, done[ch]);
            was_reset = true;
        }
        const bool plain = fixed || rng() % 8 == 0;
        size_t n_rows = fixed ? (fixed_at < 5 ? fixed_rows[fixed_at++] : total) : rng() % 3 == 0 ? rng() % (4 * N) + 1 : rng() % 40 + N - 20;
        std::vector<uint32_t> k(C);
        if (plain)
            for (uint32_t c = 0; c < C; ++c) n_rows = total - done[c] < n_rows ? total - done[c] : n_rows;
        for (uint32_t c = 0; c < C; ++c) {
            const uint32_t pick = rng() % 8;
            k[c] = plain ? (uint32_t)n_rows : pick < 5 ? special[pick] : (uint32_t)(rng() % (n_rows + 1));
            if (k[c] > total - done[c]) k[c] = (uint32_t)(total - done[c]);
            if (k[c] > n_rows) n_rows = k[c];
        }
        const int layout = run.calls % 2 ? SAME_LAYOUT_CHANNEL_MAJOR : SAME_LAYOUT_TIME_MAJOR;
        std::vector<SampleT> x(n_rows * C, blank(SampleT()));
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t t = 0; t < k[c]; ++t)
                x[layout == SAME_LAYOUT_TIME_MAJOR ? (size_t)t * C + c : (size_t)c * n_rows + t] = all[(size_t)c * total + done[c] + t];
        if (plain && n_rows == 0) continue;
        run.call(x.data(), n_rows, plain ? nullptr : k.data(), layout);
        for (uint32_t c = 0; c < C; ++c) done[c] += k[c];
    }
    FILE *f = std::fopen(out_file, "wb");
    CHECK(f != nullptr);
    CHECK(std::fwrite(run.captured.data(), sizeof(float), run.captured.size(), f) == run.captured.size());
    CHECK(std::fclose(f) == 0);
}

// The pattern that meets chunk_bound(n): a capture open on entry, max_blocks = 1, tail_blocks = 0, attention not active with
// run == 23, wat not active with run == 21; attention qualifies in blocks 0 and 1, wat in blocks 0 .. 3, and behind that each
// sees in turn 5 blocks without and 25 blocks with.  The call completes n blocks and touches one more.
static void bound()
{
    const uint32_t N = 320;
    for (uint32_t n = 0; n <= 200; ++n) {
        tn::Sm sm[2] = {tn::sm_zero(), tn::sm_zero()};
        sm[0].run = tn::kStartBlocks - 2; sm[0].start = 7 * N;
        sm[1].run = tn::kStartBlocks - 4; sm[1].start = 9 * N;
        const uint64_t block0 = 1000;
        tn::Cap cap{(block0 - 1) * N, 5 * N, 1, SAME_TONE_WAT, 0, 0};
        const tn::CapParams p{SAME_TONE_ATTENTION | SAME_TONE_WAT, 0, 1};
        std::vector<uint8_t> qual(n ? n : 1, 0);
        for (uint32_t b = 0; b < n; ++b) {
            const bool qa = b < 2 || (b - 2) % 30 >= 5, qw = b < 4 || (b - 4) % 30 >= 5;
            qual[b] = (uint8_t)((qa ? tn::kQAttention : 0u) | (qw ? tn::kQWat : 0u));
        }
        const tn::Desc d{block0, 0, n * N + 1, n + 1, n, 0, 0};
        std::vector<same_tone_event> ev(tn::events_bound(n));
        std::vector<tn::Span> spans(tn::chunk_bound(n));
        uint32_t n_ev = 0, n_spans = 0;
        const uint64_t rows = tn::run_capture(d, N, 0, 1, qual.data(), sm, cap, p, ev.data(), &n_ev, spans.data(), &n_spans);
        uint64_t sum = 0;
        for (uint32_t i = 0; i < n_spans; ++i) sum += spans[i].n;
        CHECK(sum == rows);
        std::printf("bound %u %u %u\n", n, n_spans, tn::chunk_bound(n));
    }
}

int main(int argc, char **argv)
{
    CHECK(argc >= 2);
    const std::string mode = argv[1];
    if (mode == "bound") {
        bound();
    } else {
        CHECK(mode == "streams" && argc == 14);
        const std::string kind = argv[3];
        const uint32_t rate = (uint32_t)std::strtoul(argv[4], nullptr, 10), C = (uint32_t)std::strtoul(argv[5], nullptr, 10);
        const uint32_t kinds = (uint32_t)std::strtoul(argv[7], nullptr, 10), tail = (uint32_t)std::strtoul(argv[8], nullptr, 10);
        const uint32_t maxb = (uint32_t)std::strtoul(argv[9], nullptr, 10);
        const uint64_t pool = std::strtoull(argv[10], nullptr, 10);
        const int reset_channel = std::atoi(argv[11]);
        const uint64_t reset_after = std::strtoull(argv[12], nullptr, 10);
        if (kind == "f32") streams<float>(argv[2], rate, C, argv[6], kinds, tail, maxb, pool, reset_channel, reset_after, argv[13]);
        else streams<int16_t>(argv[2], rate, C, argv[6], kinds, tail, maxb, pool, reset_channel, reset_after, argv[13]);
    }
    std::printf("OK\n");
    return 0;
}
