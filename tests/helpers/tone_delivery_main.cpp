// Host-only driver of tone-alert audio in delivery form: the plans (sameold_amd/csrc/same_tone_delivery_plan.h,
// same_tone_audio_plan.h, same_tones_plan.h) and the device cores (same_tone_delivery_dev.h, same_tone_audio_dev.h,
// same_tones_dev.h), for tests/test_tone_delivery_cpu.py under ASan + UBSan.  It runs calls the way same_tones.hip,
// same_tone_audio.hip and same_tone_delivery.hip do -- the capture work of tone_audio_main.cpp into a staging pool, then every
// chunk's outputs (td::out_of) with an exclusive prefix over the channels' delivered counts, every tile of 256 outputs from a
// window of exactly the tile's length (td::tile_of, window_at, tile_output), and td::history_step per channel on the call's input
// -- on buffers of exactly the size the library provides: the input with NaN (f32) or 32767 (int16) behind every channel's
// count, the two record buffers of exactly the layout's bytes (same_tone_queue.h), a staging pool of samples_per_call floats, a
// delivery pool of samples_per_call int16, T - 1 history floats per channel that start as NaN.  Behind a call comes the library's
// own harvest: the unit's chunk log takes the call's records and fetches the delivery pool's used part with a memcpy, and what
// is printed is what the published view holds (ROWS, which the public record does not carry, from the call's chunk slots in the
// view's order).  Layouts alternate from call to call.
//
//     tone_delivery_main IN_FILE f32|i16 RATE CHANNELS CUT KINDS TAIL_BLOCKS MAX_BLOCKS POOL RESET_CHANNEL RESET_AFTER OUT_RATE GAIN OUT_FILE
//         IN_FILE: [CHANNELS x samples] channel-major, little-endian f32 or int16.  CUT: "fixed" -- plain calls of 1, 319, 320,
//         321, 1000 rows and the rest; "short" -- one plain call of 29 N + 3 rows, plain calls of 1, 1, 2, T - 2, T - 1 and T rows
//         (those that are positive), a ragged call that gives channel 0 no row and the others 5, and the rest; or a seed: random
//         ragged calls.  RESET_CHANNEL (-1: none) is reset between two calls once it has consumed RESET_AFTER samples.
//         stdout: "plan L M T", "reset CHANNEL POSITION", "call INDEX K_0 .. K_C-1" (the counts), "chunk CALL CHANNEL FLAGS KIND
//         COUNTER ROWS TONE_START OUT_INDEX N_SAMPLES AT" in queue order (ROWS: the placed rows; AT: the first sample's index in
//         OUT_FILE, int16), "OK".
#include "../../sameold_amd/csrc/same_tone_delivery_plan.h"
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
namespace td = same::td;
namespace tq = same::tq;
using same::ToneAudioPlan;
using same::ToneDeliveryPlan;
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

// A handle in delivery mode: the plans and the device's memory
struct Runner {
    TonesPlan plan;
    ToneDeliveryPlan delivery;
    std::vector<float> acc;
    std::vector<tn::Sm> sm;
    std::vector<tn::Cap> cap;
    std::vector<float> hist;                             // [C][T - 1]
    std::vector<uint64_t> a_next;                        // [C]
    tq::ChunkLog<same_tone_delivery_chunk, int16_t, std::vector<int16_t>> log{tq::kSlots + 1};
    std::vector<int16_t> delivered;                      // every queued chunk's samples, in queue order
    uint32_t calls = 0;

    Runner(uint32_t C, uint32_t rate, uint32_t kinds, uint32_t tail, uint32_t maxb, uint64_t pool, uint32_t out_rate, float gain)
    {
        CHECK(plan.init(C, rate) == SAME_OK);
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        CHECK(delivery.set(0, tail, maxb, pool, rate, out_rate, gain) == SAME_EINVAL && delivery.set(kinds, tail, 0, pool, rate, out_rate, gain) == SAME_EINVAL);
        CHECK(delivery.set(kinds, tail, maxb, pool, rate, 0, gain) == SAME_EINVAL && delivery.set(kinds, tail, maxb, pool, rate, rate + 1, gain) == SAME_EINVAL);
        for (float g : {0.0f, -1.0f, inf, -inf, nan}) CHECK(delivery.set(kinds, tail, maxb, pool, rate, out_rate, g) == SAME_EINVAL && !delivery.on());
        CHECK(delivery.set(kinds, tail, maxb, pool, 96000, 8000, gain) == SAME_ERATE && !delivery.on());
        CHECK(delivery.set(kinds, tail, maxb, 0, rate, out_rate, gain) == SAME_OK && !delivery.on());
        CHECK(delivery.set(kinds, tail, maxb, pool, rate, out_rate, gain) == SAME_OK && delivery.on());
        const td::Params &p = delivery.params;
        CHECK(p.L <= p.M && p.T <= same::rs::kMaxT && delivery.taps_t.size() == (size_t)p.T * p.L);
        std::printf("plan %u %u %u\n", p.L, p.M, p.T);
        // (garbage: the first call that runs makes the state machines and the capture state idle, and nothing reads a history
        // or a clock that history_step has not written)
        acc.assign((size_t)2 * tn::kAccWords * C, nan);
        tn::Sm junk;
        std::memset(&junk, 0x5a, sizeof(junk));
        sm.assign((size_t)2 * C, junk);
        tn::Cap cjunk;
        std::memset(&cjunk, 0x5a, sizeof(cjunk));
        cap.assign(C, cjunk);
        hist.assign((size_t)C * (p.T - 1), nan);
        a_next.assign(C, 0x5a5a5a5a5a5a5a5aull);
    }

    template <typename SampleT>
    void call(const SampleT *x, size_t n_rows, const uint32_t *counts, int layout)
    {
        const uint32_t C = plan.n_channels(), N = plan.coef.N;
        const ToneAudioPlan &audio = delivery.audio;
        const td::Params &p = delivery.params;
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
        CHECK(at.set_events(C, shape.event_slots) == SAME_OK && at.set_capture(C, slots, true) == SAME_OK);
        std::vector<uint8_t> out((size_t)at.out_bytes, 0xee), cap_out((size_t)at.cap_bytes, 0xee);
        same_tone_event *ev = (same_tone_event *)(out.data() + at.events_at);
        tn::Span *spans = (tn::Span *)(cap_out.data() + at.spans_at);
        td::Out *outs = (td::Out *)(cap_out.data() + at.outs_at);
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
        // the capture work: state machines, the prefix over captured rows, the copy into the staging pool
        std::vector<uint32_t> n_ev(C, 0), n_spans(C, 0);
        std::vector<uint64_t> count(C, 0), entry_first(C, 0);
        for (uint32_t c = 0; c < C; ++c) entry_first[c] = cap[c].first;
        for (uint32_t c = 0; c < C; ++c)
            count[c] = tn::run_capture(desc[c], N, c, C, qual.data(), &sm[2 * (size_t)c], cap[c], audio.params, ev, &n_ev[c],
                                       spans + span_off[c], &n_spans[c]);
        uint64_t base = 0;
        for (uint32_t c = 0; c < C; ++c) {
            for (uint32_t i = 0; i < n_spans[c]; ++i) tn::span_place(spans[span_off[c] + i], base, audio.pool_cap);
            base += count[c];
        }
        std::vector<float> pool((size_t)audio.pool_cap, blank(float()));
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t i = 0; i < n_spans[c]; ++i) {
                const tn::Span &s = spans[span_off[c] + i];
                for (uint64_t t = 0; t < s.n; ++t) {
                    const size_t row = (size_t)s.row0 + t;
                    pool[(size_t)(s.off + t)] = (float)(layout == SAME_LAYOUT_TIME_MAJOR ? x[row * C + c] : x[(size_t)c * n_rows + row]);
                }
            }
        // the output-offset kernel: every chunk's outputs, then the delivery pool in chunk order
        uint64_t used = 0;
        std::vector<uint64_t> rows;                          // the chunks' placed rows, by channel
        for (uint32_t c = 0; c < C; ++c) {
            uint64_t v = 0;
            for (uint32_t i = 0; i < n_spans[c]; ++i) {
                const tn::Span &s = spans[span_off[c] + i];
                CHECK((s.flags & SAME_TONE_AUDIO_FIRST) || s.row0 == 0);           // no third case
                td::Out &o = outs[span_off[c] + i];
                o = td::out_of(s, a_next[c], p, v);
                CHECK((s.flags & SAME_TONE_AUDIO_FIRST) ? o.a == 0 : o.a == s.sample_counter - entry_first[c]);     // the capture's own clock
                CHECK(o.n_out <= s.n);                                             // L <= M: never more outputs than placed rows
                v += o.n_out;
                rows.push_back(s.n);
            }
            for (uint32_t i = 0; i < n_spans[c]; ++i) outs[span_off[c] + i].off += used;
            used += v;
        }
        CHECK(used <= audio.pool_cap);
        // the decimator, tile by tile, into a pool of exactly the capacity
        std::vector<int16_t> dpool((size_t)audio.pool_cap, (int16_t)-12345);
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t i = 0; i < n_spans[c]; ++i) {
                const tn::Span &s = spans[span_off[c] + i];
                const td::Out &o = outs[span_off[c] + i];
                const uint64_t tiles = (o.n_out + td::kTileOutputs - 1) / td::kTileOutputs;
                for (uint64_t t = 0; t < tiles; ++t) {
                    const td::Tile tl = td::tile_of(o, (uint32_t)t, p);
                    CHECK(tl.W <= td::kWindowMax && tl.n >= 1);
                    std::vector<float> w(tl.W);
                    for (uint32_t q = 0; q < tl.W; ++q) w[q] = td::window_at(s, o, tl, q, p.T, pool.data(), hist.data() + (size_t)c * (p.T - 1));
                    for (uint32_t l = 0; l < tl.n; ++l) dpool[(size_t)(o.off + t * td::kTileOutputs + l)] = td::tile_output(w.data(), delivery.taps_t.data(), p, tl, l);
                }
            }
        // the history kernel, behind the decimator
        for (uint32_t c = 0; c < C; ++c) {
            const SampleT *xc = layout == SAME_LAYOUT_TIME_MAJOR ? x + c : x + (size_t)c * n_rows;
            td::history_step(desc[c], cap[c], N, p.T, xc, layout == SAME_LAYOUT_TIME_MAJOR ? (size_t)C : (size_t)1,
                             hist.data() + (size_t)c * (p.T - 1), 1, &a_next[c]);
        }
        // the delivery pool is filled without a gap and without padding
        uint64_t seen = 0;
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t i = 0; i < n_spans[c]; ++i) {
                CHECK(outs[span_off[c] + i].off == seen);
                seen += outs[span_off[c] + i].n_out;
            }
        CHECK(seen == used);
        // the harvest: the unit's, into the slot the library would use; then what the view holds, and all of it leaves
        const uint64_t header[3] = {base, base < audio.pool_cap ? base : audio.pool_cap, used};
        std::memcpy(cap_out.data(), header, sizeof(header));
        std::memcpy(out.data(), n_ev.data(), (size_t)C * sizeof(uint32_t));
        std::memcpy(cap_out.data() + same::kCapHeaderBytes, n_spans.data(), (size_t)C * sizeof(uint32_t));
        const tq::Records r{C, desc.data(), span_off.data(), out.data(), cap_out.data(), p.rate};
        log.harvest(at, r, (int)(calls % tq::kSlots));         // (this driver prints no events: tone_audio_main.cpp harvests them)
        const same_tone_delivery_chunk *view = nullptr;
        size_t n_view = 0;
        const auto fetch = [&](int, uint64_t n, std::vector<int16_t> &mem) {
            if (mem.size() < n) mem.resize((size_t)n);
            std::memcpy(mem.data(), dpool.data(), (size_t)n * sizeof(int16_t));
            return (int)SAME_OK;
        };
        CHECK(log.publish(fetch, &view, &n_view) == SAME_OK && n_view == rows.size());
        for (size_t i = 0; i < n_view; ++i) {
            const same_tone_delivery_chunk &ch = view[i];
            CHECK(ch.rate == p.rate && (ch.samples != nullptr) == (ch.n_samples != 0));
            std::printf("chunk %u %u %u %u %llu %llu %llu %llu %llu %zu\n", calls, ch.channel, ch.flags, ch.kind, (unsigned long long)ch.sample_counter,
                        (unsigned long long)rows[i], (unsigned long long)ch.tone_start, (unsigned long long)ch.out_index,
                        (unsigned long long)ch.n_samples, delivered.size());
            delivered.insert(delivered.end(), ch.samples, ch.samples + ch.n_samples);
        }
        CHECK(log.drop(n_view + 1) == SAME_EINVAL && log.drop(n_view) == SAME_OK && log.n_free() <= (size_t)tq::kSlots + 1);
        plan.commit(desc.data());
        ++calls;
    }
};

template <typename SampleT>
static void streams(const char *in_file, uint32_t rate, uint32_t C, const std::string &cut, uint32_t kinds, uint32_t tail, uint32_t maxb,
                    uint64_t pool, int reset_channel, uint64_t reset_after, uint32_t out_rate, float gain, const char *out_file)
{
    const std::vector<SampleT> all = read_file<SampleT>(in_file);
    CHECK(all.size() % C == 0);
    const size_t total = all.size() / C;
    Runner run(C, rate, kinds, tail, maxb, pool, out_rate, gain);
    const uint32_t N = run.plan.coef.N, T = run.delivery.params.T;
    const bool fixed = cut == "fixed", shorts = cut == "short";
    std::mt19937 rng(fixed || shorts ? 0u : (uint32_t)std::strtoul(cut.c_str(), nullptr, 10));
    // the plain calls of the two stated cuts; "short" has its ragged call behind them (-1), and both end with the rest
    std::vector<long> stated;
    if (fixed) stated = {1, 319, 320, 321, 1000};
    if (shorts) {
        stated = {(long)(29 * N + 3)};
        for (long n : {1l, 1l, 2l, (long)T - 2, (long)T - 1, (long)T})
            if (n > 0) stated.push_back(n);
        stated.push_back(-1);
    }
    size_t stated_at = 0;
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
        const bool is_stated = fixed || shorts;
        const long want = is_stated ? (stated_at < stated.size() ? stated[stated_at++] : (long)total) : 0;
        const bool plain = is_stated ? want >= 0 : rng() % 8 == 0;
        size_t n_rows = is_stated ? (want >= 0 ? (size_t)want : 5) : rng() % 3 == 0 ? rng() % (4 * N) + 1 : rng() % 40 + N - 20;
        std::vector<uint32_t> k(C);
        bool level = true;                                   // every channel has as many samples left
        for (uint32_t c = 0; c < C; ++c) level &= done[c] == done[0];
        if (plain && level)
            for (uint32_t c = 0; c < C; ++c) n_rows = total - done[c] < n_rows ? total - done[c] : n_rows;
        for (uint32_t c = 0; c < C; ++c) {
            const uint32_t pick = rng() % 8;
            k[c] = is_stated ? (want < 0 && c == 0 ? 0u : (uint32_t)n_rows) : plain ? (uint32_t)n_rows : pick < 5 ? special[pick] : (uint32_t)(rng() % (n_rows + 1));
            if (k[c] > total - done[c]) k[c] = (uint32_t)(total - done[c]);
            if (k[c] > n_rows) n_rows = k[c];
        }
        if (is_stated) {
            n_rows = 0;
            for (uint32_t c = 0; c < C; ++c) n_rows = k[c] > n_rows ? k[c] : n_rows;
        }
        const bool ragged = !(plain && level);
        const int layout = run.calls % 2 ? SAME_LAYOUT_CHANNEL_MAJOR : SAME_LAYOUT_TIME_MAJOR;
        std::vector<SampleT> x(n_rows * C, blank(SampleT()));
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t t = 0; t < k[c]; ++t)
                x[layout == SAME_LAYOUT_TIME_MAJOR ? (size_t)t * C + c : (size_t)c * n_rows + t] = all[(size_t)c * total + done[c] + t];
        if (!ragged && n_rows == 0) continue;
        run.call(x.data(), n_rows, ragged ? k.data() : nullptr, layout);
        for (uint32_t c = 0; c < C; ++c) done[c] += k[c];
    }
    FILE *f = std::fopen(out_file, "wb");
    CHECK(f != nullptr);
    CHECK(std::fwrite(run.delivered.data(), sizeof(int16_t), run.delivered.size(), f) == run.delivered.size());
    CHECK(std::fclose(f) == 0);
}

int main(int argc, char **argv)
{
    CHECK(argc == 15);
    const std::string kind = argv[2];
    const uint32_t rate = (uint32_t)std::strtoul(argv[3], nullptr, 10), C = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    const uint32_t kinds = (uint32_t)std::strtoul(argv[6], nullptr, 10), tail = (uint32_t)std::strtoul(argv[7], nullptr, 10);
    const uint32_t maxb = (uint32_t)std::strtoul(argv[8], nullptr, 10);
    const uint64_t pool = std::strtoull(argv[9], nullptr, 10);
    const int reset_channel = std::atoi(argv[10]);
    const uint64_t reset_after = std::strtoull(argv[11], nullptr, 10);
    const uint32_t out_rate = (uint32_t)std::strtoul(argv[12], nullptr, 10);
    const float gain = std::strtof(argv[13], nullptr);
    if (kind == "f32") streams<float>(argv[1], rate, C, argv[5], kinds, tail, maxb, pool, reset_channel, reset_after, out_rate, gain, argv[14]);
    else streams<int16_t>(argv[1], rate, C, argv[5], kinds, tail, maxb, pool, reset_channel, reset_after, out_rate, gain, argv[14]);
    std::printf("OK\n");
    return 0;
}
