// Host-only driver of the tone detector's plan (sameold_amd/csrc/same_tones_plan.h) and arithmetic (same_tones_dev.h), for
// tests/test_tones_cpu.py under ASan + UBSan.  It runs calls the way same_tones.hip does -- describe, every (channel, block)
// item on its own, the state machines over the call's qualify bits, the harvest of the channels' event slots, commit -- on
// buffers of exactly the size a caller and the library provide: the input with NaN (f32) or 32767 (int16) behind every
// channel's count, d_blocks of [max_blocks x C x 4] pre-filled with a sentinel, qualify bits of [max_blocks x C], event slots of
// exactly the plan's number.  Layouts alternate from call to call.  A call's items run last block first, so that the item that
// saves a channel's open block runs before the item that loads the one saved by the call before: the two Acc banks keep them
// apart, as they do on the device, where the two run at the same time.
//
//     tones_main streams IN_FILE f32|i16 RATE CHANNELS SEED RESET_CHANNEL RESET_AFTER OUT_DIR
//         IN_FILE: [CHANNELS x samples] channel-major, little-endian f32 or int16.  The streams are cut into random ragged
//         calls; RESET_CHANNEL (-1: none) is reset between two calls once it has consumed RESET_AFTER samples.
//         stdout: "reset CHANNEL POSITION", "event CALL CHANNEL KIND EDGE SAMPLE_COUNTER DURATION" in poll order,
//         "counter CHANNEL POSITION", "calls N", "saw COUNT" for each special count a call used, "OK".
//         Files: OUT_DIR/blocks_cCHANNEL.f32, the channel's completed blocks [n x 4] in stream order.
//     tones_main bound
//         stdout: "bound N EVENTS LIMIT" for N = 0 .. 200: the events one class emits over N blocks of the adversarial pattern
//         (entered not active with run == 24: q = 1, then 5 x 0 and 25 x 1 in turn) and half of events_bound(N); "OK".
//     tones_main coef RATE ...
//         stdout: "coef RATE N C0 C1 C2" with the coefficients' bit patterns in hex, "erate RATE RC" for a refused rate; "OK".
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
using same::TonesPlan;

static const float kSentinel = -12345.5f;

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

// A plan and the device's memory as same_tones.hip holds them
struct Runner {
    TonesPlan plan;
    std::vector<float> acc;                              // two banks of [kAccWords x C]
    std::vector<tn::Sm> sm;                              // [C x 2]
    std::vector<std::vector<float>> blocks;              // per channel: its completed blocks, 4 floats each
    uint32_t calls = 0;

    Runner(uint32_t C, uint32_t rate)
    {
        CHECK(plan.init(C, rate) == SAME_OK);
        // (garbage: an Acc is read only where a call saved one, the state machines are made idle by the first call)
        acc.assign((size_t)2 * tn::kAccWords * C, std::numeric_limits<float>::quiet_NaN());
        tn::Sm junk;
        std::memset(&junk, 0x5a, sizeof(junk));
        sm.assign((size_t)2 * C, junk);
        blocks.resize(C);
    }

    // x: the call's buffer in `layout`, n_rows rows; counts: null for a plain call
    template <typename SampleT>
    void call(const SampleT *x, size_t n_rows, const uint32_t *counts, int layout)
    {
        const uint32_t C = plan.n_channels(), N = plan.coef.N;
        std::vector<uint32_t> nb(C, 0);
        uint32_t max_blocks = 0;
        CHECK(plan.block_counts(counts, n_rows, nb.data(), &max_blocks) == SAME_OK);
        std::vector<tn::Desc> desc(C);
        const TonesPlan::Shape shape = plan.describe(counts, n_rows, desc.data());
        CHECK(shape.max_complete == max_blocks);
        if (!shape.any_samples) return;                  // a no-op: nothing moves, a pending reset stays pending
        std::vector<float> out((size_t)max_blocks * C * 4, kSentinel);
        std::vector<uint8_t> qual((size_t)max_blocks * C, 0xff);
        std::vector<same_tone_event> ev((size_t)shape.event_slots);
        const size_t bank_words = (size_t)tn::kAccWords * C;
        for (uint32_t c = 0; c < C; ++c) {
            const tn::Desc &d = desc[c];
            CHECK(d.n_complete == nb[c]);
            const float *bank_in = acc.data() + ((d.flags & tn::kDescBank) ? bank_words : 0);
            float *bank_out = acc.data() + ((d.flags & tn::kDescBank) ? 0 : bank_words);
            for (uint32_t j = d.n_touch; j-- > 0;) {
                uint32_t r0, r1;
                tn::block_rows(d, N, j, r0, r1);
                CHECK(r0 < r1 && r1 <= d.count && r1 - r0 <= N);
                tn::Acc a = tn::block_continues(d, j) ? tn::acc_load(bank_in, C, c) : tn::acc_zero();
                if (layout == SAME_LAYOUT_TIME_MAJOR) tn::run_rows(a, plan.coef, x + c, C, r0, r1);
                else tn::run_rows(a, plan.coef, x + (size_t)c * n_rows, 1, r0, r1);
                tn::block_end(d, plan.coef, j, a, c, C, out.data(), qual.data(), bank_out);
            }
        }
        std::vector<uint32_t> n_ev(C, 0);
        for (uint32_t c = 0; c < C; ++c) {
            n_ev[c] = tn::run_state_machines(desc[c], N, c, C, qual.data(), &sm[2 * (size_t)c], ev.data());
            CHECK(n_ev[c] <= tn::events_bound(desc[c].n_complete));
        }
        for (uint32_t c = 0; c < C; ++c) {
            for (uint32_t i = 0; i < n_ev[c]; ++i) {
                const same_tone_event &e = ev[desc[c].ev_off + i];
                CHECK(e.channel == c && e.reserved == 0);
                std::printf("event %u %u %u %u %llu %llu\n", calls, c, e.kind, e.edge, (unsigned long long)e.sample_counter,
                            (unsigned long long)e.duration);
            }
            for (uint32_t j = 0; j < max_blocks; ++j)
                for (uint32_t w = 0; w < 4; ++w) {
                    const float v = out[((size_t)j * C + c) * 4 + w];
                    if (j < nb[c]) blocks[c].push_back(v);
                    else CHECK(v == kSentinel);          // rows at or beyond block_counts[c] are never written
                }
        }
        plan.commit(desc.data());
        ++calls;
    }
};

template <typename SampleT>
static void streams(const char *in_file, uint32_t rate, uint32_t C, uint32_t seed, int reset_channel, uint64_t reset_after, const std::string &dir)
{
    const std::vector<SampleT> all = read_file<SampleT>(in_file);
    CHECK(all.size() % C == 0);
    const size_t total = all.size() / C;
    Runner run(C, rate);
    const uint32_t N = run.plan.coef.N;
    std::mt19937 rng(seed);
    std::vector<size_t> done(C, 0);
    const uint32_t special[5] = {0, 1, N - 1, N, N + 1};
    bool saw[5] = {false, false, false, false, false};
    bool was_reset = reset_channel < 0;
    for (;;) {
        bool any = false;
        for (uint32_t c = 0; c < C; ++c) any |= done[c] < total;
        if (!any) break;
        if (!was_reset && done[(size_t)reset_channel] >= reset_after) {
            const uint32_t ch = (uint32_t)reset_channel, bad = C;
            CHECK(run.plan.reset(&bad, 1) == SAME_EINVAL);
            CHECK(run.plan.pos[ch] == done[ch]);             // nothing was reset
            CHECK(run.plan.reset(&ch, 1) == SAME_OK);
            CHECK(run.plan.pos[ch] == 0);
            std::printf("reset %u %zu\n", ch, done[ch]);
            was_reset = true;
        }
        const bool plain = rng() % 8 == 0;
        size_t n_rows = rng() % 3 == 0 ? rng() % (4 * N) + 1 : rng() % 40 + N - 20;
        std::vector<uint32_t> k(C);
        if (plain)                                           // a plain call takes the same from all: what the shortest has left
            for (uint32_t c = 0; c < C; ++c) n_rows = total - done[c] < n_rows ? total - done[c] : n_rows;
        for (uint32_t c = 0; c < C; ++c) {
            const uint32_t pick = rng() % 8;
            k[c] = plain ? (uint32_t)n_rows : pick < 5 ? special[pick] : (uint32_t)(rng() % (n_rows + 1));
            if (k[c] > total - done[c]) k[c] = (uint32_t)(total - done[c]);
            if (k[c] > n_rows) n_rows = k[c];                // (a special count may exceed the rows drawn)
            for (int s = 0; s < 5; ++s) saw[s] |= k[c] == special[s];
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
    for (int s = 0; s < 5; ++s)
        if (saw[s]) std::printf("saw %u\n", special[s]);
    for (uint32_t c = 0; c < C; ++c) {
        std::printf("counter %u %llu\n", c, (unsigned long long)run.plan.pos[c]);
        const std::string path = dir + "/blocks_c" + std::to_string(c) + ".f32";
        FILE *f = std::fopen(path.c_str(), "wb");
        CHECK(f != nullptr);
        CHECK(std::fwrite(run.blocks[c].data(), sizeof(float), run.blocks[c].size(), f) == run.blocks[c].size());
        CHECK(std::fclose(f) == 0);
    }
    std::printf("calls %u\n", run.calls);
}

static void bound()
{
    for (uint32_t n = 0; n <= 200; ++n) {
        tn::Sm s = tn::sm_zero();
        s.run = tn::kStartBlocks - 1;
        s.start = 7;
        uint32_t events = 0;
        for (uint32_t b = 0; b < n; ++b) {
            // q = 1, then 5 x 0 and 25 x 1 in turn
            const uint32_t ph = b == 0 ? 0 : (b - 1) % 30;
            const bool q = b == 0 || ph >= 5;
            same_tone_event e;
            events += tn::sm_step(s, q, 1000 + b, 320, 0, SAME_TONE_WAT, &e);
        }
        CHECK(tn::events_bound(n) % 2 == 0);
        std::printf("bound %u %u %u\n", n, events, tn::events_bound(n) / 2);
    }
}

int main(int argc, char **argv)
{
    CHECK(argc >= 2);
    const std::string mode = argv[1];
    if (mode == "bound") {
        bound();
    } else if (mode == "coef") {
        for (int i = 2; i < argc; ++i) {
            const uint32_t rate = (uint32_t)std::strtoul(argv[i], nullptr, 10);
            tn::Coef cf{};
            const int rc = TonesPlan::coefficients(rate, cf);
            if (rc) { std::printf("erate %u %d\n", rate, rc); continue; }
            uint32_t bits[3];
            std::memcpy(bits, cf.c, sizeof(bits));
            std::printf("coef %u %u %08x %08x %08x\n", rate, cf.N, bits[0], bits[1], bits[2]);
        }
    } else {
        CHECK(mode == "streams" && argc == 10);
        const std::string kind = argv[3];
        const uint32_t rate = (uint32_t)std::strtoul(argv[4], nullptr, 10), C = (uint32_t)std::strtoul(argv[5], nullptr, 10);
        const uint32_t seed = (uint32_t)std::strtoul(argv[6], nullptr, 10);
        const int reset_channel = std::atoi(argv[7]);
        const uint64_t reset_after = std::strtoull(argv[8], nullptr, 10);
        if (kind == "f32") streams<float>(argv[2], rate, C, seed, reset_channel, reset_after, argv[9]);
        else streams<int16_t>(argv[2], rate, C, seed, reset_channel, reset_after, argv[9]);
    }
    std::printf("OK\n");
    return 0;
}
