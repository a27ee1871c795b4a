// Host-only driver of the mixed-rate resampler's plan (sameold_amd/csrc/same_resample_plan.h) and per-output arithmetic
// (same_resample_dev.h), for tests/test_resample_plan_cpu.py under ASan + UBSan.  It runs calls the way same_resample.hip does
// -- describe, clear the reset channels' histories, every lane's rows in blocks of 64, the history behind the call, commit --
// on buffers of exactly the size a caller must provide (time-major [n_rows x C] with NaN behind every channel's count, an
// output of [max_out x C] pre-filled with a sentinel), and writes what went in and what came out, per channel, for the test to
// hold against the numpy reference.
//
//     resample_plan_main OUT_DIR SEED
// stdout: "plan RATE L M T" per rate, "erate RATE RC", "ratios17 RC", "stream TAG CHANNEL RATE N_IN N_OUT" per written stream,
// and "OK" at the end.  Files: taps_RATE.f32; TAG_cCHANNEL_x.f32 | _x.i16 and TAG_cCHANNEL_y.f32.
#include "../../sameold_amd/csrc/same_resample_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace rs = same::rs;
using same::ResamplePlan;

static const uint32_t kOutRate = 22050;
static const uint32_t kRates[] = {48000, 44100, 32000, 24000, 16000, 11025, 8000, 96000, 22050};
static const uint32_t kNRates = sizeof(kRates) / sizeof(kRates[0]);
static const float kSentinel = -12345.5f;

static std::string g_dir;

template <typename T>
static void write_file(const std::string &name, const std::vector<T> &v)
{
    const std::string path = g_dir + "/" + name;
    FILE *f = std::fopen(path.c_str(), "wb");
    CHECK(f != nullptr);
    CHECK(std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size());
    CHECK(std::fclose(f) == 0);
}

static float noise(std::mt19937 &rng, float) { return (float)(rng() >> 8) / 16777216.0f * 65535.0f - 32768.0f; }
static int16_t noise(std::mt19937 &rng, int16_t) { return (int16_t)(uint16_t)(rng() >> 12); }
static float blank(float) { return std::numeric_limits<float>::quiet_NaN(); }
static int16_t blank(int16_t) { return 0x7fff; }
static const char *suffix(float) { return "f32"; }
static const char *suffix(int16_t) { return "i16"; }

// A plan and the device's memory as a caller of the C ABI and same_resample.hip hold them
template <typename SampleT>
struct Runner {
    ResamplePlan plan;
    std::vector<float> hist;                             // [rs::kHistRows x C]
    std::vector<std::vector<SampleT>> xlog;
    std::vector<std::vector<float>> ylog;
    std::vector<uint64_t> out_sum;
    uint32_t calls = 0, short_calls = 0;

    explicit Runner(const std::vector<uint32_t> &rates)
    {
        CHECK(plan.init((uint32_t)rates.size(), rates.data(), kOutRate) == SAME_OK);
        // (garbage: the first call must clear every column)
        hist.assign((size_t)rs::kHistRows * rates.size(), std::numeric_limits<float>::quiet_NaN());
        xlog.resize(rates.size()); ylog.resize(rates.size()); out_sum.assign(rates.size(), 0);
    }
    void forget() { for (auto &v : xlog) v.clear(); for (auto &v : ylog) v.clear(); out_sum.assign(out_sum.size(), 0); }

    void call(size_t n_rows, const std::vector<uint32_t> &in_counts, std::mt19937 &rng)
    {
        const uint32_t C = plan.n_channels();
        std::vector<SampleT> x(n_rows * C, blank(SampleT()));
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t t = 0; t < in_counts[c]; ++t) {
                x[(size_t)t * C + c] = noise(rng, SampleT());
                xlog[c].push_back(x[(size_t)t * C + c]);
            }
        std::vector<uint32_t> out(C, 0);
        uint32_t max_out = 0;
        CHECK(plan.out_counts(in_counts.data(), n_rows, out.data(), &max_out) == SAME_OK);
        std::vector<rs::Desc> desc(C);
        plan.describe(in_counts.data(), out.data(), desc.data());
        std::vector<float> y((size_t)max_out * C, kSentinel);
        // clear_kernel
        for (uint32_t c = 0; c < C; ++c)
            if (desc[c].clear)
                for (uint32_t i = 0; i < rs::kHistRows; ++i) hist[(size_t)i * C + c] = 0.0f;
        // resample_kernel: a lane's rows in the kernel's blocks
        for (uint32_t c = 0; c < C; ++c) {
            const rs::Ratio &r = plan.ratios[desc[c].ratio];
            for (uint32_t row0 = 0; row0 < desc[c].out_count; row0 += 64) {
                const uint32_t left = desc[c].out_count - row0;
                rs::lane_rows(desc[c], r, plan.taps.data(), x.data() + c, C, hist.data() + c, C, y.data() + c, C, row0, row0 + (left < 64 ? left : 64));
            }
        }
        // history_kernel
        for (uint32_t c = 0; c < C; ++c) {
            const uint32_t T = plan.ratios[desc[c].ratio].T;
            if (desc[c].in_count == 0 || T == 1) continue;
            rs::update_history(hist.data() + c, C, T, x.data() + c, C, desc[c].in_count);
            if (desc[c].in_count < T - 1) ++short_calls;
        }
        plan.commit(in_counts.data(), out.data());
        for (uint32_t c = 0; c < C; ++c) {
            for (uint32_t n = 0; n < max_out; ++n) {
                const float v = y[(size_t)n * C + c];
                if (n < out[c]) ylog[c].push_back(v);
                else CHECK(v == kSentinel);                  // rows at or beyond out_counts[c] are never written
            }
            out_sum[c] += out[c];
        }
        ++calls;
    }

    // feed every channel `total` more samples in random calls: long ones, empty ones, and runs of calls of 0, 1 and a few
    // samples (fewer than T - 1: the history shifts) several in a row
    void feed(uint32_t total, std::mt19937 &rng)
    {
        const uint32_t C = plan.n_channels();
        std::vector<uint32_t> left(C, total), k(C);
        int run = 0;
        for (;;) {
            bool any = false;
            for (uint32_t c = 0; c < C; ++c) any |= left[c] != 0;
            if (!any) break;
            if (run == 0 && rng() % 4 == 0) run = 5;
            size_t n_rows;
            if (run > 0) {
                --run;
                n_rows = 12;
                for (uint32_t c = 0; c < C; ++c) {
                    const uint32_t pick = rng() % 4;
                    k[c] = pick == 0 ? 0 : pick == 1 ? 1 : rng() % 13;
                }
            } else {
                n_rows = rng() % 700 + 1;
                for (uint32_t c = 0; c < C; ++c) k[c] = rng() % 5 == 0 ? (uint32_t)n_rows : (uint32_t)(rng() % (n_rows + 1));
            }
            for (uint32_t c = 0; c < C; ++c) { if (k[c] > left[c]) k[c] = left[c]; left[c] -= k[c]; }
            call(n_rows, k, rng);
        }
    }

    void dump(const char *tag)
    {
        for (uint32_t c = 0; c < plan.n_channels(); ++c) {
            const rs::Ratio &r = plan.ratio(c);
            // exactly ceil(N L / M) outputs after N samples, whatever the calls were
            CHECK(plan.n_out[c] == rs::outputs_after(plan.n_in[c], r.L, r.M));
            CHECK(out_sum[c] == ylog[c].size());
            const std::string base = std::string(tag) + "_c" + std::to_string(c);
            write_file(base + "_x." + suffix(SampleT()), xlog[c]);
            write_file(base + "_y.f32", ylog[c]);
            std::printf("stream %s %u %u %zu %zu\n", tag, c, plan.chan_rate[c], xlog[c].size(), ylog[c].size());
        }
    }
};

template <typename SampleT>
static void streams(const char *tag, uint32_t seed)
{
    std::mt19937 rng(seed);
    Runner<SampleT> run(std::vector<uint32_t>(kRates, kRates + kNRates));
    run.feed(6000, rng);
    CHECK(run.short_calls > 50);
    run.dump(tag);
    for (uint32_t c = 0; c < kNRates; ++c) CHECK(run.plan.n_in[c] == 6000);

    // resets: channels 0 and 3 take new sources (8 kHz: a ratio the plan has; 12 kHz: a new one), channel 5 restarts at its rate
    const uint32_t chans[2] = {0, 3}, rates[2] = {8000, 12000}, keep[1] = {5};
    const uint32_t bad[1] = {kNRates}, far[1] = {192000};
    CHECK(run.plan.reset(bad, 1, nullptr) == SAME_EINVAL);
    CHECK(run.plan.reset(keep, 1, far) == SAME_ERATE);
    CHECK(run.plan.n_in[5] == 6000 && run.plan.clear[5] == 0);           // nothing was reset
    CHECK(run.plan.reset(chans, 2, rates) == SAME_OK);
    CHECK(run.plan.reset(keep, 1, nullptr) == SAME_OK);
    CHECK(run.plan.n_in[0] == 0 && run.plan.n_out[3] == 0 && run.plan.n_in[5] == 0 && run.plan.n_in[1] == 6000);
    CHECK(run.plan.ratios.size() == kNRates + 1);
    run.forget();
    run.feed(1500, rng);
    run.dump((std::string(tag) + "reset").c_str());
}

int main(int argc, char **argv)
{
    CHECK(argc == 3);
    g_dir = argv[1];
    const uint32_t seed = (uint32_t)std::strtoul(argv[2], nullptr, 10);

    for (uint32_t r : kRates) {
        uint32_t L = 0, M = 0, T = 0;
        CHECK(ResamplePlan::ratio_of(r, kOutRate, L, M, T) == SAME_OK);
        std::printf("plan %u %u %u %u\n", r, L, M, T);
        ResamplePlan one;
        CHECK(one.init(1, &r, kOutRate) == SAME_OK);
        CHECK(one.taps.size() == (size_t)T * L && one.ratio(0).T == T);
        write_file("taps_" + std::to_string(r) + ".f32", one.taps);
        std::printf("delay %u %.9f\n", r, one.delay(0));
    }
    {
        const uint32_t r = 192000;
        ResamplePlan p;
        const int rc = p.init(1, &r, kOutRate);
        CHECK(p.n_channels() == 0);
        std::printf("erate %u %d\n", r, rc);
        std::vector<uint32_t> many;
        for (uint32_t i = 0; i < 17; ++i) many.push_back(8000 + 100 * i);
        CHECK(p.init(16, many.data(), kOutRate) == SAME_OK);
        std::printf("ratios17 %d\n", p.init(17, many.data(), kOutRate));
    }

    streams<float>("f32", seed);
    streams<int16_t>("i16", seed + 1);

    // clocks at 2^40 source samples: the positions are 64-bit through and through
    {
        std::mt19937 rng(seed + 2);
        Runner<float> run(std::vector<uint32_t>(kRates, kRates + kNRates));
        for (uint32_t c = 0; c < kNRates; ++c) {
            const rs::Ratio &r = run.plan.ratio(c);
            run.plan.n_in[c] = (1ull << 40) + c;
            run.plan.n_out[c] = rs::outputs_after(run.plan.n_in[c], r.L, r.M);
        }
        run.feed(2000, rng);
        run.dump("far");
        for (uint32_t c = 0; c < kNRates; ++c) CHECK(run.plan.n_in[c] == (1ull << 40) + c + 2000);
    }
    std::printf("OK\n");
    return 0;
}
