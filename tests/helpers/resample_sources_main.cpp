// Host-only driver of the mixed-rate resampler's per-source calls (same_resampler_process_device_sources): the plan
// (sameold_amd/csrc/same_resample_plan.h) and the per-source arithmetic of same_resample_dev.h, for
// tests/test_resample_sources_cpu.py under ASan + UBSan.  It runs a per-source call the way same_resample.hip does -- the
// entry point's checks, describe, clear the reset channels' histories, source_resample_kernel's tiles of 64 channels x 64 rows
// (every channel's rows into the tile with lane = row, then the tile's rows into y masked by each channel's count), the
// history behind the call, commit -- with every channel's samples of every call in a heap block of its own of exactly
// in_count samples, so that a load one sample before or behind a source is a sanitizer report.  Time-major calls (lane_rows,
// as tests/helpers/resample_plan_main.cpp runs them) can be mixed in on the same plan and history.
//
//     resample_sources_main OUT_DIR SEED
// stdout: "stream TAG CHANNEL RATE N_IN N_OUT" per written stream, "phases N" (lane phases compared with phase_of), "OK" at the
// end.  Files: TAG_cCHANNEL_x.f32 | _x.i16 and TAG_cCHANNEL_y.f32.
#include "../../sameold_amd/csrc/same_resample_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
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
static const uint32_t kTileCh = 64, kTileRows = 64, kTilePitch = 65;          // source_resample_kernel's

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

template <typename SampleT>
struct Runner {
    ResamplePlan plan;
    std::vector<float> hist;                             // [rs::kHistRows x C]
    std::vector<std::vector<SampleT>> xlog;
    std::vector<std::vector<float>> ylog;
    std::vector<uint64_t> out_sum;
    uint32_t source_calls = 0, matrix_calls = 0, short_calls = 0, first_rows_from_history = 0, partial_blocks = 0;

    explicit Runner(const std::vector<uint32_t> &rates)
    {
        CHECK(plan.init((uint32_t)rates.size(), rates.data(), kOutRate) == SAME_OK);
        CHECK(plan.taps_t.size() == plan.taps.size());
        for (const rs::Ratio &r : plan.ratios)             // the [j][p] copy is the [p][j] table, value for value
            for (uint32_t p = 0; p < r.L; ++p)
                for (uint32_t j = 0; j < r.T; ++j) {
                    const float a = plan.taps[r.tap_off + (size_t)p * r.T + j], b = plan.taps_t[r.tap_off + (size_t)j * r.L + p];
                    CHECK(a == b);
                }
        // (garbage: the first call must clear every column)
        hist.assign((size_t)rs::kHistRows * rates.size(), std::numeric_limits<float>::quiet_NaN());
        xlog.resize(rates.size()); ylog.resize(rates.size()); out_sum.assign(rates.size(), 0);
    }
    void forget() { for (auto &v : xlog) v.clear(); for (auto &v : ylog) v.clear(); out_sum.assign(out_sum.size(), 0); }

    void clear_histories(const std::vector<rs::Desc> &desc)
    {
        const uint32_t C = plan.n_channels();
        for (uint32_t c = 0; c < C; ++c)
            if (desc[c].clear)
                for (uint32_t i = 0; i < rs::kHistRows; ++i) hist[(size_t)i * C + c] = 0.0f;
    }
    void collect(const std::vector<float> &y, uint32_t max_out, const std::vector<uint32_t> &out)
    {
        const uint32_t C = plan.n_channels();
        for (uint32_t c = 0; c < C; ++c) {
            for (uint32_t n = 0; n < max_out; ++n) {
                const float v = y[(size_t)n * C + c];
                if (n < out[c]) ylog[c].push_back(v);
                else CHECK(v == kSentinel);                  // rows at or beyond out_counts[c] are never written
            }
            out_sum[c] += out[c];
        }
    }

    // same_resampler_process_device_sources
    void call_sources(const std::vector<uint32_t> &in_counts, std::mt19937 &rng)
    {
        const uint32_t C = plan.n_channels();
        std::vector<std::unique_ptr<SampleT[]>> block(C);
        std::vector<const SampleT *> src(C, nullptr);        // NULL where the count is zero
        for (uint32_t c = 0; c < C; ++c) {
            if (in_counts[c] == 0) continue;
            block[c].reset(new SampleT[in_counts[c]]);
            for (uint32_t t = 0; t < in_counts[c]; ++t) {
                block[c][t] = noise(rng, SampleT());
                xlog[c].push_back(block[c][t]);
            }
            src[c] = block[c].get();
        }
        for (uint32_t c = 0; c < C; ++c) CHECK(in_counts[c] == 0 || (src[c] && (uintptr_t)src[c] % sizeof(SampleT) == 0));
        std::vector<uint32_t> out(C, 0);
        uint32_t max_out = 0;
        CHECK(plan.out_counts(in_counts.data(), 0xffffffffu, out.data(), &max_out) == SAME_OK);
        std::vector<rs::Desc> desc(C);
        plan.describe(in_counts.data(), out.data(), desc.data());
        std::vector<float> y((size_t)max_out * C, kSentinel);
        clear_histories(desc);
        // source_resample_kernel
        std::vector<float> tile((size_t)kTileRows * kTilePitch);
        for (uint32_t c0 = 0; c0 < C; c0 += kTileCh) {
            uint32_t tile_out = 0;
            for (uint32_t ch = 0; ch < kTileCh && c0 + ch < C; ++ch) tile_out = desc[c0 + ch].out_count > tile_out ? desc[c0 + ch].out_count : tile_out;
            for (uint32_t row0 = 0; row0 < tile_out; row0 += kTileRows) {
                tile.assign(tile.size(), std::numeric_limits<float>::quiet_NaN());
                for (uint32_t ch = 0; ch < kTileCh && c0 + ch < C; ++ch) {
                    const rs::Desc &d = desc[c0 + ch];
                    if (row0 >= d.out_count) continue;
                    const uint32_t left = d.out_count - row0;
                    const rs::Ratio &r = plan.ratios[d.ratio];
                    rs::source_rows(d, r, plan.taps_t.data(), src[c0 + ch], hist.data() + c0 + ch, C, tile.data() + ch, kTilePitch, row0,
                                    row0 + (left < kTileRows ? left : kTileRows), 0u, 1u);
                    if (left < kTileRows) ++partial_blocks;
                    if (row0 == 0 && r.T > 1 && rs::phase_of(d.n_out, r.L, r.M).k - d.n_in + 1 < r.T) ++first_rows_from_history;
                }
                for (uint32_t r = 0; r < kTileRows; ++r)
                    for (uint32_t ch = 0; ch < kTileCh && c0 + ch < C; ++ch)
                        if (row0 + r < desc[c0 + ch].out_count) y[(size_t)(row0 + r) * C + c0 + ch] = tile[(size_t)r * kTilePitch + ch];
            }
        }
        // source_history_kernel
        for (uint32_t c = 0; c < C; ++c) {
            const uint32_t T = plan.ratios[desc[c].ratio].T;
            rs::update_history_source(hist.data() + c, C, T, src[c], desc[c].in_count);
            if (T > 1 && desc[c].in_count && desc[c].in_count < T - 1) ++short_calls;
        }
        plan.commit(in_counts.data(), out.data());
        collect(y, max_out, out);
        ++source_calls;
    }

    // same_resampler_process_device: time-major [n_rows x C], blank behind every channel's count
    void call_matrix(size_t n_rows, const std::vector<uint32_t> &in_counts, std::mt19937 &rng)
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
        clear_histories(desc);
        for (uint32_t c = 0; c < C; ++c) {
            const rs::Ratio &r = plan.ratios[desc[c].ratio];
            for (uint32_t row0 = 0; row0 < desc[c].out_count; row0 += 64) {
                const uint32_t left = desc[c].out_count - row0;
                rs::lane_rows(desc[c], r, plan.taps.data(), x.data() + c, C, hist.data() + c, C, y.data() + c, C, row0, row0 + (left < 64 ? left : 64));
            }
        }
        for (uint32_t c = 0; c < C; ++c) {
            const uint32_t T = plan.ratios[desc[c].ratio].T;
            if (desc[c].in_count == 0 || T == 1) continue;
            rs::update_history(hist.data() + c, C, T, x.data() + c, C, desc[c].in_count);
        }
        plan.commit(in_counts.data(), out.data());
        collect(y, max_out, out);
        ++matrix_calls;
    }

    // feed every channel `total` more samples in random calls: long ones, empty ones, and runs of calls of 0, 1 and a few
    // samples (fewer than T - 1: the history shifts) several in a row.  mixed: each call is of either kind at random.
    void feed(uint32_t total, std::mt19937 &rng, bool mixed)
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
            if (mixed && rng() % 2) call_matrix(n_rows, k, rng);
            else call_sources(k, rng);
        }
    }

    void dump(const char *tag)
    {
        for (uint32_t c = 0; c < plan.n_channels(); ++c) {
            const rs::Ratio &r = plan.ratio(c);
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
static void streams(const std::string &tag, uint32_t seed)
{
    std::mt19937 rng(seed);
    Runner<SampleT> run(std::vector<uint32_t>(kRates, kRates + kNRates));
    run.feed(6000, rng, false);
    CHECK(run.matrix_calls == 0 && run.short_calls > 50 && run.first_rows_from_history > 50 && run.partial_blocks > 50);
    run.dump(tag.c_str());
    for (uint32_t c = 0; c < kNRates; ++c) CHECK(run.plan.n_in[c] == 6000);

    // resets between per-source calls: channels 0 and 3 take new sources (8 kHz: a ratio the plan has; 12 kHz: a new one),
    // channel 5 restarts at its rate
    const uint32_t chans[2] = {0, 3}, rates[2] = {8000, 12000}, keep[1] = {5};
    CHECK(run.plan.reset(chans, 2, rates) == SAME_OK);
    CHECK(run.plan.reset(keep, 1, nullptr) == SAME_OK);
    CHECK(run.plan.n_in[0] == 0 && run.plan.n_out[3] == 0 && run.plan.n_in[5] == 0 && run.plan.n_in[1] == 6000);
    CHECK(run.plan.ratios.size() == kNRates + 1 && run.plan.taps_t.size() == run.plan.taps.size());
    run.forget();
    run.feed(1500, rng, false);
    run.dump((tag + "reset").c_str());
}

template <typename SampleT>
static void mixed(const std::string &tag, uint32_t seed)
{
    std::mt19937 rng(seed);
    Runner<SampleT> run(std::vector<uint32_t>(kRates, kRates + kNRates));
    run.feed(6000, rng, true);
    CHECK(run.matrix_calls > 10 && run.source_calls > 10);
    run.dump(tag.c_str());
}

int main(int argc, char **argv)
{
    CHECK(argc == 3);
    g_dir = argv[1];
    const uint32_t seed = (uint32_t)std::strtoul(argv[2], nullptr, 10);

    // the 32-bit per-lane phase is phase_of, at small clocks and at clocks of 2^40 source samples
    {
        std::mt19937_64 rng(seed + 9);
        uint64_t n_checked = 0;
        for (uint32_t rate : kRates) {
            uint32_t L = 0, M = 0, T = 0;
            CHECK(ResamplePlan::ratio_of(rate, kOutRate, L, M, T) == SAME_OK);
            CHECK(L + 63ull * M < (1ull << 19));
            for (int t = 0; t < 400; ++t) {
                const uint64_t n_in = t < 100 ? (uint64_t)t : t < 250 ? (1ull << 40) + rng() % 100000 : rng() % (1ull << 41);
                const uint64_t n = rs::outputs_after(n_in, L, M) + rng() % 3;
                const rs::Phase ph0 = rs::phase_of(n, L, M);
                for (uint32_t i = 0; i < 64; ++i) {
                    const rs::Phase a = rs::lane_phase(ph0, i, L, M), b = rs::phase_of(n + i, L, M);
                    CHECK(a.k == b.k && a.p == b.p);
                    ++n_checked;
                }
            }
        }
        std::printf("phases %llu\n", (unsigned long long)n_checked);
    }

    streams<float>("f32", seed);
    streams<int16_t>("i16", seed + 1);
    mixed<float>("f32mixed", seed + 3);
    mixed<int16_t>("i16mixed", seed + 4);

    // clocks at 2^40 source samples
    {
        std::mt19937 rng(seed + 2);
        Runner<float> run(std::vector<uint32_t>(kRates, kRates + kNRates));
        for (uint32_t c = 0; c < kNRates; ++c) {
            const rs::Ratio &r = run.plan.ratio(c);
            run.plan.n_in[c] = (1ull << 40) + c;
            run.plan.n_out[c] = rs::outputs_after(run.plan.n_in[c], r.L, r.M);
        }
        run.feed(2000, rng, false);
        run.dump("far");
        for (uint32_t c = 0; c < kNRates; ++c) CHECK(run.plan.n_in[c] == (1ull << 40) + c + 2000);
    }
    std::printf("OK\n");
    return 0;
}
