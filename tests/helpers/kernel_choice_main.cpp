// kernel_choice_main.cpp -- prints the kernel choice of same_select.cpp over a grid of configurations, one row per case
// (tests/test_kernel_choice_cpu.py compares the output with tests/golden/kernel_choice.txt).  Host-only: built with
// g++ -fsanitize=address,undefined from this file, same_select.cpp and same_config.cpp.
//
// A row: rate channels flags variation | block kernels, relaxed, relaxed in ordinary launches (0 / 1 each) and the kernel named
// before the first launch | the ordinary launch's kernel : block length (0: none) | tm: time-major calls with max_chunks = 0 (default), 2,
// 8, 16 -- the pieces a long call is cut into, then kernel and block length, or "-" where it is not cut | cm: channel-major calls
// read where they lie (22.05 kHz), the column cap and the same four | on the rows without flags (x on tp rows too), the
// families' form selectors: f fast built, m mirror, d dense, b block; l pipeline lanes, s stages, h share, p split, r FASTMATH
// built; y sym built; w wave built, k duo, x solo-wide.
// Kernels: G<B> demod_kernel<B>, F demod_fast_kernel, P demod_pipe_kernel, PF demod_pipe_kernel<fastmath>, S demod_sym_kernel,
// W demod_relaxed_kernel.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sameold_amd/csrc/same_config.h"
#include "../../sameold_amd/csrc/same_select.h"

namespace {

struct Flags { const char *name; bool relaxed, time_parallel, generic; };
const Flags kFlags[] = {{"none", false, false, false}, {"relaxed", true, false, false}, {"tp", false, true, false},
                        {"tp+relaxed", true, true, false}, {"generic", false, false, true}};
enum : unsigned { kNone = 1, kRelaxed = 2, kTp = 4, kBoth = 8, kGeneric = 16 };      // bit i: kFlags[i]

// one change to the default builder, Params' knobs or the batch's knobs (named by the SAME_... environment variable that sets it)
struct Variation {
    const char *name;
    unsigned flags;      // the flag sets it bears on
    void (*builder)(same_rx_builder &);
    void (*knobs)(same::Params &, same::Request &);
};
const Variation kVariations[] = {
    {"base", kNone | kRelaxed | kTp | kBoth | kGeneric, nullptr, nullptr},
    {"eq-off", kNone | kRelaxed | kBoth, [](same_rx_builder &b) { b.equalizer = false; }, nullptr},
    {"eq-8+4", kNone | kRelaxed, [](same_rx_builder &b) { b.eq_nfeedforward = 8; }, nullptr},
    {"agc-min--0", kNone | kRelaxed, [](same_rx_builder &b) { b.agc_gain_limits[0] = -0.0f; }, nullptr},
    {"agc-min--1", kNone | kRelaxed, [](same_rx_builder &b) { b.agc_gain_limits[0] = -1.0f; }, nullptr},
    {"SYM=0", kRelaxed | kBoth, nullptr, [](same::Params &P, same::Request &) { P.knob_sym = -1; }},
    {"PIPE=0", kNone | kTp, nullptr, [](same::Params &P, same::Request &) { P.knob_pipe = -1; }},
    {"PIPE=1", kNone | kTp, nullptr, [](same::Params &P, same::Request &) { P.knob_pipe = 1; }},
    {"PIPE_LANES=16", kNone, nullptr, [](same::Params &P, same::Request &) { P.knob_pipe_lanes = 16; }},
    {"PIPE_SPLIT=0", kNone, nullptr, [](same::Params &P, same::Request &) { P.knob_pipe_split = -1; }},
    {"FAST_DENSE=1", kNone, nullptr, [](same::Params &P, same::Request &) { P.knob_fast_dense = 1; }},
    {"RELAXED=0", kRelaxed | kTp, nullptr, [](same::Params &, same::Request &rq) { rq.knob_relaxed = -1; }},
    {"RELAXED=1", kNone | kTp, nullptr, [](same::Params &, same::Request &rq) { rq.knob_relaxed = 1; }},
    {"RELAXED_KERNEL=solo", kRelaxed | kBoth, nullptr, [](same::Params &P, same::Request &) { P.knob_relaxed_kernel = 1; }},
    {"RELAXED_KERNEL=duo", kRelaxed | kBoth, nullptr, [](same::Params &P, same::Request &) { P.knob_relaxed_kernel = 2; }},
    {"TP_KERNEL=wave", kTp | kBoth, nullptr, [](same::Params &, same::Request &rq) { rq.knob_tp_kernel = 2; }},
    {"TP_KERNEL=pipe", kTp | kBoth, nullptr, [](same::Params &, same::Request &rq) { rq.knob_tp_kernel = 1; }},
    {"SYM_MAX=32768", kRelaxed | kBoth, nullptr, [](same::Params &, same::Request &rq) { rq.sym_max_channels = 32768u; }},
};

const uint32_t kRates[] = {22050u, 44100u, 48000u};
// rates without block kernels, where no threshold applies: a few channel counts across the range
const uint32_t kOtherRates[] = {11025u, 32000u};
const uint32_t kOtherChannels[] = {1u, 64u, 4112u, 65536u, 1u << 22};
// every threshold of the choice with its neighbour on each side of the 16- / 64-divisibility rules
const uint32_t kChannels[] = {1u, 16u, 48u, 64u, 100u, 4096u, 4112u, 8192u, 8256u, 16384u, 16448u, 32768u, 32832u, 49152u,
                              65536u, 65600u, 131072u, 262144u, 1u << 22};
// the variations run at 22.05 kHz, where every family is built, on these
const uint32_t kVarChannels[] = {16u, 64u, 100u, 4096u, 4112u, 8192u, 8256u, 16384u, 16448u, 32768u, 32832u, 65536u, 65600u, 262144u};
const uint32_t kMaxChunks[] = {0u, 2u, 8u, 16u};

struct Cut { uint32_t pieces = 1; const char *name = "-"; uint32_t block_len = 0; };
// the table's short form of a kernel name
std::string abbr(const char *name)
{
    const std::string n(name);
    if (n == "demod_fast_kernel") return "F";
    if (n == "demod_pipe_kernel") return "P";
    if (n == "demod_pipe_kernel<fastmath>") return "PF";
    if (n == "demod_sym_kernel") return "S";
    if (n == "demod_relaxed_kernel") return "W";
    if (n.rfind("demod_kernel<B=", 0) == 0) return "G" + n.substr(15, n.size() - 16);
    return n;
}
struct Row {
    bool block_kernels, relaxed, relaxed_plain;
    const char *first_name, *plain_name;
    uint32_t plain_block;
    Cut tm[4], cm[4];
    uint32_t cm_cap;
    // forms
    uint32_t fast_ok, mirror, dense, fast_block, lanes, stages, share, split, pipe_fm, sym, wave, wave_kind, wave_wide;
};

// the pieces a long call is cut into: the first candidate from k_max down (every candidate's geometry fits a long call)
Cut long_call_cut(const same::Params &P, const same::Mode &m, const same::Request &rq, uint32_t max_chunks, uint32_t column_cap, bool channel_major)
{
    const same::TpRule r = same::tp_rule(P, m, rq, max_chunks, column_cap, channel_major);
    for (uint32_t K = r.k_max; K >= 2u; --K) {
        same::Choice c;
        if (same::tp_candidate(P, r, K, c)) return Cut{K, same::family_name(c.family, P.block_len), c.block_len};
    }
    return Cut{};
}

Row evaluate(const same::Params &P, const same::Request &rq)
{
    Row w{};
    const same::Mode m = same::select_mode(P, rq);
    w.block_kernels = m.block_kernels; w.relaxed = m.relaxed; w.relaxed_plain = m.relaxed_plain;
    w.first_name = same::family_name(same::strict_family(P, m), P.block_len);
    const same::Choice plain = same::select_plain(P, m, rq);
    w.plain_name = same::family_name(plain.family, P.block_len);
    w.plain_block = plain.block_len;
    w.cm_cap = 0;
    for (int i = 0; i < 4; ++i) {
        w.tm[i] = long_call_cut(P, m, rq, kMaxChunks[i], same::kTpColumnCap, false);
        if (P.ntaps == 42u) {
            w.cm_cap = same::tp_native_column_cap(P, m, 0u);
            w.cm[i] = long_call_cut(P, m, rq, kMaxChunks[i], same::tp_native_column_cap(P, m, kMaxChunks[i]), true);
        }
    }
    w.fast_ok = same::fast_kernel_supported(P);
    w.mirror = same::fast_use_mirror(P); w.dense = same::fast_use_dense(P); w.fast_block = same::fast_block_len(P);
    w.lanes = same::pipe_workgroup_channels(P); w.stages = same::pipe_kernel_stages(P);
    w.share = same::pipe_share(P); w.split = same::pipe_split(P, w.share != 0u);
    w.pipe_fm = same::pipe_relaxed_supported(same::fm_params(P));
    w.sym = same::sym_kernel_supported(P);
    w.wave = same::relaxed_kernel_supported(P); w.wave_kind = same::relaxed_kernel_kind(P); w.wave_wide = same::relaxed_solo_wide(P);
    return w;
}

void print_cuts(const Cut *cuts)
{
    for (int i = 0; i < 4; ++i) {
        if (cuts[i].pieces < 2u) std::printf(" -");
        else std::printf(" %u%s%u", cuts[i].pieces, abbr(cuts[i].name).c_str(), cuts[i].block_len);
    }
}

int run_case(uint32_t rate, uint32_t channels, const Flags &f, const Variation &v)
{
    same_rx_builder b{};
    same::builder_defaults(b, rate);
    if (v.builder) v.builder(b);
    same::Params P{};
    std::vector<float> taps;
    const int rc = same::derive_params(b, channels, P, taps);
    if (rc) { std::fprintf(stderr, "derive_params failed: %d\n", rc); return 1; }
    same::Request rq;
    rq.relaxed = f.relaxed; rq.time_parallel = f.time_parallel; rq.generic = f.generic;
    if (v.knobs) v.knobs(P, rq);
    P.ticks = f.time_parallel ? 0u : 1u;      // as same_batch_new sets it (no SAME_BATCH_LINK_ONLY)
    const Row w = evaluate(P, rq);
    std::printf("%u %u %s %s|%d%d%d %s|%s:%u", rate, channels, f.name, v.name, (int)w.block_kernels, (int)w.relaxed,
                (int)w.relaxed_plain, abbr(w.first_name).c_str(), abbr(w.plain_name).c_str(), w.plain_block);
    if (f.time_parallel) {
        std::printf("|tm");
        print_cuts(w.tm);
        if (P.ntaps == 42u) { std::printf("|cm %u", w.cm_cap); print_cuts(w.cm); }
    }
    if (f.time_parallel && !f.relaxed) std::printf("|x%u", w.wave_wide);      // (the one selector that reads Params::ticks)
    if (!f.relaxed && !f.generic && !f.time_parallel)
        std::printf("|f%u m%u d%u b%u l%u s%u h%u p%u r%u y%u w%u k%u x%u", w.fast_ok, w.mirror, w.dense, w.fast_block, w.lanes, w.stages,
                    w.share, w.split, w.pipe_fm, w.sym, w.wave, w.wave_kind, w.wave_wide);
    std::printf("\n");
    return 0;
}

}  // namespace

int main()
{
    int bad = 0;
    for (uint32_t rate : kRates)
        for (uint32_t c : kChannels)
            for (const Flags &f : kFlags) bad |= run_case(rate, c, f, kVariations[0]);
    for (uint32_t rate : kOtherRates)
        for (uint32_t c : kOtherChannels)
            for (const Flags &f : kFlags) bad |= run_case(rate, c, f, kVariations[0]);
    for (size_t vi = 1; vi < sizeof(kVariations) / sizeof(kVariations[0]); ++vi)
        for (uint32_t c : kVarChannels)
            for (size_t fi = 0; fi < sizeof(kFlags) / sizeof(kFlags[0]); ++fi)
                if (kVariations[vi].flags & (1u << fi)) bad |= run_case(22050u, c, kFlags[fi], kVariations[vi]);
    return bad;
}
