// tp_plan_main.cpp -- prints how same_tp_plan.cpp cuts a call over a grid of configurations and call lengths, one row per
// case (tests/test_tp_plan_cpu.py compares the output with tests/golden/tp_plan.txt; tests/test_tp_plan_gpu.py reads the
// library's answers against the same rows).  Host-only: built with g++ -fsanitize=address,undefined from this file,
// same_tp_plan.cpp, same_select.cpp and same_config.cpp.
//
// A row, key=value fields: r rate, c channels, a arithmetic (strict: SAME_RELAXED=0; rel: a time-parallel batch as created),
// cfg SAME_TP_KERNEL / max_chunks / min_own / warmup / SAME_TP_SORT / SAME_TP_PLAN_STREAM, l layout (tm, cm), n samples, b the
// base address's low bits, why this length | the uniform cut: k pieces (1: not cut; then plain, the kernel the call runs) by
// kern in blocks of fb, st stride / wb warm-up / nom nominal blocks, pc PipeChunks' pieces x channels, c0 counter0 | a
// time-parallel launch's output: on samples it is sized for, ev events, bu bursts, bins, sw sort words | cm rows: q qualifies
// (0: every other field of the record is zero, which the driver checks), wh whole samples, ws second warm-up, sc scout blocks,
// in pitch, sort mode / pair groups / lpt, hist floats (0: no scratch), ef energy floats, w the geometry words own_start,row0,
// nominal,perm,wg,wg2,perm2,total,harvest, side planning beside the previous launch on the library's own stream.
#include <cstdio>
#include <cstdlib>
#include <vector>

#ifndef TP_PLAN_HEADER
#define TP_PLAN_HEADER "../../sameold_amd/csrc/same_tp_plan.h"
#endif
#include TP_PLAN_HEADER

namespace {

struct Config {
    uint32_t rate = 22050, channels = 64;
    bool strict = false;
    int tp_kernel = 0;      // 0 unset, 1 pipe, 2 wave
    same::TpConfig tp;
    bool channel_major = false;
};
struct Derived { same::Params P{}; same::Request rq; same::Mode mode; };
bool ok = true;

Derived derive(const Config &c)
{
    Derived d;
    same_rx_builder b{};
    same::builder_defaults(b, c.rate);
    std::vector<float> taps;
    if (same::derive_params(b, c.channels, d.P, taps)) { std::fprintf(stderr, "derive_params failed\n"); std::exit(1); }
    d.P.ticks = 0u;      // as same_batch_new sets it for a time-parallel batch
    d.rq.time_parallel = true; d.rq.knob_relaxed = c.strict ? -1 : 0; d.rq.knob_tp_kernel = c.tp_kernel;
    d.mode = same::select_mode(d.P, d.rq);
    return d;
}

same::TpCut cut_of(const Config &c, const Derived &d, size_t n, uint64_t counter0)
{
    return c.channel_major ? same::tp_native_cut(d.P, d.mode, d.rq, c.tp, n, counter0)
                           : same::tp_uniform_cut(d.P, d.mode, d.rq, c.tp, n, counter0);
}

// the smallest call that is cut at all (a piece's conditions only ease as the call grows), 0: none up to the launch cap
size_t smallest_cut(const Config &c, const Derived &d)
{
    size_t hi = c.channel_major ? same::kMaxLaunchSamples : same::max_launch_samples(c.rate), lo = 0;
    if (cut_of(c, d, hi, 0).n_chunks < 2u) return 0;
    while (hi - lo > 1) {      // (lo is not cut, hi is)
        const size_t mid = lo + (hi - lo) / 2;
        (cut_of(c, d, mid, 0).n_chunks < 2u ? lo : hi) = mid;
    }
    return hi;
}

// prints the row; returns q of a channel-major row (-1: a time-major row)
int row(const Config &c, size_t n, const char *why, unsigned base_low = 0, uint64_t counter0 = 0)
{
    static const char *const kTpk[] = {"-", "pipe", "wave"};
    const Derived d = derive(c);
    const uintptr_t base = 0x7f0000000000ull + base_low;
    const same::TpCut cut = cut_of(c, d, n, counter0);
    std::printf("r=%u c=%u a=%s cfg=%s/%u/%u/%u/%d/%d l=%s n=%zu b=%u why=%s", c.rate, c.channels, c.strict ? "strict" : "rel", kTpk[c.tp_kernel],
                c.tp.max_chunks, c.tp.min_own, c.tp.warmup, c.tp.sort_mode, c.tp.knob_plan_stream, c.channel_major ? "cm" : "tm", n, base_low, why);
    if (cut.n_chunks > 1u)
        std::printf(" | k=%u kern=%s fb=%u st=%u wb=%u nom=%u pc=%ux%u c0=%llu", cut.n_chunks, same::family_name(cut.choice.family, d.P.block_len),
                    cut.geom.block_len, cut.geom.stride_blocks, cut.geom.warmup_blocks, cut.pc.nominal_blocks, cut.pc.n_chunks, cut.pc.in_channels,
                    (unsigned long long)cut.geom.counter0);
    else {
        std::printf(" | k=1 plain=%s", same::family_name(same::select_plain(d.P, d.mode, d.rq).family, d.P.block_len));
        ok &= !cut.geom.block_len && !cut.geom.stride_blocks && !cut.geom.warmup_blocks && !cut.geom.counter0 && !cut.pc.nominal_blocks && !cut.pc.in_channels;
    }
    const same::TpNative np = c.channel_major ? same::tp_native_plan(d.P, c.tp, cut, n, base) : same::TpNative{};
    // the launch's output: a time-parallel launch's (the native one sizes it for its whole blocks), else the ordinary launch's
    const bool tp_launch = cut.n_chunks > 1u && (!c.channel_major || np.qualifies);
    const size_t out_n = tp_launch ? same::tp_output_samples(np.qualifies ? np.whole_samples : n, cut.pc, cut.geom.block_len) : n;
    // (an ordinary launch's capacities: the caps rows at the end)
    if (tp_launch) {
        const same::OutputCaps o = same::output_caps(d.P, out_n, cut.n_chunks * d.P.n_channels, false, false, 0, 0);
        std::printf(" | on=%zu ev=%zu bu=%zu bins=%zu sw=%zu", out_n, o.events, o.bursts, o.bins, o.sort_words);
    }
    const same::TpGeomWords &w = np.words;
    if (np.qualifies)
        std::printf(" | q=1 wh=%u ws=%u sc=%u in=%llu sort=%d/%d/%d hist=%zu ef=%zu w=%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu side=%d%d", np.whole_samples,
                    np.warmup_samples, np.scout_blocks, (unsigned long long)np.in_samples, np.sort_mode, (int)np.pair_groups, (int)np.lpt,
                    np.hist_floats, np.energy_floats, w.own_start, w.row0, w.nominal, w.perm, w.wg, w.wg2, w.perm2, w.total, w.harvest,
                    (int)same::tp_plan_beside(c.tp, true), (int)same::tp_plan_beside(c.tp, false));
    else if (c.channel_major) {
        std::printf(" | q=0");
        ok &= !np.whole_samples && !np.warmup_samples && !np.scout_blocks && !np.in_samples && !np.sort_mode && !np.pair_groups && !np.lpt &&
              !np.need_hist && !np.hist_floats && !np.energy_floats && !w.row0 && !w.nominal && !w.perm && !w.wg && !w.wg2 && !w.perm2 && !w.total && !w.harvest;
    }
    ok &= np.need_hist == (np.hist_floats != 0);
    std::printf("\n");
    return c.channel_major ? (int)np.qualifies : -1;
}
// a row on one side of a qualification limit: it must (q = 1) or must not (q = 0) qualify, else the pair does not show the limit
void limit_row(int q, const Config &c, size_t n, const char *why, unsigned base_low = 0, uint64_t counter0 = 0)
{
    if (row(c, n, why, base_low, counter0) == q) return;
    std::fprintf(stderr, "limit row %s n=%zu: q is not %d\n", why, n, q);
    ok = false;
}

// the rows of one configuration: the smallest call that is cut and the one a sample shorter, and the headline length (10 s)
void config_rows(const Config &c, bool headline = true)
{
    const size_t n_min = smallest_cut(c, derive(c));
    if (n_min) { row(c, n_min, "min"); row(c, n_min - 1, "min-1"); }
    if (headline || !n_min) row(c, (size_t)c.rate * 10, n_min ? "10s" : "10s-never-cut");
}
Config config(uint32_t rate, uint32_t ch, bool strict, bool cm, int tp_kernel = 0, uint32_t max_chunks = 0)
{
    Config c; c.rate = rate; c.channels = ch; c.strict = strict; c.channel_major = cm; c.tp_kernel = tp_kernel; c.tp.max_chunks = max_chunks;
    return c;
}

const uint32_t kChannels[] = {16u, 48u, 64u, 65u, 256u, 4096u, 16384u, 16448u, 32768u, 65536u, 131072u};

}  // namespace

int main()
{
    // every channel count at the standard rates, both arithmetics; both layouts at 22.05 kHz (a channel-major call is read
    // where it lies there only: elsewhere, and at a rate without block kernels, a few channel counts)
    for (uint32_t rate : {22050u, 44100u, 48000u})
        for (uint32_t ch : kChannels)
            for (int strict = 0; strict < (rate == 44100u ? 1 : 2); ++strict)
                for (int cm = 0; cm < (rate == 22050u || (ch == 4096u && !strict) ? 2 : 1); ++cm) config_rows(config(rate, ch, strict, cm));
    for (uint32_t ch : {64u, 4096u, 65536u})
        for (int cm = 0; cm < 2; ++cm) config_rows(config(32000u, ch, false, cm));
    // SAME_TP_KERNEL
    for (uint32_t ch : {64u, 16384u, 65536u})
        for (int k = 1; k <= 2; ++k)
            for (int strict = 0; strict < (ch == 64u ? 2 : 1); ++strict)
                for (int cm = 0; cm < 2; ++cm) config_rows(config(22050u, ch, strict, cm, k), false);
    for (int k = 1; k <= 2; ++k) config_rows(config(48000u, 64u, false, false, k), false);
    // max_chunks
    for (uint32_t mk : {2u, 10u, 12u, 63u, 64u}) {
        for (int cm = 0; cm < 2; ++cm) {
            config_rows(config(22050u, 64u, false, cm, 0, mk), false);
            config_rows(config(22050u, 4096u, false, cm, 0, mk), false);
            config_rows(config(22050u, 4096u, true, cm, 0, mk), false);
        }
        config_rows(config(48000u, 256u, false, false, 0, mk), false);
    }
    // a custom min_own and a custom warm-up (the native plan's second warm-up is capped by the uniform one)
    for (int strict = 0; strict < 2; ++strict)
        for (int cm = 0; cm < 2; ++cm)
            for (int which = 0; which < 3; ++which) {
                Config c = config(22050u, 64u, strict, cm);
                if (which != 1) c.tp.min_own = 30000u;
                if (which != 0) c.tp.warmup = which == 1 ? 1000u : 5000u;
                config_rows(c, false);
            }
    // SAME_TP_SORT, within one round of workgroups and beyond; SAME_TP_PLAN_STREAM=0
    for (int sort : {-1, 0, 1, 2})
        for (int which = 0; which < 3; ++which)
            for (uint32_t mk : {0u, 12u}) {
                Config c = config(22050u, which ? 4096u : 64u, which == 2, true, 0, mk);
                c.tp.sort_mode = sort; c.tp.knob_plan_stream = sort == 1 ? -1 : 0;
                row(c, 220500, "10s");
            }
    // the qualification limits of the native plan: on each side of every limit a row that differs in nothing else (limit_row
    // checks that q flips)
    {
        const Config c = config(22050u, 64u, false, true);
        for (size_t n : {220501u, 220502u, 220503u}) limit_row(0, c, n, "n%4");
        limit_row(1, c, 220504, "n%4");
        for (unsigned off : {4u, 8u}) limit_row(0, c, 220500, "base", off, 1000000007ull);
        limit_row(1, c, 220500, "base", 16u, 1000000007ull);
        // 7000 readings of the call's whole blocks (36 samples here), in at most 63 pieces: 6999, 7000, 7000 and 7001 readings
        const size_t sb = same::kScoutBlock;
        const Config m63 = config(22050u, 64u, false, true, 0, 63u);
        for (size_t n : {7000 * sb, 7000 * sb + 252, 7001 * sb}) limit_row(1, m63, n, "7000-readings");
        limit_row(0, m63, 7001 * sb + 72, "7000-readings");
        // (the 2^22 cap is read off k, not q: up to it the call is cut, beyond it tp_native_cut does not cut at all; on either
        // side such a call has more than 7000 readings and does not qualify)
        for (size_t n : {same::kMaxLaunchSamples - 4, same::kMaxLaunchSamples, same::kMaxLaunchSamples + 4}) limit_row(0, c, n, "2^22");
        // 64 readings: 63 (two lengths), then 64 (a short call is cut only with a short warm-up and pieces allowed to be short)
        Config s = c; s.tp.warmup = 512u; s.tp.min_own = 512u; s.tp.max_chunks = 2u;
        for (size_t n : {64 * sb - 4, 64 * sb}) limit_row(0, s, n, "64-readings");
        for (size_t n : {64 * sb + 32, 64 * sb + 36, 64 * sb + 72}) limit_row(1, s, n, "64-readings");
        // 63 pieces and 64 (the one-wavefront kernel never takes more than 63; the strict pipeline of so small a batch does not
        // qualify on its workgroup width)
        for (uint32_t mk : {63u, 64u})
            for (int strict = 0; strict < 2; ++strict)
                for (int k = 0; k <= 2; ++k) {
                    const Config p = config(22050u, 64u, strict, true, k, mk);
                    if (strict) row(p, 1000000, "63-pieces");
                    else limit_row(mk == 63u || k == 2, p, 1000000, "63-pieces");
                }
        // whole groups of 64 channels, in strict arithmetic: 4096 channels qualify, 48 do not
        limit_row(1, config(22050u, 4096u, true, true), 220500, "c%64");
        limit_row(0, config(22050u, 48u, true, true), 220500, "c%64");
        limit_row(0, config(22050u, 4096u, true, true), 220502, "n%4");
    }
    // the rows tests/test_tp_plan_gpu.py runs: 64 channels, a channel-major call within one transposed slab and one two samples longer
    for (uint32_t rate : {22050u, 48000u}) {
        Config c = config(rate, 64u, false, false);
        const size_t n = (smallest_cut(c, derive(c)) + 3) / 4 * 4 + 4096;
        for (int cm = 0; cm < 2; ++cm) { c.channel_major = cm; row(c, n, "tie"); row(c, n + 2, "tie+2"); }
    }
    // the launch cap, and the capacities: ordinary launches with the transport layer and the capture on the device, the clamps
    for (uint32_t rate : {22050u, 44100u, 48000u, 32000u}) std::printf("r=%u max_launch=%zu\n", rate, same::max_launch_samples(rate));
    std::printf("scout_block=%u scan_threads=%u sort_extra(1)=%u sort_extra(1024)=%u sort_extra(1025)=%u span_bytes=%zu\n", same::kScoutBlock,
                same::kScanThreads, same::event_sort_extra_words(1u), same::event_sort_extra_words(1024u), same::event_sort_extra_words(1025u), same::kSpanBytes);
    struct CapCase { uint32_t rate, channels; size_t n, columns; bool dev_transport, audio; size_t near_cap, msg_cap; };
    const CapCase caps[] = {
        {22050, 262144, 22050 * 45, 262144, false, false, 0, 0}, {22050, 4096, 22050 * 45, 262144, false, false, 0, 0},
        {48000, 262144, 48000 * 45, 0, true, true, 0, 0},        {48000, 262144, (size_t)1 << 22, 0, true, true, 4096, 0},
        {22050, 64, 44100, 0, true, false, 0, 0},                {22050, 64, 44100, 0, true, true, 0, 0},
        {22050, 64, 44100, 0, true, true, 4096, 100000},         {22050, 32768, 44100, 0, true, true, 0, 0},
        {22050, 32768, 44100, 0, false, true, 0, 0},             {22050, 32768, 1, 0, true, true, 8192, 7},
        {44100, 4096, 441000, 40960, true, true, 0, 0},          {32000, 65, 320000, 0, false, false, 0, 0},
    };
    for (const CapCase &cc : caps) {
        const Derived d = derive(config(cc.rate, cc.channels, false, false));
        const same::OutputCaps o = same::output_caps(d.P, cc.n, cc.columns, cc.dev_transport, cc.audio, cc.near_cap, cc.msg_cap);
        std::printf("caps r=%u c=%u n=%zu columns=%zu transport=%d audio=%d near_cap=%zu msg_cap=%zu | ev=%zu bu=%zu msg=%zu near=%zu sp=%zu bins=%zu sw=%zu\n",
                    cc.rate, cc.channels, cc.n, cc.columns, (int)cc.dev_transport, (int)cc.audio, cc.near_cap, cc.msg_cap, o.events, o.bursts,
                    o.messages, o.near, o.spans, o.bins, o.sort_words);
    }
    if (!ok) std::fprintf(stderr, "a record that should be zero is not\n");
    return ok ? 0 : 1;
}
