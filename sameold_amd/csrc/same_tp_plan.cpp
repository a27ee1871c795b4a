// same_tp_plan.cpp -- how a call is cut (same_tp_plan.h).  Host-only.
#include "same_tp_plan.h"

#include <algorithm>

namespace same {

TpCut tp_uniform_cut(const Params &P, const Mode &m, const Request &rq, const TpConfig &cfg, size_t n, uint64_t counter0,
                     uint32_t column_cap, bool channel_major)
{
    TpCut cut;
    const uint32_t C = P.n_channels;
    const double sps = (double)P.input_rate / 520.83;
    // K pieces of whole blocks of fb samples: a warm-up of 64 symbols in front of every piece but the first, and a piece
    // owns four warm-ups at least -- unless the caller set either
    auto fill = [&](uint32_t K, uint32_t fb) -> bool {
        const uint32_t warm = cfg.warmup ? cfg.warmup : (uint32_t)(64.0 * sps + 0.5);
        const uint32_t WB = (warm + fb - 1u) / fb;
        const uint64_t TB = n / fb;
        if (TB <= WB) return false;
        const uint64_t SB = (TB - WB) / K;
        const uint64_t min_own = cfg.min_own ? cfg.min_own : 4ull * WB * fb;
        if (SB == 0 || SB * fb < min_own) return false;
        cut.geom.counter0 = counter0;
        cut.geom.n_chunks = K; cut.geom.block_len = fb; cut.geom.stride_blocks = (uint32_t)SB; cut.geom.warmup_blocks = WB;
        cut.pc.n_chunks = K; cut.pc.in_channels = C; cut.pc.stride_blocks = (uint32_t)SB; cut.pc.nominal_blocks = (uint32_t)SB + WB;
        return true;
    };
    // the candidates, most pieces first (same_select.h: which batches are cut, into how many pieces at most, by which kernel)
    const TpRule rule = tp_rule(P, m, rq, cfg.max_chunks, column_cap, channel_major);
    for (uint32_t K = rule.k_max; K >= 2u; --K) {
        Choice c;
        if (tp_candidate(P, rule, K, c) && fill(K, c.block_len)) { cut.n_chunks = K; cut.choice = c; return cut; }
    }
    return cut;
}

TpCut tp_native_cut(const Params &P, const Mode &m, const Request &rq, const TpConfig &cfg, size_t n_call, uint64_t counter0)
{
    // 22.05 kHz only: per-lane input streams are read by the sample stage of the 64-channel pipeline forms and by the
    // relaxed kernels; the 44.1 / 48 kHz pipeline reads its input on the DC wavefront, which takes time-major rows only
    // (such a call is transposed on the device and cut uniformly)
    if (n_call > kMaxLaunchSamples || P.ntaps != 42u) return TpCut{};
    // (how many state columns the call may become: tp_native_column_cap, with the measurements behind it)
    return tp_uniform_cut(P, m, rq, cfg, n_call, counter0, tp_native_column_cap(P, m, cfg.max_chunks), true);
}

TpNative tp_native_plan(const Params &P, const TpConfig &cfg, const TpCut &cut, size_t n_call, uintptr_t base)
{
    TpNative np;
    if (cut.n_chunks < 2u) return np;
    const uint32_t C = P.n_channels, columns = cut.n_chunks * C, fb = cut.geom.block_len;
    const Family family = cut.choice.family;
    const bool wave = family == Family::kWaveRelaxed;
    // (the pipeline kernel whatever the column count; the launch's own configuration has it only beyond one round of
    // workgroups: DESIGN.md 4.6, open question)
    const Params Pv = wide_params(P, columns, is_fastmath(family), true);
    // 16-byte loads from every lane's stream (the scout's too: 16-byte aligned base and pitch; the relaxed kernel reads
    // 8 bytes at a time from even rows), full 64-column workgroups, an energy map of 64 to 7000 readings per channel, at
    // most 63 pieces.  What is left of the call behind its last whole block (less than a block) goes through the
    // any-configuration kernel on the channels' own state afterwards.
    const size_t n = n_call - n_call % fb;
    if (n_call % 4 != 0 || (base & 15u) != 0u || n < 64u * (size_t)kScoutBlock || n / kScoutBlock > 7000u || cut.n_chunks > 63u || C % kWave != 0u) return np;
    if (wave ? fb % 2 != 0 : (fb % 4 != 0 || pipe_workgroup_channels(Pv) != (uint32_t)kWave)) return np;
    np.qualifies = true;
    // Warm-up: a per-channel boundary lies in silence, so all a fresh receiver needs before the next burst begins is a
    // full squelch history (32 symbols; the preamble that follows is 128): 40 symbols unless the caller set one
    const double sps = (double)P.input_rate / 520.83;
    const uint32_t warm = cfg.warmup ? cfg.warmup : (uint32_t)(40.0 * sps + 0.5);
    np.warmup_samples = std::min(cut.geom.warmup_blocks, (warm + fb - 1u) / fb) * fb;
    np.whole_samples = (uint32_t)n; np.in_samples = n_call;
    np.scout_blocks = (uint32_t)(n / kScoutBlock);
    np.energy_floats = (size_t)C * np.scout_blocks;
    // pieces sorted by length into workgroups only when the workgroups come in more than one round (the long ones first;
    // SAME_TP_SORT=0 / 1 overrides).  Within one round neither the sorted order nor a long workgroup beside a short one on
    // every CU pays (round 2).
    // SAME_TP_SORT=2 (measurement knob): grid order inside the groups of 64 columns, the groups paired longest with shortest into
    // the symbol-paced pipeline's two-group workgroups, so that a long group runs the second part of its launch alone on its CU
    // (a step is ~12 % shorter there).  One launch by itself: demodulation kernel 1.746 -> 1.706 ms; launches back to back, the
    // way the bench and a stream step: 1.695 -> 1.732 (the shorter tail hides less of the next call's planning) -- not the default.
    np.pair_groups = cfg.sort_mode == 2 && family == Family::kSym;
    np.sort_mode = np.pair_groups ? 0 : (cfg.sort_mode >= 0 ? (cfg.sort_mode ? 1 : 0) : (tp_more_than_one_round(columns) ? 1 : 0));
    // (sorted: the workgroups once more, longest first whatever their group -- those that wait for a free CU are then the short ones)
    np.lpt = np.sort_mode != 0 || np.pair_groups;
    // (a kernel that keeps the squelch's sample history in global memory works on a copy by grid position where the columns are permuted)
    np.need_hist = np.lpt && family == Family::kSym;
    np.hist_floats = np.need_hist ? (size_t)columns * kSquelchHist : 0;
    const size_t groups = columns / kWave;
    TpGeomWords &w = np.words;
    w.own_start = 0; w.row0 = columns; w.nominal = 2 * (size_t)columns; w.perm = 3 * (size_t)columns; w.wg = 4 * (size_t)columns;
    w.wg2 = w.wg + groups; w.perm2 = w.wg2 + 2 * groups;
    w.total = w.perm2 + columns;
    w.harvest = 2 * (size_t)columns;
    return np;
}

OutputCaps output_caps(const Params &P, size_t n_samples, size_t n_columns, bool dev_transport, bool audio, size_t near_cap, size_t msg_cap)
{
    OutputCaps o;
    const size_t n_ch = n_columns ? n_columns : P.n_channels;
    // Worst case per channel: an acquisition attempt (Searching ... NoCarrier) needs a
    // fresh byte sync, i.e. at least 32 symbols, so < 2 link events per 32 symbols; bursts
    // are rarer still.  Size generously: 4 events per 32 symbols + slack.
    const double symbols = (double)n_samples * 520.83 / (double)P.input_rate;
    const size_t per_chan_events = (size_t)(symbols / 8.0) + 16;
    const size_t per_chan_bursts = (size_t)(symbols / 160.0) + 4;   // a burst is >= 20 bytes
    o.events = std::min<size_t>(per_chan_events * n_ch, 0x7fffffffu / sizeof(DevEvent));
    o.bursts = std::min<size_t>(per_chan_bursts * n_ch, 0x7fffffffu / kBurstCap);
    if (dev_transport && !n_columns) {
        // a message needs a burst, except a pending one from an earlier launch and a forced end of message: two per channel more
        o.messages = std::min<size_t>(o.bursts + 2 * n_ch, 0x7fffffffu / sizeof(DevMessage));
        // (a copy of a few kilobytes beside a launch that fills the machine waits for that launch: measured 2.7 ms at the
        // 32 768-channel shard, the host spinning on it; writes into mapped memory need no copy)
        o.near = near_cap ? near_cap : std::max<uint32_t>(4096u, (uint32_t)(n_ch / 4u));
        // a message ends at most one span, a channel's tail or flush adds one: spans past this are lost only when the
        // message log overflows too
        if (audio) o.spans = std::min<size_t>(n_ch + o.near + std::max(msg_cap, o.messages), 0x7fffffffu / kSpanBytes);
    }
    o.bins = n_ch;
    o.sort_words = 2 * n_ch + 1 + event_sort_extra_words((uint32_t)n_ch);
    return o;
}

}  // namespace same
