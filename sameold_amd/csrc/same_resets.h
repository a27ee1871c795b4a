// same_resets.h -- bookkeeping of per-channel resets (same_batch_reset_channels, include/same_rx.h).
//
// A reset of some channels happens at a STREAM position: behind every sample of the calls made before it, ahead of every
// sample of the calls after it.  Its three halves are applied where the stream reaches that position, not when it is asked for:
//   - the device state columns: re-initialised by a small kernel queued in front of the next launch, on that launch's stream;
//   - the host state of the channel (transport layer, time-parallel symbol clock, wake-up instant): once the harvest has
//     replayed the last launch before the position -- that launch may still be running when the reset is asked for;
//   - the sample counter of the channel's queued events: they count from the position on, from the same instant.
// A ragged launch (same_batch_process_*_ragged) leaves some channels behind the batch's counter: their counter bases move by the
// rows they did not consume, with the same two halves (ResetLedger::shift).
// Host-only (no HIP): tests/helpers/reset_ledger_main.cpp and ragged_ledger_main.cpp drive it under ASan + UBSan without a device.
#ifndef SAME_RESETS_H
#define SAME_RESETS_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <vector>

namespace same {

struct ResetLedger {
    // per channel: stream position of its last reset, as the caller sees it (same_batch_channel_input_sample_counter) ...
    std::vector<uint64_t> api_base;
    // ... and as far as the harvest has got: subtracted from the sample counters of the channel's queued events
    std::vector<uint64_t> rec_base;
    // channels whose device state columns are re-initialised in front of the next launch (ascending, unique)
    std::vector<uint32_t> device;
    // per launch slot: channels whose host state is reset, at stream position `pos`, once that slot has been harvested
    struct SlotResets { std::vector<uint32_t> channels; uint64_t pos = 0; };
    SlotResets slot[2];

    void init(uint32_t n_channels)
    {
        api_base.assign(n_channels, 0);
        rec_base.assign(n_channels, 0);
        device.clear();
        for (SlotResets &s : slot) { s.channels.clear(); s.pos = 0; }
        for (SlotShift &h : shift_) { h.channels.clear(); h.by.clear(); h.pos = 0; }
    }
    // the whole batch was reset (same_batch_reset): the stream starts again at 0 for every channel
    void clear() { init((uint32_t)api_base.size()); }

    // `list` as ascending unique channels into `out`; false (and `out` untouched) if one is >= n_channels
    static bool normalise(const uint32_t *list, size_t n, uint32_t n_channels, std::vector<uint32_t> &out)
    {
        for (size_t i = 0; i < n; ++i)
            if (list[i] >= n_channels) return false;
        out.assign(list, list + n);
        std::sort(out.begin(), out.end());
        out.erase(std::unique(out.begin(), out.end()), out.end());
        return true;
    }
    // ascending unique union of `into` and `add` (both ascending unique)
    static void merge(std::vector<uint32_t> &into, const std::vector<uint32_t> &add)
    {
        if (add.empty()) return;
        std::vector<uint32_t> out;
        out.reserve(into.size() + add.size());
        std::set_union(into.begin(), into.end(), add.begin(), add.end(), std::back_inserter(out));
        into.swap(out);
    }

    // A reset of `chans` (ascending unique) at stream position `pos`.  `in_flight_slot`: the slot of the newest launch not yet
    // harvested, or -1 when the harvest has already reached `pos` -- the host half is then due now, and the channels are
    // returned in `host_now` (with their counter base moved) for the caller to reset.
    void request(const std::vector<uint32_t> &chans, uint64_t pos, int in_flight_slot, std::vector<uint32_t> &host_now)
    {
        host_now.clear();
        if (chans.empty()) return;
        merge(device, chans);
        for (uint32_t c : chans) api_base[c] = pos;
        if (in_flight_slot < 0) {
            for (uint32_t c : chans) rec_base[c] = pos;
            host_now = chans;
            return;
        }
        SlotResets &s = slot[in_flight_slot & 1];
        s.pos = pos;                               // (every request attached to a slot lies at that launch's end)
        merge(s.channels, chans);
    }
    // the device half: the channels to re-initialise in front of the launch about to be queued (the list is handed over)
    void take_device(std::vector<uint32_t> &out) { out.clear(); out.swap(device); }
    // the harvest has replayed slot `s`: the channels whose host half is due now (their counter base is moved); the caller
    // resets them and then calls done_host(s)
    const std::vector<uint32_t> &host_due(int s)
    {
        SlotResets &r = slot[s & 1];
        for (uint32_t c : r.channels) rec_base[c] = r.pos;
        return r.channels;
    }
    void done_host(int s) { slot[s & 1].channels.clear(); }

    // A ragged launch (same_batch_process_*_ragged) in slot `s` that ends at stream position `pos` and gave channel c only
    // n - by[c] of its n rows: the channel's own stream lags the batch's by by[c] more from `pos` on, i.e. its counter base
    // moves by by[c] there.  The caller's view moves at once; the queued records' when the harvest has replayed the launch
    // (its own records still count with the old base).  `by`: n_channels entries.
    struct SlotShift { std::vector<uint32_t> channels, by; uint64_t pos = 0; };
    SlotShift shift_[2];
    void shift(const uint32_t *by, uint64_t pos, int s)
    {
        SlotShift &h = shift_[s & 1];
        h.channels.clear(); h.by.clear(); h.pos = pos;
        for (uint32_t c = 0; c < (uint32_t)api_base.size(); ++c)
            if (by[c]) { api_base[c] += by[c]; h.channels.push_back(c); h.by.push_back(by[c]); }
    }
    // the harvest has replayed slot `s`: its shifts are due (before its resets, which lie at the same position and win)
    const SlotShift &shift_due(int s)
    {
        SlotShift &h = shift_[s & 1];
        for (size_t i = 0; i < h.channels.size(); ++i) rec_base[h.channels[i]] += h.by[i];
        return h;
    }
    void done_shift(int s) { shift_[s & 1].channels.clear(); shift_[s & 1].by.clear(); }
    // the shift of slot `s` still to come for channel c (0 if none): a launch in flight that the harvest has not reached
    uint32_t pending_shift(int s, uint32_t c) const
    {
        const SlotShift &h = shift_[s & 1];
        auto it = std::lower_bound(h.channels.begin(), h.channels.end(), c);
        return it != h.channels.end() && *it == c ? h.by[(size_t)(it - h.channels.begin())] : 0u;
    }
    uint64_t rec_pos(int s) const { return slot[s & 1].pos; }

    // sample counter of a record of channel c as queued: the device counts from the batch's first sample
    uint64_t rebase(uint32_t c, uint64_t device_counter) const { return device_counter > rec_base[c] ? device_counter - rec_base[c] : 0; }
};

// One launch of a ragged call: the launch covers the call's rows [row0, row0 + n), of which channel c consumes those below
// counts[c] (m: the smallest count of the call).  Returns n_lock, the launch's rows that every channel consumes (its common
// prefix), and writes by[c] = n - min(max(counts[c] - row0, 0), n), the rows channel c does not consume: what
// ResetLedger::shift takes.  Over the launches that cover a call's rows [0, M) the by[c] sum to M - counts[c].
inline size_t ragged_launch_split(const uint32_t *counts, uint32_t n_channels, uint32_t m, size_t row0, size_t n, uint32_t *by)
{
    for (uint32_t c = 0; c < n_channels; ++c) {
        const size_t have = counts[c] > row0 ? std::min<size_t>(counts[c] - row0, n) : 0;
        by[c] = (uint32_t)(n - have);
    }
    return m > row0 ? std::min<size_t>(m - row0, n) : 0;
}

}  // namespace same
#endif  // SAME_RESETS_H
