// same_tones_plan.h -- the host half of the tone detector (include/same_tones.h): what a rate fixes (block length and
// coefficients, computed in double and rounded once), every channel's position in its stream, and a call's work plan: for
// each channel which blocks the call touches, where each begins, whether the first continues the saved open block and which
// complete (tn::Desc and tn::block_rows, same_tones_dev.h), and where its event slots lie.  The device is told everything per
// call: the plan is the only place where a position lives.
// Host-only (no HIP): tests/helpers/tones_main.cpp drives it, with the device core, under ASan + UBSan without a device.
#ifndef SAME_TONES_PLAN_H
#define SAME_TONES_PLAN_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/same_rx.h"
#include "same_tones_dev.h"

namespace same {

struct TonesPlan {
    uint32_t rate = 0;
    tn::Coef coef{};
    std::vector<uint64_t> pos;               // per channel: samples since its start or last reset
    std::vector<uint8_t> clear;              // per channel: reset since the last call that ran
    std::vector<uint8_t> bank;               // per channel: the Acc bank that holds its open block

    static int coefficients(uint32_t r, tn::Coef &cf)
    {
        if (r < SAME_TONES_MIN_RATE || r > SAME_TONES_MAX_RATE) return SAME_ERATE;
        const double pi = 3.14159265358979323846;
        cf.N = r / tn::kBlocksPerSecond;
        for (int k = 0; k < 3; ++k) cf.c[k] = (float)(2.0 * std::cos(2.0 * pi * tn::kToneHz[k] / (double)r));
        cf.halfN = (float)cf.N * 0.5f;
        cf.invN = 1.0f / (float)cf.N;
        return SAME_OK;
    }

    // On an error the plan is empty.
    int init(uint32_t n_channels, uint32_t r)
    {
        *this = TonesPlan();
        tn::Coef cf{};
        const int rc = coefficients(r, cf);
        if (rc) return rc;
        if (n_channels == 0) return SAME_EINVAL;
        rate = r; coef = cf;
        pos.assign(n_channels, 0);
        clear.assign(n_channels, 1);          // (fresh state machines hold anything: the first call that runs makes them idle)
        bank.assign(n_channels, 0);
        return SAME_OK;
    }
    uint32_t n_channels() const { return (uint32_t)pos.size(); }
    uint32_t count_of(const uint32_t *counts, size_t n_rows, uint32_t c) const { return counts ? counts[c] : (uint32_t)n_rows; }

    // Blocks each channel completes in a call of these counts (null: every channel n_rows) and their maximum.  Nothing changes.
    // SAME_EINVAL: a count above n_rows, or n_rows beyond 2^32 - 1.
    int block_counts(const uint32_t *counts, size_t n_rows, uint32_t *out, uint32_t *max_blocks) const
    {
        if (n_rows > 0xffffffffull) return SAME_EINVAL;
        uint32_t mx = 0;
        for (uint32_t c = 0; c < n_channels(); ++c) {
            const uint32_t k = count_of(counts, n_rows, c);
            if (k > n_rows) return SAME_EINVAL;
            const uint32_t nb = (uint32_t)((pos[c] % coef.N + k) / coef.N);
            if (out) out[c] = nb;
            if (nb > mx) mx = nb;
        }
        if (max_blocks) *max_blocks = mx;
        return SAME_OK;
    }

    struct Shape { uint32_t max_touch = 0, max_complete = 0; uint64_t event_slots = 0; bool any_samples = false; };

    // The call's work plan, for counts block_counts() accepted: d[c] per channel, event slots handed out in channel order.
    Shape describe(const uint32_t *counts, size_t n_rows, tn::Desc *d) const
    {
        Shape s;
        for (uint32_t c = 0; c < n_channels(); ++c) {
            const uint32_t k = count_of(counts, n_rows, c), N = coef.N;
            const uint32_t fill = (uint32_t)(pos[c] % N);
            const uint64_t span = (uint64_t)fill + k;
            tn::Desc &e = d[c];
            e.block0 = pos[c] / N;
            e.fill = fill;
            e.count = k;
            e.n_touch = k ? (uint32_t)((span + N - 1) / N) : 0;
            e.n_complete = (uint32_t)(span / N);
            e.ev_off = (uint32_t)s.event_slots;
            e.flags = (clear[c] ? tn::kDescClear : 0u) | (bank[c] ? tn::kDescBank : 0u);
            s.event_slots += tn::events_bound(e.n_complete);
            if (e.n_touch > s.max_touch) s.max_touch = e.n_touch;
            if (e.n_complete > s.max_complete) s.max_complete = e.n_complete;
            s.any_samples |= k != 0;
        }
        return s;
    }
    // does the described call leave the channel an open block in the other bank?
    static bool saves(const tn::Desc &e) { return e.n_touch > e.n_complete; }

    // the described call was queued: positions move, banks flip where an open block was saved, the pending clears are spent
    void commit(const tn::Desc *d)
    {
        for (uint32_t c = 0; c < n_channels(); ++c) {
            pos[c] += d[c].count;
            if (saves(d[c])) bank[c] ^= 1;
            clear[c] = 0;
        }
    }

    // The listed channels start again behind the calls so far: position 0 (no open block), state machines idle in front of the
    // next call.  A channel out of range: SAME_EINVAL, and nothing is reset.
    int reset(const uint32_t *channels, size_t n)
    {
        for (size_t i = 0; i < n; ++i)
            if (channels[i] >= n_channels()) return SAME_EINVAL;
        for (size_t i = 0; i < n; ++i) { pos[channels[i]] = 0; clear[channels[i]] = 1; }
        return SAME_OK;
    }
};

}  // namespace same
#endif  // SAME_TONES_PLAN_H
