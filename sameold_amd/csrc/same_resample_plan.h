// same_resample_plan.h -- the host half of the mixed-rate resampler (include/same_resample.h): which ratio a channel runs, the
// tap table of every distinct ratio (designed in double, rounded once to f32), the channels' clocks, what a call of given
// in_counts produces, and resets.  The device half is told everything per call (rs::Desc, same_resample_dev.h): the plan is the
// only place where a clock lives.
// Host-only (no HIP): tests/helpers/resample_plan_main.cpp drives it, with the device core, under ASan + UBSan without a device.
#ifndef SAME_RESAMPLE_PLAN_H
#define SAME_RESAMPLE_PLAN_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/same_rx.h"
#include "same_resample_dev.h"

namespace same {

struct ResamplePlan {
    uint32_t out_rate = 0;
    std::vector<rs::Ratio> ratios;           // at most rs::kMaxRatios, only ever appended to
    std::vector<float> taps;                 // every ratio's table, [p][j] at its tap_off
    std::vector<float> taps_t;               // the same tables stored [j][p] (taps_t[off + j L + p] == taps[off + p T + j]): per-source calls
    std::vector<uint32_t> chan_rate, chan_ratio;
    std::vector<uint64_t> n_in, n_out;       // per channel, since its start or last reset
    std::vector<uint8_t> clear;              // per channel: reset since the last call that ran; its history is to be zeroed

    static uint32_t gcd(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }

    // modified Bessel function of the first kind, order 0: sum_k ((x/2)^k / k!)^2
    static double bessel_i0(double x)
    {
        const double q = x * x / 4.0;
        double term = 1.0, sum = 1.0;
        for (int k = 1; k < 500; ++k) {
            term = term * (q / ((double)k * (double)k));
            sum = sum + term;
            if (term < sum * 1e-17) break;
        }
        return sum;
    }

    // L, M, T of r_in -> r_out: SAME_OK, SAME_EINVAL (a zero rate) or SAME_ERATE (beyond kMaxL phases or kMaxT taps)
    static int ratio_of(uint32_t r_in, uint32_t r_out, uint32_t &L, uint32_t &M, uint32_t &T)
    {
        if (r_in == 0 || r_out == 0) return SAME_EINVAL;
        const uint32_t g = gcd(r_in, r_out);
        L = r_out / g; M = r_in / g;
        if (L == 1 && M == 1) { T = 1; return SAME_OK; }
        if (L > rs::kMaxL) return SAME_ERATE;
        // T = 2 ceil(8 max(1, M / L))
        const uint64_t half = M > L ? (8ull * M + L - 1) / L : 8;
        if (2 * half > rs::kMaxT) return SAME_ERATE;
        T = (uint32_t)(2 * half);
        return SAME_OK;
    }

    // the prototype of T L points: a Kaiser window (beta 8.6) on a sinc cut at 0.45 of the lower rate, gain L
    static double prototype(uint32_t i, uint32_t r_in, uint32_t r_out, uint32_t L, uint32_t T)
    {
        const double pi = 3.14159265358979323846;
        const double n = (double)T * (double)L;
        const double w = 2.0 * 0.45 * (double)(r_in < r_out ? r_in : r_out) / ((double)L * (double)r_in);
        const double t = (double)i - (n - 1.0) / 2.0;
        const double a = pi * (w * t);
        const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
        const double u = t / (n / 2.0);
        return (double)L * w * sinc * bessel_i0(8.6 * std::sqrt(1.0 - u * u)) / bessel_i0(8.6);
    }

    // index of the ratio r_in -> out_rate, designing its taps if it is new
    int ratio_index(uint32_t r_in, uint32_t &index)
    {
        uint32_t L = 0, M = 0, T = 0;
        const int rc = ratio_of(r_in, out_rate, L, M, T);
        if (rc) return rc;
        for (uint32_t i = 0; i < (uint32_t)ratios.size(); ++i)
            if (ratios[i].L == L && ratios[i].M == M) { index = i; return SAME_OK; }
        if (ratios.size() >= rs::kMaxRatios) return SAME_EINVAL;
        const rs::Ratio r{L, M, T, (uint32_t)taps.size()};
        taps.resize(taps.size() + (size_t)T * L);
        taps_t.resize(taps.size());
        float *h = taps.data() + r.tap_off, *ht = taps_t.data() + r.tap_off;
        if (T == 1) h[0] = 1.0f;
        else
            for (uint32_t p = 0; p < L; ++p)
                for (uint32_t j = 0; j < T; ++j) h[(size_t)p * T + j] = (float)prototype(p + j * L, r_in, out_rate, L, T);
        for (uint32_t p = 0; p < L; ++p)
            for (uint32_t j = 0; j < T; ++j) ht[(size_t)j * L + p] = h[(size_t)p * T + j];
        index = (uint32_t)ratios.size();
        ratios.push_back(r);
        return SAME_OK;
    }

    // On an error the plan is empty.
    int init(uint32_t n_channels, const uint32_t *in_rates, uint32_t r_out)
    {
        *this = ResamplePlan();
        out_rate = r_out;
        chan_rate.assign(in_rates, in_rates + n_channels);
        chan_ratio.assign(n_channels, 0);
        for (uint32_t c = 0; c < n_channels; ++c) {
            const int rc = ratio_index(in_rates[c], chan_ratio[c]);
            if (rc) { *this = ResamplePlan(); return rc; }
        }
        n_in.assign(n_channels, 0);
        n_out.assign(n_channels, 0);
        clear.assign(n_channels, 1);          // (a fresh history buffer holds anything: the first call zeroes every column)
        return SAME_OK;
    }
    uint32_t n_channels() const { return (uint32_t)chan_ratio.size(); }
    const rs::Ratio &ratio(uint32_t c) const { return ratios[chan_ratio[c]]; }
    // output samples by which the output stream lags the source: (T L - 1) / (2 M)
    double delay(uint32_t c) const
    {
        const rs::Ratio &r = ratio(c);
        return ((double)r.T * (double)r.L - 1.0) / (2.0 * (double)r.M);
    }

    // What a call of in_counts[c] <= n_rows source samples per channel produces: out_counts (n_channels entries) and their
    // maximum.  Nothing changes.  SAME_EINVAL: a count above n_rows, or an output count beyond 2^32 - 1.
    int out_counts(const uint32_t *in_counts, size_t n_rows, uint32_t *out, uint32_t *max_out) const
    {
        uint32_t mx = 0;
        for (uint32_t c = 0; c < n_channels(); ++c) {
            if (in_counts[c] > n_rows) return SAME_EINVAL;
            const rs::Ratio &r = ratio(c);
            const uint64_t k = rs::outputs_after(n_in[c] + in_counts[c], r.L, r.M) - n_out[c];
            if (k > 0xffffffffull) return SAME_EINVAL;
            out[c] = (uint32_t)k;
            if (out[c] > mx) mx = out[c];
        }
        *max_out = mx;
        return SAME_OK;
    }
    // the call's descriptors, from the counts out_counts() gave; true if a history is to be zeroed in front of it
    bool describe(const uint32_t *in_counts, const uint32_t *out, rs::Desc *d) const
    {
        bool any = false;
        for (uint32_t c = 0; c < n_channels(); ++c) {
            d[c] = rs::Desc{n_in[c], n_out[c], in_counts[c], out[c], chan_ratio[c], clear[c]};
            any |= clear[c] != 0;
        }
        return any;
    }
    // the described call was queued: the clocks move, the pending clears are spent
    void commit(const uint32_t *in_counts, const uint32_t *out)
    {
        for (uint32_t c = 0; c < n_channels(); ++c) { n_in[c] += in_counts[c]; n_out[c] += out[c]; clear[c] = 0; }
    }

    // The listed channels start again at the stream position between the calls so far and the next one: clocks 0, history
    // zero, and with new_rates (one per list entry; null keeps the rates) the ratio of the new source.  On an error -- a
    // channel out of range, SAME_ERATE, a 17th ratio -- nothing is reset (a ratio designed on the way stays in the table).
    int reset(const uint32_t *channels, size_t n, const uint32_t *new_rates)
    {
        std::vector<uint32_t> idx(n, 0);
        for (size_t i = 0; i < n; ++i) {
            if (channels[i] >= n_channels()) return SAME_EINVAL;
            if (!new_rates) continue;
            const int rc = ratio_index(new_rates[i], idx[i]);
            if (rc) return rc;
        }
        for (size_t i = 0; i < n; ++i) {
            const uint32_t c = channels[i];
            if (new_rates) { chan_rate[c] = new_rates[i]; chan_ratio[c] = idx[i]; }
            n_in[c] = 0; n_out[c] = 0; clear[c] = 1;
        }
        return SAME_OK;
    }
};

}  // namespace same
#endif  // SAME_RESAMPLE_PLAN_H
