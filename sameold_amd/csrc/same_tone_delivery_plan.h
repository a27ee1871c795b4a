// same_tone_delivery_plan.h -- the host half of tone-alert audio in delivery form (include/same_tone_delivery.h): the capture's
// parameters (same_tone_audio_plan.h), the ratio and the taps of rate -> out_rate from the resampler's design
// (same_resample_plan.h: ResamplePlan::ratio_of and prototype), stored [tap j][phase p] as the lanes along output time read them.
// Host-only (no HIP): tests/helpers/tone_delivery_main.cpp drives it, with the device core, under ASan + UBSan without a device.
#ifndef SAME_TONE_DELIVERY_PLAN_H
#define SAME_TONE_DELIVERY_PLAN_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/same_rx.h"
#include "same_resample_plan.h"
#include "same_tone_audio_plan.h"
#include "same_tone_delivery_dev.h"

namespace same {

struct ToneDeliveryPlan {
    ToneAudioPlan audio;
    td::Params params{0, 0, 0, 0, 0.0f};
    std::vector<float> taps_t;               // [j][p]: taps_t[j L + p] = (float)prototype(p + j L)

    bool on() const { return audio.on() && params.T != 0; }

    // samples_per_call == 0: off, SAME_OK.  SAME_EINVAL: what ToneAudioPlan::set refuses, a gain that is not finite and positive,
    // out_rate == 0 or above rate.  SAME_ERATE: a ratio the resampler refuses.  On an error the plan is off.
    int set(uint32_t kinds, uint32_t tail_blocks, uint32_t max_blocks, uint64_t samples_per_call, uint32_t rate, uint32_t out_rate, float gain)
    {
        *this = ToneDeliveryPlan();
        if (samples_per_call == 0) return SAME_OK;
        ToneAudioPlan a;
        if (a.set(kinds, tail_blocks, max_blocks, samples_per_call)) return SAME_EINVAL;
        if (!(gain > 0.0f) || std::isinf(gain)) return SAME_EINVAL;
        if (out_rate == 0 || out_rate > rate) return SAME_EINVAL;
        uint32_t L = 0, M = 0, T = 0;
        const int rc = ResamplePlan::ratio_of(rate, out_rate, L, M, T);
        if (rc) return rc;
        taps_t.assign((size_t)T * L, 1.0f);
        if (T > 1)
            for (uint32_t p = 0; p < L; ++p)
                for (uint32_t j = 0; j < T; ++j) taps_t[(size_t)j * L + p] = (float)ResamplePlan::prototype(p + j * L, rate, out_rate, L, T);
        audio = a;
        params = td::Params{L, M, T, out_rate, gain};
        return SAME_OK;
    }
};

}  // namespace same
#endif  // SAME_TONE_DELIVERY_PLAN_H
