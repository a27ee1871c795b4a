// same_tone_audio_plan.h -- the host half of tone-alert audio (include/same_tone_audio.h): the capture's parameters, and
// where each channel's chunk slots of a call lie, handed out in channel order beside the event slots of same_tones_plan.h.
// Host-only (no HIP): tests/helpers/tone_audio_main.cpp drives it, with the device core, under ASan + UBSan without a device.
#ifndef SAME_TONE_AUDIO_PLAN_H
#define SAME_TONE_AUDIO_PLAN_H

#include <cstddef>
#include <cstdint>

#include "../../include/same_rx.h"
#include "same_tone_audio_dev.h"

namespace same {

struct ToneAudioPlan {
    tn::CapParams params{0, 0, 0};
    uint64_t pool_cap = 0;                   // samples_per_call; 0: capture is off

    bool on() const { return pool_cap != 0; }

    // SAME_EINVAL: a mask that is empty or names another kind, max_blocks == 0.  samples_per_call == 0 turns capture off.
    int set(uint32_t kinds, uint32_t tail_blocks, uint32_t max_blocks, uint64_t samples_per_call)
    {
        if (samples_per_call == 0) { *this = ToneAudioPlan(); return SAME_OK; }
        if (kinds == 0 || (kinds & ~(uint32_t)(SAME_TONE_ATTENTION | SAME_TONE_WAT)) || max_blocks == 0) return SAME_EINVAL;
        params = tn::CapParams{kinds, tail_blocks, max_blocks};
        pool_cap = samples_per_call;
        return SAME_OK;
    }

    // The chunk slots of the call d[0 .. C) describes: span_off[c] is channel c's first slot, it owns chunk_bound(n_complete).
    // Returns the call's slots.
    static uint64_t describe(const tn::Desc *d, uint32_t C, uint32_t *span_off)
    {
        uint64_t slots = 0;
        for (uint32_t c = 0; c < C; ++c) {
            span_off[c] = (uint32_t)slots;
            slots += tn::chunk_bound(d[c].n_complete);
        }
        return slots;
    }
};

}  // namespace same
#endif  // SAME_TONE_AUDIO_PLAN_H
