// same_tone_audio_kernels.h -- what same_tones.hip queues for a call with capture on (same_tone_audio.hip has the kernels).
#pragma once

#include <hip/hip_runtime.h>

#include "same_tone_audio_dev.h"

namespace same {

// the device buffers of one call's capture work
struct ToneAudioCall {
    const tn::Desc *desc;
    const uint32_t *span_off;     // [C]: each channel's first chunk slot
    const uint8_t *qual;
    tn::Sm *sm;
    tn::Cap *cap;
    tn::CapParams params;
    uint32_t *ev_counts;
    same_tone_event *ev;
    uint8_t *out;                 // header, chunk counts, chunk slots
    uint64_t *counts;             // [C]: captured rows of the call
    uint32_t *flags;              // [ceil(C / 64)]: someone of the group captures
    float *pool;
    uint64_t pool_cap;
    uint32_t N, n_channels;
};

// the capture-aware state-machine kernel and the prefix kernel
hipError_t tone_audio_launch_sm(const ToneAudioCall &k, hipStream_t stream);
// the copy kernel of the layout; n_rows > 0
hipError_t tone_audio_launch_copy(const ToneAudioCall &k, const float *x, size_t n_rows, int layout, hipStream_t stream);
hipError_t tone_audio_launch_copy(const ToneAudioCall &k, const int16_t *x, size_t n_rows, int layout, hipStream_t stream);

}  // namespace same
