// same_tone_delivery_kernels.h -- what same_tones.hip queues behind the capture work of a call in delivery mode
// (same_tone_delivery.hip has the kernels).
#pragma once

#include <hip/hip_runtime.h>

#include "same_tone_audio_kernels.h"
#include "same_tone_delivery_dev.h"

namespace same {

// A call's output records lie behind its chunk slots (ToneAudioCall::out + out_bytes_before): one td::Out per slot, in the
// slots' order.  The header's third uint64 holds the delivered samples of the call: the delivery pool's use.
struct ToneDeliveryCall {
    td::Params params;
    const float *taps_t;          // [T][L]
    float *hist;                  // [C][T - 1]: a channel's history is contiguous, as the lanes along time read it
    uint64_t *a_next;             // [C]
    int16_t *dpool;               // the call's delivery pool, pool_cap entries
    size_t outs_offset;           // of the output records in ToneAudioCall::out
    uint32_t max_tiles;           // tiles of 256 outputs a chunk of this call can have
};

// the output-offset kernel and the decimator, behind tone_audio_launch_copy
hipError_t tone_delivery_launch(const ToneAudioCall &k, const ToneDeliveryCall &dk, hipStream_t stream);
// the history kernel, behind the decimator; n_rows > 0
hipError_t tone_delivery_launch_history(const ToneAudioCall &k, const ToneDeliveryCall &dk, const float *x, size_t n_rows, int layout, hipStream_t stream);
hipError_t tone_delivery_launch_history(const ToneAudioCall &k, const ToneDeliveryCall &dk, const int16_t *x, size_t n_rows, int layout, hipStream_t stream);

}  // namespace same
