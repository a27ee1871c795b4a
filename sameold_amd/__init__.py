"""sameold_amd -- MI355X-native batched SAME/EAS AFSK demodulator (hot path of sameold).

The package holds only what the path needs: csrc/ (gfx950 HIP kernels + the C ABI of
include/same_rx.h) and receiver.py (a Python mirror of SameReceiverBuilder/SameReceiver); resample.py puts the device
resampler of include/same_resample.h in front of a batch whose sources run at different rates; tones.py wraps the device
detector of the attention signal and the 1050 Hz tone (include/same_tones.h).
"""
from .receiver import (  # noqa: F401
    Event, SameBatchReceiver, SameError, SameReceiver, SameReceiverBuilder,
    LAYOUT_CHANNEL_MAJOR, LAYOUT_TIME_MAJOR,
    LINK_BURST, LINK_NO_CARRIER, LINK_READING, LINK_SEARCHING,
    TRANSPORT_ASSEMBLING, TRANSPORT_IDLE, TRANSPORT_MSG_END, TRANSPORT_MSG_ERR, TRANSPORT_MSG_START,
    decode_recordings, load_library, synth_afsk, synth_payload,
    AUDIO_END, AUDIO_END_FLUSH, AUDIO_END_MESSAGE, AUDIO_END_RESET, AUDIO_FIRST, AUDIO_TRUNCATED, AudioChunk, AudioJoiner,
)
from .resample import MixedRateReceiver, Resampler  # noqa: F401
from .tones import (  # noqa: F401
    ToneDetector, TONE_ATTENTION, TONE_END, TONE_START, TONE_WAT,
    TONE_ATTENTION_EACH_SHARE, TONE_ATTENTION_SUM_SHARE, TONE_END_BLOCKS, TONE_EVENT_DTYPE, TONE_START_BLOCKS, TONE_WAT_SHARE,
    block_length,
    TONE_AUDIO_CHUNK_DTYPE, TONE_AUDIO_END, TONE_AUDIO_END_MAX, TONE_AUDIO_END_TAIL, TONE_AUDIO_FIRST, TONE_AUDIO_TRUNCATED,
    tone_audio_chunk_bound, TONE_DELIVERY_CHUNK_DTYPE,
)
