"""The tones in front of the voice message (include/same_tones.h): `ToneDetector`, a ctypes wrapper of the device detector of
the EAS two-tone attention signal (853 + 960 Hz) and of NOAA Weather Radio's 1050 Hz warning alarm tone.  It reads the tensors
a batch reads and reports tone events that count in each channel's own samples.

    td = ToneDetector(n_channels, 22050)
    td.process(x)                   # x: CUDA tensor [n_rows, C], float32 or int16 -- the tensor given to the batch
    td.process(x, counts)           # or a ragged call: channel c owns its first counts[c] rows
    td.sync(); events = td.poll()   # numpy records: channel, kind, edge, reserved, sample_counter, duration

Tone alert (include/same_tone_audio.h): `td.set_audio_capture(TONE_WAT | TONE_ATTENTION, tail_blocks, max_blocks,
samples_per_call)` before the first sample makes the same `process` calls copy what follows a confirmed tone out of `x` on the
device; `td.sync(); td.poll_audio()` hands the chunks out.  In delivery form (include/same_tone_delivery.h):
`td.set_audio_delivery(kinds, tail_blocks, max_blocks, samples_per_call, out_rate, gain)` instead, and `td.poll_delivery()` hands
out int16 at `out_rate`, decimated and quantised on the device.

There is no CPU fallback: the detection runs in the library's gfx950 kernels or not at all.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .receiver import LAYOUT_CHANNEL_MAJOR, LAYOUT_TIME_MAJOR, SameError, load_library

TONE_ATTENTION, TONE_WAT = 1, 2              # same_tone_event.kind
TONE_START, TONE_END = 1, 2                  # same_tone_event.edge
TONE_START_BLOCKS, TONE_END_BLOCKS = 25, 5   # qualifying blocks in a row before START, missing blocks in a row before END
TONE_WAT_SHARE = 0.5                         # P_2 >= this share of ref
TONE_ATTENTION_EACH_SHARE = 0.15             # P_0 and P_1, each
TONE_ATTENTION_SUM_SHARE = 0.5               # P_0 + P_1
TONE_FREQUENCIES = (853.0, 960.0, 1050.0)
TONE_MIN_RATE, TONE_MAX_RATE = 8000, 96000

TONE_EVENT_DTYPE = np.dtype([("channel", "<u4"), ("kind", "<u4"), ("edge", "<u4"), ("reserved", "<u4"),
                             ("sample_counter", "<u8"), ("duration", "<u8")])
assert TONE_EVENT_DTYPE.itemsize == 32

# tone-alert audio (include/same_tone_audio.h): same_tone_audio_chunk.flags, and the record as the library lays it out
TONE_AUDIO_FIRST, TONE_AUDIO_END_TAIL, TONE_AUDIO_END_MAX, TONE_AUDIO_TRUNCATED = 1, 2, 4, 8
TONE_AUDIO_END = TONE_AUDIO_END_TAIL | TONE_AUDIO_END_MAX
TONE_AUDIO_CHUNK_DTYPE = np.dtype([("channel", "<u4"), ("flags", "<u4"), ("kind", "<u4"), ("reserved", "<u4"),
                                   ("sample_counter", "<u8"), ("n_samples", "<u8"), ("tone_start", "<u8"), ("samples", "<u8")])
assert TONE_AUDIO_CHUNK_DTYPE.itemsize == 48
# the delivery form (include/same_tone_delivery.h): same_tone_delivery_chunk
TONE_DELIVERY_CHUNK_DTYPE = np.dtype([("channel", "<u4"), ("flags", "<u4"), ("kind", "<u4"), ("rate", "<u4"), ("sample_counter", "<u8"),
                                      ("out_index", "<u8"), ("n_samples", "<u8"), ("tone_start", "<u8"), ("samples", "<u8")])
assert TONE_DELIVERY_CHUNK_DTYPE.itemsize == 56


def tone_audio_chunk_bound(n_blocks: int) -> int:
    """SAME_TONE_AUDIO_CHUNK_BOUND: the chunks of a channel in a call in which it completes n_blocks"""
    return 1 + (int(n_blocks) + 28) // 30 + (int(n_blocks) + 26) // 30


def block_length(rate: int) -> int:
    """N = rate / 25 by integer division: 40 ms"""
    return int(rate) // 25


_declared = False


def _lib() -> C.CDLL:
    """libsame_rx.so with the prototypes of include/same_tones.h declared."""
    global _declared
    L = load_library()
    if _declared:
        return L
    P, vp, u32, u64 = C.POINTER, C.c_void_p, C.c_uint32, C.c_uint64

    def sig(name, res, *args):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = list(args)

    sig("same_tones_new", C.c_int, u32, u32, C.c_int, P(vp))
    sig("same_tones_free", None, vp)
    sig("same_tones_last_error", C.c_char_p)
    sig("same_tones_n_channels", u32, vp)
    sig("same_tones_rate", u32, vp)
    sig("same_tones_block_length", u32, vp)
    sig("same_tones_coefficients", C.c_int, vp, P(C.c_float))
    sig("same_tones_block_counts", C.c_int, vp, P(u32), C.c_size_t, P(u32), P(u32))
    sig("same_tones_process_device", C.c_int, vp, vp, C.c_size_t, P(u32), C.c_int, vp, C.c_size_t, vp)
    sig("same_tones_process_device_i16", C.c_int, vp, vp, C.c_size_t, P(u32), C.c_int, vp, C.c_size_t, vp)
    sig("same_tones_sync", C.c_int, vp)
    sig("same_tones_poll", C.c_int, vp, vp, C.c_size_t, P(C.c_size_t), P(C.c_size_t))
    sig("same_tones_reset_channels", C.c_int, vp, P(u32), C.c_size_t)
    sig("same_tones_channel_sample_counter", u64, vp, u32)
    sig("same_tone_audio_set", C.c_int, vp, u32, u32, u32, C.c_size_t)
    sig("same_tone_audio_peek", C.c_int, vp, P(vp), P(C.c_size_t))
    sig("same_tone_audio_drop", C.c_int, vp, C.c_size_t)
    sig("same_tone_audio_chunk_bound", u32, u32)
    sig("same_tone_delivery_set", C.c_int, vp, u32, u32, u32, C.c_size_t, u32, C.c_float)
    sig("same_tone_delivery_peek", C.c_int, vp, P(vp), P(C.c_size_t))
    sig("same_tone_delivery_drop", C.c_int, vp, C.c_size_t)
    _declared = True
    return L


def _check(rc: int) -> int:
    if rc < 0:
        raise SameError(rc, _lib().same_tones_last_error().decode(errors="replace"))
    return rc


def _u32(values, n: Optional[int], what: str) -> np.ndarray:
    """`values` (a sequence, an ndarray or a CPU tensor) as contiguous uint32; n entries if n is given"""
    if hasattr(values, "detach"):
        values = values.detach().cpu().numpy()
    a = np.atleast_1d(np.asarray(values))
    if a.ndim != 1 or (n is not None and a.shape[0] != n):
        raise SameError(-1, f"{what}: {a.shape} entries for {n} channels; nothing was consumed")
    if a.size and (a.dtype.kind not in "iu" or a.min() < 0 or a.max() > 0xffffffff):
        raise SameError(-1, f"{what}: non-negative integers below 2^32; nothing was consumed")
    return np.ascontiguousarray(a, dtype=np.uint32)


def _p32(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))


class ToneDetector:
    """`same_tones`: n_channels streams at one rate, on one device."""

    def __init__(self, n_channels: int, rate: int, device: Optional[int] = None):
        self._L = _lib()
        h = C.c_void_p()
        _check(self._L.same_tones_new(int(n_channels), int(rate), 0 if device is None else int(device), C.byref(h)))
        self._h = h
        self._inflight = []          # the tensors of calls that may still be running (the library keeps three in flight)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.same_tones_free(self._h)
            self._h = None

    @property
    def n_channels(self) -> int:
        return self._L.same_tones_n_channels(self._h)

    @property
    def rate(self) -> int:
        return self._L.same_tones_rate(self._h)

    @property
    def block_length(self) -> int:
        return self._L.same_tones_block_length(self._h)

    def coefficients(self) -> np.ndarray:
        """c_k = (float)(2 cos(2 pi f_k / rate)) for 853, 960 and 1050 Hz"""
        out = np.empty(3, dtype=np.float32)
        _check(self._L.same_tones_coefficients(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def block_counts(self, n_rows: int, counts=None):
        """(block_counts, max_blocks): the blocks each channel would complete in a call of these counts (None: every channel
        n_rows).  Nothing changes."""
        k = None if counts is None else _u32(counts, self.n_channels, "counts")
        out = np.empty(self.n_channels, dtype=np.uint32)
        mx = C.c_uint32()
        _check(self._L.same_tones_block_counts(self._h, _p32(k), int(n_rows), _p32(out), C.byref(mx)))
        return out, mx.value

    def process_device_ptr(self, x_ptr: int, n_rows: int, counts=None, layout: int = LAYOUT_TIME_MAJOR, blocks_ptr: int = 0,
                           block_rows: int = 0, stream: int = 0, i16: bool = False) -> None:
        """same_tones_process_device(_i16) on device pointers; `stream`: a hipStream_t handle, 0 = the legacy default stream.
        The caller keeps both buffers valid until the stream has passed the call."""
        k = None if counts is None else _u32(counts, self.n_channels, "counts")
        fn = self._L.same_tones_process_device_i16 if i16 else self._L.same_tones_process_device
        _check(fn(self._h, C.c_void_p(x_ptr), int(n_rows), _p32(k), int(layout), C.c_void_p(blocks_ptr), int(block_rows),
                  C.c_void_p(stream)))

    def process(self, x, counts=None, layout: int = LAYOUT_TIME_MAJOR, blocks=None, stream: Optional[int] = None) -> np.ndarray:
        """x: CUDA tensor, float32 or int16, [n_rows, C] (time-major) or [C, n_rows]; channel c owns its first counts[c]
        samples (None: a plain call, every channel n_rows).  `blocks`: None, or a float32 CUDA tensor [block_rows, C, 4] that
        receives P_0, P_1, P_2, Em of every block a channel completes in this call, in its first rows.  Runs on `stream` (a
        hipStream_t handle; None: torch's current stream of x's device).  References to x and blocks are held until the call
        can no longer be running (three calls later, or `sync()`).  Returns the blocks each channel completed."""
        import torch
        assert x.is_cuda and x.is_contiguous() and x.dim() == 2
        if layout == LAYOUT_CHANNEL_MAJOR:
            ch, n = x.shape
        else:
            n, ch = x.shape
        if ch != self.n_channels:
            raise SameError(-1, f"x has {ch} channels, the detector {self.n_channels}; nothing was consumed")
        if x.dtype not in (torch.float32, torch.int16):
            raise TypeError("float32 or int16 input")
        bptr, brows = 0, 0
        if blocks is not None:
            assert blocks.is_cuda and blocks.is_contiguous() and blocks.dtype == torch.float32
            assert blocks.dim() == 3 and blocks.shape[1] == self.n_channels and blocks.shape[2] == 4
            bptr, brows = blocks.data_ptr(), blocks.shape[0]
        done, _ = self.block_counts(n, counts)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        self.process_device_ptr(x.data_ptr(), n, counts, layout, bptr, brows, stream, x.dtype == torch.int16)
        self._inflight.append((x, blocks))
        if len(self._inflight) > 3:
            del self._inflight[0]
        return done

    def sync(self) -> None:
        _check(self._L.same_tones_sync(self._h))
        self._inflight.clear()

    def poll(self, max_events: int = 1 << 22) -> np.ndarray:
        """The events of the calls that have passed, as TONE_EVENT_DTYPE records: calls in call order; inside a call by
        channel, then by the block that emitted the event, then by kind.  Never blocks: `sync()` first to include the calls in
        flight."""
        parts = []
        taken = 0
        while taken < max_events:
            buf = np.zeros(min(4096, max_events - taken), dtype=TONE_EVENT_DTYPE)
            n, left = C.c_size_t(), C.c_size_t()
            _check(self._L.same_tones_poll(self._h, C.c_void_p(buf.ctypes.data), buf.size, C.byref(n), C.byref(left)))
            parts.append(buf[: n.value])
            taken += n.value
            if left.value == 0 or n.value == 0:
                break
        return np.concatenate(parts) if parts else np.zeros(0, dtype=TONE_EVENT_DTYPE)

    def set_audio_capture(self, kinds: int, tail_blocks: int, max_blocks: int, samples_per_call: int) -> None:
        """Tone alert (same_tone_audio_set): capture what follows a confirmed tone of `kinds` (a mask of TONE_ATTENTION |
        TONE_WAT) until no enabled tone has been active for `tail_blocks` blocks more, `max_blocks` blocks at the most.  Before
        the detector's first sample.  `samples_per_call`: the pool of one call (three are allocated on the device now); 0 turns
        capture off."""
        _check(self._L.same_tone_audio_set(self._h, int(kinds), int(tail_blocks), int(max_blocks), int(samples_per_call)))

    def _take(self, peek, drop, dtype: np.dtype, sample) -> list:
        """The view `peek` hands out as (record, owned samples) pairs, dropped with `drop`; `sample`: the ctypes type of a sample"""
        ptr, n = C.c_void_p(), C.c_size_t()
        _check(peek(self._h, C.byref(ptr), C.byref(n)))
        out = []
        if n.value:
            raw = (C.c_char * (n.value * dtype.itemsize)).from_address(ptr.value)
            recs = np.frombuffer(raw, dtype=dtype).copy()
            for r in recs:
                k = int(r["n_samples"])
                a = np.ctypeslib.as_array(C.cast(int(r["samples"]), C.POINTER(sample)), shape=(k,)).copy() if k else np.zeros(0, sample)
                r["samples"] = 0
                out.append((r, a))
            _check(drop(self._h, n.value))
        return out

    def poll_audio(self) -> list:
        """The queued audio chunks of the calls that have passed, which are then dropped: (record, samples) pairs, the record a
        TONE_AUDIO_CHUNK_DTYPE scalar (its `samples` field is 0) and the samples an owned float32 array.  Calls in call order;
        inside a call by channel, then by sample_counter.  `sync()` first to include the calls in flight."""
        return self._take(self._L.same_tone_audio_peek, self._L.same_tone_audio_drop, TONE_AUDIO_CHUNK_DTYPE, C.c_float)

    def set_audio_delivery(self, kinds: int, tail_blocks: int, max_blocks: int, samples_per_call: int, out_rate: int, gain: float = 1.0) -> None:
        """Tone alert in delivery form (same_tone_delivery_set), in place of `set_audio_capture` and under its rules: the same
        captures, handed out by `poll_delivery` as int16 at `out_rate` (at most the detector's rate; a ratio the resampler refuses
        raises SAME_ERATE), each sample the resampler's f32 sum times `gain`, rounded to nearest even and clamped.
        `samples_per_call` counts captured source samples; 0 turns capture off."""
        _check(self._L.same_tone_delivery_set(self._h, int(kinds), int(tail_blocks), int(max_blocks), int(samples_per_call), int(out_rate),
                                              float(gain)))

    def poll_delivery(self) -> list:
        """The queued delivery chunks of the calls that have passed, which are then dropped: (record, samples) pairs, the record a
        TONE_DELIVERY_CHUNK_DTYPE scalar (its `samples` field is 0) and the samples an owned int16 array.  The order is
        `poll_audio`'s.  `sync()` first to include the calls in flight.  Empty on a detector that is not in delivery form."""
        return self._take(self._L.same_tone_delivery_peek, self._L.same_tone_delivery_drop, TONE_DELIVERY_CHUNK_DTYPE, C.c_int16)

    def reset_channels(self, channels) -> None:
        """The listed channels start again at this point of the stream (same_tones_reset_channels).  An active tone emits no
        END.  On an error nothing is reset."""
        ch = _u32(channels, None, "channels")
        _check(self._L.same_tones_reset_channels(self._h, _p32(ch), ch.size))

    def channel_sample_counter(self, channel: int) -> int:
        return int(self._L.same_tones_channel_sample_counter(self._h, channel))
