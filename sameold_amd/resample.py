"""Mixed-rate sources for a batch (include/same_resample.h): `Resampler`, a ctypes wrapper of the device resampler that takes
every channel from its own source rate to one output rate, and `MixedRateReceiver`, a resampler in front of a
`SameBatchReceiver` at the builder's rate, fed through the batch's ragged call.

    rx = MixedRateReceiver(SameReceiverBuilder(22050).samedec(), rates=[48000, 8000, 22050, ...])
    rx.process(x, in_counts)        # x: CUDA tensor [n_rows, C], float32 or int16; channel c owns its first in_counts[c] rows
    rx.process_sources(sources)     # or: one 1-D CUDA tensor (or None) per channel, each of its own length
    rx.sync(); events = rx.poll_events()

The batch's events count in samples at the batch's rate; `source_position` maps a counter back to the channel's source.
There is no CPU fallback: the resampling runs in the library's gfx950 kernels or not at all.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from .receiver import LAYOUT_TIME_MAJOR, SameBatchReceiver, SameError, SameReceiverBuilder, load_library

_declared = False


def _lib() -> C.CDLL:
    """libsame_rx.so with the prototypes of include/same_resample.h declared."""
    global _declared
    L = load_library()
    if _declared:
        return L
    P, vp, u32, u64 = C.POINTER, C.c_void_p, C.c_uint32, C.c_uint64

    def sig(name, res, *args):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = list(args)

    sig("same_resampler_new", C.c_int, u32, P(u32), u32, C.c_int, P(vp))
    sig("same_resampler_free", None, vp)
    sig("same_resampler_last_error", C.c_char_p)
    sig("same_resampler_n_channels", u32, vp)
    sig("same_resampler_out_rate", u32, vp)
    sig("same_resampler_plan", C.c_int, vp, u32, P(u32), P(u32), P(u32))
    sig("same_resampler_taps", C.c_int, vp, u32, P(C.c_float), C.c_size_t, P(C.c_size_t))
    sig("same_resampler_delay", C.c_double, vp, u32)
    sig("same_resampler_out_counts", C.c_int, vp, P(u32), P(u32), P(u32))
    sig("same_resampler_process_device", C.c_int, vp, vp, C.c_size_t, P(u32), vp, C.c_size_t, P(u32), vp)
    sig("same_resampler_process_device_i16", C.c_int, vp, vp, C.c_size_t, P(u32), vp, C.c_size_t, P(u32), vp)
    sig("same_resampler_process_device_sources", C.c_int, vp, vp, P(u32), vp, C.c_size_t, P(u32), vp)
    sig("same_resampler_process_device_sources_i16", C.c_int, vp, vp, P(u32), vp, C.c_size_t, P(u32), vp)
    sig("same_resampler_reset_channels", C.c_int, vp, P(u32), C.c_size_t, P(u32))
    sig("same_resampler_channel_input_counter", u64, vp, u32)
    sig("same_resampler_channel_output_counter", u64, vp, u32)
    _declared = True
    return L


def _check(rc: int) -> int:
    if rc < 0:
        raise SameError(rc, _lib().same_resampler_last_error().decode(errors="replace"))
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


def _p32(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


class Resampler:
    """`same_resampler`: n channels, each from its own source rate to `out_rate`, on one device."""

    def __init__(self, in_rates: Sequence[int], out_rate: int, device: int = 0):
        self._L = _lib()
        rates = _u32(in_rates, None, "in_rates")
        h = C.c_void_p()
        _check(self._L.same_resampler_new(rates.size, _p32(rates), int(out_rate), device, C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.same_resampler_free(self._h)
            self._h = None

    @property
    def n_channels(self) -> int:
        return self._L.same_resampler_n_channels(self._h)

    def out_rate(self) -> int:
        return self._L.same_resampler_out_rate(self._h)

    def plan(self, channel: int):
        """(L, M, T) of the channel: L / M = out_rate / its rate, T taps per phase."""
        L, M, T = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(self._L.same_resampler_plan(self._h, channel, C.byref(L), C.byref(M), C.byref(T)))
        return L.value, M.value, T.value

    def taps(self, channel: int) -> np.ndarray:
        """The channel's taps, float32 [L, T] (phase, tap)."""
        L, _, T = self.plan(channel)
        out = np.empty(L * T, dtype=np.float32)
        n = C.c_size_t()
        _check(self._L.same_resampler_taps(self._h, channel, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n)))
        return out.reshape(L, T)

    def delay(self, channel: int) -> float:
        """Output samples by which the channel's output lags its source: (T L - 1) / (2 M)."""
        if not 0 <= channel < self.n_channels:
            raise IndexError(f"channel {channel} of {self.n_channels}")
        return float(self._L.same_resampler_delay(self._h, channel))

    def out_counts(self, in_counts):
        """(out_counts, max_out) a process call with these in_counts would produce; nothing changes."""
        k = _u32(in_counts, self.n_channels, "in_counts")
        out = np.empty(self.n_channels, dtype=np.uint32)
        mx = C.c_uint32()
        _check(self._L.same_resampler_out_counts(self._h, _p32(k), _p32(out), C.byref(mx)))
        return out, mx.value

    def process_device_ptr(self, x_ptr: int, n_rows: int, in_counts, y_ptr: int, out_rows: int, stream: int = 0,
                           i16: bool = False) -> np.ndarray:
        """same_resampler_process_device(_i16) on device pointers; `stream`: a hipStream_t handle, 0 = the legacy default
        stream.  Returns out_counts.  The caller keeps both buffers valid until the stream has passed the call."""
        k = _u32(in_counts, self.n_channels, "in_counts")
        out = np.empty(self.n_channels, dtype=np.uint32)
        fn = self._L.same_resampler_process_device_i16 if i16 else self._L.same_resampler_process_device
        _check(fn(self._h, C.c_void_p(x_ptr), n_rows, _p32(k), C.c_void_p(y_ptr), out_rows, _p32(out), C.c_void_p(stream)))
        return out

    def process(self, x, in_counts, y=None):
        """x: CUDA tensor [n_rows, C], float32 or int16, of which channel c owns its first in_counts[c] rows.  Resamples on
        torch's current stream into `y` (float32 [out_rows, C]; a fresh tensor of exactly the rows the call makes if None) and
        returns (y, out_counts).  Rows of y at or beyond out_counts[c] are not written."""
        import torch
        assert x.is_cuda and x.is_contiguous() and x.dim() == 2 and x.shape[1] == self.n_channels
        if x.dtype not in (torch.float32, torch.int16):
            raise TypeError("float32 or int16 input")
        if y is None:
            _, rows = self.out_counts(in_counts)
            y = torch.empty((rows, self.n_channels), dtype=torch.float32, device=x.device)
        assert y.is_cuda and y.is_contiguous() and y.dtype == torch.float32 and y.dim() == 2 and y.shape[1] == self.n_channels
        stream = torch.cuda.current_stream(x.device).cuda_stream
        out = self.process_device_ptr(x.data_ptr(), x.shape[0], in_counts, y.data_ptr(), y.shape[0], stream, x.dtype == torch.int16)
        return y, out

    def process_source_ptrs(self, ptrs, in_counts, y_ptr: int, out_rows: int, stream: int = 0, i16: bool = False) -> np.ndarray:
        """same_resampler_process_device_sources(_i16): `ptrs` is a uint64 numpy array of n_channels device addresses, channel
        c's in_counts[c] contiguous samples at ptrs[c] (0 where the count is 0).  Returns out_counts.  The caller keeps every
        source buffer and the output valid until the stream has passed the call."""
        p = np.ascontiguousarray(ptrs, dtype=np.uint64)
        if p.ndim != 1 or p.shape[0] != self.n_channels:
            raise SameError(-1, f"ptrs: {p.shape} entries for {self.n_channels} channels; nothing was consumed")
        k = _u32(in_counts, self.n_channels, "in_counts")
        out = np.empty(self.n_channels, dtype=np.uint32)
        fn = self._L.same_resampler_process_device_sources_i16 if i16 else self._L.same_resampler_process_device_sources
        _check(fn(self._h, p.ctypes.data_as(C.c_void_p), _p32(k), C.c_void_p(y_ptr), out_rows, _p32(out), C.c_void_p(stream)))
        return out

    def _process_ptrs(self, ptrs, in_counts, i16, device, y):
        import torch
        if y is None:
            _, rows = self.out_counts(in_counts)
            y = torch.empty((rows, self.n_channels), dtype=torch.float32, device=device)
        assert y.is_cuda and y.is_contiguous() and y.dtype == torch.float32 and y.dim() == 2 and y.shape[1] == self.n_channels
        stream = torch.cuda.current_stream(y.device).cuda_stream
        return y, self.process_source_ptrs(ptrs, in_counts, y.data_ptr(), y.shape[0], stream, i16)

    def process_sources(self, sources, y=None):
        """sources: n_channels items, each a 1-D contiguous CUDA tensor -- the channel's next samples, all float32 or all int16
        -- or None for a channel without samples in this call.  Resamples on torch's current stream into `y` (as `process`)
        and returns (y, out_counts).  The caller keeps the tensors alive until the stream has passed the call."""
        import torch
        if len(sources) != self.n_channels:
            raise SameError(-1, f"sources: {len(sources)} entries for {self.n_channels} channels; nothing was consumed")
        ptrs = np.zeros(self.n_channels, np.uint64)
        counts = np.zeros(self.n_channels, np.uint32)
        dtype, device = None, None
        for c, t in enumerate(sources):
            if t is None:
                continue
            assert t.is_cuda and t.dim() == 1 and t.is_contiguous()
            if t.dtype not in (torch.float32, torch.int16) or (dtype is not None and t.dtype != dtype):
                raise TypeError("every source float32, or every source int16")
            dtype, device = t.dtype, t.device
            counts[c] = t.shape[0]
            ptrs[c] = t.data_ptr() if t.shape[0] else 0
        if device is None:
            device = torch.device("cuda") if y is None else y.device
        return self._process_ptrs(ptrs, counts, dtype == torch.int16, device, y)

    def process_channel_major(self, x, in_counts, y=None):
        """x: CUDA tensor [C, n_rows], float32 or int16, of which channel c owns the first in_counts[c] samples of its row: a
        per-source call with the rows as the sources.  Returns (y, out_counts) like `process`."""
        import torch
        assert x.is_cuda and x.is_contiguous() and x.dim() == 2 and x.shape[0] == self.n_channels
        if x.dtype not in (torch.float32, torch.int16):
            raise TypeError("float32 or int16 input")
        k = _u32(in_counts, self.n_channels, "in_counts")
        if k.size and k.max() > x.shape[1]:
            raise SameError(-1, f"an in_count above n_rows = {x.shape[1]}; nothing was consumed")
        ptrs = np.uint64(x.data_ptr()) + np.arange(self.n_channels, dtype=np.uint64) * np.uint64(x.shape[1] * x.element_size())
        return self._process_ptrs(ptrs, k, x.dtype == torch.int16, x.device, y)

    def reset_channels(self, channels, rates=None) -> None:
        """The listed channels start again at this point of the stream (same_resampler_reset_channels); `rates`: their new
        source rates, one per channel listed, or None to keep them.  On an error nothing is reset."""
        ch = _u32(channels, None, "channels")
        r = None if rates is None else _u32(rates, ch.size, "rates")
        _check(self._L.same_resampler_reset_channels(self._h, _p32(ch), ch.size, None if r is None else _p32(r)))

    def channel_input_counter(self, channel: int) -> int:
        return int(self._L.same_resampler_channel_input_counter(self._h, channel))

    def channel_output_counter(self, channel: int) -> int:
        return int(self._L.same_resampler_channel_output_counter(self._h, channel))


class MixedRateReceiver:
    """A `Resampler` in front of a `SameBatchReceiver` at builder.input_rate(): channel c is a source at rates[c].

    `batch_flags` go to `build_batch` (relaxed=True, messages_only=True, ...).  The kinds of batch the ragged call refuses --
    time_parallel, call_invariant, trace_symbols -- are refused here with the batch's own SAME_EINVAL."""

    def __init__(self, builder: SameReceiverBuilder, rates: Sequence[int], device: int = 0, **batch_flags):
        rates = _u32(rates, None, "rates")
        self.batch: SameBatchReceiver = builder.build_batch(int(rates.size), device=device, **batch_flags)
        # an empty ragged call consumes nothing; a batch that takes no ragged calls says so (SameError, EINVAL)
        self.batch.process_host_ragged(np.zeros((0, rates.size), dtype=np.float32), np.zeros(rates.size, dtype=np.uint32))
        self.resampler = Resampler(rates, builder.input_rate(), device)
        self._sources = []           # the source tensors of calls whose resampling may still be running

    @property
    def n_channels(self) -> int:
        return self.batch.n_channels

    def process(self, x, in_counts) -> np.ndarray:
        """x: CUDA tensor [n_rows, C], float32 or int16; channel c consumes its first in_counts[c] rows, samples at rates[c].
        Resamples on torch's current stream into a fresh tensor and hands it to the batch's ragged call, which runs on the
        batch's own stream, ordered behind it.  References to x and to the resampled tensor are held until their kernels can
        no longer be running (two calls later, or `sync()`).  Returns the samples each channel's receiver was given."""
        y, out_counts = self.resampler.process(x, in_counts)
        self._sources.append(x)
        if len(self._sources) > 2:
            del self._sources[0]
        if y.shape[0]:
            self.batch.process_ragged(y, out_counts, LAYOUT_TIME_MAJOR)
        return out_counts

    def process_sources(self, sources) -> np.ndarray:
        """sources: one 1-D contiguous CUDA tensor per channel (all float32 or all int16), or None: the channel's next samples
        at rates[c], each of its own length.  As `process`: resampled on torch's current stream, handed to the batch's ragged
        call, references to the sources and to the resampled tensor held for two calls or until `sync()`."""
        y, out_counts = self.resampler.process_sources(sources)
        self._sources.append(list(sources))
        if len(self._sources) > 2:
            del self._sources[0]
        if y.shape[0]:
            self.batch.process_ragged(y, out_counts, LAYOUT_TIME_MAJOR)
        return out_counts

    def reset_channels(self, channels, rates=None) -> None:
        """Both halves at the same stream position: the channels' resampler clocks and histories (with `rates`: their new
        source rates) and `SameReceiver::reset()` of their receivers."""
        self.resampler.reset_channels(channels, rates)
        self.batch.reset_channels(channels)

    def source_position(self, channel: int, sample_counter: int) -> float:
        """The source sample an event counter of the batch lies at: (counter - delay) * M / L."""
        L, M, _ = self.resampler.plan(channel)
        return (sample_counter - self.resampler.delay(channel)) * M / L

    def flush(self):
        self.batch.flush()

    def sync(self):
        self.batch.sync()
        self._sources.clear()

    def poll_events(self, max_events: int = 1 << 20):
        return self.batch.poll_events(max_events)

    def poll_events_np(self, max_events: int = 1 << 22):
        return self.batch.poll_events_np(max_events)

    def poll_audio(self):
        return self.batch.poll_audio()
