// same_transport.hip -- the transport layer on the device (SAME_BATCH_MESSAGES_ONLY): one lane per channel runs
// same_transport_dev.h over the channel's events of a launch and logs the messages it yields.
//
// The kernel runs behind launch_event_sort, on the launch's stream: the launch's event log is then in column order
// (first[c] .. first[c + 1] of `sorted` are channel c's records, each `channel` field holding the record's index in the
// log).  Inside a range the records stand in the order the scatter's atomics landed; the lane puts them back into log
// order, which is the channel's time order, exactly as the host's replay does (same_harvest.cpp Replay::replay).
#include <hip/hip_runtime.h>

#include "same_device.h"
#include "same_launch.h"
#include "same_capture_dev.h"
#include "same_transport_dev.h"

namespace same {

namespace {

__global__ __launch_bounds__(64) void transport_kernel(TransportLaunch T)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= T.n_channels) return;
    const uint32_t b = T.first[c], e = T.first[c + 1u];
    DevEvent *ev = T.sorted;
    // the range back into log order (insertion sort: a range holds a handful of records)
    for (uint32_t i = b + 1u; i < e; ++i) {
        const DevEvent x = ev[i];
        uint32_t j = i;
        while (j > b && ev[j - 1u].channel > x.channel) { ev[j] = ev[j - 1u]; --j; }
        ev[j] = x;
    }
    // bursts the pool holds: a burst past its capacity has no bytes (length 0; the launch reported SAME_EOVERFLOW)
    const uint32_t n_bursts = min(T.counters[1], T.burst_cap);
    dt::Hot *hot = static_cast<dt::Hot *>(T.hot);
    dt::Hot h = hot[c];
    dt::Transport tr{h, static_cast<dt::Cold *>(T.cold)[c]};
    dt::Msg msg;
    dt::Event out;
    uint32_t seq = 0;
    // same_batch_set_audio_capture: the spans of this launch's rows that belong to an open message (same_capture_dev.h)
    const bool capture = T.cap.rec != nullptr;
    cap::Walker w(T.cap, capture ? c : 0u);
    for (uint32_t i = b; i < e; ++i) {
        const DevEvent d = ev[i];
        const uint8_t *bytes = nullptr;
        uint32_t len = 0;
        if (d.kind == SAME_LINK_BURST && d.burst_slot < n_bursts) {
            bytes = T.bursts + (size_t)d.burst_slot * kBurstCap;
            len = min(d.burst_len, (uint32_t)kBurstCap);
        }
        if (!tr.on_link_event(d.kind, d.sample_counter, d.symbol_count, bytes, len, T.input_rate, msg, &out)) continue;
        if (out.kind != SAME_TRANSPORT_MSG_START && out.kind != SAME_TRANSPORT_MSG_END) continue;
        if (capture) w.on_message(out.kind, out.sample_counter);
        const uint32_t k = atomicAdd(T.log_cursor, 1u);
        if (k >= T.near_cap && k - T.near_cap >= T.log_cap) { atomicOr(T.overflow, kMessageLogOverflow); continue; }
        DevMessage &m = k < T.near_cap ? T.near[k] : T.log[k - T.near_cap];
        m.channel = c; m.kind = out.kind; m.sample_counter = out.sample_counter; m.symbol_count = out.symbol_count;
        m.len = out.len; m.aux = out.aux; m.aux2 = out.aux2; m.seq = seq++;
        if (out.kind == SAME_TRANSPORT_MSG_START) dt::copy_bytes(m.text, out.text, out.len < kDevMessageText ? out.len : kDevMessageText);
    }
    // force_eom_at_sample (receiver.rs:321-328): the demodulation kernels wake the channel after that instant
    // (State::wake_sample); a changed instant is armed for the next launch, which is ordered behind this kernel
    if (tr.force_eom_dirty()) T.wake_sample[c] = tr.force_eom_at();
    hot[c] = h;
    if (capture) w.finish();
}

// A ragged launch (same_batch_process_*_ragged): transport_kernel's lane, where channel c consumed only the first
// k = min(counts[c] - row_sub, n_rows) of the launch's n_rows rows and lags the batch by n_rows - k more when it ends.  Its
// captures stop at its own end, and an armed forced-EOM instant (batch sample coordinates) moves with the lag.  (A function
// of its own: transport_kernel's code stays exactly what it was.)
__global__ __launch_bounds__(64) void transport_ragged_kernel(TransportLaunch T, const uint32_t *__restrict__ counts, uint32_t row_sub,
                                                              uint32_t n_rows)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= T.n_channels) return;
    const uint32_t want = counts[c];
    const uint32_t own = want > row_sub ? min(want - row_sub, n_rows) : 0u;
    const uint32_t b = T.first[c], e = T.first[c + 1u];
    DevEvent *ev = T.sorted;
    for (uint32_t i = b + 1u; i < e; ++i) {
        const DevEvent x = ev[i];
        uint32_t j = i;
        while (j > b && ev[j - 1u].channel > x.channel) { ev[j] = ev[j - 1u]; --j; }
        ev[j] = x;
    }
    const uint32_t n_bursts = min(T.counters[1], T.burst_cap);
    dt::Hot *hot = static_cast<dt::Hot *>(T.hot);
    dt::Hot h = hot[c];
    dt::Transport tr{h, static_cast<dt::Cold *>(T.cold)[c]};
    dt::Msg msg;
    dt::Event out;
    uint32_t seq = 0;
    const bool capture = T.cap.rec != nullptr;
    cap::WalkerT<true> w(T.cap, capture ? c : 0u, own);
    for (uint32_t i = b; i < e; ++i) {
        const DevEvent d = ev[i];
        const uint8_t *bytes = nullptr;
        uint32_t len = 0;
        if (d.kind == SAME_LINK_BURST && d.burst_slot < n_bursts) {
            bytes = T.bursts + (size_t)d.burst_slot * kBurstCap;
            len = min(d.burst_len, (uint32_t)kBurstCap);
        }
        if (!tr.on_link_event(d.kind, d.sample_counter, d.symbol_count, bytes, len, T.input_rate, msg, &out)) continue;
        if (out.kind != SAME_TRANSPORT_MSG_START && out.kind != SAME_TRANSPORT_MSG_END) continue;
        if (capture) w.on_message(out.kind, out.sample_counter);
        const uint32_t k = atomicAdd(T.log_cursor, 1u);
        if (k >= T.near_cap && k - T.near_cap >= T.log_cap) { atomicOr(T.overflow, kMessageLogOverflow); continue; }
        DevMessage &m = k < T.near_cap ? T.near[k] : T.log[k - T.near_cap];
        m.channel = c; m.kind = out.kind; m.sample_counter = out.sample_counter; m.symbol_count = out.symbol_count;
        m.len = out.len; m.aux = out.aux; m.aux2 = out.aux2; m.seq = seq++;
        if (out.kind == SAME_TRANSPORT_MSG_START) dt::copy_bytes(m.text, out.text, out.len < kDevMessageText ? out.len : kDevMessageText);
    }
    // the instant in the coordinates after the launch (the ragged kernel in front of this one moved the device's copy by the
    // lag already: this writes the same value, or the instant this launch armed)
    const bool moved = tr.shift_force_eom(n_rows - own);
    if (tr.force_eom_dirty() || moved) T.wake_sample[c] = tr.force_eom_at();
    hot[c] = h;
    if (capture) w.finish();
}

// SameReceiver::reset() of the transport layer (receiver.rs:195-196): the listed channels, or all of them (cols == nullptr)
// (cap: the channels' capture records, or nullptr: an open capture ends at the reset -- the host queues its END_RESET chunk)
__global__ __launch_bounds__(64) void transport_reset_kernel(dt::Hot *hot, dt::Cold *cold, uint32_t n_channels, const uint32_t *cols,
                                                             uint32_t n, int fresh, cap::Rec *rec)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (cols ? n : n_channels)) return;
    const uint32_t c = cols ? cols[i] : i;
    if (c >= n_channels) return;
    dt::Hot h = hot[c];
    if (fresh) { h = dt::Hot{}; h.state_kind = SAME_TRANSPORT_IDLE; }
    dt::Transport tr{h, cold[c]};
    tr.reset();
    hot[c] = h;
    if (rec) rec[c] = cap::Rec{0, 0, 0};
}

}  // namespace

size_t transport_hot_bytes() { return sizeof(dt::Hot); }
size_t transport_cold_bytes() { return sizeof(dt::Cold); }

hipError_t launch_transport(const TransportLaunch &T, hipStream_t stream)
{
    if (T.n_channels == 0) return hipSuccess;
    hipLaunchKernelGGL(transport_kernel, dim3((T.n_channels + 63u) / 64u), dim3(64), 0, stream, T);
    return hipGetLastError();
}

hipError_t launch_transport_ragged(const TransportLaunch &T, const uint32_t *counts, uint32_t row_sub, uint32_t n_rows, hipStream_t stream)
{
    if (T.n_channels == 0) return hipSuccess;
    hipLaunchKernelGGL(transport_ragged_kernel, dim3((T.n_channels + 63u) / 64u), dim3(64), 0, stream, T, counts, row_sub, n_rows);
    return hipGetLastError();
}

hipError_t launch_transport_reset(void *hot, void *cold, uint32_t n_channels, const uint32_t *cols, uint32_t n, int fresh,
                                  hipStream_t stream, void *capture_rec)
{
    const uint32_t count = cols ? n : n_channels;
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(transport_reset_kernel, dim3((count + 63u) / 64u), dim3(64), 0, stream, static_cast<dt::Hot *>(hot),
                       static_cast<dt::Cold *>(cold), n_channels, cols, n, fresh, static_cast<cap::Rec *>(capture_rec));
    return hipGetLastError();
}

}  // namespace same
