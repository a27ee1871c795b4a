// same_batch.cpp -- host side of the C ABI: owns the per-channel receiver state in HBM,
// launches the gfx950 kernels, and brings the device's append-only event log back for the
// ordered event stream `SameReceiver::iter_events` yields (receiver.rs:119-130, 233-274).
// What turns a launch's log into that stream once it is in host memory -- the replay, the event
// and audio queues -- is host-only code in same_harvest.cpp; everything here launches, waits or copies.
//
// There is deliberately no CPU fallback here: if the HIP runtime or a gfx950 device is
// missing, every compute entry point fails with SAME_ENODEVICE / SAME_EHIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/same_rx.h"
#include "same_config.h"
#include "same_device.h"
#include "same_harvest.h"
#include "same_hipmem.h"
#include "same_launch.h"
#include "same_resets.h"
#include "same_tp_plan.h"
#include "same_transport.h"

using same::fail;        // (the one error channel: same_harvest.h)
static_assert(sizeof(same::cap::Span) == same::kSpanBytes, "same_tp_plan.h sizes the span list");

namespace {

#define HIP_TRY(expr)                                                                     \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail(SAME_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),  \
                        __FILE__, __LINE__);                                               \
    } while (0)

}  // namespace

struct same_batch {
    same_rx_builder builder{};
    same::Params P{};
    same::State S{};
    int device = 0;
    uint32_t flags = 0;
    uint64_t counter = 0;            // input_sample_counter (common to all channels)
    hipStream_t own_stream = nullptr;
    hipStream_t last_stream = nullptr;
    same::DevBuf<float4> d_taps;
    same::DevBuf<void> d_state_blob; // one allocation backing every State array
    // Output of a launch: event log + burst pool + cursors.  Two slots, so the host can
    // harvest launch k (copy back, order, transport layer) while launch k+1 runs.
    struct Slot {
        same::DevBuf<same::DevEvent> d_events;
        uint32_t event_cap() const { return (uint32_t)d_events.size(); }
        // the log's indices ordered by state column, made on the device behind the launch (launch_event_sort)
        same::DevBuf<uint32_t> d_sort;              // cnt [bins] | first [bins + 1] | the scan's workgroup totals
        same::PinnedBuf<uint32_t> h_sort;           // first [bins + 1]
        same::DevBuf<same::DevEvent> d_sorted;      // the log's records in column order
        uint32_t sort_bins = 0;
        same::DevBuf<uint8_t> d_bursts;             // kBurstCap bytes per burst
        uint32_t burst_cap() const { return (uint32_t)(d_bursts.size() / same::kBurstCap); }
        same::DevBuf<uint32_t> d_counters;          // [0] n_events [1] n_bursts [2] overflow
        same::MappedBuf<uint32_t> h_counters;       // their copy the host reads in place
        same::Event ev_start, ev_stop, ev_done, ev_planned;
        same::Event ev_k0, ev_k1;                   // around the demodulation kernel alone (time-parallel launches bracket more with ev_start / ev_stop)
        bool have_k = false;
        bool timed = false;               // ev_start / ev_stop were recorded for this launch (latched when it was made)
        // pinned landing buffers of the read-back, grown on demand.  A copy into pageable memory
        // is staged by the runtime (blit kernel + host memcpy per chunk) and, queued beside the
        // next launch, holds that launch up for as long as the host is busy.
        same::PinnedBuf<void> h_events, h_bursts;
        bool in_flight = false;
        uint64_t seq = 0;                // launch order
        uint64_t end_counter = 0;        // input sample counter after this launch
        // time-parallel launch: geometry, the end of its last whole block, the hand-over instants
        bool chunked = false;
        same::ChunkGeom geom{};
        uint32_t columns(uint32_t n_channels) const { return chunked ? geom.n_chunks * n_channels : n_channels; }      // state columns of the launch
        uint64_t end_blocks = 0;
        same::DevBuf<uint64_t> d_handover;
        same::PinnedBuf<uint64_t> h_handover;
        // per-channel chunk boundaries (channel-major input): device arrays of the launch, host copies for the stitch
        bool per_channel = false;
        same::TpGeomWords words;             // where each array lies in d_geom, and how much of it comes back
        same::DevBuf<uint32_t> d_geom;
        same::PinnedBuf<uint32_t> h_geom;    // own_start | row0
        // what the planning kernels were launched with (same_batch_debug_tp_plan reads it back)
        same::TpPlan plan{};
        uint64_t plan_counter0 = 0;
        bool plan_sorted = false, plan_lpt = false, plan_pairs = false;
        // channels re-initialised in front of this launch (same_batch_reset_channels): read in place by the reset kernel
        same::CoherentBuf<uint32_t> h_reset;
        // a ragged call's per-channel counts (same_batch_process_*_ragged): read in place by the ragged kernel
        same::CoherentBuf<uint32_t> h_counts;
        // the wake table as uploaded behind the launch after this slot's harvest (batches that ran ragged launches)
        same::PinnedBuf<uint64_t> h_wake_up;
        // SAME_BATCH_MESSAGES_ONLY: the launch's message log (same_transport.hip; its cursor is d_counters[3]) and its landing buffer
        bool dev_transport = false;      // this launch ran the transport layer on the device
        // (its first records land in host-mapped pinned memory, read in place; the rest in HBM, copied when there are any)
        same::CoherentBuf<same::DevMessage> h_near;
        uint32_t near_cap() const { return (uint32_t)h_near.size(); }
        same::DevBuf<same::DevMessage> d_msgs;
        uint32_t msg_cap() const { return (uint32_t)d_msgs.size(); }
        same::PinnedBuf<void> h_msgs;
        // same_batch_set_audio_capture: the launch's span list and sample pool (same_capture_dev.h, same_capture.hip), their
        // cursors (device; published to the host-mapped copy by the capture kernel's epilogue) and pinned landing buffers
        bool captured = false;           // this launch ran the capture kernel
        same::DevBuf<same::cap::Span> d_spans;
        uint32_t span_cap() const { return (uint32_t)d_spans.size(); }
        same::DevBuf<float> d_pool;
        same::DevBuf<same::cap::Cursors> d_cap_cur;
        same::MappedBuf<same::cap::Cursors> h_cap_cur;
        same::PinnedBuf<void> h_spans, h_pool;
    } slot[2];
    // time-parallel mode (SAME_BATCH_TIME_PARALLEL)
    struct TimePar {
        bool enabled = false;
        same::TpConfig cfg;                                   // same_batch_time_parallel_config and the mode's knobs (same_tp_plan.h)
        uint32_t cap_columns = 0;                             // columns the wide state blob holds
        uint32_t carved_columns = 0;                          // columns Pv / Sv / the descriptor tables are laid out for
        int carved_family = -1;                               // ... and the kernel family Pv's knobs were set for
        same::Params Pv{};
        same::State Sv{};
        same::DevBuf<void> blob;
        same::DevBuf<void> blob_fresh;                        // the same layout, every column a freshly built receiver: the template a launch's prologue copies
        size_t fresh_bytes = 0;                               // ... and how much of it a launch copies (the [rows][column] arrays; not the framer's rows)
        same::DevBuf<same::StateArrayDesc> d_desc_in, d_desc_out;           // real -> wide, wide -> real
        uint32_t n_desc = 0;
        same::DevBuf<uint32_t> d_final_col;
        same::DevBuf<float> d_energy;                       // scout scratch
        same::DevBuf<float> d_hist;                         // squelch histories by grid position (PipeChunks::hist_scratch)
        same::Event ev_plan_prev; bool plan_recorded = false;
        uint32_t last_chunks = 1;
        bool last_per_channel = false;
        same::Family family = same::Family::kPipe;            // which kernel runs the chunks of the launch being queued (TpCut::choice)
    } tp;
    uint64_t launch_seq = 0;
    hipStream_t copy_stream = nullptr;   // read-back of finished launches, beside the compute stream
    // SAME_BATCH_CALL_INVARIANT: the stream is demodulated in windows of kInvWindow samples that begin at fixed positions of the
    // STREAM (multiples of the window from the batch's first sample, or from its last flush / reset), whatever the calls that
    // deliver it look like: samples wait in `d_buf` (f32, time-major) until their window is whole
    struct Windowed {
        bool on = false;
        uint32_t window = 0;           // samples per window
        uint32_t fill = 0;             // samples of the current window that have arrived
        same::DevBuf<void> d_buf;
        same::Event ev_buf;            // behind the last operation on d_buf (a later call may come on another stream)
        hipStream_t buf_stream = nullptr; bool buf_used = false;
        // behind the last operation of each of the two latest process calls that read the caller's buffer (or the batch's
        // staging / upload buffers): call k waits for call k - 2's before it returns (inv_reads_end)
        same::Event ev_read[2];
        uint64_t n_reads = 0;          // process calls so far; the latest one's event is ev_read[(n_reads - 1) & 1]
        hipStream_t read_stream = nullptr;
    } inv;
    // Time-parallel launches on the library's own stream: scout, planner and sort of call k + 1 run here, beside the tail of
    // launch k (whose short workgroups have left their CUs by then); the own stream waits for them (Slot::ev_planned)
    hipStream_t plan_stream = nullptr;
    float last_ms = 0.0f;
    bool overflowed = false;
    std::string record_path;         // SAME_RECORD_HARVEST (measurement aid of tools/host_step_probe.py: read once per batch, like every knob)
    bool kernel_fault = false;       // counters[2] bit 2: a wavefront pipeline's bounded hand-over wait ran out (same_kernels_sym.hip)
    // which kernel runs a launch (same_select.h): what the batch was created with, its arithmetic mode, the block kernel of its
    // ordinary launches (fixed with the batch: P and the knobs never change) and the family same_batch_kernel_name reports
    same::Request want;
    same::Mode mode;
    same::Choice plain;
    same::Params Pfm{};              // fm_params(P): what the relaxed pipelines launch with
    same::Family last_family = same::Family::kGeneric;
    bool sym_launched = false;       // an ordinary launch has run the symbol-paced pipeline (until then its name is the FASTMATH build's, whose place it takes)
    bool debug = false;              // SAME_DEBUG: harvest statistics on stderr
    // staging for host / channel-major inputs
    same::DevBuf<void> d_stage, d_stage2;
    same::DevBuf<void> d_upload;                            // host-buffer entry points: grow-only upload slab
    same::DevBuf<void> d_zero;                              // flush: grow-only slab of zeros
    same::Event ev_order;                                   // same_batch_order_after
    // kernel timing
    bool timing = false;
    bool have_timing = false;
    float last_demod_ms = 0.0f;         // the demodulation kernel alone (= last_ms unless the launch brackets planning kernels too)
    same::PinnedBuf<uint64_t> h_wake; // host mirror of State::wake_sample (n_channels words, zero = unarmed)
    // A ragged launch moves the device's wake-up instants itself (the ragged kernel), in stream order.  From the first one on the
    // host's re-arming of the table is stream-ordered as well (behind the launch in flight, with its shifts added), so that an
    // upload can no longer land across a ragged launch and undo its shift.
    bool wake_ordered = false;
    std::vector<uint32_t> ragged_by;  // scratch: the counter shifts of the ragged launch being queued
    // SAME_BATCH_MESSAGES_ONLY: only MSG_START / MSG_END are queued; unless the batch is time-parallel the transport layer runs on
    // the device (same_transport.hip) over per-channel records in HBM, and the device arms State::wake_sample itself
    bool messages_only = false;
    bool dev_transport = false;
    bool last_dev_transport = false; // the last process call's launches ran it there (same_batch_transport_on_device)
    same::DevBuf<void> d_thot, d_tcold;
    // per-channel resets (same_batch_reset_channels): where each half of a reset is due, the channels' counter bases
    same::ResetLedger resets;
    std::vector<uint32_t> reset_list, reset_now, reset_cols;       // scratch: the entry point's, the reset kernel's list
    // the host half of the harvest (same_harvest.h): the ordered host-side event queue, and the channels' host state (transport
    // layer, time-parallel symbol clocks) with the replay of a launch's log over it, its worker threads and SAME_HOST_THREADS
    same::EventLog events;
    same::Replay replay{resets, events};
    // alert audio per message (same_batch_set_audio_capture)
    struct Audio {
        size_t per_launch = 0;                   // pool samples per slot; 0: capture is off
        same::DevBuf<same::cap::Rec> d_rec;      // per channel: the device's capture record
        uint64_t flush_at = UINT64_MAX;          // batch counter where the running same_batch_flush began
        same::AudioLog log;                      // the queued chunks, and which channels have a capture open
    } audio;
};

namespace {

struct Carver {
    size_t off = 0;
    template <typename T> size_t take(size_t n)
    {
        off = (off + 255) & ~size_t(255);
        size_t o = off;
        off += n * sizeof(T);
        return o;
    }
};

// every State array that is laid out [rows][channel]: field, element type, rows
#define SAME_STATE_ARRAYS(X, P)                                                                            \
    X(dc_ff_ring, float, (P).dc_len) X(dc_fb_ring, float, (P).dc_len)                                        \
    X(dc_sum0, float, 1) X(dc_sum1, float, 1) X(agc_gain, float, 1)                                          \
    X(win_ring, float, (P).win_ring)                                                                         \
    X(ted_clock, uint32_t, 1) X(until_next_ted, float, 1)                                                    \
    X(ted_h0, float, 1) X(ted_h1, float, 1) X(ted_h2, float, 1)                                              \
    X(period_avg, float, 1) X(period_inst, float, 1)                                                         \
    X(sq_data, uint32_t, 1) X(sq_power, float, 1) X(sq_phist, uint32_t, 1)                                   \
    X(sq_fill, uint32_t, 1) X(sq_clock, int32_t, 1) X(sq_symbols, uint64_t, 1)                               \
    X(sq_hist, float, same::kSquelchHist)                                                                    \
    X(eq_ffc, float, (P).eq_nff) X(eq_fbc, float, (P).eq_nfb)                                                \
    X(eq_ffw, float, (P).eq_nff) X(eq_fbw, float, (P).eq_nfb)                                                \
    X(eq_word, uint32_t, 1) X(eq_count, uint32_t, 1)                                                         \
    X(eq_snap_ffc, float, (P).eq_nff) X(eq_snap_fbc, float, (P).eq_nfb)                                      \
    X(eq_snap_ffw, float, (P).eq_nff) X(eq_snap_fbw, float, (P).eq_nfb)                                      \
    X(fr_word, uint32_t, 1) X(fr_count, uint32_t, 1) X(fr_invalid, uint32_t, 1) X(fr_len, uint32_t, 1)       \
    X(flags, uint32_t, 1)                                                                                    \
    X(tk_next, uint64_t, 1) X(tk_last, uint64_t, 1) X(tk_ring, uint64_t, same::kTickRing)                    \
    X(tk_n, uint32_t, 1) X(wake_sample, uint64_t, 1) X(wake_fired, uint64_t, 1)

// lays out every State array inside one blob; with base == nullptr only sizes it
size_t carve_state(const same::Params &P, char *base, same::State &S)
{
    const size_t C = P.n_channels;
    Carver cv;
#define CARVE(field, type, count) \
    do { size_t o = cv.take<type>(count); if (base) S.field = reinterpret_cast<type *>(base + o); } while (0)
#define CARVE_ROWS(field, type, rows) CARVE(field, type, (size_t)(rows) * C);
    SAME_STATE_ARRAYS(CARVE_ROWS, P)
#undef CARVE_ROWS
    CARVE(fr_msg, uint8_t, (size_t)same::kBurstCap * C);      // [channel][kBurstCap]
    if (P.trace_cap) {
        CARVE(trace_n, uint32_t, C);
        CARVE(trace, float, (size_t)P.trace_cap * 4 * C);
        CARVE(trace_idx, uint64_t, (size_t)P.trace_cap * C);
    }
#undef CARVE
    return (cv.off + 255) & ~size_t(255);
}

// the same arrays as (source, destination) pairs for launch_copy_state_columns (no trace arrays: the
// time-parallel mode does not record one)
void list_state_arrays(const same::Params &P, const same::State &src, const same::State &dst,
                       std::vector<same::StateArrayDesc> &out)
{
    out.clear();
#define DESC_ROWS(field, type, rows)                                                                     \
    out.push_back(same::StateArrayDesc{reinterpret_cast<char *>(src.field), reinterpret_cast<char *>(dst.field), \
                                       (uint32_t)(rows), (uint32_t)(sizeof(type) / 4)});
    SAME_STATE_ARRAYS(DESC_ROWS, P)
#undef DESC_ROWS
    static_assert(same::kBurstCap % 4 == 0, "framer rows are copied in words");
    out.push_back(same::StateArrayDesc{reinterpret_cast<char *>(src.fr_msg), reinterpret_cast<char *>(dst.fr_msg), 1u,
                                       (uint32_t)(same::kBurstCap / 4)});
}

// every environment knob of the library, read once per batch
void read_knobs(same_batch *rx)
{
    auto num = [](const char *name, int unset) { const char *e = std::getenv(name); return e ? std::atoi(e) : unset; };
    auto tri = [](const char *name) { const char *e = std::getenv(name); return e ? (std::atoi(e) ? 1 : -1) : 0; };
    rx->P.knob_pipe = tri("SAME_PIPE");
    rx->P.knob_pipe_lanes = num("SAME_PIPE_LANES", 0);
    rx->P.knob_pipe_split = tri("SAME_PIPE_SPLIT");            // (test knob: tests/test_gpu_parity.py pits the two stage-2 forms against each other)
#ifdef SAME_PROFILE
    // measurement knobs: read by profile builds only (python -m sameold_amd.build with SAME_PROFILE set), never by the shipped library
    rx->P.knob_mirror = tri("SAME_MIRROR");
    rx->P.knob_pipe_share = tri("SAME_PIPE_SHARE");
    rx->P.knob_prio = num("SAME_PIPE_PRIO", 0);
#endif
    rx->P.knob_fast_dense = tri("SAME_FAST_DENSE");
    rx->P.knob_sym = tri("SAME_SYM");
    rx->want.sym_max_channels = (uint32_t)std::max(0, num("SAME_SYM_MAX", 1 << 30));     // (measurement knob: up to where an ordinary relaxed launch takes the symbol-paced pipeline; default: always)
    rx->debug = rx->replay.debug = std::getenv("SAME_DEBUG") != nullptr;
    { const char *e = std::getenv("SAME_RECORD_HARVEST"); rx->record_path = e ? e : ""; }
    rx->replay.host_threads = std::max(0, num("SAME_HOST_THREADS", 0));
    rx->tp.cfg.sort_mode = num("SAME_TP_SORT", -1);
    rx->tp.cfg.knob_plan_stream = tri("SAME_TP_PLAN_STREAM");
    rx->tp.cfg.knob_prologue = tri("SAME_TP_PROLOGUE");
    rx->want.knob_relaxed = tri("SAME_RELAXED");
    { const char *e = std::getenv("SAME_RELAXED_KERNEL"); rx->P.knob_relaxed_kernel = !e ? 0 : (std::strcmp(e, "solo") == 0 ? 1 : (std::strcmp(e, "duo") == 0 ? 2 : 0)); }
    { const char *e = std::getenv("SAME_TP_KERNEL"); rx->want.knob_tp_kernel = !e ? 0 : (std::strcmp(e, "wave") == 0 ? 2 : (std::strcmp(e, "pipe") == 0 ? 1 : 0)); }
}

// the launch's output buffers, sized by output_caps (same_tp_plan.h); n_columns: the state columns of a time-parallel launch
int ensure_output(same_batch *rx, same_batch::Slot &sl, size_t n_samples, same::Output &O, size_t n_columns = 0)
{
    const same::OutputCaps caps = same::output_caps(rx->P, n_samples, n_columns, rx->dev_transport, rx->audio.per_launch != 0, sl.near_cap(), sl.msg_cap());
    HIP_TRY(sl.d_events.ensure(caps.events));
    HIP_TRY(sl.d_bursts.ensure(caps.bursts * same::kBurstCap));
    if (caps.messages) HIP_TRY(sl.d_msgs.ensure(caps.messages));
    if (caps.near) HIP_TRY(sl.h_near.ensure(caps.near));
    if (caps.spans) HIP_TRY(sl.d_spans.ensure(caps.spans));
    HIP_TRY(sl.d_sorted.ensure(sl.d_events.size()));
    HIP_TRY(sl.d_sort.ensure(caps.sort_words));
    HIP_TRY(sl.h_sort.ensure(caps.bins + 1));
    sl.sort_bins = (uint32_t)caps.bins;
    O.events = sl.d_events; O.event_cap = sl.event_cap();
    O.bursts = sl.d_bursts; O.burst_cap = sl.burst_cap();
    O.n_events = sl.d_counters; O.n_bursts = sl.d_counters + 1; O.overflow = sl.d_counters + 2;
    return SAME_OK;
}

// The block kernel of family `f` over n_blocks whole blocks (pc: the chunks of a time-parallel launch; the one-wavefront kernel
// takes ordinary launches only)
template <typename SampleT>
hipError_t launch_family(same::Family f, const same::Params &P, const same::State &S, const same::Output &O, const float4 *taps, const SampleT *x,
                         uint32_t n_blocks, uint64_t counter0, hipStream_t stream, const same::PipeChunks &pc = same::PipeChunks{})
{
    switch (f) {
    case same::Family::kSym: return same::launch_demod_sym(P, S, O, taps, x, n_blocks, counter0, stream, pc);
    case same::Family::kPipeFastmath: return same::launch_demod_pipe(P, S, O, taps, x, n_blocks, counter0, stream, pc, true);
    case same::Family::kPipe: return same::launch_demod_pipe(P, S, O, taps, x, n_blocks, counter0, stream, pc, false);
    case same::Family::kWaveRelaxed: return same::launch_demod_relaxed(P, S, O, taps, x, n_blocks, counter0, stream, pc);
    case same::Family::kFast: return same::launch_demod_fast(P, S, O, taps, x, n_blocks, counter0, stream);
    case same::Family::kGeneric: break;
    }
    return hipErrorInvalidValue;
}

// The host half of a reset of channel c at stream position `pos` (same_batch_reset_channels): the channel's host state
// (Replay::reset_channel); the channel's wake-up entry is cleared (the reset kernel clears the device's copy)
void reset_channel_host(same_batch *rx, uint32_t c, uint64_t pos)
{
    rx->replay.reset_channel(c, pos);
    if (rx->h_wake) rx->h_wake[c] = 0;
}

// The device half of the resets asked for since the last launch: the channels' state columns re-initialised on the stream of
// the launch about to be queued, in front of it.  The list goes through this slot's pinned buffer, which the kernel reads in
// place (no copy in the stream); the slot's previous launch -- and the reset kernel in front of it -- has been harvested.
int launch_pending_resets(same_batch *rx, same_batch::Slot &sl, hipStream_t stream)
{
    if (rx->resets.device.empty()) return SAME_OK;
    std::vector<uint32_t> &cols = rx->reset_cols;
    rx->resets.take_device(cols);
    const uint32_t n = (uint32_t)cols.size();
    if (n > sl.h_reset.size()) HIP_TRY(sl.h_reset.ensure(std::max<uint32_t>(256u, n + n / 2u)));
    std::memcpy(sl.h_reset, cols.data(), (size_t)n * sizeof(uint32_t));
    hipError_t e = same::launch_reset_columns(rx->P, rx->S, sl.h_reset.dev(), n, stream);
    // (SAME_BATCH_MESSAGES_ONLY: the transport layer lives on the device, and is reset there at the same position)
    if (e == hipSuccess && rx->dev_transport)
        e = same::launch_transport_reset(rx->d_thot, rx->d_tcold, rx->P.n_channels, sl.h_reset.dev(), n, 0, stream, rx->audio.d_rec);
    if (e != hipSuccess) return fail(SAME_EHIP, "channel reset launch failed: %s", hipGetErrorString(e));
    return SAME_OK;
}

// SAME_RECORD_HARVEST=<path>: the third harvest of a batch writes what the host half reads to <path> (same_harvest.h)
int record_harvest(same_batch *rx, same_batch::Slot &sl, const same::HarvestInput &in, uint32_t n_events, uint32_t n_bursts, const char *path)
{
    if (sl.seq != 3u) return SAME_OK;
    const uint32_t n_ch = rx->P.n_channels, n_bins = sl.columns(n_ch);
    same::HarvestFileHeader h{};
    h.n_channels = n_ch; h.n_bins = n_bins; h.n_events = n_events; h.n_bursts = n_bursts;
    h.chunked = sl.chunked; h.per_channel = sl.per_channel; h.flags = rx->flags; h.input_rate = rx->P.input_rate; h.tp_enabled = rx->tp.enabled;
    h.geom = sl.geom; h.end_blocks = sl.end_blocks; h.end_counter = sl.end_counter;
    return same::write_harvest_file(path, h, in);
}

// a pinned landing buffer of at least `need` bytes
hipError_t grow_pinned(same::PinnedBuf<void> &b, size_t need)
{
    return need <= b.size() ? hipSuccess : b.ensure(need + need / 2 + 4096);
}

// The audio of a launch that captured (same_capture.hip): the spans and the used part of the pool come back on the copy stream
// (nothing when no capture was open), then go to the queue by (channel, emission order) -- a lane lists its spans in counter order.
int harvest_audio(same_batch *rx, same_batch::Slot &sl)
{
    sl.captured = false;
    same_batch::Audio &A = rx->audio;
    const same::cap::Cursors cur = *sl.h_cap_cur.get();
    if (cur.overflow) rx->overflowed = true;
    const uint32_t n_spans = std::min(cur.n_spans, sl.span_cap());
    if (!n_spans) return SAME_OK;
    const size_t used = (size_t)std::min<unsigned long long>(cur.pool_used, (unsigned long long)A.per_launch);
    HIP_TRY(grow_pinned(sl.h_spans, (size_t)n_spans * sizeof(same::cap::Span)));
    HIP_TRY(hipMemcpyAsync(sl.h_spans, sl.d_spans, (size_t)n_spans * sizeof(same::cap::Span), hipMemcpyDeviceToHost, rx->copy_stream));
    if (used) {
        HIP_TRY(grow_pinned(sl.h_pool, used * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(sl.h_pool, sl.d_pool, used * sizeof(float), hipMemcpyDeviceToHost, rx->copy_stream));
    }
    HIP_TRY(hipStreamSynchronize(rx->copy_stream));
    const same::cap::Span *sp = static_cast<const same::cap::Span *>(sl.h_spans.get());
    const float *pool = static_cast<const float *>(sl.h_pool.get());
    size_t n_samples = 0;
    if (const int arc = A.log.append_spans(sp, n_spans, pool, used, rx->resets, &n_samples)) return arc;
    if (rx->debug)
        std::fprintf(stderr, "[same] audio: %u chunks, %zu samples (pool %zu of %zu)%s\n", n_spans, n_samples, used, A.per_launch,
                     cur.overflow ? ", truncated" : "");
    return SAME_OK;
}

// The harvest of a launch that ran the transport layer on the device (SAME_BATCH_MESSAGES_ONLY): its message log is all that
// comes back -- no event log, no burst pool, no replay.  The log's order across lanes is that of their atomics; the queue
// takes it by channel and, per channel, in the order the lane logged it (= iter_events() filtered to messages).
int harvest_messages(same_batch *rx, same_batch::Slot &sl, std::chrono::steady_clock::time_point t_begin,
                     std::chrono::steady_clock::time_point t_waited)
{
    const uint32_t n_msgs = std::min(sl.h_counters[3], sl.near_cap() + sl.msg_cap());
    const uint32_t n_near = std::min(n_msgs, sl.near_cap()), n_far = n_msgs - n_near;
    const size_t far_bytes = (size_t)n_far * sizeof(same::DevMessage);
    if (n_far) {
        HIP_TRY(grow_pinned(sl.h_msgs, far_bytes));
        HIP_TRY(hipMemcpyAsync(sl.h_msgs, sl.d_msgs, far_bytes, hipMemcpyDeviceToHost, rx->copy_stream));
        HIP_TRY(hipStreamSynchronize(rx->copy_stream));
    }
    auto t_copied = std::chrono::steady_clock::now();
    const same::DevMessage *far = static_cast<const same::DevMessage *>(sl.h_msgs.get());
    if (const int mrc = rx->replay.append_messages(sl.h_near.get(), n_near, far, n_far)) return mrc;
    if (sl.captured) {
        const int arc = harvest_audio(rx, sl);
        if (arc) return arc;
    }
    const int si = (int)(&sl - rx->slot);
    // a ragged launch's counter shifts (the device moved its own forced-EOM instants), before the resets at the same position
    rx->resets.shift_due(si);
    rx->resets.done_shift(si);
    // the harvest has reached the resets asked for behind this launch: their host half (the counter bases) is due
    // (the open captures of the channels end there, in their counters before the reset)
    if (const int arc = rx->audio.log.end_reset(rx->resets.slot[si & 1].channels, rx->resets.rec_pos(si), rx->resets)) return arc;
    for (uint32_t c : rx->resets.host_due(si)) reset_channel_host(rx, c, rx->resets.rec_pos(si));
    rx->resets.done_host(si);
    if (rx->debug) {
        auto t_end = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "[same] harvest timing: wait %.2f ms, copy %.2f ms, %u messages queued in %.2f ms (transport layer on the device)\n",
                     ms(t_begin, t_waited), ms(t_waited, t_copied), n_msgs, ms(t_copied, t_end));
    }
    return SAME_OK;
}

// The wake table re-armed in stream order (batches that ran ragged launches): the launch still in flight, if any, moves its
// channels' instants on the device as it ends (demod_kernel's RAGGED form), so the table goes in behind it with that launch's shifts
// added -- what the device would hold had the host's values been there before it.  The copy is queued on that launch's stream
// and its done event moves behind the copy (later launches, harvests and the input-lifetime contract wait for that event).
// The pinned source is the harvested slot's: the next write to it is that slot's next harvest, behind the copy.
int upload_wake_ordered(same_batch *rx, same_batch::Slot &sl)
{
    const uint32_t C = rx->P.n_channels;
    HIP_TRY(sl.h_wake_up.ensure(C));
    same_batch::Slot &other = rx->slot[(&sl - rx->slot) ^ 1];
    const int oi = (int)(&other - rx->slot);
    for (uint32_t c = 0; c < C; ++c) {
        const uint64_t w = rx->h_wake[c];
        sl.h_wake_up[c] = w && other.in_flight ? w + rx->resets.pending_shift(oi, c) : w;
    }
    if (other.in_flight) {
        HIP_TRY(hipMemcpyAsync(rx->S.wake_sample, sl.h_wake_up, (size_t)C * sizeof(uint64_t), hipMemcpyHostToDevice, rx->last_stream));
        HIP_TRY(hipEventRecord(other.ev_done, rx->last_stream));
    } else {
        HIP_TRY(hipMemcpyAsync(rx->S.wake_sample, sl.h_wake_up, (size_t)C * sizeof(uint64_t), hipMemcpyHostToDevice, rx->copy_stream));
        HIP_TRY(hipStreamSynchronize(rx->copy_stream));
    }
    return SAME_OK;
}

// Collect the finished launch (device half): wait for it, copy its ordered log, burst pool and geometry back
int harvest_slot(same_batch *rx, same_batch::Slot &sl)
{
    if (!sl.in_flight) return SAME_OK;
    const bool dbg = rx->debug;
    auto t_begin = std::chrono::steady_clock::now();
    // wait for THIS launch only (its cursors have landed in pinned memory); a later launch
    // may still be running on the compute stream
    HIP_TRY(hipEventSynchronize(sl.ev_done));
    sl.in_flight = false;
    if (sl.timed) {
        HIP_TRY(hipEventElapsedTime(&rx->last_ms, sl.ev_start, sl.ev_stop));
        rx->last_demod_ms = rx->last_ms;
        if (sl.have_k) HIP_TRY(hipEventElapsedTime(&rx->last_demod_ms, sl.ev_k0, sl.ev_k1));
        rx->have_timing = true;
    }
    auto t_waited = std::chrono::steady_clock::now();
    const uint32_t n_events = std::min(sl.h_counters[0], sl.event_cap());
    if (dbg)
        std::fprintf(stderr, "[same] harvest: %u device events (%u bursts), cap %u/%u\n", sl.h_counters[0],
                     sl.h_counters[1], sl.event_cap(), sl.burst_cap());
    const uint32_t n_bursts = std::min(sl.h_counters[1], sl.burst_cap());
    if (sl.h_counters[2] & (3u | same::kMessageLogOverflow)) rx->overflowed = true;
    if (sl.h_counters[2] & 4u) rx->kernel_fault = true;
    if (sl.dev_transport) return harvest_messages(rx, sl, t_begin, t_waited);
    const size_t ev_bytes = (size_t)n_events * sizeof(same::DevEvent), bu_bytes = (size_t)n_bursts * same::kBurstCap;
    HIP_TRY(grow_pinned(sl.h_events, ev_bytes));
    HIP_TRY(grow_pinned(sl.h_bursts, bu_bytes));
    // the event log first: it is what the sort below needs, and the sort runs while the burst pool (the larger copy) and
    // the chunk geometry are still on their way
    const uint32_t n_bins = sl.columns(rx->P.n_channels);
    if (n_bins != sl.sort_bins) return fail(SAME_EINVAL, "internal: event sort made for %u columns, launch has %u", sl.sort_bins, n_bins);
    // (the log arrives ordered by column, with the columns' offsets: the device did that behind the launch; at most
    // n_events records are real, the exact count is the last offset)
    HIP_TRY(hipMemcpyAsync(sl.h_sort, sl.d_sort + n_bins, ((size_t)n_bins + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, rx->copy_stream));
    if (n_events) HIP_TRY(hipMemcpyAsync(sl.h_events, sl.d_sorted, ev_bytes, hipMemcpyDeviceToHost, rx->copy_stream));
    HIP_TRY(hipStreamSynchronize(rx->copy_stream));
    if (n_bursts) HIP_TRY(hipMemcpyAsync(sl.h_bursts, sl.d_bursts, bu_bytes, hipMemcpyDeviceToHost, rx->copy_stream));
    if (sl.chunked) {
        HIP_TRY(hipMemcpyAsync(sl.h_handover, sl.d_handover, (size_t)n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, rx->copy_stream));
        if (sl.per_channel)
            HIP_TRY(hipMemcpyAsync(sl.h_geom, sl.d_geom + sl.words.own_start, sl.words.harvest * sizeof(uint32_t), hipMemcpyDeviceToHost, rx->copy_stream));
    }
    if (n_bursts || sl.chunked) HIP_TRY(hipStreamSynchronize(rx->copy_stream));      // bursts, hand-overs, geometry
    auto t_copied = std::chrono::steady_clock::now();
    const same::HarvestInput in{sl.h_sort, static_cast<same::DevEvent *>(sl.h_events.get()), static_cast<const uint8_t *>(sl.h_bursts.get()),
                                sl.h_handover, sl.h_geom};
    if (!rx->record_path.empty()) { const int rrc = record_harvest(rx, sl, in, n_events, n_bursts, rx->record_path.c_str()); if (rrc != SAME_OK) return rrc; }
    std::vector<uint32_t> rearm;     // channels whose forced-EOM instant changed
    same::HarvestTimes times;
    same::HarvestLaunch launch;
    launch.chunked = sl.chunked; launch.per_channel = sl.per_channel; launch.geom = sl.geom;
    launch.end_blocks = sl.end_blocks; launch.end_counter = sl.end_counter;
    int rc = rx->replay.replay(launch, in, n_events, n_bursts, rearm, times);
    if (rc) return rc;
    // a ragged launch's counter shifts are due now that its own events are replayed: the channels' armed forced-EOM instants
    // move with them (and are re-armed), then the queued records' counter bases
    {
        const int si = (int)(&sl - rx->slot);
        const same::ResetLedger::SlotShift &sh = rx->resets.shift_due(si);
        if (!rx->replay.thot.empty())
            for (size_t i = 0; i < sh.channels.size(); ++i)
                if (rx->replay.tr(sh.channels[i]).shift_force_eom(sh.by[i])) rearm.push_back(sh.channels[i]);
        rx->resets.done_shift(si);
    }
    // the harvest has reached the resets asked for behind this launch: their host half is due (before the wake table is
    // re-armed below, so that a reset channel's entry goes back to the device as 0)
    {
        const int si = (int)(&sl - rx->slot);
        const std::vector<uint32_t> &due = rx->resets.host_due(si);
        for (uint32_t c : due) reset_channel_host(rx, c, rx->resets.rec_pos(si));
        rx->resets.done_host(si);
    }
    // force_eom_at_sample (receiver.rs:321-328) lives on the host; tell the device when to
    // wake the transport layer for it.  Launches are capped well below the 135 s timeout,
    // so the instant is always armed before the device reaches it.
    if (!rearm.empty()) {
        // one upload of the whole wake table (a device word the kernel already cleared is
        // re-armed at worst to an instant in the past: one harmless extra poll)
        if (!rx->h_wake) {
            HIP_TRY(rx->h_wake.ensure(rx->P.n_channels));
            std::memset(rx->h_wake, 0, (size_t)rx->P.n_channels * sizeof(uint64_t));
        }
        for (uint32_t c : rearm) rx->h_wake[c] = rx->replay.tr(c).force_eom_at();
        if (rx->wake_ordered) {
            int rc2 = upload_wake_ordered(rx, sl);
            if (rc2) return rc2;
        } else {
        // the kernels only read this table (it is host-owned), so it may be updated while a
        // later launch runs; launches are capped at 45 s, two launches < the 135 s timeout
        HIP_TRY(hipMemcpyAsync(rx->S.wake_sample, rx->h_wake, (size_t)rx->P.n_channels * sizeof(uint64_t), hipMemcpyHostToDevice, rx->copy_stream));
        HIP_TRY(hipStreamSynchronize(rx->copy_stream));
        }
    }
    if (dbg) {
        auto t_end = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "[same] harvest timing: wait %.2f ms, copy %.2f ms, sort %.2f ms, replay on %u threads %.2f ms, "
                             "queue %.2f ms\n",
                     ms(t_begin, t_waited), ms(t_waited, t_copied), ms(t_copied, times.sorted), times.n_threads,
                     ms(times.sorted, times.replayed), ms(times.replayed, t_end));
    }
    return SAME_OK;
}

// harvest every launch still in flight, oldest first
int harvest(same_batch *rx)
{
    same_batch::Slot *order[2] = {&rx->slot[0], &rx->slot[1]};
    if (order[0]->seq > order[1]->seq) std::swap(order[0], order[1]);
    for (same_batch::Slot *sl : order) {
        int rc = harvest_slot(rx, *sl);
        if (rc) return rc;
    }
    return SAME_OK;
}

// the wide state blob: `columns` state columns laid out like the channel state, plus the copy tables
int ensure_wide_state(same_batch *rx, uint32_t columns)
{
    same_batch::TimePar &tp = rx->tp;
    if (tp.carved_columns == columns && tp.carved_family == (int)tp.family) return SAME_OK;
    int rc = harvest(rx);                    // nothing in flight may still use the old layout
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    tp.Pv = same::wide_params(rx->P, columns, same::is_fastmath(tp.family), same::tp_more_than_one_round(columns));
    if (columns > tp.cap_columns) {
        // (both go before either comes back: the two are the batch's largest allocations)
        tp.cap_columns = 0;
        HIP_TRY(tp.blob.reset());
        HIP_TRY(tp.blob_fresh.reset());
        const size_t bytes = carve_state(tp.Pv, nullptr, tp.Sv);
        HIP_TRY(tp.blob.ensure(bytes));
        HIP_TRY(hipMemset(tp.blob, 0, bytes));
        HIP_TRY(tp.blob_fresh.ensure(bytes));
        tp.cap_columns = columns;
    }
    const size_t blob_bytes = carve_state(tp.Pv, (char *)tp.blob.get(), tp.Sv);
    {
        // The template of a launch's fresh state columns (launch_tp_prologue): this layout with SameReceiver::from's state in
        // every column (receiver.rs:539-558), made once per layout by the kernel that used to run over the columns of every launch
        same::State Sf{};
        carve_state(tp.Pv, (char *)tp.blob_fresh.get(), Sf);
        HIP_TRY(hipMemset(tp.blob_fresh, 0, blob_bytes));
        HIP_TRY(same::launch_init_state(tp.Pv, Sf, 0, nullptr, 0));
        HIP_TRY(hipDeviceSynchronize());
        tp.fresh_bytes = (size_t)(reinterpret_cast<char *>(tp.Sv.fr_msg) - static_cast<char *>(tp.blob.get()));      // (carved in 256-byte steps)
    }
    std::vector<same::StateArrayDesc> in, out;
    list_state_arrays(rx->P, rx->S, tp.Sv, in);
    list_state_arrays(rx->P, tp.Sv, rx->S, out);
    tp.n_desc = (uint32_t)in.size();
    HIP_TRY(tp.d_desc_in.ensure(in.size()));
    HIP_TRY(tp.d_desc_out.ensure(out.size()));
    HIP_TRY(tp.d_final_col.ensure(rx->P.n_channels));
    HIP_TRY(hipMemcpy(tp.d_desc_in, in.data(), in.size() * sizeof(same::StateArrayDesc), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(tp.d_desc_out, out.data(), out.size() * sizeof(same::StateArrayDesc), hipMemcpyHostToDevice));
    tp.carved_columns = columns;
    tp.carved_family = (int)tp.family;
    return SAME_OK;
}

// A ragged call (same_batch_process_*_ragged) as the launches of one time-major piece see it: the call's per-channel counts
// (host, n_channels entries), the smallest of them and the call row of the piece's first row
struct Ragged {
    const uint32_t *counts = nullptr;
    uint32_t m = 0;
    uint32_t row_off = 0;
};

// One launch of a ragged call: the call row of its first row, and how many of its rows every channel consumes
struct RaggedLaunch {
    uint32_t row0 = 0;
    size_t n_lock = 0;
};

// ---- The pieces every launch is made of.  process_time_major_launches and process_channel_major_native queue them in this order:
// begin_launch, the demodulation kernels and a sub-block tail (a time-parallel launch, of either layout: launch_time_parallel),
// end_launch; how the call is cut is same_tp_plan.h's, the ragged remainder the caller's. ----

// The begin of a launch into `sl`: the slot's previous launch is collected (its buffers are about to be reused), the stream is
// ordered behind the launch before this one, and the channel resets asked for since then go in front
int begin_launch(same_batch *rx, same_batch::Slot &sl, const same_batch::Slot &prev, hipStream_t stream)
{
    int rc = harvest_slot(rx, sl);
    if (rc) return rc;
    // a launch continues the state the previous one leaves: on another stream than that one, wait for it
    if (prev.in_flight && rx->last_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, prev.ev_done, 0));
    return launch_pending_resets(rx, sl, stream);
}

// kernel timing is latched per launch: ev_start goes in front of the launch's first kernel
int begin_timing(same_batch *rx, same_batch::Slot &sl, hipStream_t stream)
{
    sl.timed = rx->timing;
    if (sl.timed) HIP_TRY(hipEventRecord(sl.ev_start, stream));
    return SAME_OK;
}

// The start of a time-parallel launch on the stream: fresh receivers in every column (with the hand-over records, the event sort's bins and the
// launch cursors: one kernel, launch_tp_prologue), then the channels' own state into chunk 0's columns.
// *sort_bins_empty: the prologue kernel has emptied the event sort's bins
int tp_start(same_batch *rx, same_batch::Slot &sl, uint32_t columns, const char *layout, hipStream_t stream, bool *sort_bins_empty)
{
    same_batch::TimePar &tp = rx->tp;
    const uint32_t C = rx->P.n_channels;
    *sort_bins_empty = false;
    if (tp.cfg.knob_prologue >= 0) {
        HIP_TRY(same::launch_tp_prologue(tp.blob, tp.blob_fresh, tp.fresh_bytes, sl.d_handover, sl.d_sort, columns, sl.d_counters, stream));
        *sort_bins_empty = sl.sort_bins == columns;
    } else {
        // (SAME_TP_PROLOGUE=0, A/B measurements: the launches' start as rounds 2-5 made it)
        HIP_TRY(same::launch_counters(sl.d_counters, sl.h_counters.dev(), 0, stream));
        HIP_TRY(same::launch_init_state(tp.Pv, tp.Sv, 0, stream, C));
        HIP_TRY(same::launch_fill_u64(sl.d_handover, columns, same::kNoHandover, stream));
    }
    if (rx->debug) std::fprintf(stderr, "[same] time-parallel launch: %u columns (%s), start-up: %s\n", columns, layout,
                                tp.cfg.knob_prologue >= 0 ? "prologue kernel" : "separate launches");
    HIP_TRY(same::launch_copy_state_columns(tp.d_desc_in, tp.n_desc, C, columns, nullptr, C, stream));
    return SAME_OK;
}

// What the block kernels leave of a launch (less than a block; every row where the configuration has no block kernel): the
// any-configuration kernel on the channels' own state, over n time-major rows
template <typename SampleT>
int demod_tail(same_batch *rx, const same::Output &O, const SampleT *rows, size_t n, uint64_t counter0, hipStream_t stream)
{
    const hipError_t e = same::launch_demod(rx->P, rx->S, O, rx->d_taps, rows, (uint32_t)n, counter0, stream);
    if (e != hipSuccess) return fail(SAME_EHIP, "demod kernel launch failed: %s", hipGetErrorString(e));
    return SAME_OK;
}
// ... over the [channels][r] corner at `corner` of a channel-major input (row pitch `pitch`), transposed to rows first
int demod_tail_corner(same_batch *rx, const same::Output &O, const float *corner, size_t pitch, size_t r, uint64_t counter0, hipStream_t stream)
{
    const uint32_t C = rx->P.n_channels;
    HIP_TRY(rx->d_stage.ensure(r * C * sizeof(float)));
    HIP_TRY(rx->d_stage2.ensure(r * C * sizeof(float)));
    float *staged = static_cast<float *>(rx->d_stage.get()), *rows = static_cast<float *>(rx->d_stage2.get());
    HIP_TRY(hipMemcpy2DAsync(staged, r * sizeof(float), corner, pitch * sizeof(float), r * sizeof(float), C, hipMemcpyDeviceToDevice, stream));
    const hipError_t e = same::launch_transpose(staged, rows, C, (uint32_t)r, stream);
    if (e != hipSuccess) return fail(SAME_EHIP, "demod kernel launch failed: %s", hipGetErrorString(e));
    return demod_tail(rx, O, rows, r, counter0, stream);
}

// The planning kernels of a channel-major launch with per-channel boundaries: an energy scout and the boundary
// planner fill the slot's geometry buffer (np.words) ahead of the demodulation kernel; pc gets the arrays that kernel reads
int tp_plan_boundaries(same_batch *rx, same_batch::Slot &sl, const same::TpCut &cut, const same::TpNative &np, const float *d_x,
                       hipStream_t stream, same::PipeChunks &pc)
{
    same_batch::TimePar &tp = rx->tp;
    const same::TpGeomWords &w = np.words;
    same::TpPlan plan{};
    plan.channels = rx->P.n_channels; plan.n_chunks = cut.n_chunks; plan.block_len = cut.geom.block_len;
    plan.warmup_samples = np.warmup_samples; plan.whole_samples = np.whole_samples; plan.in_samples = np.in_samples;
    plan.scout_blocks = np.scout_blocks;
    sl.plan = plan; sl.plan_counter0 = rx->counter;
    sl.plan_sorted = np.sort_mode != 0; sl.plan_lpt = np.lpt; sl.plan_pairs = np.pair_groups;
    uint32_t *g = sl.d_geom;
    // On the library's own stream the planning kernels go to the plan stream: they need the input (ordered by
    // same_batch_order_after, which both streams honour) and this slot's geometry buffers (free since the harvest above),
    // not the previous launch -- so they run beside its tail instead of after it (~0.25 ms of small kernels per call at
    // configs[1]).  On a caller's stream everything stays in that stream's order.
    const bool side = same::tp_plan_beside(tp.cfg, stream == rx->own_stream);
    hipStream_t ps = side ? rx->plan_stream : stream;
    // (the energy map is one buffer for both slots: this call's scout after the previous call's planner, whichever
    // streams the two ran on)
    if (tp.plan_recorded) HIP_TRY(hipStreamWaitEvent(ps, tp.ev_plan_prev, 0));
    HIP_TRY(same::launch_tp_plan(d_x, plan, tp.d_energy, g + w.own_start, g + w.row0, g + w.nominal, g + w.perm, g + w.wg, np.sort_mode != 0, ps,
                                 np.lpt ? g + w.perm2 : nullptr, np.lpt ? g + w.wg2 : nullptr, np.pair_groups));
    HIP_TRY(tp.ev_plan_prev.ensure());
    HIP_TRY(hipEventRecord(tp.ev_plan_prev, ps));
    tp.plan_recorded = true;
    if (side) {
        HIP_TRY(hipEventRecord(sl.ev_planned, ps));
        HIP_TRY(hipStreamWaitEvent(stream, sl.ev_planned, 0));
    }
    pc.col_row0 = g + w.row0; pc.col_nominal = g + w.nominal;
    pc.wg_blocks = g + (np.lpt ? w.wg2 : w.wg); pc.col_perm = np.lpt ? g + w.perm2 : nullptr;
    pc.in_samples = np.in_samples; pc.whole_samples = np.whole_samples;
    pc.hist_scratch = np.need_hist ? tp.d_hist.get() : nullptr;
    return SAME_OK;
}

// A time-parallel launch of the n_call samples at x, cut as `cut`: every channel as cut.n_chunks state columns
// side by side.  np null: time-major rows, the uniform cut; else a channel-major input read where it lies, every column from
// its own first row (tp_plan_boundaries).  Between the caller's begin_launch and end_launch.
template <typename SampleT>
int launch_time_parallel(same_batch *rx, same_batch::Slot &sl, hipStream_t stream, const same::TpCut &cut, const same::TpNative *np,
                         const SampleT *x, size_t n_call, bool *sort_bins_empty)
{
    same_batch::TimePar &tp = rx->tp;
    const same::ChunkGeom &geom = cut.geom;
    const uint32_t C = rx->P.n_channels, columns = cut.n_chunks * C, fb = geom.block_len;
    const uint32_t total_blocks = (uint32_t)(n_call / fb);
    const size_t n_whole = (size_t)total_blocks * fb;
    tp.family = cut.choice.family;
    // the wide state, the output (a channel-major launch sizes it for its whole blocks) and the hand-over records, one per
    // state column, before anything is queued
    same::Output O{};
    int rc = ensure_wide_state(rx, columns);
    if (rc == SAME_OK) rc = ensure_output(rx, sl, same::tp_output_samples(np ? n_whole : n_call, cut.pc, fb), O, columns);
    if (rc) return rc;
    HIP_TRY(sl.d_handover.ensure(columns));
    HIP_TRY(sl.h_handover.ensure(columns));
    same::PipeChunks pc = cut.pc;
    pc.handover = sl.d_handover;
    if (np) {
        HIP_TRY(sl.d_geom.ensure(np->words.total));
        HIP_TRY(sl.h_geom.ensure(np->words.harvest));
        HIP_TRY(tp.d_energy.ensure(np->energy_floats));
        if (np->need_hist) HIP_TRY(tp.d_hist.ensure(np->hist_floats));
        sl.words = np->words;
    }
    rc = begin_timing(rx, sl, stream);
    if (rc) return rc;
    const float *xf = nullptr;      // the input as the per-channel form reads it (np is null for an int16 call)
    if constexpr (std::is_same_v<SampleT, float>) xf = x;
    if (np && (rc = tp_plan_boundaries(rx, sl, cut, *np, xf, stream, pc)) != SAME_OK) return rc;
    rc = tp_start(rx, sl, columns, np ? "channel-major" : "time-major", stream, sort_bins_empty);
    if (rc) return rc;
    // (a launch with planning kernels brackets the demodulation kernel alone as well)
    sl.have_k = np && sl.timed;
    if (sl.have_k) HIP_TRY(hipEventRecord(sl.ev_k0, stream));
    const hipError_t e = launch_family(tp.family, tp.Pv, tp.Sv, O, rx->d_taps, x, total_blocks, rx->counter, stream, pc);
    rx->last_family = tp.family;
    if (e != hipSuccess) return fail(SAME_EHIP, "time-parallel demod kernel launch failed: %s", hipGetErrorString(e));
    if (sl.have_k) HIP_TRY(hipEventRecord(sl.ev_k1, stream));
    // The channels' state afterwards: that of the chunk the hand-over chain ends in, as the host's stitch follows it --
    // the last chunk as a rule (its columns end with the input); an earlier one where a burst ran on to the end of the
    // call without a hand-over (a forced cut on a channel that is never quiet: its events are the ones that are kept).
    if (np) HIP_TRY(same::launch_chunk_final_column_pc(sl.d_handover, sl.d_geom + np->words.own_start, C, geom.n_chunks, rx->counter, tp.d_final_col, stream));
    else HIP_TRY(same::launch_chunk_final_column(sl.d_handover, C, geom, tp.d_final_col, stream));
    HIP_TRY(same::launch_copy_state_columns(tp.d_desc_out, tp.n_desc, columns, C, tp.d_final_col, C, stream));
    // less than a block is left: on the channels' own state (channel-major: its [C][r] corner of the input)
    if (n_whole < n_call) {
        rc = np ? demod_tail_corner(rx, O, xf + n_whole, n_call, n_call - n_whole, rx->counter + n_whole, stream)
                : demod_tail(rx, O, x + n_whole * C, n_call - n_whole, rx->counter + n_whole, stream);
        if (rc) return rc;
    }
    sl.chunked = true; sl.per_channel = np != nullptr;
    sl.geom = geom;
    sl.end_blocks = rx->counter + n_whole;
    tp.last_chunks = cut.n_chunks; tp.last_per_channel = sl.per_channel;
    return SAME_OK;
}

// The end of a launch of n samples: the stop event, the event sort, the transport layer and the audio capture on the device
// where the launch has them (rows: its time-major input, which the capture kernel reads; a channel-major launch has none),
// the cursors published, the done event, the slot's and the batch's books, and -- while this launch runs -- the harvest of
// the previous one
template <typename SampleT>
int end_launch(same_batch *rx, same_batch::Slot &sl, same_batch::Slot &prev, hipStream_t stream, const SampleT *rows, size_t n,
               bool sort_bins_empty, const RaggedLaunch *rl = nullptr)
{
    if (sl.timed) HIP_TRY(hipEventRecord(sl.ev_stop, stream));
    HIP_TRY(same::launch_event_sort(sl.d_events, sl.d_counters, sl.event_cap(), sl.sort_bins, sl.d_sort, sl.d_sort + sl.sort_bins,
                                    sl.d_sorted, stream, sort_bins_empty));
    // SAME_BATCH_MESSAGES_ONLY: the transport layer over the ordered log, a lane per channel, on the launch's stream (the next
    // launch, which reads the forced-EOM instants it arms, is ordered behind it)
    sl.dev_transport = rx->dev_transport && !sl.chunked;
    rx->last_dev_transport = sl.dev_transport;
    if (sl.dev_transport) {
        same::TransportLaunch T{};
        T.n_channels = rx->P.n_channels; T.input_rate = rx->P.input_rate;
        T.first = sl.d_sort + sl.sort_bins; T.sorted = sl.d_sorted; T.counters = sl.d_counters;
        T.bursts = sl.d_bursts; T.burst_cap = sl.burst_cap();
        T.hot = rx->d_thot; T.cold = rx->d_tcold; T.wake_sample = rx->S.wake_sample;
        T.near = sl.h_near.dev(); T.near_cap = sl.near_cap();
        T.log = sl.d_msgs; T.log_cap = sl.msg_cap(); T.log_cursor = sl.d_counters + 3; T.overflow = sl.d_counters + 2;
        // same_batch_set_audio_capture: the lanes list the spans of open messages, the capture kernel copies them out of the
        // input behind it -- before the launch's done event, which every later reuse of the input waits for
        sl.captured = rx->audio.per_launch != 0;
        if (sl.captured) {
            same::cap::Launch &K = T.cap;
            const uint64_t fa = rx->audio.flush_at;
            K.start = rx->counter; K.n_rows = (uint32_t)n;
            K.flush_row = fa >= rx->counter + n ? same::cap::kNoFlush : (uint32_t)(fa > rx->counter ? fa - rx->counter : 0);
            K.rec = rx->audio.d_rec; K.spans = sl.d_spans; K.span_cap = sl.span_cap();
            K.n_spans = &sl.d_cap_cur->n_spans; K.pool_used = &sl.d_cap_cur->pool_used; K.pool_cap = rx->audio.per_launch;
            K.overflow = &sl.d_cap_cur->overflow;
        }
        if (rl && rl->n_lock < n)
            HIP_TRY(same::launch_transport_ragged(T, sl.h_counts.dev(), rl->row0, (uint32_t)n, stream));
        else
            HIP_TRY(same::launch_transport(T, stream));
        if (sl.captured) {
            const hipError_t e = same::launch_capture(sl.d_spans, sl.d_cap_cur, sl.span_cap(), sl.d_pool, rx->audio.per_launch, rows,
                                                      rx->P.n_channels, (uint32_t)n, sl.h_cap_cur.dev(), stream);
            if (e != hipSuccess) return fail(SAME_EHIP, "capture kernel launch failed: %s", hipGetErrorString(e));
        }
    }
    HIP_TRY(same::launch_counters(sl.d_counters, sl.h_counters.dev(), 1, stream));
    HIP_TRY(hipEventRecord(sl.ev_done, stream));
    sl.in_flight = true;
    sl.seq = ++rx->launch_seq;
    rx->last_stream = stream;
    // a ragged launch: the channels that consumed fewer than n rows lag the batch by that much more from here on
    if (rl) rx->resets.shift(rx->ragged_by.data(), rx->counter + n, (int)(&sl - rx->slot));
    rx->counter += n;
    sl.end_counter = rx->counter;
    // while this launch runs, bring in the previous one
    return harvest_slot(rx, prev);
}

template <typename SampleT>
int process_time_major_launches(same_batch *rx, const SampleT *d_x, size_t n_samples, hipStream_t stream, const Ragged *rg = nullptr)
{
    const size_t kMaxChunk = same::max_launch_samples(rx->P.input_rate);
    size_t done = 0;
    while (done < n_samples) {
        const size_t n = std::min(kMaxChunk, n_samples - done);
        same_batch::Slot &sl = rx->slot[rx->launch_seq & 1];
        same_batch::Slot &prev = rx->slot[(rx->launch_seq & 1) ^ 1];
        int rc = begin_launch(rx, sl, prev, stream);
        if (rc) return rc;
        // a ragged call: rows [0, n_lock) of this launch are every channel's (the common prefix: the lockstep kernels below),
        // rows [n_lock, n) only some channels' (the ragged kernel, behind them in the same launch)
        size_t n_lock = n;
        if (rg) {
            const size_t row0 = (size_t)rg->row_off + done;
            const uint32_t C = rx->P.n_channels;
            HIP_TRY(sl.h_counts.ensure(C));
            // (the slot's previous launch, the last reader of this buffer, has been harvested above)
            std::memcpy(sl.h_counts, rg->counts, (size_t)C * sizeof(uint32_t));
            rx->ragged_by.resize(C);
            n_lock = same::ragged_launch_split(rg->counts, C, rg->m, row0, n, rx->ragged_by.data());
        }
        const same::TpCut cut = rg ? same::TpCut{} : same::tp_uniform_cut(rx->P, rx->mode, rx->want, rx->tp.cfg, n, rx->counter);
        rx->tp.last_chunks = cut.n_chunks;
        sl.have_k = false;
        bool sort_bins_empty = false;          // the launch's prologue kernel has emptied the event sort's bins
        if (cut.n_chunks > 1u) {
            rc = launch_time_parallel(rx, sl, stream, cut, nullptr, d_x + done * rx->P.n_channels, n, &sort_bins_empty);
            if (rc) return rc;
        } else {
        same::Output O{};
        sl.chunked = false; sl.per_channel = false;
        rc = ensure_output(rx, sl, n, O);
        if (rc) return rc;
        HIP_TRY(same::launch_counters(sl.d_counters, sl.h_counters.dev(), 0, stream));
        rc = begin_timing(rx, sl, stream);
        if (rc) return rc;
        const SampleT *xp = d_x + done * rx->P.n_channels;
        hipError_t e = hipSuccess;
        // whole blocks go to the batch's block kernel (same_select.h: select_plain) where it has one; the any-configuration
        // kernel takes the remainder (and every other configuration)
        const same::Choice &plain = rx->plain;
        const size_t fb = plain.block_len;
        const size_t n_fast = fb ? (n_lock / fb) * fb : 0;
        if (n_fast) {
            e = launch_family(plain.family, same::is_fastmath(plain.family) ? rx->Pfm : rx->P, rx->S, O, rx->d_taps, xp, (uint32_t)(n_fast / fb), rx->counter, stream);
            if (e != hipSuccess) return fail(SAME_EHIP, "%s launch failed: %s", same::family_name(plain.family, rx->P.block_len), hipGetErrorString(e));
            rx->sym_launched |= plain.family == same::Family::kSym;
        }
        rx->last_family = plain.family == same::Family::kSym && !rx->sym_launched ? same::Family::kPipeFastmath : plain.family;
        if (n_fast < n_lock &&
            (rc = demod_tail(rx, O, xp + n_fast * rx->P.n_channels, n_lock - n_fast, rx->counter + n_fast, stream)) != SAME_OK) return rc;
        if (n_lock < n) {
            // the ragged remainder: each lane its own count, the state left canonical at the launch's end
            e = same::launch_demod_ragged(rx->P, rx->S, O, rx->d_taps, xp + n_lock * rx->P.n_channels, (uint32_t)(n - n_lock), sl.h_counts.dev(),
                                          (uint32_t)(rg->row_off + done + n_lock), rx->counter + n_lock, stream);
            if (e != hipSuccess) return fail(SAME_EHIP, "ragged demod kernel launch failed: %s", hipGetErrorString(e));
        }
        }
        const RaggedLaunch rl{rg ? (uint32_t)(rg->row_off + done) : 0u, n_lock};
        rc = end_launch(rx, sl, prev, stream, d_x + done * rx->P.n_channels, n, sort_bins_empty, rg ? &rl : nullptr);
        if (rc) return rc;
        done += n;
    }
    return SAME_OK;
}

// SAME_BATCH_CALL_INVARIANT (include/same_rx.h): launches cover whole windows of the stream, from fixed stream positions on.  What
// a launch computes is a function of the state it starts from and of the samples it covers -- the relaxed kernels drain their
// pipeline at a launch's end and apply the feedback in flight at once, the time-parallel mode plans its cuts per launch -- so a
// stream fed in different calls came out different near a lock or an end of burst wherever the calls' boundaries fell.  With the
// launches' boundaries tied to the stream instead of to the calls, it cannot: any list of calls that delivers the same samples
// makes the same launches.  The price is latency: the events of a window arrive when its last sample has (same_batch_flush
// demodulates what is waiting).  Whole windows that lie inside a call's buffer are launched where they lie; the pieces before
// and behind them are copied into the waiting buffer (f32; int16 pieces are cast the way the kernels cast them: unscaled).
// Window lengths (same_batch_set_call_window changes them): whole blocks of the kernels that take such launches (16, 18, 32, 36, 72
// samples).  Short windows keep the latency and the share of a call that has to be copied low (a call shorter than a window is
// copied whole: at 32 768 channels a 2-s call costs 4.4 ms with 73 728-sample windows, 3.5 with 18 432, 2.0 without the flag); a
// time-parallel batch needs long ones -- its planner cuts every LAUNCH into pieces of a burst's length and more.
constexpr uint32_t kInvWindow = 18432;                 // 0.84 s at 22.05 kHz, 0.38 s at 48 kHz
constexpr uint32_t kInvWindowTimeParallel = 73728;     // 3.3 s at 22.05 kHz, 1.5 s at 48 kHz
static int inv_buffer_wait(same_batch *rx, hipStream_t stream)
{
    same_batch::Windowed &iv = rx->inv;
    if (iv.buf_used && iv.buf_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, iv.ev_buf, 0));
    return SAME_OK;
}
static int inv_buffer_done(same_batch *rx, hipStream_t stream)
{
    same_batch::Windowed &iv = rx->inv;
    HIP_TRY(iv.ev_buf.ensure());
    HIP_TRY(hipEventRecord(iv.ev_buf, stream));
    iv.buf_stream = stream; iv.buf_used = true;
    return SAME_OK;
}
// n samples into the waiting buffer, as f32
static int inv_copy(const float *d_x, float *dst, size_t n, hipStream_t stream)
{
    HIP_TRY(hipMemcpyAsync(dst, d_x, n * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return SAME_OK;
}
static int inv_copy(const int16_t *d_x, float *dst, size_t n, hipStream_t stream)
{
    const hipError_t e = same::launch_cast_i16_f32(d_x, dst, n, stream);
    if (e != hipSuccess) return fail(SAME_EHIP, "cast launch failed: %s", hipGetErrorString(e));
    return SAME_OK;
}
template <typename SampleT>
static int inv_append(same_batch *rx, const SampleT *d_x, size_t n, hipStream_t stream)
{
    // n samples (rows of n_channels) behind the ones already waiting
    same_batch::Windowed &iv = rx->inv;
    const size_t C = rx->P.n_channels;
    HIP_TRY(iv.d_buf.ensure((size_t)iv.window * C * sizeof(float)));
    int rc = inv_buffer_wait(rx, stream);
    if (rc) return rc;
    rc = inv_copy(d_x, static_cast<float *>(iv.d_buf.get()) + (size_t)iv.fill * C, n * C, stream);
    if (rc) return rc;
    iv.fill += (uint32_t)n;
    return inv_buffer_done(rx, stream);
}
// demodulate what is waiting (a whole window, or -- flush -- whatever there is) and begin a new window
static int inv_launch_waiting(same_batch *rx, hipStream_t stream)
{
    same_batch::Windowed &iv = rx->inv;
    if (!iv.fill) return SAME_OK;
    int rc = inv_buffer_wait(rx, stream);
    if (rc) return rc;
    const uint32_t n = iv.fill;
    iv.fill = 0;
    rc = process_time_major_launches<float>(rx, static_cast<const float *>(iv.d_buf.get()), n, stream);
    if (rc) return rc;
    return inv_buffer_done(rx, stream);
}
// The input-lifetime contract (include/same_rx.h) in windowed mode.  A call's reads of the caller's buffer -- whole windows launched
// in place, the pieces copied or cast into the waiting buffer, a channel-major call's copies into the staging buffers -- are all
// queued on its stream, and a call shorter than a window launches nothing, so no harvest waits for them.  Each call therefore
// records an event behind its last operation and, before it returns, waits for the one of the call before the previous one.
// Successive calls' operations are kept in stream order whatever their streams (they share the staging and waiting buffers
// too), so the latest event stands for every call before it: same_batch_sync and the host uploads wait for that one.
static int inv_reads_begin(same_batch *rx, hipStream_t stream)
{
    same_batch::Windowed &iv = rx->inv;
    if (iv.n_reads && iv.read_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, iv.ev_read[(iv.n_reads - 1) & 1], 0));
    return SAME_OK;
}
static int inv_reads_end(same_batch *rx, hipStream_t stream)
{
    same_batch::Windowed &iv = rx->inv;
    same::Event &ev = iv.ev_read[iv.n_reads & 1];
    if (!ev) HIP_TRY(ev.ensure());
    else HIP_TRY(hipEventSynchronize(ev));           // call k - 2's reads: its buffer may be reused once this call returns
    HIP_TRY(hipEventRecord(ev, stream));
    iv.read_stream = stream;
    ++iv.n_reads;
    return SAME_OK;
}
static int inv_reads_wait(same_batch *rx)
{
    same_batch::Windowed &iv = rx->inv;
    if (iv.n_reads) HIP_TRY(hipEventSynchronize(iv.ev_read[(iv.n_reads - 1) & 1]));
    return SAME_OK;
}
template <typename SampleT>
int process_time_major(same_batch *rx, const SampleT *d_x, size_t n_samples, hipStream_t stream)
{
    same_batch::Windowed &iv = rx->inv;
    if (!iv.on) return process_time_major_launches(rx, d_x, n_samples, stream);
    const size_t C = rx->P.n_channels;
    size_t pos = 0;
    if (iv.fill) {
        // complete the window that is waiting
        const size_t take = std::min<size_t>(iv.window - iv.fill, n_samples);
        int rc = inv_append(rx, d_x, take, stream);
        if (rc) return rc;
        pos = take;
        if (iv.fill < iv.window) return SAME_OK;
        rc = inv_launch_waiting(rx, stream);
        if (rc) return rc;
    }
    // whole windows where they lie
    while (n_samples - pos >= iv.window) {
        int rc = process_time_major_launches(rx, d_x + pos * C, iv.window, stream);
        if (rc) return rc;
        pos += iv.window;
    }
    if (pos < n_samples) return inv_append(rx, d_x + pos * C, n_samples - pos, stream);
    return SAME_OK;
}

// Time-parallel launch over a CHANNEL-MAJOR input with chunk boundaries chosen per channel at idle instants.
// Returns 1 when the call was handled, 0 when it does not qualify (same_tp_plan.h: tp_native_plan; the caller then takes the
// transposing path), < 0 on error.  The lanes' own streams are read as f32: an int16 call never qualifies.
template <typename SampleT>
int process_channel_major_native(same_batch *rx, const SampleT *d_x, size_t n, hipStream_t stream)
{
    if constexpr (!std::is_same_v<SampleT, float>) return 0;
    else {
    if (!rx->tp.enabled) return 0;
    const same::TpCut cut = same::tp_native_cut(rx->P, rx->mode, rx->want, rx->tp.cfg, n, rx->counter);
    const same::TpNative np = same::tp_native_plan(rx->P, rx->tp.cfg, cut, n, (uintptr_t)d_x);
    if (!np.qualifies) return 0;
    same_batch::Slot &sl = rx->slot[rx->launch_seq & 1];
    same_batch::Slot &prev = rx->slot[(rx->launch_seq & 1) ^ 1];
    int rc = begin_launch(rx, sl, prev, stream);
    if (rc) return rc;
    bool sort_bins_empty = false;
    rc = launch_time_parallel(rx, sl, stream, cut, &np, d_x, n, &sort_bins_empty);
    if (rc) return rc;
    rc = end_launch<float>(rx, sl, prev, stream, nullptr, n, sort_bins_empty);
    return rc ? rc : 1;
    }
}

// A channel-major input of n_rows rows (row pitch `pitch`) as time-major launches: slabs of time are transposed through the
// staging buffers, and launch(rows, n, t0) takes each -- n time-major rows that begin at the input's row t0
template <typename SampleT, typename Launch>
int transpose_in_slabs(same_batch *rx, const SampleT *d_x, size_t pitch, size_t n_rows, hipStream_t stream, Launch &&launch)
{
    const uint32_t C = rx->P.n_channels;
    // (the staging buffers are the batch's own: a launch still in flight on ANOTHER stream may be reading its input out of
    // them -- successive launches are ordered whatever their streams, so this call's first staging write waits for it)
    for (same_batch::Slot &sl : rx->slot)
        if (sl.in_flight && rx->last_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, sl.ev_done, 0));
    // (slabs of 65 520 samples: whole blocks of every kernel -- 16, 18, 20, 36 and 42 samples -- so that only the call's own
    // tail goes through the any-configuration kernel, not one per slab)
    const size_t slab = std::min<size_t>(n_rows, (size_t)65520);
    HIP_TRY(rx->d_stage2.ensure(slab * C * sizeof(SampleT)));
    for (size_t t0 = 0; t0 < n_rows; t0 += slab) {
        const size_t n = std::min(slab, n_rows - t0);
        // stream order keeps the previous slab's kernel ahead of this slab's staging writes
        // the transpose kernel takes a dense [C][n] view, so the [C][n] window at t0 is copied out of the rows first
        // (2D copy keeps this simple and is only used on the non-native layout)
        HIP_TRY(rx->d_stage.ensure(n * C * sizeof(SampleT)));
        SampleT *staged = static_cast<SampleT *>(rx->d_stage.get()), *rows = static_cast<SampleT *>(rx->d_stage2.get());
        HIP_TRY(hipMemcpy2DAsync(staged, n * sizeof(SampleT), d_x + t0, pitch * sizeof(SampleT), n * sizeof(SampleT), C,
                                 hipMemcpyDeviceToDevice, stream));
        const hipError_t e = same::launch_transpose(staged, rows, C, (uint32_t)n, stream);
        if (e != hipSuccess) return fail(SAME_EHIP, "transpose launch failed: %s", hipGetErrorString(e));
        const int rc = launch(rows, n, t0);
        if (rc) return rc;
    }
    return SAME_OK;
}

template <typename SampleT>
int process_device_on(same_batch *rx, const SampleT *d_x, size_t n_samples, uint32_t layout, hipStream_t stream);
template <typename SampleT>
int process_device_any(same_batch *rx, const SampleT *d_x, size_t n_samples, uint32_t layout, void *hip_stream)
{
    if (!rx || (!d_x && n_samples)) return fail(SAME_EINVAL, "null argument");
    if (n_samples == 0) return SAME_OK;
    HIP_TRY(hipSetDevice(rx->device));
    // SAME_STREAM_OWN: the library's private stream; anything else (NULL included) is the caller's stream
    hipStream_t stream = hip_stream == SAME_STREAM_OWN ? rx->own_stream : (hipStream_t)hip_stream;
    if (!rx->inv.on) return process_device_on(rx, d_x, n_samples, layout, stream);
    int rc = inv_reads_begin(rx, stream);
    if (rc == SAME_OK) rc = process_device_on(rx, d_x, n_samples, layout, stream);
    const int rc_end = inv_reads_end(rx, stream);      // (also after a failed call: whatever it queued may read d_x)
    return rc ? rc : rc_end;                            // the first error is the one reported; a second one is not
}
template <typename SampleT>
int process_device_on(same_batch *rx, const SampleT *d_x, size_t n_samples, uint32_t layout, hipStream_t stream)
{
    if (layout == SAME_LAYOUT_TIME_MAJOR) return process_time_major(rx, d_x, n_samples, stream);
    if (layout != SAME_LAYOUT_CHANNEL_MAJOR) return fail(SAME_EINVAL, "unknown layout %u", layout);
    // (its cuts are planned per CALL: a batch that is to be independent of its calls takes the transposing path and windows)
    const int done = rx->inv.on ? 0 : process_channel_major_native(rx, d_x, n_samples, stream);
    if (done) return done < 0 ? done : SAME_OK;
    return transpose_in_slabs(rx, d_x, n_samples, n_samples, stream,
                              [&](const SampleT *rows, size_t n, size_t) { return process_time_major(rx, rows, n, stream); });
}

// Uploads the rows [0, n_rows) of a host buffer (channel-major: row pitch `pitch`) in slabs, so that arbitrarily long host
// streams need bounded device memory; process(d_rows, n, t0) takes each slab -- n rows that begin at row t0, in the buffer's
// layout with pitch n -- and every launch is collected before the next slab overwrites it
template <typename SampleT, typename Process>
int upload_in_slabs(same_batch *rx, const SampleT *h_x, size_t pitch, size_t n_rows, uint32_t layout, Process &&process)
{
    const size_t C = rx->P.n_channels;
    const size_t slab = std::max<size_t>(1, std::min<size_t>(n_rows, ((size_t)256 << 20) / (C * sizeof(SampleT))));
    HIP_TRY(rx->d_upload.ensure(slab * C * sizeof(SampleT)));
    SampleT *d_in = static_cast<SampleT *>(rx->d_upload.get());
    int rc = SAME_OK;
    for (size_t t0 = 0; t0 < n_rows && rc == SAME_OK; t0 += slab) {
        const size_t n = std::min(slab, n_rows - t0);
        // (the previous slab's launch was collected below, so the buffer is free again -- unless a windowed batch only copied
        // it into its waiting buffer, asynchronously: wait for that copy)
        if (rx->inv.on && (rc = inv_reads_wait(rx)) != SAME_OK) break;
        const hipError_t e = layout == SAME_LAYOUT_TIME_MAJOR
                                 ? hipMemcpy(d_in, h_x + t0 * C, n * C * sizeof(SampleT), hipMemcpyHostToDevice)
                                 : hipMemcpy2D(d_in, n * sizeof(SampleT), h_x + t0, pitch * sizeof(SampleT), n * sizeof(SampleT), C,
                                               hipMemcpyHostToDevice);
        if (e != hipSuccess) { rc = fail(SAME_EHIP, "upload failed: %s", hipGetErrorString(e)); break; }
        rc = process(d_in, n, t0);
        if (rc == SAME_OK) rc = harvest(rx);
    }
    if (rc == SAME_OK && rx->kernel_fault) return fail(SAME_EKERNEL, "a demodulation kernel's wavefronts lost step (internal hand-over timed out)");
    if (rc == SAME_OK && rx->overflowed) return fail(SAME_EOVERFLOW, "event/burst pool overflow");
    return rc;
}

template <typename SampleT>
int process_host_any(same_batch *rx, const SampleT *h_x, size_t n_samples, uint32_t layout)
{
    if (!rx || (!h_x && n_samples)) return fail(SAME_EINVAL, "null argument");
    if (n_samples == 0) return SAME_OK;
    HIP_TRY(hipSetDevice(rx->device));
    return upload_in_slabs(rx, h_x, n_samples, n_samples, layout, [&](const SampleT *d_in, size_t n, size_t) {
        return process_device_any(rx, d_in, n, layout, SAME_STREAM_OWN);
    });
}

// A ragged call (same_batch_process_*_ragged, include/same_rx.h): channel c consumes the first counts[c] of the buffer's n_rows
// rows.  The common prefix (the smallest count) runs through the batch's lockstep kernels, the rows up to the largest count
// through the ragged kernel in the same launch; the per-channel counter shifts go to the ledger.
int ragged_check(same_batch *rx, size_t n_rows, const uint32_t *counts, uint32_t layout, uint32_t *m_out, uint32_t *M_out)
{
    if (!rx) return fail(SAME_EINVAL, "null handle");
    if (!counts) return fail(SAME_EINVAL, "null counts");
    if (layout != SAME_LAYOUT_TIME_MAJOR && layout != SAME_LAYOUT_CHANNEL_MAJOR) return fail(SAME_EINVAL, "unknown layout %u", layout);
    if (rx->tp.enabled) return fail(SAME_EINVAL, "ragged calls: a SAME_BATCH_TIME_PARALLEL batch plans its cuts over one common row range");
    if (rx->inv.on) return fail(SAME_EINVAL, "ragged calls: SAME_BATCH_CALL_INVARIANT windows begin at positions of one common stream");
    if (rx->P.trace_cap) return fail(SAME_EINVAL, "ragged calls: SAME_BATCH_TRACE_SYMBOLS records batch sample positions");
    if (n_rows > 0xffffffffull) return fail(SAME_EINVAL, "ragged calls: n_rows beyond 2^32 - 1");
    uint32_t m = UINT32_MAX, M = 0;
    for (uint32_t c = 0; c < rx->P.n_channels; ++c) {
        if (counts[c] > n_rows) return fail(SAME_EINVAL, "counts[%u] = %u exceeds n_rows = %zu; nothing was consumed", c, counts[c], n_rows);
        m = std::min(m, counts[c]); M = std::max(M, counts[c]);
    }
    *m_out = m; *M_out = M;
    return SAME_OK;
}

// The rows [row_base, row_base + n_buf) of a ragged call, in a buffer of their own (channel-major: row pitch `pitch`), as far as
// they reach into [0, M)
template <typename SampleT>
int process_ragged_on(same_batch *rx, const SampleT *d_x, size_t pitch, size_t n_buf, size_t row_base, const uint32_t *counts,
                      uint32_t m, uint32_t M, uint32_t layout, hipStream_t stream)
{
    const size_t n_p = std::min<size_t>(M, row_base + n_buf) - row_base;
    Ragged rg; rg.counts = counts; rg.m = m;
    if (layout == SAME_LAYOUT_TIME_MAJOR) {
        // (read in place: rows at stride C)
        if (m == M) return process_time_major_launches(rx, d_x, n_p, stream);
        rg.row_off = (uint32_t)row_base;
        return process_time_major_launches(rx, d_x, n_p, stream, &rg);
    }
    // channel-major: every row's samples, in slabs, through the staging buffers into time-major
    return transpose_in_slabs(rx, d_x, pitch, n_p, stream, [&](const SampleT *rows, size_t n, size_t t0) {
        if (m == M) return process_time_major_launches(rx, rows, n, stream);
        rg.row_off = (uint32_t)(row_base + t0);
        return process_time_major_launches(rx, rows, n, stream, &rg);
    });
}

template <typename SampleT>
int process_ragged_device(same_batch *rx, const SampleT *d_x, size_t n_rows, const uint32_t *counts, uint32_t layout, void *hip_stream)
{
    uint32_t m = 0, M = 0;
    int rc = ragged_check(rx, n_rows, counts, layout, &m, &M);
    if (rc) return rc;
    if (M == 0) return SAME_OK;
    if (!d_x) return fail(SAME_EINVAL, "null argument");
    // every channel all n_rows: exactly the plain call
    if (m == M && M == n_rows) return process_device_any(rx, d_x, n_rows, layout, hip_stream);
    HIP_TRY(hipSetDevice(rx->device));
    hipStream_t stream = hip_stream == SAME_STREAM_OWN ? rx->own_stream : (hipStream_t)hip_stream;
    if (m != M) rx->wake_ordered = true;
    return process_ragged_on(rx, d_x, n_rows, n_rows, 0, counts, m, M, layout, stream);
}

template <typename SampleT>
int process_ragged_host(same_batch *rx, const SampleT *h_x, size_t n_rows, const uint32_t *counts, uint32_t layout)
{
    uint32_t m = 0, M = 0;
    int rc = ragged_check(rx, n_rows, counts, layout, &m, &M);
    if (rc) return rc;
    if (M == 0) return SAME_OK;
    if (!h_x) return fail(SAME_EINVAL, "null argument");
    if (m == M && M == n_rows) return process_host_any(rx, h_x, n_rows, layout);
    HIP_TRY(hipSetDevice(rx->device));
    if (m != M) rx->wake_ordered = true;
    // (the upload buffer may still be read by a launch in flight: every launch of the batch is collected first)
    rc = harvest(rx);
    if (rc) return rc;
    // the first M rows
    return upload_in_slabs(rx, h_x, n_rows, M, layout, [&](const SampleT *d_in, size_t n, size_t t0) {
        return process_ragged_on(rx, d_in, n, n, t0, counts, m, M, layout, rx->own_stream);
    });
}

}  // namespace

// ------------------------------------------------------------------------------------
extern "C" {

const char *same_last_error(void) { return same::last_error(); }

#ifndef SAME_SOURCE_HASH
#define SAME_SOURCE_HASH "unknown"
#endif
// sha256 of the sources this binary was built from (sameold_amd/build.py compares it with the tree)
const char *same_rx_source_hash(void) { return "SAME_SOURCE_HASH=" SAME_SOURCE_HASH; }

int same_batch_new(const same_rx_builder *b, uint32_t n_channels, int device, uint32_t flags,
                   same_batch **out)
{
    if (!b || !out || n_channels == 0) return fail(SAME_EINVAL, "null builder/out or zero channels");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SAME_ENODEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(SAME_ENODEVICE, "device %d out of range (%d visible)", device, ndev);
    same_batch *rx = new (std::nothrow) same_batch;
    if (!rx) return fail(SAME_ENOMEM, "out of memory");
    rx->builder = *b;
    rx->device = device;
    rx->flags = flags;
    rx->inv.on = (flags & SAME_BATCH_CALL_INVARIANT) != 0;
    rx->inv.window = (flags & SAME_BATCH_TIME_PARALLEL) ? kInvWindowTimeParallel : kInvWindow;
    if (const char *e = std::getenv("SAME_INV_WINDOW")) { const long v = std::atol(e); if (v >= 64 && v <= (1 << 22)) rx->inv.window = (uint32_t)v; }      // (tests: short windows)
    std::vector<float> taps;
    int rc = same::derive_params(*b, n_channels, rx->P, taps);
    if (rc) { delete rx; return fail(rc, "builder rejected (code %d)", rc); }
    read_knobs(rx);
    rx->P.trace_cap = (flags & SAME_BATCH_TRACE_SYMBOLS) ? 4096u : 0u;
    if ((flags & SAME_BATCH_TIME_PARALLEL) && (flags & SAME_BATCH_TRACE_SYMBOLS)) {
        delete rx;
        return fail(SAME_EINVAL, "SAME_BATCH_TIME_PARALLEL cannot record a symbol trace");
    }
    if ((flags & SAME_BATCH_MESSAGES_ONLY) && (flags & SAME_BATCH_LINK_ONLY)) {
        delete rx;
        return fail(SAME_EINVAL, "SAME_BATCH_MESSAGES_ONLY needs the transport layer that SAME_BATCH_LINK_ONLY skips");
    }
    rx->tp.enabled = (flags & SAME_BATCH_TIME_PARALLEL) != 0;
    rx->messages_only = (flags & SAME_BATCH_MESSAGES_ONLY) != 0;
    rx->dev_transport = rx->messages_only && !rx->tp.enabled;      // (time-parallel: the stitch needs the transport layer on the host)
    // transport wake-ups come from the device in strict mode, from the host's symbol clock in time-parallel mode
    rx->P.ticks = ((flags & SAME_BATCH_LINK_ONLY) || rx->tp.enabled) ? 0u : 1u;
    rx->P.tick_interburst = (uint32_t)same::max_interburst_symbols();
    rx->P.tick_history = (uint32_t)same::max_history_duration();

    auto cleanup = [&](int code) { same_batch_free(rx); return code; };
#define TRY_OR_CLEAN(expr)                                                                     \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return cleanup(fail(SAME_EHIP, "%s failed: %s", #expr, hipGetErrorString(_e)));    \
    } while (0)
    TRY_OR_CLEAN(hipSetDevice(device));
    hipDeviceProp_t prop;
    TRY_OR_CLEAN(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return cleanup(fail(SAME_ENODEVICE, "device %d is %s; this build carries gfx950 code only", device, prop.gcnArchName));
    rx->want.relaxed = (flags & SAME_BATCH_RELAXED) != 0;
    rx->want.time_parallel = rx->tp.enabled;
    rx->want.generic = (flags & SAME_BATCH_GENERIC_KERNEL) != 0;      // (tests compare both kernels)
    rx->mode = same::select_mode(rx->P, rx->want);
    rx->plain = same::select_plain(rx->P, rx->mode, rx->want);
    rx->Pfm = same::fm_params(rx->P);
    rx->last_family = same::strict_family(rx->P, rx->mode);
    if (same::demod_lds_bytes(rx->P) > 160 * 1024)
        return cleanup(fail(SAME_EINVAL, "configuration needs %zu bytes of LDS per wavefront (limit 160 KiB)", same::demod_lds_bytes(rx->P)));
    TRY_OR_CLEAN(hipStreamCreateWithFlags(&rx->own_stream, hipStreamNonBlocking));
    TRY_OR_CLEAN(hipStreamCreateWithFlags(&rx->copy_stream, hipStreamNonBlocking));
    TRY_OR_CLEAN(hipStreamCreateWithFlags(&rx->plan_stream, hipStreamNonBlocking));
    TRY_OR_CLEAN(rx->ev_order.ensure());
    for (auto &sl : rx->slot) {
        TRY_OR_CLEAN(sl.ev_start.ensure(hipEventDefault));
        TRY_OR_CLEAN(sl.ev_stop.ensure(hipEventDefault));
        TRY_OR_CLEAN(sl.ev_k0.ensure(hipEventDefault));
        TRY_OR_CLEAN(sl.ev_k1.ensure(hipEventDefault));
        TRY_OR_CLEAN(sl.ev_done.ensure());
        TRY_OR_CLEAN(sl.ev_planned.ensure());
        TRY_OR_CLEAN(sl.d_counters.ensure(4));
        TRY_OR_CLEAN(sl.h_counters.ensure(4));
    }
    static_assert(sizeof(float4) == 4 * sizeof(float), "the taps are uploaded in fours");
    TRY_OR_CLEAN(rx->d_taps.ensure(taps.size() / 4));
    TRY_OR_CLEAN(hipMemcpy(rx->d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
    const size_t state_bytes = carve_state(rx->P, nullptr, rx->S);
    TRY_OR_CLEAN(rx->d_state_blob.ensure(state_bytes));
    TRY_OR_CLEAN(hipMemset(rx->d_state_blob, 0, state_bytes));
    carve_state(rx->P, (char *)rx->d_state_blob.get(), rx->S);
    TRY_OR_CLEAN(same::launch_init_state(rx->P, rx->S, 0, rx->own_stream));
    if (rx->dev_transport) {
        // the transport layer's per-channel records in HBM: a hot line and a cold record each (same_transport_dev.h)
        TRY_OR_CLEAN(rx->d_thot.ensure((size_t)n_channels * same::transport_hot_bytes()));
        TRY_OR_CLEAN(rx->d_tcold.ensure((size_t)n_channels * same::transport_cold_bytes()));
        TRY_OR_CLEAN(hipMemsetAsync(rx->d_tcold, 0, (size_t)n_channels * same::transport_cold_bytes(), rx->own_stream));
        TRY_OR_CLEAN(same::launch_transport_reset(rx->d_thot, rx->d_tcold, n_channels, nullptr, 0, 1, rx->own_stream));
    }
    TRY_OR_CLEAN(hipStreamSynchronize(rx->own_stream));
#undef TRY_OR_CLEAN
    rx->replay.link_only = (flags & SAME_BATCH_LINK_ONLY) != 0;
    rx->replay.messages_only = rx->messages_only;
    rx->replay.time_parallel = rx->tp.enabled;
    rx->replay.init(n_channels, rx->P.input_rate, !(flags & SAME_BATCH_LINK_ONLY) && !rx->dev_transport);
    rx->resets.init(n_channels);
    *out = rx;
    return SAME_OK;
}

void same_batch_free(same_batch *rx)
{
    if (!rx) return;
    (void)hipSetDevice(rx->device);
    if (rx->last_stream) (void)hipStreamSynchronize(rx->last_stream);
    // the members let their memory and events go; the streams last
    const hipStream_t streams[3] = {rx->copy_stream, rx->plan_stream, rx->own_stream};
    delete rx;
    for (hipStream_t st : streams)
        if (st) (void)hipStreamDestroy(st);
}

int same_batch_reset(same_batch *rx)
{
    if (!rx) return fail(SAME_EINVAL, "null handle");
    HIP_TRY(hipSetDevice(rx->device));
    int rc = harvest(rx);
    if (rc) return rc;
    hipError_t e = same::launch_init_state(rx->P, rx->S, 1, rx->own_stream);
    if (e == hipSuccess && rx->dev_transport)
        e = same::launch_transport_reset(rx->d_thot, rx->d_tcold, rx->P.n_channels, nullptr, 0, 0, rx->own_stream, rx->audio.d_rec);
    if (e != hipSuccess) return fail(SAME_EHIP, "reset launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(rx->own_stream));
    rx->counter = 0;
    rx->inv.fill = 0;                        // (samples that were waiting for their window are dropped with the rest of the state)
    rx->events.clear();                      // event_queue.clear() receiver.rs:194
    rx->replay.reset();
    if (rx->h_wake) std::memset(rx->h_wake, 0, (size_t)rx->P.n_channels * sizeof(uint64_t));
    rx->resets.clear();                      // (per-channel resets still due are covered: every column was re-initialised)
    rx->overflowed = false;
    rx->kernel_fault = false;
    // the audio queue goes with the event queue, and every capture is closed (the reset kernel closed the device's records)
    rx->audio.log.clear();
    rx->audio.flush_at = UINT64_MAX;
    return SAME_OK;
}

int same_batch_reset_channels(same_batch *rx, const uint32_t *channels, size_t n)
{
    if (!rx) return fail(SAME_EINVAL, "null handle");
    if (n && !channels) return fail(SAME_EINVAL, "null channel list");
    if (!same::ResetLedger::normalise(channels, n, rx->P.n_channels, rx->reset_list))
        return fail(SAME_EINVAL, "a channel of the list is out of range (the batch has %u); nothing was reset", rx->P.n_channels);
    if (rx->reset_list.empty()) return SAME_OK;
    HIP_TRY(hipSetDevice(rx->device));
    if (rx->inv.on && rx->inv.fill) {
        // SAME_BATCH_CALL_INVARIANT: what waits for its window is demodulated now and the next window begins at the reset, as
        // behind a flush -- the reset's stream position fixes the launches around it, whatever the calls look like
        const int rc = inv_launch_waiting(rx, rx->own_stream);
        if (rc) return rc;
    }
    // the position is behind the newest launch; if the harvest has not reached it yet, the host half waits for that launch's
    // harvest (no waiting here: it may still be running)
    int newest = -1;
    for (int s = 0; s < 2; ++s)
        if (rx->slot[s].in_flight && (newest < 0 || rx->slot[s].seq > rx->slot[newest].seq)) newest = s;
    if (newest < 0) {
        // every launch before the position is harvested: the open captures end here (in the counters before the reset)
        const int arc = rx->audio.log.end_reset(rx->reset_list, rx->counter, rx->resets);
        if (arc) return arc;
    }
    rx->resets.request(rx->reset_list, rx->counter, newest, rx->reset_now);
    for (uint32_t c : rx->reset_now) reset_channel_host(rx, c, rx->counter);
    return SAME_OK;
}

uint64_t same_batch_channel_input_sample_counter(const same_batch *rx, uint32_t channel)
{
    if (!rx || channel >= rx->P.n_channels) return 0;
    return rx->counter + rx->inv.fill - rx->resets.api_base[channel];
}

uint32_t same_batch_input_rate(const same_batch *rx) { return rx ? rx->P.input_rate : 0; }
uint32_t same_batch_n_channels(const same_batch *rx) { return rx ? rx->P.n_channels : 0; }
uint64_t same_batch_input_sample_counter(const same_batch *rx) { return rx ? rx->counter + rx->inv.fill : 0; }      // (samples accepted: demodulated or waiting for their window)
int same_batch_device(const same_batch *rx) { return rx ? rx->device : -1; }

int same_batch_process_device(same_batch *rx, const float *d_x, size_t n_samples, uint32_t layout, void *hip_stream)
{ return process_device_any<float>(rx, d_x, n_samples, layout, hip_stream); }
int same_batch_process_device_i16(same_batch *rx, const int16_t *d_x, size_t n_samples, uint32_t layout, void *hip_stream)
{ return process_device_any<int16_t>(rx, d_x, n_samples, layout, hip_stream); }
int same_batch_process_host(same_batch *rx, const float *h_x, size_t n_samples, uint32_t layout)
{ return process_host_any<float>(rx, h_x, n_samples, layout); }
int same_batch_process_host_i16(same_batch *rx, const int16_t *h_x, size_t n_samples, uint32_t layout)
{ return process_host_any<int16_t>(rx, h_x, n_samples, layout); }

int same_batch_process_device_ragged(same_batch *rx, const float *d_x, size_t n_rows, const uint32_t *counts, uint32_t layout, void *hip_stream)
{ return process_ragged_device<float>(rx, d_x, n_rows, counts, layout, hip_stream); }
int same_batch_process_device_ragged_i16(same_batch *rx, const int16_t *d_x, size_t n_rows, const uint32_t *counts, uint32_t layout,
                                         void *hip_stream)
{ return process_ragged_device<int16_t>(rx, d_x, n_rows, counts, layout, hip_stream); }
int same_batch_process_host_ragged(same_batch *rx, const float *h_x, size_t n_rows, const uint32_t *counts, uint32_t layout)
{ return process_ragged_host<float>(rx, h_x, n_rows, counts, layout); }
int same_batch_process_host_ragged_i16(same_batch *rx, const int16_t *h_x, size_t n_rows, const uint32_t *counts, uint32_t layout)
{ return process_ragged_host<int16_t>(rx, h_x, n_rows, counts, layout); }

int same_batch_flush(same_batch *rx)
{
    if (!rx) return fail(SAME_EINVAL, "null handle");
    HIP_TRY(hipSetDevice(rx->device));
    // four seconds of zeros per channel (receiver.rs:216-224), generated on the device
    const size_t n = (size_t)rx->P.input_rate * 4;
    const size_t slab = std::max<size_t>(1, std::min<size_t>(n, ((size_t)256 << 20) / ((size_t)rx->P.n_channels * sizeof(float))));
    if (slab * rx->P.n_channels * sizeof(float) > rx->d_zero.size()) {
        HIP_TRY(rx->d_zero.ensure(slab * rx->P.n_channels * sizeof(float)));
        HIP_TRY(hipMemset(rx->d_zero, 0, rx->d_zero.size()));       // once per growth: the kernels only read it
    }
    int rc = SAME_OK;
    rx->audio.flush_at = rx->counter + rx->inv.fill;      // (the zeros are never captured: a launch's rows from here on are clipped)
    for (size_t t0 = 0; t0 < n && rc == SAME_OK; t0 += slab) {
        rc = process_device_any<float>(rx, static_cast<const float *>(rx->d_zero.get()), std::min(slab, n - t0), SAME_LAYOUT_TIME_MAJOR, SAME_STREAM_OWN);
        if (rc == SAME_OK) rc = harvest(rx);
    }
    if (rc == SAME_OK && rx->inv.on) {
        // the end of the stream as far as the windows go: what is waiting is demodulated, the next window begins here
        rc = inv_launch_waiting(rx, rx->own_stream);
        if (rc == SAME_OK) rc = harvest(rx);
    }
    rx->audio.flush_at = UINT64_MAX;
    return rc;
}

int same_batch_set_call_window(same_batch *rx, uint32_t samples)
{
    if (!rx) return fail(SAME_EINVAL, "null handle");
    if (!rx->inv.on) return fail(SAME_EINVAL, "the batch was not made with SAME_BATCH_CALL_INVARIANT");
    if (samples < 64u || samples > (1u << 22)) return fail(SAME_EINVAL, "window of %u samples (64 .. 4 194 304)", samples);
    if (rx->counter || rx->inv.fill) return fail(SAME_EINVAL, "the window is set before the first sample (or right behind a reset)");
    rx->inv.window = samples;
    return SAME_OK;
}

int same_batch_order_after(same_batch *rx, void *producer_stream)
{
    if (!rx) return fail(SAME_EINVAL, "null handle");
    if (producer_stream == SAME_STREAM_OWN) return SAME_OK;
    HIP_TRY(hipSetDevice(rx->device));
    HIP_TRY(hipEventRecord(rx->ev_order, (hipStream_t)producer_stream));
    HIP_TRY(hipStreamWaitEvent(rx->own_stream, rx->ev_order, 0));
    HIP_TRY(hipStreamWaitEvent(rx->plan_stream, rx->ev_order, 0));      // (the planner reads the input too)
    return SAME_OK;
}

int same_batch_sync(same_batch *rx)
{
    if (!rx) return fail(SAME_EINVAL, "null handle");
    HIP_TRY(hipSetDevice(rx->device));
    int rc = harvest(rx);
    if (rc == SAME_OK && rx->inv.on) rc = inv_reads_wait(rx);      // (a call that only filled the waiting buffer made no launch)
    if (rc) return rc;
    if (rx->kernel_fault) return fail(SAME_EKERNEL, "a demodulation kernel's wavefronts lost step (internal hand-over timed out)");
    if (rx->overflowed) return fail(SAME_EOVERFLOW, "event/burst pool overflow");
    return SAME_OK;
}

size_t same_batch_pending_events(same_batch *rx)
{
    // events already brought back to the host; does not wait for launches still in flight
    if (!rx) return 0;
    return rx->events.pending();
}

int same_batch_poll_events(same_batch *rx, same_rx_event *out, size_t cap, size_t *n_out, size_t *n_left)
{
    if (!rx || (!out && cap)) return fail(SAME_EINVAL, "null argument");
    return rx->events.poll(rx->replay.workers, out, cap, n_out, n_left);
}

int same_batch_peek_events(same_batch *rx, const same_rx_event **events, size_t *n)
{
    if (!rx || !events || !n) return fail(SAME_EINVAL, "null argument");
    return rx->events.peek(rx->replay.workers, events, n);
}

int same_batch_drop_events(same_batch *rx, size_t n)
{
    if (!rx) return fail(SAME_EINVAL, "null argument");
    return rx->events.drop(n);
}

int same_batch_set_audio_capture(same_batch *rx, size_t samples_per_launch)
{
    if (!rx) return fail(SAME_EINVAL, "null handle");
    if (!rx->messages_only) return fail(SAME_EINVAL, "audio capture needs SAME_BATCH_MESSAGES_ONLY (the transport layer on the device)");
    if (rx->tp.enabled) return fail(SAME_EINVAL, "audio capture is not available in SAME_BATCH_TIME_PARALLEL batches");
    if (rx->counter || rx->inv.fill) return fail(SAME_EINVAL, "audio capture is set before the first sample (or right behind a reset)");
    HIP_TRY(hipSetDevice(rx->device));
    int rc = harvest(rx);
    if (rc) return rc;
    same_batch::Audio &A = rx->audio;
    auto release = [&]() {
        for (same_batch::Slot &sl : rx->slot) { (void)sl.d_pool.reset(); (void)sl.d_spans.reset(); }
        (void)A.d_rec.reset();
        A.per_launch = 0;
        A.log.open.clear();
    };
    release();
    if (!samples_per_launch) return SAME_OK;
    if (samples_per_launch > ((size_t)1 << 40)) return fail(SAME_EINVAL, "%zu samples per launch", samples_per_launch);
    auto oom = [&](const char *what) {
        (void)hipGetLastError();
        release();
        return fail(SAME_ENOMEM, "audio capture: %s (%zu samples per launch)", what, samples_per_launch);
    };
    for (same_batch::Slot &sl : rx->slot) {
        if (sl.d_pool.ensure(samples_per_launch) != hipSuccess) return oom("sample pool");
        if (!sl.d_cap_cur) {
            if (sl.d_cap_cur.ensure(1) != hipSuccess) return oom("cursors");
            HIP_TRY(hipMemset(sl.d_cap_cur, 0, sizeof(same::cap::Cursors)));
            if (sl.h_cap_cur.ensure(1) != hipSuccess) return oom("cursors");
        }
    }
    if (A.d_rec.ensure(rx->P.n_channels) != hipSuccess) return oom("capture records");
    HIP_TRY(hipMemset(A.d_rec, 0, (size_t)rx->P.n_channels * sizeof(same::cap::Rec)));
    A.log.open.assign(rx->P.n_channels, 0);
    A.per_launch = samples_per_launch;
    return SAME_OK;
}

int same_batch_peek_audio(same_batch *rx, const same_audio_chunk **chunks, size_t *n)
{
    if (!rx || !chunks || !n) return fail(SAME_EINVAL, "null argument");
    return rx->audio.log.peek(chunks, n);
}

int same_batch_drop_audio(same_batch *rx, size_t n)
{
    if (!rx) return fail(SAME_EINVAL, "null argument");
    return rx->audio.log.drop(n);
}

int same_batch_pack_bursts(same_batch *rx, uint32_t first_channel, uint8_t *out, size_t cap, size_t *n_records)
{
    if (!rx || !n_records) return fail(SAME_EINVAL, "null argument");
    return rx->events.pack_bursts(rx->replay.workers, first_channel, out, cap, n_records);
}

int same_batch_read_trace(same_batch *rx, uint32_t channel, same_symbol_trace *out, size_t cap, size_t *n_out)
{
    if (!rx || !n_out) return fail(SAME_EINVAL, "null argument");
    if (!rx->P.trace_cap) return fail(SAME_EINVAL, "batch was not created with SAME_BATCH_TRACE_SYMBOLS");
    if (channel >= rx->P.n_channels) return fail(SAME_EINVAL, "channel out of range");
    HIP_TRY(hipSetDevice(rx->device));
    int rc = harvest(rx);
    if (rc) return rc;
    uint32_t n = 0;
    HIP_TRY(hipMemcpy(&n, rx->S.trace_n + channel, sizeof(n), hipMemcpyDeviceToHost));
    n = std::min(n, rx->P.trace_cap);
    n = (uint32_t)std::min<size_t>(n, cap);
    std::vector<float> f((size_t)n * 4);
    std::vector<uint64_t> idx(n);
    if (n) {
        HIP_TRY(hipMemcpy(f.data(), rx->S.trace + (size_t)channel * rx->P.trace_cap * 4, f.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(idx.data(), rx->S.trace_idx + (size_t)channel * rx->P.trace_cap, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    for (uint32_t i = 0; i < n; ++i) {
        out[i].sample_counter = idx[i];
        out[i].zero = f[4 * i]; out[i].sym = f[4 * i + 1]; out[i].err = f[4 * i + 2];
        out[i].samples_until_next_ted = f[4 * i + 3];
    }
    *n_out = n;
    return SAME_OK;
}

void same_batch_set_kernel_timing(same_batch *rx, int enable) { if (rx) { rx->timing = enable != 0; rx->have_timing = false; } }
int same_batch_last_kernel_ms(same_batch *rx, float *ms)
{
    if (!rx || !ms) return fail(SAME_EINVAL, "null argument");
    // duration of the most recently collected launch; never waits for one still running
    if (!rx->have_timing) return fail(SAME_EINVAL, "no timed launch yet");
    *ms = rx->last_ms;
    return SAME_OK;
}
int same_batch_last_demod_kernel_ms(same_batch *rx, float *ms)
{
    if (!rx || !ms) return fail(SAME_EINVAL, "null argument");
    if (!rx->have_timing) return fail(SAME_EINVAL, "no timed launch yet");
    *ms = rx->last_demod_ms;
    return SAME_OK;
}
int same_batch_time_parallel_config(same_batch *rx, uint32_t max_chunks, uint32_t min_own_samples, uint32_t warmup_samples)
{
    if (!rx) return fail(SAME_EINVAL, "null handle");
    if (!rx->tp.enabled) return fail(SAME_EINVAL, "batch was not created with SAME_BATCH_TIME_PARALLEL");
    rx->tp.cfg.max_chunks = max_chunks; rx->tp.cfg.min_own = min_own_samples; rx->tp.cfg.warmup = warmup_samples;
    return SAME_OK;
}
uint32_t same_batch_time_parallel_chunks(const same_batch *rx) { return rx ? rx->tp.last_chunks : 0; }
int same_batch_transport_on_device(const same_batch *rx) { return rx && rx->last_dev_transport ? 1 : 0; }
int same_batch_time_parallel_per_channel(const same_batch *rx) { return rx && rx->tp.last_chunks > 1u && rx->tp.last_per_channel ? 1 : 0; }

int same_batch_debug_tp_plan(same_batch *rx, same_tp_plan_info *info, float *energy, size_t energy_cap, uint32_t *geom,
                             size_t geom_cap, uint64_t *handover, size_t handover_cap, uint32_t *final_col, size_t final_col_cap)
{
    if (!rx || !info) return fail(SAME_EINVAL, "null argument");
    if (rx->launch_seq == 0) return fail(SAME_EINVAL, "no launch yet");
    // the most recent launch's slot: its geometry and hand-over buffers are its own; the energy map and the final columns are
    // the batch's, last written by that launch
    const same_batch::Slot &sl = rx->slot[(rx->launch_seq - 1) & 1];
    if (!sl.chunked || !sl.per_channel) return fail(SAME_EINVAL, "the last launch had no per-channel plan");
    if (rx->slot[0].in_flight || rx->slot[1].in_flight) return fail(SAME_EINVAL, "a launch is in flight: same_batch_sync first");
    const same::TpPlan &p = sl.plan;
    const same::TpGeomWords &w = sl.words;
    const size_t columns = (size_t)p.n_chunks * p.channels, n_energy = (size_t)p.channels * p.scout_blocks;
    *info = same_tp_plan_info{};
    info->channels = p.channels; info->n_chunks = p.n_chunks; info->block_len = p.block_len;
    info->warmup_samples = p.warmup_samples; info->whole_samples = p.whole_samples; info->scout_blocks = p.scout_blocks;
    info->sort_mode = sl.plan_sorted ? 1u : 0u; info->lpt = sl.plan_lpt ? 1u : 0u; info->pair_groups = sl.plan_pairs ? 1u : 0u;
    info->in_samples = p.in_samples; info->counter0 = sl.plan_counter0;
    info->w_own_start = w.own_start; info->w_row0 = w.row0; info->w_nominal = w.nominal; info->w_perm = w.perm;
    info->w_wg = w.wg; info->w_wg2 = w.wg2; info->w_perm2 = w.perm2; info->w_total = w.total;
    if ((energy && energy_cap < n_energy) || (geom && geom_cap < w.total) || (handover && handover_cap < columns) ||
        (final_col && final_col_cap < p.channels))
        return fail(SAME_EINVAL, "a read-back buffer is too small");
    if (w.total > sl.d_geom.size() || columns > sl.d_handover.size() || n_energy > rx->tp.d_energy.size() ||
        p.channels > rx->tp.d_final_col.size())
        return fail(SAME_EINVAL, "the plan's buffers are gone");
    HIP_TRY(hipSetDevice(rx->device));
    if (energy) HIP_TRY(hipMemcpy(energy, rx->tp.d_energy, n_energy * sizeof(float), hipMemcpyDeviceToHost));
    if (geom) HIP_TRY(hipMemcpy(geom, sl.d_geom, w.total * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (handover) HIP_TRY(hipMemcpy(handover, sl.d_handover, columns * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (final_col) HIP_TRY(hipMemcpy(final_col, rx->tp.d_final_col, (size_t)p.channels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SAME_OK;
}

const char *same_batch_kernel_name(const same_batch *rx)
{
    return rx ? same::family_name(rx->last_family, rx->P.block_len) : "";
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// single receiver with the reference's pull semantics
// ------------------------------------------------------------------------------------

struct same_rx {
    same_batch *batch = nullptr;
    uint64_t reported = 0;           // samples the caller has logically consumed
    uint64_t zeros_until = 0;        // the device ran over flush zeros up to this sample (0 = no such run-ahead)
    std::deque<same_rx_event> events;
};

static int rx_pump(same_rx *rx)
{
    same_rx_event buf[64];
    for (;;) {
        size_t n = 0, left = 0;
        int rc = same_batch_poll_events(rx->batch, buf, 64, &n, &left);
        if (rc) return rc;
        for (size_t i = 0; i < n; ++i) rx->events.push_back(buf[i]);
        if (!left) return SAME_OK;
    }
}

extern "C" {

int same_rx_build(const same_rx_builder *b, int device, same_rx **out)
{
    if (!out) return fail(SAME_EINVAL, "null out");
    *out = nullptr;
    same_rx *rx = new (std::nothrow) same_rx;
    if (!rx) return fail(SAME_ENOMEM, "out of memory");
    int rc = same_batch_new(b, 1, device, 0, &rx->batch);
    if (rc) { delete rx; return rc; }
    *out = rx;
    return SAME_OK;
}
void same_rx_free(same_rx *rx) { if (rx) { same_batch_free(rx->batch); delete rx; } }

static int rx_process(same_rx *rx, const float *x, size_t n, size_t *consumed, same_rx_event *ev);

int same_rx_process(same_rx *rx, const float *x, size_t n, size_t *consumed, same_rx_event *ev)
{
    if (!rx || !consumed || !ev || (!x && n)) return fail(SAME_EINVAL, "null argument");
    *consumed = 0;
    if (rx->zeros_until > rx->reported && n)
        return fail(SAME_EINVAL, "a flush returned at its first message with the device %llu zero samples ahead; "
                                 "reset the receiver (or flush again) before presenting audio",
                    (unsigned long long)(rx->zeros_until - rx->reported));
    return rx_process(rx, x, n, consumed, ev);
}

static int rx_process(same_rx *rx, const float *x, size_t n, size_t *consumed, same_rx_event *ev)
{
    *consumed = 0;
    // x[0] sits at absolute sample `reported`; the device may already be past it
    const uint64_t device_at = same_batch_input_sample_counter(rx->batch);
    const uint64_t end = rx->reported + n;
    if (end > device_at) {
        const size_t skip = (size_t)(device_at - rx->reported);
        int rc = same_batch_process_host(rx->batch, x + skip, n - skip, SAME_LAYOUT_TIME_MAJOR);
        if (rc) return rc;
        rc = rx_pump(rx);
        if (rc) return rc;
    }
    if (!rx->events.empty() && rx->events.front().sample_counter <= end) {
        *ev = rx->events.front();
        rx->events.pop_front();
        // queued events are returned before any new sample is consumed (receiver.rs:238-240)
        const uint64_t at = ev->sample_counter > rx->reported ? ev->sample_counter : rx->reported;
        *consumed = (size_t)(at - rx->reported);
        rx->reported = at;
        return 1;
    }
    *consumed = n;
    rx->reported = end;
    return 0;
}

int same_rx_flush(same_rx *rx, same_rx_event *msg)
{
    // flush() receiver.rs:216-224: four seconds of zeros, first Message(Ok(..)) wins
    if (!rx) return fail(SAME_EINVAL, "null handle");
    const size_t n = (size_t)same_batch_input_rate(rx->batch) * 4;
    std::vector<float> zeros(n, 0.0f);
    size_t off = 0;
    while (off < n) {
        size_t used = 0;
        same_rx_event ev;
        int got = rx_process(rx, zeros.data() + off, n - off, &used, &ev);
        if (got < 0) return got;
        off += used;
        if (!got) break;
        if (ev.kind == SAME_TRANSPORT_MSG_START || ev.kind == SAME_TRANSPORT_MSG_END) {
            if (msg) *msg = ev;
            // the device has consumed all n zeros, the caller only those up to this event
            rx->zeros_until = same_batch_input_sample_counter(rx->batch);
            return 1;
        }
    }
    return 0;
}

int same_rx_reset(same_rx *rx)
{
    if (!rx) return fail(SAME_EINVAL, "null handle");
    rx->events.clear();
    rx->reported = 0;
    rx->zeros_until = 0;
    return same_batch_reset(rx->batch);
}
uint32_t same_rx_input_rate(const same_rx *rx) { return rx ? same_batch_input_rate(rx->batch) : 0; }
uint64_t same_rx_input_sample_counter(const same_rx *rx) { return rx ? rx->reported : 0; }

int same_synth_afsk_device(float *d_x, uint32_t n_channels, size_t n_samples, uint32_t input_rate,
                           uint64_t seed, float noise_sigma, uint32_t flags, int device, void *hip_stream)
{
    if (!d_x || !n_channels) return fail(SAME_EINVAL, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SAME_ENODEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    same::SynthParams sp{n_channels, input_rate, seed, noise_sigma, flags};
    hipError_t e = same::launch_synth(sp, d_x, n_samples, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(SAME_EHIP, "synth launch failed: %s", hipGetErrorString(e));
    return SAME_OK;
}
uint32_t same_synth_payload(uint64_t seed, uint32_t channel, uint8_t *out, uint32_t cap)
{ return same::synth_payload(seed, channel, out, cap); }

int same_synth_trials_device(float *d_x, uint32_t n_trials, uint32_t first_trial, size_t n_samples,
                             uint32_t input_rate, uint64_t seed, float ebn0_db_lo, float ebn0_db_step,
                             uint32_t n_grid, int device, void *hip_stream)
{
    if (!d_x || !n_trials || !n_grid) return fail(SAME_EINVAL, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SAME_ENODEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    same::TrialParams tp{n_trials, first_trial, input_rate, n_grid, seed, ebn0_db_lo, ebn0_db_step};
    hipError_t e = same::launch_trials(tp, d_x, n_samples, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(SAME_EHIP, "trial generator launch failed: %s", hipGetErrorString(e));
    return SAME_OK;
}

}  // extern "C"
