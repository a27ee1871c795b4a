// same_launch.h -- host-callable launchers implemented in same_kernels.hip / same_synth.hip
#pragma once

#include <hip/hip_runtime.h>

#include "same_capture_dev.h"
#include "same_device.h"
#include "same_select.h"      // which of these launchers takes a launch, and the predicates callers use

namespace same {

hipError_t launch_demod(const Params &P, const State &S, const Output &O, const float4 *taps,
                        const float *x, uint32_t n_samples, uint64_t counter0, hipStream_t stream);
hipError_t launch_demod(const Params &P, const State &S, const Output &O, const float4 *taps,
                        const int16_t *x, uint32_t n_samples, uint64_t counter0, hipStream_t stream);
// the ragged remainder of a ragged call (same_batch_process_*_ragged): rows [0, n_rows) of x, lane c consuming its first
// min(counts[c] - row_sub, n_rows) of them (counts: device-readable, n_channels entries); leaves the state canonical at
// counter0 + n_rows
hipError_t launch_demod_ragged(const Params &P, const State &S, const Output &O, const float4 *taps, const float *x,
                               uint32_t n_rows, const uint32_t *counts, uint32_t row_sub, uint64_t counter0, hipStream_t stream);
hipError_t launch_demod_ragged(const Params &P, const State &S, const Output &O, const float4 *taps, const int16_t *x,
                               uint32_t n_rows, const uint32_t *counts, uint32_t row_sub, uint64_t counter0, hipStream_t stream);
// four-stage wavefront pipeline (same_kernels_pipe.hip): up to 32 768 channels at 22.05 kHz
// relaxed: the FASTMATH build (relaxed arithmetic, same_relaxed_common.h); only where pipe_relaxed_supported(P)
hipError_t launch_demod_pipe(const Params &P, const State &S, const Output &O, const float4 *taps,
                             const float *x, uint32_t n_blocks, uint64_t counter0, hipStream_t stream,
                             const PipeChunks &chunks = PipeChunks{}, bool relaxed = false);
hipError_t launch_demod_pipe(const Params &P, const State &S, const Output &O, const float4 *taps,
                             const int16_t *x, uint32_t n_blocks, uint64_t counter0, hipStream_t stream,
                             const PipeChunks &chunks = PipeChunks{}, bool relaxed = false);
// symbol-paced pipeline (same_kernels_sym.hip): relaxed arithmetic, 22.05 kHz, 36-sample steps, whole groups of 64 state
// columns; takes time-parallel chunks like the pipeline
hipError_t launch_demod_sym(const Params &P, const State &S, const Output &O, const float4 *taps,
                            const float *x, uint32_t n_blocks, uint64_t counter0, hipStream_t stream,
                            const PipeChunks &chunks = PipeChunks{});
hipError_t launch_demod_sym(const Params &P, const State &S, const Output &O, const float4 *taps,
                            const int16_t *x, uint32_t n_blocks, uint64_t counter0, hipStream_t stream,
                            const PipeChunks &chunks = PipeChunks{});
// relaxed-arithmetic throughput kernel (same_kernels_relaxed.hip): 22.05 kHz, one wavefront per 64 state columns,
// whole blocks of relaxed_block_len() samples; takes time-parallel chunks like the pipeline
hipError_t launch_demod_relaxed(const Params &P, const State &S, const Output &O, const float4 *taps,
                                const float *x, uint32_t n_blocks, uint64_t counter0, hipStream_t stream,
                                const PipeChunks &chunks = PipeChunks{});
hipError_t launch_demod_relaxed(const Params &P, const State &S, const Output &O, const float4 *taps,
                                const int16_t *x, uint32_t n_blocks, uint64_t counter0, hipStream_t stream,
                                const PipeChunks &chunks = PipeChunks{});
// latency-optimised kernel for the standard rates (same_kernels_fast.hip); whole blocks of
// fast_block_len() samples, the generic kernel takes the rest of a call
hipError_t launch_demod_fast(const Params &P, const State &S, const Output &O, const float4 *taps,
                             const float *x, uint32_t n_blocks, uint64_t counter0, hipStream_t stream);
hipError_t launch_demod_fast(const Params &P, const State &S, const Output &O, const float4 *taps,
                             const int16_t *x, uint32_t n_blocks, uint64_t counter0, hipStream_t stream);
// zero the launch cursors (publish = 0) or copy them to host-mapped memory (publish = 1)
hipError_t launch_counters(uint32_t *dev, uint32_t *host_mapped, int publish, hipStream_t stream);
// the log ordered by state column: first [n_bins + 1] (exclusive offsets), sorted [cap] (the records, a column's in any
// order, their `channel` replaced by their index in the log), cnt [n_bins] scratch; counters[0] = events logged
// (`first` needs event_sort_extra_words(n_bins) words behind its n_bins + 1 for the scan's workgroup totals: same_tp_plan.h)
hipError_t launch_event_sort(const DevEvent *ev, const uint32_t *counters, uint32_t cap, uint32_t n_bins, uint32_t *cnt, uint32_t *first,
                             DevEvent *sorted, hipStream_t stream, bool cnt_is_zero = false);      // cnt_is_zero: the caller emptied cnt on this stream
// (first_col: columns before it are left alone -- the time-parallel launches copy the channels' own state over them next)
hipError_t launch_init_state(const Params &P, const State &S, int is_reset, hipStream_t stream, uint32_t first_col = 0);
// reset() of the columns cols[0 .. n) (device-readable, e.g. mapped pinned host memory; each < P.n_channels)
hipError_t launch_reset_columns(const Params &P, const State &S, const uint32_t *cols, uint32_t n, hipStream_t stream);
// Column copies between state blobs of different widths: for every array of `desc` (device memory,
// n_desc entries) and every column col < n_cols, dst[row][col] = src[row][src_col ? src_col[col] : col + src_base].
hipError_t launch_copy_state_columns(const StateArrayDesc *desc, uint32_t n_desc, uint32_t src_channels,
                                     uint32_t dst_channels, const uint32_t *src_col, uint32_t n_cols, hipStream_t stream,
                                     uint32_t src_base = 0);   // src_col == nullptr: source column = col + src_base
// final_col[c] = the state column (chunk * in_channels + c) whose chunk ran to the end of the input
hipError_t launch_chunk_final_column(const uint64_t *handover, uint32_t in_channels, ChunkGeom g, uint32_t *final_col,
                                     hipStream_t stream);
// ... with per-channel boundaries: own_start [n_chunks][in_channels], relative to the call's first sample (counter0)
hipError_t launch_chunk_final_column_pc(const uint64_t *handover, const uint32_t *own_start, uint32_t in_channels, uint32_t n_chunks,
                                        uint64_t counter0, uint32_t *final_col, hipStream_t stream);
hipError_t launch_fill_u64(uint64_t *p, size_t n, uint64_t v, hipStream_t stream);
hipError_t launch_cast_i16_f32(const int16_t *in, float *out, size_t n, hipStream_t stream);      // out[i] = (float)in[i]
// The start of a time-parallel launch: blob[0 .. bytes) = fresh[0 .. bytes) (a template of freshly built receivers, 16-byte
// multiples), handover[0 .. n_cols) = kNoHandover, sort_cnt[0 .. n_cols) = 0 (may be null), counters[0 .. 3) = 0 (may be null)
hipError_t launch_tp_prologue(void *blob, const void *fresh, size_t bytes, uint64_t *handover, uint32_t *sort_cnt, uint32_t n_cols,
                              uint32_t *counters, hipStream_t stream);
// Per-channel chunk boundaries for a channel-major input (time-parallel mode): an energy scout over
// one 64-byte sector per 256-sample block, then per channel the idle instant nearest to every nominal boundary.
struct TpPlan {
    uint32_t channels, n_chunks, block_len, warmup_samples, whole_samples;
    uint64_t in_samples;      // pitch of a channel in the input
    uint32_t scout_blocks;    // whole_samples / 256
};
// energy [channels][scout_blocks] (scratch), own_start [n_chunks][channels], row0 / nominal / perm [n_chunks * channels],
// wg_blocks [n_chunks * channels / 64]; perm_out / wg_blocks_out (same sizes, may be
// null; wg_blocks_out [2][workgroups]): the workgroups of perm / wg_blocks once more, longest first
hipError_t launch_tp_plan(const float *x, const TpPlan &g, float *energy, uint32_t *own_start, uint32_t *row0,
                          uint32_t *nominal, uint32_t *perm, uint32_t *wg_blocks, bool sorted, hipStream_t stream,
                          uint32_t *perm_out = nullptr, uint32_t *wg_blocks_out = nullptr, bool pairs = false);
hipError_t launch_transpose(const float *in, float *out, uint32_t n_channels, uint32_t n_samples,
                            hipStream_t stream);
hipError_t launch_transpose(const int16_t *in, int16_t *out, uint32_t n_channels, uint32_t n_samples,
                            hipStream_t stream);

// The transport layer on the device (same_transport.hip, SAME_BATCH_MESSAGES_ONLY): one lane per channel walks its range of
// the launch's column-ordered log (behind launch_event_sort), runs the transport layer over it and appends the messages to
// the log: records 0 .. near_cap - 1 go to `near` (host-mapped pinned memory the host reads in place: a launch's few hundred
// messages need no copy), the rest to `log` (HBM); a full log sets kMessageLogOverflow in *overflow.  hot / cold: n_channels records of transport_hot_bytes() /
// transport_cold_bytes() (same_transport_dev.h).
constexpr uint32_t kMessageLogOverflow = 8u;      // bit of the launch's overflow word (1: event log, 2: burst pool)
struct TransportLaunch {
    uint32_t n_channels, input_rate;
    const uint32_t *first;         // [n_channels + 1] the columns' ranges of `sorted`
    DevEvent *sorted;              // re-ordered in place, range by range
    const uint32_t *counters;      // the launch's cursors: [1] bursts logged
    const uint8_t *bursts; uint32_t burst_cap;
    void *hot, *cold;
    uint64_t *wake_sample;         // State::wake_sample: the forced-EOM instant the next launch wakes the channel after
    DevMessage *near; uint32_t near_cap;
    DevMessage *log; uint32_t log_cap;
    uint32_t *log_cursor, *overflow;
    cap::Launch cap;               // same_batch_set_audio_capture (cap.rec == nullptr: off, the kernel does nothing more)
};
size_t transport_hot_bytes();
size_t transport_cold_bytes();
hipError_t launch_transport(const TransportLaunch &T, hipStream_t stream);
// a ragged launch (same_batch_process_*_ragged): channel c consumed the first min(counts[c] - row_sub, n_rows) of the launch's
// n_rows rows (counts: device-readable); its captures stop there and an armed forced-EOM instant moves by the rows it skipped
hipError_t launch_transport_ragged(const TransportLaunch &T, const uint32_t *counts, uint32_t row_sub, uint32_t n_rows, hipStream_t stream);
// reset() of the transport layer of the columns cols[0 .. n) (device-readable), or of every channel (cols == nullptr); fresh: the
// records were never written (a new batch); capture_rec: the channels' capture records (cap::Rec), closed too, or nullptr
hipError_t launch_transport_reset(void *hot, void *cold, uint32_t n_channels, const uint32_t *cols, uint32_t n, int fresh,
                                  hipStream_t stream, void *capture_rec = nullptr);
// The capture kernel (same_capture.hip, same_batch_set_audio_capture): behind launch_transport, on the launch's stream, it copies
// the spans the transport kernel listed (their number: *n_spans, read on the device) out of the launch's input x (time-major, row
// pitch n_channels, n_rows rows) into the pool.  A fixed grid, whatever the number of spans.
// Then its epilogue copies the launch's cursors to `host` (host-mapped) and zeroes them.
hipError_t launch_capture(const cap::Span *spans, cap::Cursors *cur, uint32_t span_cap, float *pool, uint64_t pool_cap,
                          const float *x, uint32_t n_channels, uint32_t n_rows, cap::Cursors *host, hipStream_t stream);
hipError_t launch_capture(const cap::Span *spans, cap::Cursors *cur, uint32_t span_cap, float *pool, uint64_t pool_cap,
                          const int16_t *x, uint32_t n_channels, uint32_t n_rows, cap::Cursors *host, hipStream_t stream);

// synthetic workload (same_synth.hip)
struct SynthParams {
    uint32_t n_channels;
    uint32_t input_rate;
    uint64_t seed;
    float noise_sigma;     // AWGN standard deviation relative to the carrier amplitude (0 = none)
    uint32_t flags;        // bit 0: integer (even) samples per symbol like the reference's test modulator
};
hipError_t launch_synth(const SynthParams &sp, float *x, size_t n_samples, hipStream_t stream);
struct TrialParams {
    uint32_t n_trials;     // trials in this buffer (one per channel)
    uint32_t first_trial;  // global id of trial 0 of this buffer
    uint32_t input_rate;
    uint32_t n_grid;       // Eb/N0 grid points; trial t uses point t mod n_grid
    uint64_t seed;
    float ebn0_db_lo, ebn0_db_step;
};
hipError_t launch_trials(const TrialParams &tp, float *x, size_t n_samples, hipStream_t stream);
// host mirror of the per-channel payload the generator transmits (header text)
uint32_t synth_payload(uint64_t seed, uint32_t channel, uint8_t *out, uint32_t cap);

}  // namespace same
