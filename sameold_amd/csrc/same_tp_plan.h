// same_tp_plan.h -- how a call is cut: the launch cap, the uniform time-parallel cut, the plan of a channel-major call with
// per-channel boundaries (its qualification, the words of the geometry buffer, its scratch) and the capacities of a launch's
// output.  Host-only arithmetic like same_select.h, which answers WHICH kernel runs a piece: nothing of HIP, so it compiles
// with a plain C++ compiler and is tabulated without a GPU (tests/test_tp_plan_cpu.py).  same_batch.cpp asks here and only
// allocates, queues and books.  DESIGN.md 4.6 and "Which kernel runs a launch".
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "same_config.h"
#include "same_device.h"
#include "same_select.h"

namespace same {

// ---- device constants this arithmetic needs (same_kernels.hip takes them from here) ----------------------------------
#ifndef SAME_SCOUT_BLOCK
#define SAME_SCOUT_BLOCK 256
#endif
constexpr uint32_t kScoutBlock = SAME_SCOUT_BLOCK;        // samples per energy reading of the scout (one 64-byte sector of them is read)
constexpr uint32_t kScanThreads = 1024;                   // threads per workgroup of the event sort's scan
// words the event sort's `first` needs behind its n_bins + 1 (the scan's workgroup totals)
inline uint32_t event_sort_extra_words(uint32_t n_bins) { return (n_bins + kScanThreads - 1u) / kScanThreads; }

// ---- the launch cap --------------------------------------------------------------------------------------------------
// One launch stays comfortably inside u32 sample indices and bounded output pools, and well under the 135 s forced-EOM
// timeout the host arms one launch late (harvest): 45 s, 2^22 samples at the most
constexpr size_t kMaxLaunchSamples = (size_t)1 << 22;
inline size_t max_launch_samples(uint32_t input_rate) { return kMaxLaunchSamples < (size_t)input_rate * 45 ? kMaxLaunchSamples : (size_t)input_rate * 45; }

// ---- same_batch_time_parallel_config and the knobs of the time-parallel mode -------------------------------------------
struct TpConfig {
    uint32_t max_chunks = 0, min_own = 0, warmup = 0;      // same_batch_time_parallel_config (0 = default)
    int sort_mode = -1;          // SAME_TP_SORT: -1 choose, 0 grid order, 1 pieces sorted by length into workgroups, 2 groups of 64 paired long with short
    int knob_plan_stream = 0;    // SAME_TP_PLAN_STREAM=0: planning kernels stay on the launch stream (A/B measurements)
    int knob_prologue = 0;       // SAME_TP_PROLOGUE=0: init kernel, fill and cursor reset as separate launches (A/B measurements)
};

// ---- the uniform cut -------------------------------------------------------------------------------------------------
// How a call of n samples is cut into time-parallel chunks: n_chunks pieces per channel run by `choice`, or n_chunks == 1
// when the call runs as one launch (mode off, configuration without a pipeline kernel, call too short; geom and pc are
// zero then).  pc: the uniform fields; the launch adds the hand-over records and the per-column arrays.
struct TpCut {
    uint32_t n_chunks = 1;
    Choice choice;
    ChunkGeom geom{};
    PipeChunks pc{};
};
TpCut tp_uniform_cut(const Params &P, const Mode &m, const Request &rq, const TpConfig &cfg, size_t n, uint64_t counter0,
                     uint32_t column_cap = kTpColumnCap, bool channel_major = false);

// ---- a channel-major call read where it lies, boundaries per channel ----------------------------------
// the uniform cut such a call starts from; not cut (n_chunks == 1) beyond kMaxLaunchSamples and off 22.05 kHz (42 taps)
TpCut tp_native_cut(const Params &P, const Mode &m, const Request &rq, const TpConfig &cfg, size_t n_call, uint64_t counter0);
// Slot::d_geom in words: own_start | row0 | nominal | perm [columns each] | wg [columns / 64] | wg2 [2][columns / 64] | perm2 [columns]
struct TpGeomWords {
    size_t own_start = 0, row0 = 0, nominal = 0, perm = 0, wg = 0, wg2 = 0, perm2 = 0;
    size_t total = 0;
    size_t harvest = 0;      // what the harvest copies back: own_start | row0
};
struct TpNative {
    bool qualifies = false;      // false: the caller takes the transposing path (every other field is zero)
    uint32_t whole_samples = 0;  // the call's whole blocks; the rest goes through the any-configuration kernel afterwards
    uint32_t warmup_samples = 0, scout_blocks = 0;      // (TpPlan)
    uint64_t in_samples = 0;
    int sort_mode = 0;           // the planner sorts the pieces by length into workgroups
    bool pair_groups = false;    // ... or pairs the groups of 64 longest with shortest (SAME_TP_SORT=2)
    bool lpt = false;            // the workgroups once more, longest first: the launch reads perm2 / wg2 as its col_perm / wg_blocks
    bool need_hist = false;      // the squelch-history scratch by grid position (PipeChunks::hist_scratch)
    size_t hist_floats = 0, energy_floats = 0;
    TpGeomWords words;
};
// n_call: samples per channel; base: the input's address
TpNative tp_native_plan(const Params &P, const TpConfig &cfg, const TpCut &cut, size_t n_call, uintptr_t base);
// planning kernels beside the previous launch's tail: on the library's own stream unless SAME_TP_PLAN_STREAM=0
inline bool tp_plan_beside(const TpConfig &cfg, bool own_stream) { return own_stream && cfg.knob_plan_stream >= 0; }

// ---- output capacities -----------------------------------------------------------------------------------------------
constexpr size_t kSpanBytes = 32;      // sizeof(cap::Span) (same_capture_dev.h; same_batch.cpp asserts it)
struct OutputCaps {
    size_t events = 0, bursts = 0;
    size_t messages = 0, near = 0, spans = 0;      // the transport layer on the device (0: the launch has none; spans 0: no capture)
    size_t bins = 0, sort_words = 0;               // the event sort: one bin per state column
};
// A launch of n_samples over n_columns state columns (0: an ordinary launch, P.n_channels columns, which runs the transport
// layer on the device where the batch has it there).  near_cap / msg_cap: what the slot holds already (buffers only grow).
OutputCaps output_caps(const Params &P, size_t n_samples, size_t n_columns, bool dev_transport, bool audio, size_t near_cap, size_t msg_cap);
// the samples a time-parallel launch of n sizes its output for: no column runs much longer than its nominal piece
inline size_t tp_output_samples(size_t n, const PipeChunks &pc, uint32_t block_len)
{
    const size_t m = 3 * (size_t)pc.nominal_blocks * block_len + 65536;
    return n < m ? n : m;
}

}  // namespace same
