// same_select.h -- which demodulation kernel runs a launch, and in what block length.  Host-only arithmetic on Params, the
// batch's creation flags and the knobs: nothing of HIP, so the whole decision compiles with a plain C++ compiler and is
// tabulated without a GPU (tests/test_kernel_choice_cpu.py).  same_batch.cpp asks the decisions at the end of this header;
// the kernel units read the family-internal form choices (mirror / dense, lanes / share / split, solo / duo / wide) from the
// predicates in front of them.  DESIGN.md, "Which kernel runs a launch", has the table.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "same_config.h"
#include "same_device.h"

namespace same {

// ---- block geometry the decision needs (the device headers take these values or assert equality with them) -----------
// Block length of the fast kernel: 16 samples, or 18 for the mirrored-window variant.  Both
// are below the shortest interval between two TED instants at the standard rates (see
// choose_block_len: 18 is the bound at 22.05 kHz), so a block holds at most one instant.
constexpr int kBlock = 16;
constexpr int kBlockMirror = 18;
// The 22.05 kHz wavefront pipeline runs 20-sample blocks: instants are at least 19.45 samples apart
// there (the bound above), so a block can hold a SECOND instant when the timing loop runs at its
// fastest -- never a third -- and stage 2 handles that rare one on the spot (same_kernels_pipe.hip).
// Of the two, exactly one completes a symbol (the TED alternates), so everything downstream still
// sees at most one symbol per block.
constexpr int kBlockPipe22 = 20;
// 48 kHz (92 taps) and 44.1 kHz (84 taps): instants are 46 / 42 samples apart and the bound is
// 43 / 39, so the block is 32 -- the block-rate passes (the long filters, timing loop, symbol
// path) serve twice the samples.
constexpr int kBlock48k = 32;
// Samples per block of the pipeline at 48 / 44.1 kHz (bounds 43 / 39, one instant per block).  Measured at 16 384
// channels x 2 s: 48 kHz 6.03 ms with 32, 6.75 with 36, 6.48 with 40 (stage 1's registers);
// 44.1 kHz 5.35 ms with 32, 5.20 with 36.
constexpr int kBlockPipe48 = 32, kBlockPipe44 = 36;
// the symbol-paced pipeline: a step is one 36-sample sub-block at 22.05 kHz, two at 44.1 / 48 kHz; its window ring holds six steps
constexpr int kSymStep22 = 36, kSymStepHi = 72, kSymRingSteps = 6;
// the one- / two-wavefront relaxed kernel: two 21-sample sub-blocks
constexpr int kBlockRelaxed = 42;

// ---- tests that every family shares ----------------------------------------------------------------------------------
// 22.05 / 48 / 44.1 kHz with the reference's default DC-blocker length: the filter length (42 / 92 / 84), else 0
uint32_t standard_rate_taps(const Params &P);
// the default (6 + 4 taps) or the disabled (1 + 1) equalizer: the two every block kernel is built for
bool eq_default_or_disabled(const Params &P);
// v_med3_f32 == f32::clamp unless a bound is -0.0 (or NaN, which the builder rejects)
bool agc_clamp_is_med3(const Params &P);

// ---- the any-configuration kernel (same_kernels.hip) ------------------------------------------------------------------
size_t demod_lds_bytes(const Params &P);

// ---- the one-wavefront kernel (same_kernels_fast.hip): whole blocks of fast_block_len() samples ----------------------
bool fast_kernel_supported(const Params &P);
uint32_t fast_block_len(const Params &P);   // samples per block of the block kernel an ordinary strict launch runs (the pipeline's where that is selected)
bool fast_use_mirror(const Params &P);      // the mirrored window (42 taps)
bool fast_use_dense(const Params &P);       // the two-per-SIMD build (42 taps, not mirrored)
uint32_t fast_win_ring(const Params &P);

// ---- the four-stage wavefront pipeline (same_kernels_pipe.hip): up to 32 768 channels at 22.05 kHz -------------------
bool pipe_kernel_selected(const Params &P);
uint32_t pipe_kernel_stages(const Params &P);     // 0 (not selected) or non-zero
uint32_t pipe_block_len(const Params &P);         // samples per block of the pipeline at this rate
uint32_t pipe_workgroup_channels(const Params &P);   // channels per workgroup the pipeline would use for this batch
bool pipe_share(const Params &P);                 // the two-workgroups-per-CU register budget (22.05 kHz)
bool pipe_split(const Params &P, bool share);     // stage 2 split with stage 4's wavefront
bool pipe_relaxed_supported(const Params &P);     // the FASTMATH build (relaxed arithmetic, same_relaxed_common.h)

// ---- the symbol-paced pipeline (same_kernels_sym.hip): relaxed arithmetic, whole groups of 64 state columns ----------
bool sym_kernel_supported(const Params &P);
uint32_t sym_block_len(const Params &P);

// ---- the one- / two-wavefront relaxed kernel (same_kernels_relaxed.hip): 22.05 kHz -----------------------------------
bool relaxed_kernel_supported(const Params &P);
uint32_t relaxed_block_len(const Params &P);      // samples per block of the form relaxed_kernel_kind(P) picks for P.n_channels columns
uint32_t relaxed_kernel_kind(const Params &P);    // 0 solo (one wavefront per 64 columns), 1 duo (two)
bool relaxed_solo_wide(const Params &P);          // solo: a wavefront has its SIMD's registers to itself (f32 input only)

// ---- the decisions -----------------------------------------------------------------------------------------------------
// the six kernel families the batch host queues
enum class Family : uint32_t { kGeneric, kFast, kPipe, kPipeFastmath, kSym, kWaveRelaxed };
// the name same_batch_kernel_name reports (generic_block_len: Params::block_len, part of the any-configuration kernel's name)
const char *family_name(Family f, uint32_t generic_block_len);

// what a batch is created with: its flags and the knobs that are not part of Params
struct Request {
    bool relaxed = false, time_parallel = false, generic = false;      // SAME_BATCH_RELAXED, _TIME_PARALLEL, _GENERIC_KERNEL
    int32_t knob_relaxed = 0;      // SAME_RELAXED: -1 never (time-parallel chunks keep the strict pipeline), +1 as if SAME_BATCH_RELAXED were set
    int32_t knob_tp_kernel = 0;    // SAME_TP_KERNEL: 1 pipeline, 2 one-wavefront relaxed kernel, 0 choose
    uint32_t sym_max_channels = 1u << 30;      // SAME_SYM_MAX (measurement knob: up to where an ordinary relaxed launch takes the symbol-paced pipeline; default: always)
};
// the batch's arithmetic mode
struct Mode {
    bool block_kernels = false;    // the configuration has a latency-optimised kernel and SAME_BATCH_GENERIC_KERNEL does not forbid it
    bool relaxed = false;          // relaxed arithmetic in time-parallel chunks
    bool relaxed_plain = false;    // ... and in ordinary launches
};
Mode select_mode(const Params &P, const Request &rq);

// a family and its block length (0: no block kernel, every row goes to the any-configuration kernel)
struct Choice { Family family = Family::kGeneric; uint32_t block_len = 0; };
// the block kernel of an ordinary launch; the relaxed pipelines (kSym, kPipeFastmath) launch with fm_params(P)
Choice select_plain(const Params &P, const Mode &m, const Request &rq);
// ... and of a strict one: what same_batch_kernel_name answers before the first launch
Family strict_family(const Params &P, const Mode &m);

// The time-parallel candidates of a batch: pieces per channel from k_max down to 2, each with tp_candidate's family and block
// length; the first one whose geometry fits the call is taken (plan_chunks).  k_max < 2: the call is not cut.
struct TpRule {
    uint32_t k_max = 0;
    bool wave = false;         // the one- / two-wavefront relaxed kernel, any number of 64-column groups
    bool fastmath = false;     // the pipeline's relaxed builds (symbol-paced where it is built, else FASTMATH)
    bool force_pipe = false;   // the pipeline kernel whatever the column count
};
// max_chunks: same_batch_time_parallel_config (0 = default); column_cap: state columns the pipeline may take at 22.05 kHz
constexpr uint32_t kTpColumnCap = 32768u;
TpRule tp_rule(const Params &P, const Mode &m, const Request &rq, uint32_t max_chunks, uint32_t column_cap, bool channel_major);
bool tp_candidate(const Params &P, const TpRule &r, uint32_t K, Choice &c);      // false: K pieces are no option
// column_cap of a channel-major call read where it lies (per-channel boundaries)
uint32_t tp_native_column_cap(const Params &P, const Mode &m, uint32_t max_chunks);
// more state columns than the pipeline takes at full speed: its workgroups come in more than one round
bool tp_more_than_one_round(uint32_t columns);

// the configuration as the pipeline's FASTMATH build takes it: 64-channel workgroups, the split form
Params fm_params(const Params &P);
// the configuration of `columns` state columns side by side (time-parallel launches): no device ticks, no trace; fastmath:
// as fm_params takes it; force_pipe: the pipeline kernel whatever the column count
Params wide_params(const Params &P, uint32_t columns, bool fastmath, bool force_pipe);
inline bool is_fastmath(Family f) { return f == Family::kSym || f == Family::kPipeFastmath; }

}  // namespace same
