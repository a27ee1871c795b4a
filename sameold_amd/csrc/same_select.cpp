// same_select.cpp -- which demodulation kernel runs a launch (same_select.h).  Host-only: no HIP.
#include "same_select.h"

#include <algorithm>
#include <cmath>

namespace same {

// ---------------------------------------------------------------------------------
// tests that every family shares
// ---------------------------------------------------------------------------------
uint32_t standard_rate_taps(const Params &P)
{
    if (P.ntaps == 42u && P.dc_len == 16u) return 42u;
    if (P.ntaps == 92u && P.dc_len == 35u) return 92u;
    if (P.ntaps == 84u && P.dc_len == 32u) return 84u;
    return 0u;
}
static bool eq_default(const Params &P) { return P.eq_nff == 6u && P.eq_nfb == 4u; }
bool eq_default_or_disabled(const Params &P) { return eq_default(P) || (P.eq_nff == 1u && P.eq_nfb == 1u); }
bool agc_clamp_is_med3(const Params &P)
{ return !(P.agc_min == 0.0f && std::signbit(P.agc_min)) && !(P.agc_max == 0.0f && std::signbit(P.agc_max)); }

size_t demod_lds_bytes(const Params &P)
{ return (size_t)(2 * P.dc_len + P.win_ring) * kWave * sizeof(float); }

// ---------------------------------------------------------------------------------
// the one-wavefront kernel
// ---------------------------------------------------------------------------------
// The mirrored window costs 16 KB of LDS per wavefront: 3 wavefronts fit a CU's 160 KB instead
// of 4, so it is used while the batch needs at most 3 wavefronts per CU (and only for the
// 42-tap filters, whose ring is 64 slots).
bool fast_use_mirror(const Params &P)
{
    if (max_block_len(P) < (uint32_t)kBlockMirror) return false;     // 18-sample blocks need the timing bound
    if (P.knob_mirror != 0) return P.knob_mirror > 0 && P.ntaps == 42u;
    return P.ntaps == 42u && (P.n_channels + kWave - 1) / kWave <= 3u * 256u;
}
// more wavefronts than one per SIMD (1 024): the dense build, two per SIMD (22.05 kHz; SAME_FAST_DENSE=0/1 overrides)
bool fast_use_dense(const Params &P)
{
    const uint32_t grid = (P.n_channels + kWave - 1) / kWave;
    return P.ntaps == 42u && !fast_use_mirror(P) && (P.knob_fast_dense != 0 ? P.knob_fast_dense > 0 : grid > 1024u);
}

bool fast_kernel_supported(const Params &P)
{
    if (P.block_len != (uint32_t)kBlock || P.win_ring > 128u) return false;
    if (!eq_default_or_disabled(P)) return false;
    if (P.ntaps >= 84u && max_block_len(P) < (uint32_t)kBlock48k) return false;   // their block is 32 samples
    return standard_rate_taps(P) != 0u;
}

uint32_t fast_win_ring(const Params &P) { return (P.ntaps + kBlock - 1 <= 64u) ? 64u : 128u; }

// samples per block of the variant launch_demod_fast will pick for this batch
uint32_t fast_block_len(const Params &P)
{
    if (pipe_kernel_selected(P)) return pipe_block_len(P);
    if (P.ntaps == 42u && fast_use_mirror(P)) return (uint32_t)kBlockMirror;
    return P.ntaps >= 84u ? (uint32_t)kBlock48k : (uint32_t)kBlock;
}

// ---------------------------------------------------------------------------------
// the wavefront pipeline
// ---------------------------------------------------------------------------------
// channels per workgroup: 16 while that still leaves the batch within one workgroup per CU
// (default equalizer only: fewer kernels to build), else 64
uint32_t pipe_workgroup_channels(const Params &P)
{
    if (!eq_default(P) || !agc_clamp_is_med3(P)) return kWave;
    if (P.knob_pipe_lanes == 16 || P.knob_pipe_lanes == 32 || P.knob_pipe_lanes == 64) return (uint32_t)P.knob_pipe_lanes;
    if (P.n_channels <= 16u * 256u && P.n_channels % 16u == 0u) return 16u;
    if (P.n_channels <= 32u * 256u && P.n_channels % 32u == 0u) return 32u;
    return kWave;
}

// The pipeline pays while SIMDs are idle.  Whole groups of 64 channels only.  Measured at
// 22.05 kHz: it wins up to 32 768 channels (two workgroups of four wavefronts per CU), the
// one-wavefront kernel from 49 152 on.  At 44.1 / 48 kHz a workgroup's window ring is 72 KB of
// the CU's 160 KB of LDS, so one workgroup per CU and 16 384 channels at a time; two rounds of
// them (32 768 channels: 13.1 ms for 2 s at 48 kHz) still beat one wavefront per 64 channels
// (16.0 ms), three do not.  Returns 0 (not selected) or non-zero.
uint32_t pipe_kernel_stages(const Params &P)
{
    const uint32_t nt = standard_rate_taps(P);
    const bool r22 = nt == 42u;
    if (nt == 0u || (P.n_channels % pipe_workgroup_channels(P)) != 0u) return 0;
    if (!eq_default_or_disabled(P)) return 0;
    if (P.block_len != 16u || max_block_len(P) < (r22 ? (uint32_t)kBlockMirror : pipe_block_len(P))) return 0;
    if (P.knob_pipe != 0) return P.knob_pipe > 0 ? 4u : 0u;
    // beyond two workgroups per CU the pipeline runs in rounds; 22.05 kHz, sustained 2 s launches with the transport layer on
    // (tools/big_sustained_strict.py): 65 536 channels 7.97 ms against the one-wavefront kernel's 9.06, 131 072: 15.6 against
    // 15.0, 262 144: 30.5 against 29.2
    return P.n_channels <= (r22 ? 65536u : 32768u) ? 4u : 0u;
}
bool pipe_kernel_selected(const Params &P) { return pipe_kernel_stages(P) != 0u; }
uint32_t pipe_block_len(const Params &P)
{ return P.ntaps == 42u ? (uint32_t)kBlockPipe22 : (P.ntaps == 92u ? (uint32_t)kBlockPipe48 : (uint32_t)kBlockPipe44); }

// two workgroups per CU (22.05 kHz only, where their LDS allows it): the register-capped build, with
// stage 2 split (same box, 32 768 channels x 2 s: 4.27-4.29 ms unsplit, 4.18-4.24 ms split).  Which stages
// of the two workgroups meet on a SIMD makes no measurable difference there (dealt by SIMD id: like + like
// 4.14 ms, stage 1 + 2 and 3 + 4 4.19 ms, 1 + 4 and 2 + 3 4.20 ms, by wavefront number 4.20 ms, one box),
// so they are left where they fall.
bool pipe_share(const Params &P)
{ return P.ntaps == 42u && (P.knob_pipe_share != 0 ? P.knob_pipe_share > 0 : P.n_channels > 16384u); }
// one workgroup per CU: stage 2 split with stage 4's wavefront wherever stage 2 is (one of) the longest -- everywhere
// except 64-channel workgroups at 22.05 kHz, whose symbol stage is longer still (the default configuration only: the other
// equalizer and clamp forms are built unsplit there)
bool pipe_split(const Params &P, bool share)
{
    if (!share && !(eq_default(P) && agc_clamp_is_med3(P))) return false;
    if (P.knob_pipe_split != 0) return P.knob_pipe_split > 0;
    return share || P.ntaps != 42u || pipe_workgroup_channels(P) != (uint32_t)kWave;
}

// The FASTMATH build exists for the three rates the pipeline is built for, in 64-channel workgroups (whole groups of 64
// state columns), default or disabled equalizer, a non-negative AGC floor
bool pipe_relaxed_supported(const Params &P)
{
    return standard_rate_taps(P) != 0u && (P.n_channels % kWave) == 0u && P.agc_min >= 0.0f && pipe_kernel_stages(P) != 0u &&
           pipe_workgroup_channels(P) == (uint32_t)kWave && eq_default_or_disabled(P);
}

// ---------------------------------------------------------------------------------
// the symbol-paced pipeline
// ---------------------------------------------------------------------------------
// 22.05 / 44.1 / 48 kHz with the reference's default DC-blocker length, the default or the disabled equalizer, a non-negative AGC
// floor, whole groups of 64 state columns, and a timing loop whose shortest symbol is longer than a step (two instants at
// least max_block_len + 1 samples apart each: 19 / 40 / 44) and whose filters stay inside the four finished blocks of the ring
uint32_t sym_block_len(const Params &P) { return standard_rate_taps(P) == 42u ? (uint32_t)kSymStep22 : (uint32_t)kSymStepHi; }
bool sym_kernel_supported(const Params &P)
{
    if (P.knob_sym < 0) return false;
    const uint32_t nt = standard_rate_taps(P);
    if (nt == 0u || P.win_ring < 64u || P.win_ring < nt || (P.n_channels % kWave) != 0u) return false;
    if (P.n_channels >= (1u << 22)) return false;                    // (the squelch history's 24-bit row pitch, SymSquelch::hptr)
    if (!eq_default_or_disabled(P)) return false;
    if (!(P.agc_min >= 0.0f)) return false;
    const uint32_t B = sym_block_len(P), apart = max_block_len(P) + 1u;
    if (!(2u * apart > B)) return false;                             // at most one symbol per lane and step
    // How far back a filter reaches from the end of the finished samples: a lane completes its symbol up to B behind it, one more
    // B - apart after a symsync.reset() (the next instant completes a symbol by itself), the symbol's first instant lies up to
    // period_max + alpha + 0.5 (+ rounding) before its second, and the filter takes ntaps - 1 samples before that.
    const float a = P.alpha_unlocked > P.alpha_locked ? P.alpha_unlocked : P.alpha_locked;
    const uint32_t reach = (2u * B - apart) + 1u + (uint32_t)std::ceil(P.period_max + a + 1.5f) + (nt - 1u);
    return reach <= (uint32_t)(kSymRingSteps - 2) * B;
}

// ---------------------------------------------------------------------------------
// the one- / two-wavefront relaxed kernel
// ---------------------------------------------------------------------------------
// The relaxed kernel exists for 22.05 kHz with the reference's default DC-blocker length, the default or the disabled
// equalizer, a non-negative AGC floor (|x * gain| = |x| * gain) and a timing loop that cannot put three instants
// into one sub-block.
bool relaxed_kernel_supported(const Params &P)
{
    if (!(standard_rate_taps(P) == 42u && P.win_ring >= 64u)) return false;
    if (!eq_default_or_disabled(P)) return false;
    if (!(P.agc_min >= 0.0f)) return false;
    return max_block_len(P) >= (uint32_t)kBlockMirror;
}
// (Since round 4 these kernels take relaxed batches that are not whole groups of 64 channels, time-parallel calls beyond
// 16 384 channels and what SAME_RELAXED_KERNEL sends them; everything else runs the symbol-paced pipeline, which is faster
// at every channel count under sustained launches: select_plain.)
// Which form runs a launch over P.n_channels state columns: 1 duo (two wavefronts per 64 columns) while that leaves the
// launch at no more than two wavefronts per SIMD (65 536 columns), 0 solo beyond -- or what SAME_RELAXED_KERNEL asks for.  Whole groups
// of 64 columns for duo.  (A third form -- sample phase | filters + timing loop | symbol path on three wavefronts, 18-sample
// sub-blocks, the symbol stage on every step or on every other -- was built and measured in round 3: 3.9-4.1 ms where the
// pipeline's FASTMATH build takes 3.8; not kept.)
uint32_t relaxed_kernel_kind(const Params &P)
{
    const bool whole = (P.n_channels % kWave) == 0u;
    if (P.knob_relaxed_kernel == 1 || !whole) return 0u;
    if (P.knob_relaxed_kernel == 2) return 1u;
    return P.n_channels <= 65536u ? 1u : 0u;      // (measured, 2 s launches: 65 536 columns duo 6.5 against solo 7.0 ms; 81 920: 11.8 against 9.0; 98 304: 12.1 against 9.8)
}
uint32_t relaxed_block_len(const Params &P) { (void)P; return (uint32_t)kBlockRelaxed; }
// more wavefronts than SIMDs: the build for two per SIMD; otherwise a wavefront has its SIMD's registers to itself
bool relaxed_solo_wide(const Params &P) { return (P.n_channels + kWave - 1) / kWave <= 1024u && P.ticks == 0u; }

// ---------------------------------------------------------------------------------
// the decisions
// ---------------------------------------------------------------------------------
const char *family_name(Family f, uint32_t generic_block_len)
{
    switch (f) {
    case Family::kFast: return "demod_fast_kernel";
    case Family::kPipe: return "demod_pipe_kernel";
    case Family::kPipeFastmath: return "demod_pipe_kernel<fastmath>";
    case Family::kSym: return "demod_sym_kernel";
    case Family::kWaveRelaxed: return "demod_relaxed_kernel";
    case Family::kGeneric: break;
    }
    switch (generic_block_len) {
    case 16: return "demod_kernel<B=16>";
    case 8: return "demod_kernel<B=8>";
    case 4: return "demod_kernel<B=4>";
    case 2: return "demod_kernel<B=2>";
    default: return "demod_kernel<B=1>";
    }
}

Params fm_params(const Params &P)
{
    Params Pfm = P;
    Pfm.knob_pipe_lanes = 64; Pfm.knob_pipe_share = 1; Pfm.knob_pipe_split = 1; Pfm.knob_pipe = 1;
    return Pfm;
}
Params wide_params(const Params &P, uint32_t columns, bool fastmath, bool force_pipe)
{
    Params Pv = fastmath ? fm_params(P) : P;
    Pv.n_channels = columns; Pv.ticks = 0; Pv.trace_cap = 0;
    if (force_pipe) Pv.knob_pipe = 1;
    return Pv;
}

// The relaxed-arithmetic pipeline of a launch over Pv.n_channels state columns: the symbol-paced one (36-sample steps,
// same_kernels_sym.hip; 72-sample steps at 44.1 / 48 kHz) where it is built, else the FASTMATH build of the strict pipeline
static Choice fm_choice(const Params &Pv)
{
    if (sym_kernel_supported(Pv)) return Choice{Family::kSym, sym_block_len(Pv)};
    return Choice{Family::kPipeFastmath, pipe_block_len(Pv)};
}

Mode select_mode(const Params &P, const Request &rq)
{
    Mode m;
    m.block_kernels = fast_kernel_supported(P) && !rq.generic;
    // Relaxed arithmetic: asked for (SAME_BATCH_RELAXED), or implied by the time-parallel mode, whose contract is the
    // same one (SAME_RELAXED=0 keeps that mode on the strict pipeline kernel; =1 turns it on for any batch)
    m.relaxed = (((rq.relaxed || rq.time_parallel) && rq.knob_relaxed >= 0) || rq.knob_relaxed > 0) && m.block_kernels &&
                (relaxed_kernel_supported(P) || (P.n_channels % kWave == 0u && pipe_relaxed_supported(fm_params(P))));
    // (a call of a time-parallel batch that is too short to be cut stays strict unless relaxed arithmetic was asked for)
    // (... nor a batch of more than 16 384 channels, which is never cut: tp_rule)
    m.relaxed_plain = m.relaxed && (rq.relaxed || rq.knob_relaxed > 0 ||
                                    (rq.time_parallel && P.n_channels > 16384u && P.n_channels % kWave == 0u &&
                                     sym_kernel_supported(fm_params(P))));
    return m;
}

Family strict_family(const Params &P, const Mode &m)
{
    if (!m.block_kernels) return Family::kGeneric;
    return pipe_kernel_selected(P) ? Family::kPipe : Family::kFast;
}

// whole blocks (16 or 18 samples) go to the latency-optimised kernel when the
// configuration has one; the generic kernel takes the remainder (and every other
// configuration)
// SAME_BATCH_RELAXED on an ordinary launch of whole 64-channel groups: the symbol-paced pipeline at 22.05, 44.1 and 48 kHz
// (any number of channels; SAME_SYM=0 puts the pipeline's FASTMATH build in its place -- round 5's relaxed kernel at 44.1 /
// 48 kHz, up to 32 768 channels); the one- / two-wavefront relaxed kernel takes batches that are not whole groups of 64 and
// whatever SAME_RELAXED_KERNEL=solo / duo sends it
Choice select_plain(const Params &P, const Mode &m, const Request &rq)
{
    if (!m.block_kernels) return Choice{};
    const Params Pfm = fm_params(P);
    // (the symbol-paced pipeline takes any number of 64-channel workgroups: beyond two per CU they run in rounds -- and
    // it is the faster kernel at every channel count)
    // (at 44.1 / 48 kHz a CU holds one group of 64 columns: beyond 16 384 columns the workgroups run in rounds -- round 4 sent
    // such batches to the strict kernels whatever the flag said)
    const bool plain_fm = m.relaxed_plain && P.knob_relaxed_kernel == 0 && pipe_relaxed_supported(Pfm) &&
                          (P.n_channels <= 32768u || (P.n_channels <= rq.sym_max_channels && sym_kernel_supported(Pfm)) ||
                           !relaxed_kernel_supported(P));
    // (measured, 2 s launches back to back with the transport layer on, the way a stream is fed: 49 152 channels 4.26 ms;
    // 98 304: 7.2 ms against the one-wavefront relaxed kernel's 12.3; 131 072: 9.45 against 15.35; 196 608: 13.95 against
    // 24.9; 262 144: 19.5 against 29.3 -- 30 % of HBM against 18-20 %.  Round 3's figures for the one-wavefront kernel, up to
    // 26 %, were single launches on an idle machine with the link layer only; sustained, its eight wavefronts per SIMD fall
    // back launch by launch: tools/big_sustained.py.  SAME_RELAXED_KERNEL=solo / duo still selects it.)
    if (plain_fm) return fm_choice(Pfm);
    if (m.relaxed_plain && relaxed_kernel_supported(P)) return Choice{Family::kWaveRelaxed, relaxed_block_len(P)};
    return Choice{strict_family(P, m), fast_block_len(P)};
}

TpRule tp_rule(const Params &P, const Mode &m, const Request &rq, uint32_t max_chunks, uint32_t column_cap, bool channel_major)
{
    TpRule r;
    if (!rq.time_parallel || !m.block_kernels) return r;
    const uint32_t C = P.n_channels;
    const bool whole = C % kWave == 0u;
    // Relaxed batches: the pipeline's FASTMATH build while the state columns fit the pipeline (whole 64-channel
    // workgroups), the one-wavefront relaxed kernel beyond (SAME_TP_KERNEL=pipe / wave overrides)
    r.fastmath = m.relaxed && rq.knob_tp_kernel != 2 && whole && C <= 16384u;
    // A batch that fills the machine by itself (more than 16 384 channels, i.e. more than one workgroup per CU before any
    // cut) gains nothing from a cut in time -- its ordinary relaxed launches run the symbol-paced pipeline at ~30 % of HBM,
    // 262 144 state columns on the one-wavefront kernel ran at 13 % (round 3's `scaled_long`): such time-major calls are not
    // cut, and select_mode has made them relaxed launches (32 768 ch x 10 s: 21 ms per call against 31.6; SAME_TP_KERNEL=wave
    // still cuts them).  A channel-major call keeps the cut: read where it lies by the one-wavefront kernel it is 31.6 ms,
    // transposed slab by slab first 38.6.
    if (m.relaxed && !r.fastmath && !channel_major && rq.knob_tp_kernel == 0 && whole && sym_kernel_supported(fm_params(P))) return r;
    if (m.relaxed && !r.fastmath && rq.knob_tp_kernel != 1 && whole && C <= 65536u && relaxed_kernel_supported(P)) {
        // one wavefront per 64 state columns, any number of them
        // (up to 262 144 state columns, 16 pieces per channel unless the caller asks for more: a piece is a burst with its
        // margins at least, so more only sit empty)
        const uint32_t k_cap = std::min(63u, 262144u / C);
        r.wave = true;
        r.k_max = max_chunks ? std::min(max_chunks, k_cap) : std::min(k_cap, 16u);
        return r;
    }
    if (C % 16u != 0u || C > 16384u) return r;
    // state columns the pipeline takes at full speed: 32 768 at 22.05 kHz (two workgroups per CU), 16 384 at
    // 44.1 / 48 kHz (their window ring leaves room for one)
    // (column_cap 65 536: the channel-major path, whose workgroups are composed of pieces of similar length and may come
    // in two rounds)
    const uint32_t k_cap = (P.ntaps == 42u ? column_cap : 16384u) / C;
    r.force_pipe = tp_more_than_one_round(column_cap);      // (beyond 32 768: the pipeline kernel whatever the column count)
    r.k_max = max_chunks ? std::min(max_chunks, k_cap) : k_cap;
    return r;
}

bool tp_candidate(const Params &P, const TpRule &r, uint32_t K, Choice &c)
{
    const uint32_t C = P.n_channels;
    if (r.wave) {
        Params Pk = P;
        Pk.n_channels = K * C;                           // (the block length follows the form the column count selects)
        c = Choice{Family::kWaveRelaxed, relaxed_block_len(Pk)};
        return true;
    }
    const Params Pv = wide_params(P, K * C, r.fastmath, r.force_pipe);
    if (!pipe_kernel_selected(Pv) || C % pipe_workgroup_channels(Pv) != 0u) return false;
    if (r.fastmath && !pipe_relaxed_supported(Pv)) return false;
    c = r.fastmath ? fm_choice(Pv) : Choice{Family::kPipe, pipe_block_len(Pv)};
    return true;
}

// A quarter more state columns than the machine holds at once (40 960: 10 pieces per channel at 4 096 channels) unless
// the caller asks for a number of chunks: the launch is as long as its longest piece, a burst with its margins however
// many pieces there are, but with 8 pieces the planner cannot give every long burst a piece of its own (longest piece
// 39.9 k samples, with 10 or more 37.5 k), and beyond 10 the extra workgroups only add rounds.  Measured at 4 096
// channels x 10 s, pieces sorted by length into workgroups: 8 pieces 3.84 ms (unsorted 3.83), 9 3.47, 10 3.45, 11 3.70,
// 12 3.85, 16 4.2.
// With the symbol-paced pipeline (round 4): exactly the columns the machine holds at once (32 768: 8 pieces per channel at
// 4 096 channels, one round of workgroups in grid order).  Single launches on an idle machine favour 12 pieces (8: 2.16 ms,
// 10: 2.14, 12: 2.03, 16: 2.21 -- the long pieces finish with a CU to themselves), but calls back to back, the way a stream
// is fed, do not: 40 steps with 8 pieces 2.20 ms per step (kernel 2.05-2.08, launch to launch +-3 %), with 10: 2.38-2.42,
// 12: 2.41-2.48 (kernel 2.26-2.35, launch to launch 2.06-3.1), 16: 2.46 (tools/headline_steady.py).
uint32_t tp_native_column_cap(const Params &P, const Mode &m, uint32_t max_chunks)
{
    const bool sym_cols = m.relaxed && sym_kernel_supported(P);
    const uint32_t dflt_cols = sym_cols ? kTpColumnCap : 40960u;
    if (!max_chunks) return dflt_cols;
    return tp_more_than_one_round(max_chunks * P.n_channels) ? 65536u : kTpColumnCap;
}
bool tp_more_than_one_round(uint32_t columns) { return columns > kTpColumnCap; }

}  // namespace same
