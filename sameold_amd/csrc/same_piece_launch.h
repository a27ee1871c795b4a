// same_piece_launch.h -- what the launchers of the kernels that take time-parallel launches (demod_pipe_kernel,
// demod_sym_kernel, demod_relaxed_kernel, demod_duo_kernel) ask of a launch's pieces, and the opt-in to a large LDS
// allocation they share.
//
// A time-parallel launch runs every channel as n_chunks state columns side by side (PipeChunks, same_device.h;
// DESIGN.md 4.5).  Two geometries:
//   * uniform (time-major input): piece k of every channel starts at block k * stride_blocks.  A group of lanes (a
//     workgroup, or the 64 columns of a wavefront) takes its piece as a whole, so it must not straddle two.
//   * per column (channel-major input, col_row0 != null): every column has its own first row, its own nominal length and
//     its own stream; the kernels have a build of their own for it.
// Host code only.  The device side -- which column, row and block count a lane takes and when it hands over -- is written
// out in each of the four kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <map>
#include <mutex>
#include <utility>

#include "same_device.h"

namespace same {

inline bool piece_per_column(const PipeChunks &K) { return K.n_chunks > 1u && K.col_row0 != nullptr; }
// a group of `width` lanes would straddle pieces
inline bool piece_straddles(const PipeChunks &K, uint32_t width) { return K.n_chunks > 1u && (K.in_channels % width) != 0u; }

// More than the default 64 KB of dynamic LDS per workgroup: opt in, once per kernel, device and size (the largest size set
// is remembered, so a kernel launched with a larger allocation later is raised again).  Launches come from any thread, each
// on its own batch.
inline hipError_t lds_opt_in(const void *kernel, size_t lds)
{
    if (lds <= 64u * 1024u) return hipSuccess;
    if (lds > (size_t)INT_MAX) return hipErrorInvalidValue;
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> opted_in;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(mu);
    size_t &set = opted_in[std::make_pair(kernel, dev)];
    if (set < lds) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        set = lds;
    }
    return hipSuccess;
}

}  // namespace same
