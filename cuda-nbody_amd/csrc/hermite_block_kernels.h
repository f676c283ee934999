// hermite_block_kernels.h -- internal launch interface of libnbody_hip_hermite_block.so (include/nbody_hip_hermite_block.h) between its
// C-ABI unit (hermite_block_capi.hip) and its kernel unit (hermite_block.hip, contraction on), and the geometry both sides (and the
// kernels themselves) derive from (N, n_act, precision).
#pragma once

#include <hip/hip_runtime.h>

#include "wave_stream.h"

namespace nb {

// Body indices are `unsigned`, element offsets 64-bit.  The fixed-order scan of the per-block active counts is ONE workgroup of 1 024
// lanes, each folding N / 2^18 counts serially: 64 at 2^24 bodies, where the library stops.
inline constexpr unsigned kBlockMaxBodies  = 1u << 24;
inline constexpr int      kBlockMaxLevel   = 40;
#ifndef NB_BLOCK_TARGET
#define NB_BLOCK_TARGET 512  // (tools/hermite_block_bench.py measures builds with other values: make EXP=-DNB_BLOCK_TARGET=...)
#endif
inline constexpr unsigned kBlockTarget     = NB_BLOCK_TARGET;  // workgroups the evaluation aims at: two 8-wave workgroups per CU of 256
inline constexpr unsigned kBlockMinPartials = 1024; // partial minima of the schedule's first stage
inline constexpr unsigned kBlockThreads    = 256;   // block size of the schedule kernels: one body per lane
inline constexpr unsigned kBlockStopped    = 1u;    // status flag (NB_HERMITE_BLOCK_STOPPED)

struct BlockParams {  // nb_hermite_block_params_t
    double eta, eta_start, dt_max;
    int    max_level, reserved;
};
struct BlockStatus {  // nb_hermite_block_status_t, 64 bytes
    unsigned long long now_ticks, block_steps, body_steps;
    unsigned           last_active;
    int                deepest_level;
    unsigned           flags;
    unsigned           reserved[7];
};
struct BlockCtrl {  // what one block step passes from launch to launch (workspace)
    unsigned long long now;
    unsigned           go, n_act;
    unsigned           reserved[12];
};

// ---- geometry: a function of (N, n_act, precision) alone --------------------------------------------------------------------------
using BlockGeom = StreamGeom;  // tiles of 64 W active bodies; J ranges of chunks of bodies j
__host__ __device__ inline unsigned block_waves(unsigned n) { return stream_waves(n); }
__host__ __device__ inline unsigned block_chunks(unsigned n) { return stream_chunks(n); }
__host__ __device__ inline unsigned block_range_cap(unsigned n) { return stream_range_cap(n); }
// stream_geometry with this library's target, for the host; hermite_block_eval and hermite_block_finish call stream_geometry by its own
// name (wave_stream.h says why)
inline BlockGeom block_geometry(unsigned n, unsigned n_act, unsigned per_tile) { return stream_geometry(n, n_act, per_tile, kBlockTarget); }
// the launch grid: an upper bound of tiles * J over every n_act <= N (J > 1 means tiles * J / 2 < target)
__host__ __device__ inline unsigned block_launch_groups(unsigned n, unsigned per_tile) {
    const unsigned           tiles_max = (n + per_tile - 1) / per_tile;
    const unsigned long long by_cap = static_cast<unsigned long long>(tiles_max) * block_range_cap(n);
    const unsigned           by_target = tiles_max > 2 * kBlockTarget - 1 ? tiles_max : 2 * kBlockTarget - 1;
    return by_cap < by_target ? static_cast<unsigned>(by_cap) : by_target;
}

// ---- workspace layout (byte offsets, each section on a 256-byte boundary) ------------------------------------------------------------
// One function for both orders: the predicted state has body_vec4 vec4 per body (2; 3 with the acceleration) and there are `sums`
// partial planes (6; 9 with the snap).
inline constexpr unsigned kBlockSums = 6;  // ax ay az jx jy jz
struct BlockLayout {
    size_t state, partial, active, counts, min_part, lvl_part, ctrl, bytes;
};
inline BlockLayout block_layout(unsigned n, size_t size_t_of, unsigned body_vec4, unsigned sums) {
    const unsigned per_tile = size_t_of == 4 ? 128 : 64;
    const auto     up       = [](size_t b) { return (b + 255) & ~static_cast<size_t>(255); };
    BlockLayout    l;
    size_t         at = 0;
    l.state = at, at += up(static_cast<size_t>(n) * 4 * body_vec4 * size_t_of);
    l.partial = at, at += up(static_cast<size_t>(block_launch_groups(n, per_tile)) * sums * per_tile * size_t_of);
    l.active = at, at += up(static_cast<size_t>(n) * 4);
    l.counts = at, at += up(static_cast<size_t>((n + kBlockThreads - 1) / kBlockThreads) * 4);
    l.min_part = at, at += up(kBlockMinPartials * 8);
    l.lvl_part = at, at += up(kBlockMinPartials * 4);
    l.ctrl = at, at += up(sizeof(BlockCtrl));
    l.bytes = at;
    return l;
}

template <typename T> struct BlockArgs {
    T *                 pos, *vel, *acc, *jerk;  // stored state T[4N]
    unsigned long long* ticks;                   // [N]
    int*                levels;                  // [N]
    BlockStatus*        status;
    T*                  state8;                  // workspace sections
    T*                  partial;
    unsigned*           active;
    unsigned*           counts;
    unsigned long long* min_part;
    int*                lvl_part;
    BlockCtrl*          ctrl;
    unsigned            n;
    T                   eps2;  // > 0 (the C boundary replaces 0 by the floor of nbody_hip_hermite.h)
    BlockParams         p;
    double              t_stop;
};

template <typename T> hipError_t launch_block_init(const BlockArgs<T>& a, hipStream_t stream);  // after launch_hermite_eval
template <typename T> hipError_t launch_block_step(const BlockArgs<T>& a, hipStream_t stream);
template <typename T>
hipError_t launch_block_sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const unsigned long long* ticks, const BlockStatus* status, unsigned n,
                             const BlockParams& p, hipStream_t stream);

}  // namespace nb
