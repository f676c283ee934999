// hermite_block_ensemble_kernels.h -- internal launch interface of libnbody_hip_hermite_block_ensemble.so
// (include/nbody_hip_hermite_block_ensemble.h) between its C-ABI unit (hermite_block_ensemble_capi.hip) and its kernel unit
// (hermite_block_ensemble.hip, contraction on), and the per-system workspace layout both sides derive from (N, precision).
//
// The geometry of ONE system is hermite_block_kernels.h's, untouched: S, the chunks, stream_geometry(N, n_act, 64 W, kBlockTarget) and the
// launch grid block_launch_groups(N, 64 W).  B only multiplies the grids.
#pragma once

#include <hip/hip_runtime.h>

#include "hermite_block_kernels.h"

namespace nb {

inline constexpr unsigned kBlockEnsembleMaxBodies = 65536;     // per system: 256 count blocks, which one workgroup of 256 scans
inline constexpr unsigned kBlockEnsembleMaxTotal  = 1u << 28;  // N * B

struct BlockEnsembleSummary {  // nb_hermite_block_ensemble_summary_t, 64 bytes
    unsigned long long min_now_ticks, max_now_ticks, block_steps, body_steps;
    unsigned           systems, stopped;
    int                deepest_level;
    unsigned           reserved[5];
};

// schedule workgroups (256 bodies each) of one system
inline unsigned block_ensemble_blocks(unsigned n) { return (n + kBlockThreads - 1) / kBlockThreads; }

// Workgroups' worth of partial planes a system's slice holds: the launch grid of N, or that of a smaller N where it is larger (the grid
// shrinks where S doubles, at 256, 512 and 1 024 bodies), so that the workspace never shrinks as N grows.
inline unsigned block_ensemble_plane_groups(unsigned n, unsigned per_tile) {
    unsigned groups = block_launch_groups(n, per_tile);
    for (const unsigned below : {255u, 511u, 1023u}) {
        if (below < n && block_launch_groups(below, per_tile) > groups) groups = block_launch_groups(below, per_tile);
    }
    return groups;
}

// ---- workspace of ONE system (byte offsets, each section on a 256-byte boundary); system s starts at s * stride ----------------------
// The first two sections sit where block_layout (hermite_block_kernels.h) has them, so that partial_offset of the plan is the solo plan's.
// One function for both orders, as block_layout: body_vec4 vec4 per predicted body (2; 3 with the acceleration) and `sums` partial planes.
struct BlockEnsembleLayout {
    size_t state, partial, active, counts, min_part, lvl_part, ctrl, stride;
};
inline BlockEnsembleLayout block_ensemble_layout(unsigned n, size_t size_t_of, unsigned body_vec4, unsigned sums) {
    const unsigned      per_tile = size_t_of == 4 ? 128 : 64;
    const auto          up       = [](size_t b) { return (b + 255) & ~static_cast<size_t>(255); };
    BlockEnsembleLayout l;
    size_t              at = 0;
    l.state = at, at += up(static_cast<size_t>(n) * 4 * body_vec4 * size_t_of);
    l.partial = at, at += up(static_cast<size_t>(block_ensemble_plane_groups(n, per_tile)) * sums * per_tile * size_t_of);
    l.active = at, at += up(static_cast<size_t>(n) * 4);
    l.counts = at, at += up(static_cast<size_t>(block_ensemble_blocks(n)) * 4);
    l.min_part = at, at += up(static_cast<size_t>(block_ensemble_blocks(n)) * 8);
    l.lvl_part = at, at += up(static_cast<size_t>(block_ensemble_blocks(n)) * 4);
    l.ctrl = at, at += up(sizeof(BlockCtrl));
    l.stride = at;
    return l;
}

template <typename T> struct BlockEnsembleArgs {
    T *                 pos, *vel, *acc, *jerk;  // stored state T[4 N B]
    unsigned long long* ticks;                   // [N B]
    int*                levels;                  // [N B]
    BlockStatus*        status;                  // [B]
    char*               workspace;               // B * layout.stride bytes
    BlockEnsembleLayout layout;
    const T*            system_eps2;  // T[B] or nullptr
    T                   eps2;         // (0 takes the floor of nbody_hip_hermite.h, per system, on the device)
    unsigned            n, b;
    unsigned            blocks;             // schedule workgroups per system
    unsigned            groups_per_system;  // evaluation workgroups per system: block_launch_groups(N, 64 W)
    BlockParams         p;
    double              t_stop;
};

template <typename T> hipError_t launch_block_ensemble_init(const BlockEnsembleArgs<T>& a, hipStream_t stream);  // after launch_ensemble_eval
template <typename T> hipError_t launch_block_ensemble_step(const BlockEnsembleArgs<T>& a, hipStream_t stream);
template <typename T>
hipError_t launch_block_ensemble_sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const unsigned long long* ticks, const BlockStatus* status,
                                      unsigned n, unsigned b, const BlockParams& p, hipStream_t stream);
hipError_t launch_block_ensemble_summary(const BlockStatus* status, unsigned b, BlockEnsembleSummary* out, hipStream_t stream);

}  // namespace nb
