// wave_stream.h -- what the kernels on the wave-stream plan (hermite_eval, hermite_block_eval, field_eval) and their C-ABI units share
// at namespace scope, host and device: the chunk of bodies j, the unroll, and the geometry every one of them derives from N.
//
// The plan: a lane holds one vector of bodies i, the bodies j are wave-uniform and arrive through scalar loads U at a time, one group
// ahead; the S waves of a workgroup split chunks of kChunk bodies j (chunk c -> wave c mod S) and fold their sums through LDS in wave
// order.  The kernel-body text of the plan is in fragments included inside the kernels: wave_mates.inc (SIMD-mate priority),
// wave_fold.inc (the fold), hermite_stream.inc (the acceleration + jerk interaction and its chunk loop), range_sum.inc (the J ranges'
// partial planes).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

namespace nb {

inline constexpr unsigned kChunk      = 128;  // bodies j per wave and chunk
inline constexpr int      kFlushEvery = 8;    // chunks a register sum may collect
template <typename T> constexpr int unroll_for() { return sizeof(T) == 8 ? 2 : 4; }  // U: a body j is 8 (fp32) / 16 (fp64) scalar registers

// S, the waves that split j: the largest power of two up to 8 that still gives every wave a whole chunk
__host__ __device__ inline unsigned stream_waves(unsigned n) {
    unsigned s = 1;
    while (s < 8 && 2 * s * kChunk <= n) s *= 2;
    return s;
}
__host__ __device__ inline unsigned stream_chunks(unsigned n) { return (n + kChunk - 1) / kChunk; }
// the most ranges the chunks can be cut into: the largest power of two <= chunks / S, so that every wave of every range has a chunk
__host__ __device__ inline unsigned stream_range_cap(unsigned n) {
    const unsigned most = stream_chunks(n) / stream_waves(n);
    unsigned       cap  = 1;
    while (2 * cap <= most) cap *= 2;
    return cap;
}
// The division of `count` bodies i against N bodies j among workgroups: tiles of per_tile bodies i, times J contiguous ranges of the chunks
// of bodies j.  J is the smallest power of two with tiles * J >= target, capped.  (hermite_block_eval and hermite_block_finish run this
// themselves, and call it by this name: through one more function, however it is inlined, or with J in a function of its own, their
// listings change.)
struct StreamGeom {
    unsigned tiles, ranges;
};
__host__ __device__ inline StreamGeom stream_geometry(unsigned n, unsigned count, unsigned per_tile, unsigned target) {
    StreamGeom g;
    g.tiles             = (count + per_tile - 1) / per_tile;
    const unsigned need = (target + g.tiles - 1) / (g.tiles ? g.tiles : 1), cap = stream_range_cap(n);
    g.ranges            = 1;
    while (g.ranges < need && g.ranges < cap) g.ranges *= 2;
    return g;
}

// Bodies i per lane, one vector of them: fp32 a packed pair, fp64 one body (Lane<T>::W of nbody_lane.h, which lives inside the units' own
// namespaces; the evaluation units hold the two against each other).
template <typename T> constexpr int stream_lane_bodies() { return sizeof(T) == 8 ? 1 : 2; }

// The geometry of an evaluation of every body i of a system against every body j (hermite_eval, hermite6_eval and their ensembles), a
// function of (N, precision) alone.  One vector of bodies i per lane (I = W: 12 state vectors, 6 second-level sums and two chains of 9
// temporaries compile to 103 - 118 VGPRs; a second vector does not fit under 128), so a workgroup owns 64 W bodies i.  S = stream_waves(N):
// from 65 536 bodies (fp32; 32 768 fp64) the grid alone puts 16 waves on every CU of the MI355X.  The fold's LDS holds `sums` sums (6; 9
// with the snap) per body i and folded wave.  An ensemble launches `groups` workgroups per system.
struct StreamPlan {
    int      bodies_per_lane;  // I = W
    int      waves;            // S
    int      unroll;           // U bodies j per scalar load group
    unsigned groups;           // workgroups
    unsigned block_threads;
    unsigned lds_bytes;
};
template <typename T> inline StreamPlan plan_stream(unsigned n, int sums, int unroll) {
    constexpr int W = stream_lane_bodies<T>();
    const int     S = static_cast<int>(stream_waves(n));
    StreamPlan    p;
    p.bodies_per_lane = W;
    p.waves           = S;
    p.unroll          = unroll;
    p.groups          = (n + 64u * W - 1) / (64u * W);
    p.block_threads   = 64u * S;
    p.lds_bytes       = static_cast<unsigned>((S > 1 ? S - 1 : 1) * sums * W * 64 * sizeof(T));
    return p;
}
// ... into the fields that nb_hermite_plan_t, nb_hermite6_plan_t and nb_hermite_ensemble_plan_t share
template <typename Out> void fill(Out* out, const StreamPlan& p) {
    out->bodies_per_lane = p.bodies_per_lane;
    out->waves_per_group = p.waves;
    out->unroll          = p.unroll;
    out->groups          = p.groups;
    out->block_threads   = p.block_threads;
    out->lds_bytes       = p.lds_bytes;
}

// The launch of a kernel compiled for S = 1, 2, 4 and 8 waves: `launch` is called with S as a std::integral_constant.
template <typename Launch> hipError_t with_stream_waves(unsigned waves, Launch&& launch) {
    switch (waves) {
        case 1: return launch(std::integral_constant<int, 1>{});
        case 2: return launch(std::integral_constant<int, 2>{});
        case 4: return launch(std::integral_constant<int, 4>{});
        case 8: return launch(std::integral_constant<int, 8>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace nb
