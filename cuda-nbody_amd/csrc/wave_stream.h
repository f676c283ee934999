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

}  // namespace nb
