// field_kernels.h -- internal launch interface of libnbody_hip_field.so (include/nbody_hip_field.h) between its C-ABI unit
// (field_capi.hip) and its kernel unit (field.hip, contraction on), and the geometry both sides derive from (N, M, precision).
#pragma once

#include <hip/hip_runtime.h>

#include "wave_stream.h"

namespace nb {

inline constexpr unsigned kFieldMaxSources = 1u << 26;
inline constexpr unsigned kFieldMaxTargets = 1u << 24;
inline constexpr unsigned kFieldNone       = 0xFFFFFFFFu;
#ifndef NB_FIELD_TARGET
#define NB_FIELD_TARGET 512  // (a sweep builds with other values: make EXP=-DNB_FIELD_TARGET=...)
#endif
inline constexpr unsigned kFieldTarget  = NB_FIELD_TARGET;  // workgroups the evaluation aims at (hermite_block_kernels.h's, not measured for this kernel)
inline constexpr unsigned kFieldThreads = 256;              // block size of field_finish: one target per lane

// ---- geometry: a function of (N, M, precision) alone --------------------------------------------------------------------------------
struct FieldGeom {
    unsigned waves, chunks, tiles, ranges;  // S; ceil(N / 128); tiles of 64 W targets; J ranges of the chunks
};
inline unsigned  field_waves(unsigned n) { return stream_waves(n); }
inline FieldGeom field_geometry(unsigned n, unsigned m, unsigned per_tile) {
    const StreamGeom g = stream_geometry(n, m, per_tile, kFieldTarget);
    return FieldGeom{field_waves(n), stream_chunks(n), g.tiles, g.ranges};
}

// planes of a call that asks for the jerk / that does not: ax ay az (jx jy jz) sum of m / s
inline constexpr unsigned field_planes(bool jerk) { return jerk ? 7u : 4u; }

// ---- workspace: the partial planes [J][7][tiles * 64 W] of T, sized for a call with jerks; nothing when J = 1 ------------------------
struct FieldLayout {
    size_t partial, partial_bytes, bytes;
};
inline FieldLayout field_layout(unsigned n, unsigned m, size_t size_t_of) {
    const unsigned  per_tile = size_t_of == 4 ? 128 : 64;
    const FieldGeom g        = field_geometry(n, m, per_tile);
    FieldLayout     l;
    l.partial       = 0;
    l.partial_bytes = g.ranges > 1 ? static_cast<size_t>(g.ranges) * 7 * g.tiles * per_tile * size_t_of : 0;
    l.bytes         = (l.partial_bytes + 255) & ~static_cast<size_t>(255);
    return l;
}

template <typename T> struct FieldArgs {
    const T*        src;      // T[4N] {x, y, z, m}
    const T*        src_vel;  // T[4N] or null
    const T*        tgt;      // T[4M] {x, y, z, -}
    const T*        tgt_vel;  // T[4M] or null
    const unsigned* self;     // [M] or null
    T*              acc;      // outputs, each may be null: T[4M], T[4M], T[M]
    T*              jerk;
    T*              pot;
    T*              partial;  // workspace
    unsigned        n, m;
    T               eps2;  // > 0 (the C boundary replaces 0 by the floor of nbody_hip_hermite.h)
};

template <typename T> hipError_t launch_field_eval(const FieldArgs<T>& a, hipStream_t stream);

}  // namespace nb
