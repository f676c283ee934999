// hermite_stream.h -- what the acceleration + jerk kernels (hermite_eval.hip, hermite_block.hip) and field.hip share at namespace scope
// beside wave_stream.h (the chunk, the unroll, the geometry: every *_kernels.h of the three includes it): s^-2 and s^-3 from s^2
// (hermite_powers.h, which hermite6_eval.hip takes alone: its body j has three vec4), a body j as the scalar unit loads it.  Included
// inside each translation unit's own anonymous namespace, after nbody_lane.h (device code, internal linkage).  The kernel-body text the
// Hermite kernels share is hermite_stream.inc.
#pragma once

#include "hermite_powers.h"

template <typename T> struct BodyJ {
    typename Lane<T>::raw4 p, v;  // {x, y, z, m}, {vx, vy, vz, -} in scalar registers
};
