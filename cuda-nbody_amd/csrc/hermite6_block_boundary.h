// hermite6_block_boundary.h -- what the extern "C" boundaries of the two 6th-order block-step libraries (hermite6_block_boundary.hip,
// hermite6_block_ensemble_boundary.hip) check on top of hermite_block_boundary.h: the "Range of h" of include/nbody_hip_hermite6_block.h.
// Host only.
#pragma once

#include "hermite_block_boundary.h"

namespace nb {

// the cube of a step, as the corrector forms it in T (hh = h * h, h3 = hh * h): c1 divides by it
template <typename T> bool cube_is_normal(double step) {
    const T h = static_cast<T>(step), hh = h * h, h3 = hh * h;
    return std::isnormal(h3);
}

// T: the corrector's precision.  The longest step (dt_max) and the shortest (one tick) must have normal cubes in T.
template <typename T> bool block6_params_ok(const nb_hermite_block_params_t* p) {
    return block_params_ok(p) && cube_is_normal<T>(std::ldexp(p->dt_max, -p->max_level)) && cube_is_normal<T>(p->dt_max);
}

}  // namespace nb
