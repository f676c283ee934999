// hermite6_block_body.h -- what one body of the 6th-order block scheme needs on the device, one text for hermite6_block.hip
// (nb_hermite6_block_*) and hermite6_block_ensemble.hip (nb_hermite6_block_ensemble_*): the predictor to the crackle and Aarseth's step
// from the derivatives the scheme holds.  Included inside each translation unit's own anonymous namespace, after nbody_lane.h (Lane) and
// hermite_block_kernels_shared.h (norm3).
#pragma once

// One body to dt: hermite6_predict's expressions (hermite6_predict.inc).  dt = 0 gives the stored bits.
template <typename T> struct Predicted6 {
    typename Lane<T>::vec4 x, v, a;  // {x_p, m}, {v_p, 0}, {a_p, 0}
};
template <typename T>
__device__ __forceinline__ Predicted6<T> predict6_body(const typename Lane<T>::vec4& x, const typename Lane<T>::vec4& v, const typename Lane<T>::vec4& a,
                                                       const typename Lane<T>::vec4& j, const typename Lane<T>::vec4& s, const typename Lane<T>::vec4& c, T dt) {
    using vec4 = typename Lane<T>::vec4;
#include "hermite6_predict.inc"
    return {xp, vp, ap};
}

// Aarseth's step with the derivatives the scheme holds, from the stored T-typed a1, j1, s1, c1, in fp64
// (include/nbody_hip_hermite6_block.h)
template <typename V> __device__ __forceinline__ double aarseth6_dt(const V& a1, const V& j1, const V& s1, const V& c1, double eta, double dt_max) {
    const double n_a = norm3(a1.x, a1.y, a1.z), n_j = norm3(j1.x, j1.y, j1.z), n_s = norm3(s1.x, s1.y, s1.z), n_c = norm3(c1.x, c1.y, c1.z);
    const double dt  = __builtin_sqrt(eta * (n_a * n_s + n_j * n_j) / (n_j * n_c + n_s * n_s));
    return (dt == dt && dt - dt == 0) ? dt : dt_max;
}
