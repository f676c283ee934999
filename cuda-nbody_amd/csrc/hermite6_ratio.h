// hermite6_ratio.h -- (|a||s| + |j|^2) / (|j||c| + |s|^2) of one body, the quantity behind the shared time step of nb_hermite6_timestep_*
// (hermite6_eval.hip) and the per-system time steps of nb_hermite6_ensemble_* (hermite6_ensemble.hip).  Included inside each translation
// unit's own anonymous namespace, after nbody_lane.h.
#pragma once

// (|a||s| + |j|^2) / (|j||c| + |s|^2) of one body, in fp64 for either precision; +inf where the denominator is not positive or the
// ratio not finite
template <typename T> __device__ __forceinline__ double aarseth_ratio(const typename Lane<T>::vec4& a, const typename Lane<T>::vec4& j, const typename Lane<T>::vec4& s,
                                                                    const typename Lane<T>::vec4& c) {
    const auto norm2 = [](const typename Lane<T>::vec4& q) {
        const double x = q.x, y = q.y, z = q.z;
        return x * x + y * y + z * z;
    };
    const double a2 = norm2(a), j2 = norm2(j), s2 = norm2(s), c2 = norm2(c);
    const double num = __builtin_sqrt(a2 * s2) + j2, den = __builtin_sqrt(j2 * c2) + s2;
    if (!(den > 0)) return __builtin_inf();
    const double q = num / den;
    return (q == q && q - q == 0) ? q : __builtin_inf();
}
