// hermite_ratio.h -- |a|^2 / |jerk|^2 of one body, the quantity behind the shared time step of nb_hermite_timestep_* (hermite_eval.hip)
// and the per-system time steps of nb_hermite_ensemble_* (hermite_ensemble.hip).  Included inside each translation unit's own anonymous
// namespace, after nbody_lane.h.
#pragma once

// |a|^2 / |jerk|^2 of one body as a double good to ~1 ulp.  fp32 inputs: plain double arithmetic is exact enough.  fp64 inputs: the
// two sums of squares as unevaluated pairs (products split by FMA, sums by TwoSum), then one correction step on the quotient.
__device__ __forceinline__ void two_sum(double x, double y, double& s, double& e) {
    s              = x + y;
    const double b = s - x;
    e              = (x - (s - b)) + (y - b);
}
__device__ __forceinline__ void norm2_pair(double x, double y, double z, double& hi, double& lo) {
    const double px = x * x, py = y * y, pz = z * z;
    const double ex = __builtin_fma(x, x, -px), ey = __builtin_fma(y, y, -py), ez = __builtin_fma(z, z, -pz);
    double       s, e1, e2;
    two_sum(px, py, s, e1);
    two_sum(s, pz, hi, e2);
    lo = ((ex + ey) + ez) + (e1 + e2);
}
template <typename T> __device__ __forceinline__ double ratio_sq(const typename Lane<T>::vec4& a, const typename Lane<T>::vec4& j) {
    double q;
    if constexpr (sizeof(T) == 4) {
        const double ax = a.x, ay = a.y, az = a.z, jx = j.x, jy = j.y, jz = j.z;
        const double a2 = ax * ax + ay * ay + az * az, j2 = jx * jx + jy * jy + jz * jz;
        if (!(j2 > 0)) return __builtin_inf();
        q = a2 / j2;
    } else {
        double ah, al, jh, jl;
        norm2_pair(a.x, a.y, a.z, ah, al);
        norm2_pair(j.x, j.y, j.z, jh, jl);
        if (!(jh > 0)) return __builtin_inf();
        q              = ah / jh;
        const double r = __builtin_fma(-q, jh, ah) + (al - q * jl);
        const double c = q + r / jh;
        if (c == c && c - c == 0) q = c;
    }
    return (q == q && q - q == 0) ? q : __builtin_inf();  // (non-finite ratios are left out)
}
