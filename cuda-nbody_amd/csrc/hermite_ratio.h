// hermite_ratio.h -- |a| / |jerk| of one body, the quantity behind the shared time step of nb_hermite_timestep_* (hermite_eval.hip)
// and the per-system time steps of nb_hermite_ensemble_* (hermite_ensemble.hip).  Included inside each translation unit's own anonymous
// namespace, after nbody_lane.h.
#pragma once

// |a| / |jerk| of one body as a double good to ~1 ulp; +inf where the body is left out (|jerk| = 0, a NaN, a ratio beyond DBL_MAX).
// fp32 inputs: plain double arithmetic is exact enough and cannot leave double's range.  fp64 inputs: a and jerk are each scaled by
// the power of two that brings their largest component into [1/2, 1) -- exact, and it keeps the squares inside double's range for
// every finite input (in plain double |jerk|^2 underflowed from 2^-538, |a|^2 overflowed from 2^512: tests/test_hermite_domain.py) --
// then the two sums of squares as unevaluated pairs (products split by FMA, sums by TwoSum), one correction step on the quotient,
// its root, and the two powers of two back.  Scaling by a power of two commutes with every rounding on the way, so the bits are
// those of sqrt(|a|^2 / |jerk|^2) wherever that expression stayed in range; and the minimum of the roots is the root of the minimum.
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
template <typename T> __device__ __forceinline__ double norm_ratio(const typename Lane<T>::vec4& a, const typename Lane<T>::vec4& j) {
    double q;
    int    shift = 0;
    if constexpr (sizeof(T) == 4) {
        const double ax = a.x, ay = a.y, az = a.z, jx = j.x, jy = j.y, jz = j.z;
        const double a2 = ax * ax + ay * ay + az * az, j2 = jx * jx + jy * jy + jz * jz;
        if (!(j2 > 0)) return __builtin_inf();
        q = a2 / j2;
    } else {
        // v_frexp_exp_i32_f64: the exponent e with |x| in [2^(e-1), 2^e), subnormals included; 0 for 0, infinities and NaN
        const int ea = __builtin_amdgcn_frexp_exp(__builtin_fmax(__builtin_fmax(__builtin_fabs(a.x), __builtin_fabs(a.y)), __builtin_fabs(a.z)));
        const int ej = __builtin_amdgcn_frexp_exp(__builtin_fmax(__builtin_fmax(__builtin_fabs(j.x), __builtin_fabs(j.y)), __builtin_fabs(j.z)));
        double    ah, al, jh, jl;
        norm2_pair(__builtin_ldexp(a.x, -ea), __builtin_ldexp(a.y, -ea), __builtin_ldexp(a.z, -ea), ah, al);
        norm2_pair(__builtin_ldexp(j.x, -ej), __builtin_ldexp(j.y, -ej), __builtin_ldexp(j.z, -ej), jh, jl);
        if (!(jh > 0)) return __builtin_inf();
        q              = ah / jh;
        const double r = __builtin_fma(-q, jh, ah) + (al - q * jl);
        const double c = q + r / jh;
        if (c == c && c - c == 0) q = c;
        shift = ea - ej;
    }
    if (!(q == q && q - q == 0)) return __builtin_inf();  // (non-finite ratios are left out)
    q = __builtin_ldexp(__builtin_sqrt(q), shift);
    return q - q == 0 ? q : __builtin_inf();
}
