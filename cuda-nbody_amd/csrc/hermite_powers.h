// hermite_powers.h -- s^-2 and s^-3 from s^2, shared by every kernel that couples through them: the acceleration + jerk kernels and
// field.hip (through hermite_stream.h) and hermite6_eval.hip (which has a body j of its own).  Included inside each translation unit's own
// anonymous namespace, after nbody_lane.h (device code, internal linkage).
#pragma once

// s^-2 and s^-3 from s2.  fp32: v_rsq_f32 (1 ulp) and two products.  fp64: the v_rsq_f64 seed y0 (relative error <= 2^-23) and, with
// r = 1 - s2 y0^2 (|r| <= 2^-22), the series of Lane<double>::coupling for y0^3 (1-r)^(-3/2) and y0^2 (1 + r + r^2) for y0^2 / (1-r).
template <typename T> struct Powers;
template <> struct Powers<float> {
    using vec = Lane<float>::vec;
    static __device__ __forceinline__ void of(vec s2, const Lane<float>::Consts&, vec& inv2, vec& inv3) {
        const vec inv = vec{__builtin_amdgcn_rsqf(s2.x), __builtin_amdgcn_rsqf(s2.y)};
        inv2          = inv * inv;
        inv3          = inv * inv2;
    }
};
template <> struct Powers<double> {
    static __device__ __forceinline__ void of(double s2, const Lane<double>::Consts& k, double& inv2, double& inv3) {
        const double y0 = __builtin_amdgcn_rsq(s2);
        const double t0 = y0 * y0;
        const double r  = __builtin_fma(-s2, t0, 1.0);
        const double c  = y0 * t0;
        const double w  = r * __builtin_fma(r, k.c1875, k.c15);
        inv3            = __builtin_fma(c, w, c);
        const double q  = __builtin_fma(r, r, r);
        inv2            = __builtin_fma(t0, q, t0);
    }
};
