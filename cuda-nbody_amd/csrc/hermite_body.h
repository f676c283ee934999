// hermite_body.h -- the 4th-order Hermite predictor for one body, the one function behind hermite_predict (nb_hermite_step_*),
// block_predict_count and block_sync (nb_hermite_block_*).  Included inside each translation unit's own anonymous namespace, after
// nbody_lane.h.  (The corrector is TEXT, hermite_correct.inc: as a function it changed the STEP kernels of hermite_eval.s.)
#pragma once

// x_p = x + v dt + a dt^2/2 + j dt^3/6,   v_p = v + a dt + j dt^2/2;   x_p.w = x.w (the mass), v_p.w = 0
template <typename T> __device__ __forceinline__ void predict_body(const typename Lane<T>::vec4& x, const typename Lane<T>::vec4& v, const typename Lane<T>::vec4& a,
                                                                 const typename Lane<T>::vec4& j, T dt, typename Lane<T>::vec4& xp, typename Lane<T>::vec4& vp) {
    const T h = dt * T(0.5), t = dt * (T(1) / T(3));
    xp.x = __builtin_fma(dt, __builtin_fma(h, __builtin_fma(t, j.x, a.x), v.x), x.x);
    xp.y = __builtin_fma(dt, __builtin_fma(h, __builtin_fma(t, j.y, a.y), v.y), x.y);
    xp.z = __builtin_fma(dt, __builtin_fma(h, __builtin_fma(t, j.z, a.z), v.z), x.z);
    xp.w = x.w;
    vp.x = __builtin_fma(dt, __builtin_fma(h, j.x, a.x), v.x);
    vp.y = __builtin_fma(dt, __builtin_fma(h, j.y, a.y), v.y);
    vp.z = __builtin_fma(dt, __builtin_fma(h, j.z, a.z), v.z);
    vp.w = 0;
}
