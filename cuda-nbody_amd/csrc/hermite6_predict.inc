// hermite6_predict.inc -- the 6th-order predictor of one body, as text: Horner in dt.  One text for hermite6_predict (hermite6_eval.hip)
// and hermite6_ensemble_predict (hermite6_ensemble.hip).  The includer has defined T, vec4, the step dt and the body's stored state x, v,
// a, j, s, c (vec4 each); this defines xp, vp, ap = {x_p, m}, {v_p, 0}, {a_p, 0}.
//   x_p = x + v h + a h^2/2 + j h^3/6 + s h^4/24 + c h^5/120,   v_p = v + a h + j h^2/2 + s h^3/6 + c h^4/24,   a_p = a + j h + s h^2/2 + c h^3/6
    const T    h2 = dt * T(0.5), h3 = dt * (T(1) / T(3)), h4 = dt * T(0.25), h5 = dt * T(0.2);
    vec4       xp, vp, ap;
    auto       component = [&](T xq, T vq, T aq, T jq, T sq, T cq, T& xpq, T& vpq, T& apq) {
        xpq = __builtin_fma(dt, __builtin_fma(h2, __builtin_fma(h3, __builtin_fma(h4, __builtin_fma(h5, cq, sq), jq), aq), vq), xq);
        vpq = __builtin_fma(dt, __builtin_fma(h2, __builtin_fma(h3, __builtin_fma(h4, cq, sq), jq), aq), vq);
        apq = __builtin_fma(dt, __builtin_fma(h2, __builtin_fma(h3, cq, sq), jq), aq);
    };
    component(x.x, v.x, a.x, j.x, s.x, c.x, xp.x, vp.x, ap.x);
    component(x.y, v.y, a.y, j.y, s.y, c.y, xp.y, vp.y, ap.y);
    component(x.z, v.z, a.z, j.z, s.z, c.z, xp.z, vp.z, ap.z);
    xp.w = x.w, vp.w = 0, ap.w = 0;
