// hermite6_correct.inc -- the 6th-order corrector and the new crackle of one body, as text.  One text for hermite6_eval (hermite6_eval.hip),
// hermite6_ensemble_eval (hermite6_ensemble.hip), hermite6_block_finish (hermite6_block.hip) and hermite6_block_ensemble_finish.  The includer has defined T, vec4, the
// body's index i, the evaluation's a1, j1, s1 (vec4 each) and two macros, which this file undefines:
//   HERMITE6_STEP_DT          the step
//   HERMITE6_STORED(array)    the array of the stored state -- old_pos, vel, acc, jerk, snap -- that index i counts in
// It gets: x1, v replaced by v1, and c1.  The includer stores them, in an order of its own (the listings of the three differ in it).
            // v1 = v + (a0 + a1) h/2 - (j1 - j0) h^2/10 + (s0 + s1) h^3/120,   x1 = x + (v + v1) h/2 - (a1 - a0) h^2/10 + (j0 + j1) h^3/120
            // c1, the third derivative at the step's end of the quintic through (a, j, s) at both ends:
            //   D0 = a1 - a0 - j0 h - s0 h^2/2,  D1 = (j1 - j0 - s0 h) h,  D2 = (s1 - s0) h^2,  c1 = (60 D0 - 36 D1 + 9 D2) / h^3
            // (the small terms are summed first: v1 and x1 then take one rounding of their own size, like a plain v + increment)
            const T    h = HERMITE6_STEP_DT, h2 = h * T(0.5), hh = h * h, t10 = hh * T(0.1), h3 = hh * h, t120 = h3 * (T(1) / T(120));
            const vec4 x  = reinterpret_cast<const vec4*>(HERMITE6_STORED(old_pos))[i];
            vec4       v  = reinterpret_cast<const vec4*>(HERMITE6_STORED(vel))[i];
            const vec4 a0 = reinterpret_cast<const vec4*>(HERMITE6_STORED(acc))[i];
            const vec4 j0 = reinterpret_cast<const vec4*>(HERMITE6_STORED(jerk))[i];
            const vec4 s0 = reinterpret_cast<const vec4*>(HERMITE6_STORED(snap))[i];
            vec4       x1, c1;
            auto       component = [&](T xq, T& vq, T a0q, T j0q, T s0q, T a1q, T j1q, T s1q, T& x1q, T& c1q) {
                const T v1 = vq + __builtin_fma(h2, a0q + a1q, __builtin_fma(t120, s0q + s1q, -t10 * (j1q - j0q)));
                x1q        = xq + __builtin_fma(h2, vq + v1, __builtin_fma(t120, j0q + j1q, -t10 * (a1q - a0q)));
                const T d0 = __builtin_fma(-h2 * h, s0q, __builtin_fma(-h, j0q, a1q - a0q));
                const T d1 = __builtin_fma(-h, s0q, j1q - j0q) * h;
                const T d2 = (s1q - s0q) * hh;
                c1q        = __builtin_fma(T(9), d2, __builtin_fma(T(-36), d1, T(60) * d0)) / h3;
                vq         = v1;
            };
            component(x.x, v.x, a0.x, j0.x, s0.x, a1.x, j1.x, s1.x, x1.x, c1.x);
            component(x.y, v.y, a0.y, j0.y, s0.y, a1.y, j1.y, s1.y, x1.y, c1.y);
            component(x.z, v.z, a0.z, j0.z, s0.z, a1.z, j1.z, s1.z, x1.z, c1.z);
            x1.w = x.w, c1.w = 0;
#undef HERMITE6_STEP_DT
#undef HERMITE6_STORED
