// hermite6_correct.inc -- the 6th-order corrector and the new crackle of one body, as text.  One text for hermite6_eval (hermite6_eval.hip),
// hermite6_ensemble_eval (hermite6_ensemble.hip), hermite6_block_finish (hermite6_block.hip) and hermite6_block_ensemble_finish.  The includer has defined T, vec4, the
// body's index i, the evaluation's a1, j1, s1 (vec4 each) and two macros, which this file undefines:
//   HERMITE6_STEP_DT          the step
//   HERMITE6_STORED(array)    the array of the stored state -- old_pos, vel, acc, jerk, snap -- that index i counts in
// It gets: x1, v replaced by v1, and c1.  The includer stores them, in an order of its own (the listings of the three differ in it).
            // v1 = v + (a0 + a1) h/2 - (j1 - j0) h^2/10 + (s0 + s1) h^3/120,   x1 = x + (v + v1) h/2 - (a1 - a0) h^2/10 + (j0 + j1) h^3/120
            // c1, the third derivative at the step's end of the quintic through (a, j, s) at both ends:
            //   D0 = a1 - a0 - j0 h - s0 h^2/2,  D1 = (j1 - j0 - s0 h) h,  D2 = (s1 - s0) h^2,  c1 = (60 D0 - 36 D1 + 9 D2) / h^3
            // v1 and x1 are each ONE rounding of their own size: the increment is summed in twice T's precision -- fp32 in fp64, where sums of two
            // T are exact; fp64 in double-double arithmetic (unevaluated sums hi + lo from two_sum and fma, h^2/10 and h^3/120 as such sums too).
            // A body whose step is long for it -- a tight encounter, where h^3/120 |s0 + s1| can be the largest term and larger than |v| --
            // would otherwise collect a rounding of that term's size from every operation on its path (the sum, each fma, the last
            // addition): four where the bound of 2u of the term magnitudes (tests/test_hermite6.py ld_step) has room for two.  No
            // contraction inside: the error terms are exact only of plain sums.
            const T h = HERMITE6_STEP_DT, h2 = h * T(0.5), hh = h * h, h3 = hh * h;
            auto two_sum = [](T p, T q, T& e) {
#pragma clang fp contract(off)
                const T s = p + q, b = s - p;
                e         = (p - (s - b)) + (q - b);
                return s;
            };
            // base + h/2 (p + q) - h^2/10 (r1 - r0) + h^3/120 (w0 + w1)
            auto advance = [&](T base, T p, T q, T r1, T r0, T w0, T w1) -> T {
#pragma clang fp contract(off)
                if constexpr (sizeof(T) == 4) {
                    const double hd = h;  // Horner in h: (the roundings here, the constants' included, are of 2^-53: far below fp32's)
                    double       up = (1.0 / 120.0) * (static_cast<double>(w0) + w1);
                    up              = __builtin_fma(hd, up, -0.1 * (static_cast<double>(r1) - r0));
                    up              = __builtin_fma(hd, up, 0.5 * (static_cast<double>(p) + q));
                    return static_cast<T>(__builtin_fma(hd, up, static_cast<double>(base)));
                } else {
                    const T hh_lo = __builtin_fma(h, h, -hh), h3_lo = __builtin_fma(hh, h, -h3) + hh_lo * h;
                    const T t10 = hh / T(10), t10_lo = (__builtin_fma(-t10, T(10), hh) + hh_lo) / T(10);
                    const T t120 = h3 / T(120), t120_lo = (__builtin_fma(-t120, T(120), h3) + h3_lo) / T(120);
                    T       ep, er, ew, e1, e2, e3;
                    const T sp = two_sum(p, q, ep), sr = two_sum(r1, -r0, er), sw = two_sum(w0, w1, ew);
                    const T A = h2 * sp, B = t10 * sr, C = t120 * sw;
                    const T lo_a = __builtin_fma(h2, sp, -A) + h2 * ep;
                    const T lo_b = __builtin_fma(t10, sr, -B) + (t10_lo * sr + t10 * er);
                    const T lo_c = __builtin_fma(t120, sw, -C) + (t120_lo * sw + t120 * ew);
                    const T s1 = two_sum(A, C, e1), s2 = two_sum(s1, -B, e2), s3 = two_sum(base, s2, e3);
                    return s3 + (e3 + (e2 + e1 + ((lo_a + lo_c) - lo_b)));
                }
            };
            const vec4 x  = reinterpret_cast<const vec4*>(HERMITE6_STORED(old_pos))[i];
            vec4       v  = reinterpret_cast<const vec4*>(HERMITE6_STORED(vel))[i];
            const vec4 a0 = reinterpret_cast<const vec4*>(HERMITE6_STORED(acc))[i];
            const vec4 j0 = reinterpret_cast<const vec4*>(HERMITE6_STORED(jerk))[i];
            const vec4 s0 = reinterpret_cast<const vec4*>(HERMITE6_STORED(snap))[i];
            vec4       x1, c1;
            auto       component = [&](T xq, T& vq, T a0q, T j0q, T s0q, T a1q, T j1q, T s1q, T& x1q, T& c1q) {
                const T v1 = advance(vq, a0q, a1q, j1q, j0q, s0q, s1q);
                x1q        = advance(xq, vq, v1, a1q, a0q, j0q, j1q);
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
