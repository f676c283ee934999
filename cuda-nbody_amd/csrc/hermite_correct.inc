// hermite_correct.inc -- the 4th-order Hermite corrector for one body, as TEXT included inside the kernel body (hermite_eval's STEP
// epilogue, hermite_block_finish; no include guard).  The includer defines before it: T, vec4; dt; the stored x, v (not const), a0, j0 and
// the new a1, j1 of the body.  It gets: x1, and v replaced by v1.
//     v1 = v + (a0 + a1) dt/2 + (j0 - j1) dt^2/12,   x1 = x + (v + v1) dt/2 + (a0 - a1) dt^2/12
            const T h = dt * T(0.5), d12 = dt * dt * (T(1) / T(12));
            vec4    x1;
            const T v1x = __builtin_fma(d12, j0.x - j1.x, __builtin_fma(h, a0.x + a1.x, v.x));
            const T v1y = __builtin_fma(d12, j0.y - j1.y, __builtin_fma(h, a0.y + a1.y, v.y));
            const T v1z = __builtin_fma(d12, j0.z - j1.z, __builtin_fma(h, a0.z + a1.z, v.z));
            x1.x = __builtin_fma(d12, a0.x - a1.x, __builtin_fma(h, v.x + v1x, x.x));
            x1.y = __builtin_fma(d12, a0.y - a1.y, __builtin_fma(h, v.y + v1y, x.y));
            x1.z = __builtin_fma(d12, a0.z - a1.z, __builtin_fma(h, v.z + v1z, x.z));
            x1.w = x.w;
            v.x = v1x, v.y = v1y, v.z = v1z;
