// hermite6_interaction.inc -- the acceleration + jerk + snap interaction of hermite6_eval, as TEXT: the `compute` hermite_stream.inc takes
// from its includer (HERMITE_STREAM_INTERACTION).  Besides what hermite_stream.inc lists, the kernel defines the lane's accelerations
// ax, ay, az; a body j carries b.a next to b.p and b.v.  NS is 9: ax ay az jx jy jz sx sy sz.
//
// r = x_j - x_i, w = v_j - v_i, b = a_j - a_i, s2 = r.r + eps2, k = m_j s^-3:
//     alpha = (r.w) / s2          beta = (w.w + r.b) / s2 + alpha^2
//     J' = w - 3 alpha r          S' = b - 6 alpha J' - 3 beta r
//     a += k r,   jerk += k J',   snap += k S'
// fp32, per packed pair and without the mass multiply: 9 subtractions, 12 for s2, r.w and w.w + r.b, 2 powers, 6 for alpha, beta and
// their multiples, 9 for J' and S', 9 sums = 47 packed ops + 2 v_rsq_f32.
    auto compute = [&]<bool UNIT, int UB>(const BodyJ<T>* b, unsigned, vec (&sum)[NS]) {
        vec dx[UB], dy[UB], dz[UB], ex[UB], ey[UB], ez[UB], fx[UB], fy[UB], fz[UB], s2[UB], rv[UB], q[UB], k3[UB], a3[UB], b3[UB], a6[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            dx[u] = LT::splat(b[u].p.x) - px, dy[u] = LT::splat(b[u].p.y) - py, dz[u] = LT::splat(b[u].p.z) - pz;
            ex[u] = LT::splat(b[u].v.x) - vx, ey[u] = LT::splat(b[u].v.y) - vy, ez[u] = LT::splat(b[u].v.z) - vz;
            fx[u] = LT::splat(b[u].a.x) - ax, fy[u] = LT::splat(b[u].a.y) - ay, fz[u] = LT::splat(b[u].a.z) - az;
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) s2[u] = LT::fma(dx[u], dx[u], eps2), rv[u] = dx[u] * ex[u], q[u] = ex[u] * ex[u];
#pragma unroll
        for (int u = 0; u < UB; ++u) s2[u] = LT::fma(dy[u], dy[u], s2[u]), rv[u] = LT::fma(dy[u], ey[u], rv[u]), q[u] = LT::fma(ey[u], ey[u], q[u]);
#pragma unroll
        for (int u = 0; u < UB; ++u) s2[u] = LT::fma(dz[u], dz[u], s2[u]), rv[u] = LT::fma(dz[u], ez[u], rv[u]), q[u] = LT::fma(ez[u], ez[u], q[u]);
#pragma unroll
        for (int u = 0; u < UB; ++u) q[u] = LT::fma(dz[u], fz[u], LT::fma(dy[u], fy[u], LT::fma(dx[u], fx[u], q[u])));  // w.w + r.b
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            vec inv2;
            Powers<T>::of(s2[u], consts, inv2, k3[u]);
            const vec alpha = rv[u] * inv2;
            a3[u]           = alpha * minus3;                               // -3 alpha
            b3[u]           = LT::fma(alpha, alpha, q[u] * inv2) * minus3;  // -3 beta
            a6[u]           = a3[u] + a3[u];                                // -6 alpha
            if constexpr (!UNIT) k3[u] = k3[u] * LT::splat(b[u].p.w);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) ex[u] = LT::fma(a3[u], dx[u], ex[u]), ey[u] = LT::fma(a3[u], dy[u], ey[u]), ez[u] = LT::fma(a3[u], dz[u], ez[u]);  // J'
#pragma unroll
        for (int u = 0; u < UB; ++u) fx[u] = LT::fma(a6[u], ex[u], fx[u]), fy[u] = LT::fma(a6[u], ey[u], fy[u]), fz[u] = LT::fma(a6[u], ez[u], fz[u]);
#pragma unroll
        for (int u = 0; u < UB; ++u) fx[u] = LT::fma(b3[u], dx[u], fx[u]), fy[u] = LT::fma(b3[u], dy[u], fy[u]), fz[u] = LT::fma(b3[u], dz[u], fz[u]);  // S'
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            sum[0] = LT::fma(dx[u], k3[u], sum[0]), sum[1] = LT::fma(dy[u], k3[u], sum[1]), sum[2] = LT::fma(dz[u], k3[u], sum[2]);
            sum[3] = LT::fma(ex[u], k3[u], sum[3]), sum[4] = LT::fma(ey[u], k3[u], sum[4]), sum[5] = LT::fma(ez[u], k3[u], sum[5]);
            sum[6] = LT::fma(fx[u], k3[u], sum[6]), sum[7] = LT::fma(fy[u], k3[u], sum[7]), sum[8] = LT::fma(fz[u], k3[u], sum[8]);
        }
    };
