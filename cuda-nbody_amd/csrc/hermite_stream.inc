// hermite_stream.inc -- the interaction and the streaming loops of the acceleration + jerk kernels, as TEXT included inside the kernel body
// (hermite_eval in hermite_eval.hip, hermite_block_eval in hermite_block.hip; no include guard).  The kernel defines before it: T, LT, vec, U;
// the lane's bodies i px, py, pz, vx, vy, vz; eps2, minus3, consts; the sums first[6], second[6]; and group(j0, b): the scalar loads of U
// bodies j.  It gets: compute, whole, arrived, stream (a chunk's groups, one load group ahead), pending_scale and flush.
    // UB bodies j against the lane's vector of bodies i, written stage by stage: UB independent chains in flight
    auto compute = [&]<bool UNIT, int UB>(const BodyJ<T>* b, vec (&sum)[6]) {
        vec dx[UB], dy[UB], dz[UB], ex[UB], ey[UB], ez[UB], s2[UB], rv[UB], k3[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            dx[u] = LT::splat(b[u].p.x) - px, dy[u] = LT::splat(b[u].p.y) - py, dz[u] = LT::splat(b[u].p.z) - pz;
            ex[u] = LT::splat(b[u].v.x) - vx, ey[u] = LT::splat(b[u].v.y) - vy, ez[u] = LT::splat(b[u].v.z) - vz;
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) s2[u] = LT::fma(dx[u], dx[u], eps2), rv[u] = dx[u] * ex[u];
#pragma unroll
        for (int u = 0; u < UB; ++u) s2[u] = LT::fma(dy[u], dy[u], s2[u]), rv[u] = LT::fma(dy[u], ey[u], rv[u]);
#pragma unroll
        for (int u = 0; u < UB; ++u) s2[u] = LT::fma(dz[u], dz[u], s2[u]), rv[u] = LT::fma(dz[u], ez[u], rv[u]);
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            vec inv2;
            Powers<T>::of(s2[u], consts, inv2, k3[u]);
            rv[u] = (rv[u] * inv2) * minus3;  // -3 (r.w) / s^2
            if constexpr (!UNIT) k3[u] = k3[u] * LT::splat(b[u].p.w);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) ex[u] = LT::fma(rv[u], dx[u], ex[u]), ey[u] = LT::fma(rv[u], dy[u], ey[u]), ez[u] = LT::fma(rv[u], dz[u], ez[u]);
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            sum[0] = LT::fma(dx[u], k3[u], sum[0]), sum[1] = LT::fma(dy[u], k3[u], sum[1]), sum[2] = LT::fma(dz[u], k3[u], sum[2]);
            sum[3] = LT::fma(ex[u], k3[u], sum[3]), sum[4] = LT::fma(ey[u], k3[u], sum[4]), sum[5] = LT::fma(ez[u], k3[u], sum[5]);
        }
    };
    // a group of U bodies j in stage blocks of UB: fp32 2 x 2 (four chains' temporaries at once took the kernel to 127 VGPRs, and the
    // S = 1 instantiation into scratch; two blocks of two compile to 93 - 95), fp64 one block of 2
    constexpr int UB = sizeof(T) == 8 ? U : U / 2;
    auto whole = [&]<bool UNIT>(const BodyJ<T> (&b)[U]) {
#pragma unroll
        for (int h = 0; h < U; h += UB) compute.template operator()<UNIT, UB>(b + h, first);
    };
    auto arrived = [](const BodyJ<T> (&b)[U]) { asm volatile("" : : "s"(b[0].p) : "memory"); };  // what follows is issued after the set's wait
    // b0 holds (or is loading) group 0 of the chunk at body `chunk`; on return it is loading the first group at body `next`
    auto stream = [&]<bool UNIT>(size_t chunk, unsigned groups, size_t next, BodyJ<T> (&b0)[U], BodyJ<T> (&b1)[U]) {
        unsigned g = 0;
#pragma unroll 1
        for (; g + 2 <= groups; g += 2) {
            arrived(b0);
            group(chunk + (g + 1) * U, b1);
            __builtin_amdgcn_sched_barrier(0);  // (the load stays ahead of the compute it overlaps)
            whole.template operator()<UNIT>(b0);
            arrived(b1);
            group(g + 2 < groups ? chunk + (g + 2) * U : next, b0);
            __builtin_amdgcn_sched_barrier(0);
            whole.template operator()<UNIT>(b1);
        }
        if (g < groups) whole.template operator()<UNIT>(b0);  // (odd count: the ragged last chunk, nothing follows it)
    };
    T    pending_scale = T(1);  // what `first` is still to be multiplied by
    auto flush         = [&]() {
        const vec scale = LT::splat(pending_scale);
#pragma unroll
        for (int q = 0; q < 6; ++q) second[q] = LT::fma(first[q], scale, second[q]), first[q] = LT::splat(0);
    };
