// wave_groups.inc -- a chunk's groups of U bodies j streamed against the lane's bodies i, one load group ahead, as TEXT included inside the
// kernel body (hermite_stream.inc, field_eval; no include guard).  The includer defines before it: T, U, first; group(j0, b): the scalar
// loads of the U bodies j from j0 on; compute<FORM, UB>(b, j0, sum): UB bodies j (the first is body j0) against the lane's bodies i in one
// of the kernel's two forms.  It gets: UB, whole, arrived, stream.
    // a group of U bodies j in stage blocks of UB: fp32 2 x 2 (four chains' temporaries at once took hermite_eval to 127 VGPRs, and its
    // S = 1 instantiation into scratch; two blocks of two compile to 93 - 95), fp64 one block of 2
    constexpr int UB = sizeof(T) == 8 ? U : U / 2;
    auto whole = [&]<bool FORM>(const BodyJ<T> (&b)[U], unsigned j0) {
#pragma unroll
        for (int h = 0; h < U; h += UB) compute.template operator()<FORM, UB>(b + h, j0 + h, first);
    };
    auto arrived = [](const BodyJ<T> (&b)[U]) { asm volatile("" : : "s"(b[0].p) : "memory"); };  // what follows is issued after the set's wait
    // b0 holds (or is loading) group 0 of the chunk at body `chunk`; on return it is loading the first group at body `next`
    auto stream = [&]<bool FORM>(unsigned chunk, unsigned groups, size_t next, BodyJ<T> (&b0)[U], BodyJ<T> (&b1)[U]) {
        unsigned g = 0;
#pragma unroll 1
        for (; g + 2 <= groups; g += 2) {
            arrived(b0);
            group(static_cast<size_t>(chunk) + (g + 1) * U, b1);
            __builtin_amdgcn_sched_barrier(0);  // (the load stays ahead of the compute it overlaps)
            whole.template operator()<FORM>(b0, chunk + g * U);
            arrived(b1);
            group(g + 2 < groups ? static_cast<size_t>(chunk) + (g + 2) * U : next, b0);
            __builtin_amdgcn_sched_barrier(0);
            whole.template operator()<FORM>(b1, chunk + (g + 1) * U);
        }
        if (g < groups) whole.template operator()<FORM>(b0, chunk + g * U);  // (odd count: the ragged last chunk, nothing follows it)
    };
