// range_sum.inc -- sum[NS] = the partial planes [J][NS][slots] of one slot added over the J ranges in range order, as TEXT included
// inside the kernel body (hermite_block_finish, field_finish; no include guard).  The includer defines before it: T, NS; partial (the
// planes), ranges (J), slots, slot.  It gets: sum[NS].
//
// Eight ranges' loads are in flight at a time: one lane's J x NS dependent round trips to L2 were a third of a block step with a handful of
// active bodies.
    T sum[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) sum[q] = partial[q * slots + slot];
#pragma unroll 1
    for (unsigned r0 = 1; r0 < ranges; r0 += 8) {
        T part[8][NS];
#pragma unroll
        for (unsigned u = 0; u < 8; ++u) {
            const size_t r = r0 + u < ranges ? r0 + u : r0;
#pragma unroll
            for (int q = 0; q < NS; ++q) part[u][q] = partial[(r * NS + q) * slots + slot];
        }
#pragma unroll
        for (unsigned u = 0; u < 8; ++u) {
            if (r0 + u < ranges) {
#pragma unroll
                for (int q = 0; q < NS; ++q) sum[q] += part[u][q];
            }
        }
    }
