// wave_fold.inc -- the S waves' second-level sums folded into wave 0 through LDS, in wave order, as TEXT included inside the kernel body
// behind the chunk loop.  Requires T, LT, W, S, NS, wave, lane and second[NS]; defines red.  A __syncthreads inside; the waves other than
// wave 0 return, and wave 0 goes on with the workgroup's sums in second[NS].
    __shared__ T red[(S > 1 ? S - 1 : 1) * NS * W * 64];
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
#pragma unroll
            for (int k = 0; k < W; ++k) red[(((wave - 1) * NS + q) * W + k) * 64 + lane] = LT::get(second[q], k);
        }
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll 1
    for (int g = 1; g < S; ++g) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
#pragma unroll
            for (int k = 0; k < W; ++k) LT::set(second[q], k, LT::get(second[q], k) + red[(((g - 1) * NS + q) * W + k) * 64 + lane]);
        }
    }
