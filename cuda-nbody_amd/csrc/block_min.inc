// block_min.inc -- the minimum over a workgroup of 256 lanes through LDS, behind the time steps of hermite_eval.hip, hermite6_eval.hip and the
// two ensembles (hermite_ensemble_clock.inc).  Exact in any order.  Included inside each translation unit's own anonymous namespace.
__device__ __forceinline__ double block_min(double m, double* lds) {
    const int tid = threadIdx.x;
    lds[tid]      = m;
    __syncthreads();
#pragma unroll 1
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half) lds[tid] = fmin(lds[tid], lds[tid + half]);
        __syncthreads();
    }
    return lds[0];
}
