// hermite_block_kernels_shared.h -- the small device helpers of the block time step scheme, one text for hermite_block.hip
// (nb_hermite_block_*), hermite6_block.hip (nb_hermite6_block_*), hermite_block_ensemble.hip (nb_hermite_block_ensemble_*) and
// hermite6_block_ensemble.hip (nb_hermite6_block_ensemble_*): the ticks of
// a level, the length of a tick, the minimum / deepest-level fold and the active count of a workgroup of 256, the level a run starts at,
// and Aarseth's step.  Included inside each translation unit's own anonymous namespace, after hermite_block_kernels.h (BlockParams).
// (What the listings did not allow as functions is text: hermite_block_parts.inc.)
#pragma once

__device__ __forceinline__ unsigned long long ticks_of(int level, int max_level) {
    const int k = level < 0 ? 0 : (level > max_level ? max_level : level);
    return 1ull << (max_level - k);
}
__device__ __forceinline__ double tick_length(const BlockParams& p) { return __builtin_ldexp(p.dt_max, -p.max_level); }

struct MinLevel {
    unsigned long long next;
    int                level;
};
// the minimum of `next` and the maximum of `level` over a workgroup of 256
__device__ __forceinline__ MinLevel block_fold(MinLevel m, unsigned long long* lds_next, int* lds_level) {
    const int tid  = threadIdx.x;
    lds_next[tid]  = m.next;
    lds_level[tid] = m.level;
    __syncthreads();
#pragma unroll 1
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half) {
            const unsigned long long other = lds_next[tid + half];
            if (other < lds_next[tid]) lds_next[tid] = other;
            const int deeper = lds_level[tid + half];
            if (deeper > lds_level[tid]) lds_level[tid] = deeper;
        }
        __syncthreads();
    }
    return MinLevel{lds_next[0], lds_level[0]};
}

// the number of active lanes of a workgroup of 256 -> counts[block]
__device__ __forceinline__ void block_count(bool active, unsigned* wave_count, unsigned* counts, unsigned block) {
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(active);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = static_cast<unsigned>(__builtin_popcountll(mask));
    __syncthreads();
    if (threadIdx.x == 0) counts[block] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

__device__ __forceinline__ double norm3(double x, double y, double z) { return __builtin_sqrt(x * x + y * y + z * z); }

// level k deepened until its step is no longer than `want` (q: the length of a tick)
__device__ __forceinline__ int deepened(int k, double want, const BlockParams& p, double q) {
    while (k < p.max_level && static_cast<double>(1ull << (p.max_level - k)) * q > want) ++k;
    return k;
}
// the level a run starts at: the longest step within eta_start |a| / |jerk|, dt_max where that is no positive number
template <typename V> __device__ __forceinline__ int first_level(const V& acc, const V& jerk, const BlockParams& p) {
    const double want0 = p.eta_start * norm3(acc.x, acc.y, acc.z) / norm3(jerk.x, jerk.y, jerk.z);
    const double want  = (want0 == want0 && want0 - want0 == 0 && want0 > 0) ? want0 : p.dt_max;
    return deepened(0, want, p, tick_length(p));
}

// Aarseth's step from the stored T-typed a0, j0, a1, j1, in fp64 (include/nbody_hip_hermite_block.h)
template <typename V> __device__ __forceinline__ double aarseth_dt(const V& a0, const V& j0, const V& a1, const V& j1, double h, double eta, double dt_max) {
    const double d[3]  = {static_cast<double>(a0.x) - static_cast<double>(a1.x), static_cast<double>(a0.y) - static_cast<double>(a1.y), static_cast<double>(a0.z) - static_cast<double>(a1.z)};
    const double p0[3] = {static_cast<double>(j0.x), static_cast<double>(j0.y), static_cast<double>(j0.z)};
    const double p1[3] = {static_cast<double>(j1.x), static_cast<double>(j1.y), static_cast<double>(j1.z)};
    double       a2e[3], a3[3];
    const double h2 = h * h, h3 = h2 * h;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a2 = (-6.0 * d[c] - h * (4.0 * p0[c] + 2.0 * p1[c])) / h2;
        a3[c]           = (12.0 * d[c] + 6.0 * h * (p0[c] + p1[c])) / h3;
        a2e[c]          = a2 + h * a3[c];
    }
    const double n_a1 = norm3(a1.x, a1.y, a1.z), n_j1 = norm3(p1[0], p1[1], p1[2]), n_a2 = norm3(a2e[0], a2e[1], a2e[2]), n_a3 = norm3(a3[0], a3[1], a3[2]);
    const double dt = __builtin_sqrt(eta * (n_a1 * n_a2 + n_j1 * n_j1) / (n_j1 * n_a3 + n_a2 * n_a2));
    return (dt == dt && dt - dt == 0) ? dt : dt_max;
}
