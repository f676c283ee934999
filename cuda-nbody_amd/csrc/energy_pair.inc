// energy_pair.inc -- the arithmetic nbody_energy.hip (nb_energy_*: one system) and energy_ensemble.hip (nb_energy_ensemble_*: many) share as
// text: the record's fields, the fixed tree over a workgroup, d^(-1/2), and the sweep of a run of bodies j over a lane's bodies i.
// Included inside the unit's own anonymous namespace, after nbody_lane.h (device code, internal linkage).

constexpr int      kFields = 12;  // potential sum, 2*kinetic, mass, momentum[3], angular momentum[3], sum m p[3]
constexpr unsigned kRecord = 16;  // doubles per workgroup record (12 used): 128 bytes

// The fixed tree over the THREADS threads of a workgroup: field f < FIELDS of thread 0 ends up holding the sum.  Same shape every launch.
template <int FIELDS = kFields, int THREADS> __device__ __forceinline__ void tree_sum(double (&lds)[kFields][THREADS], const double (&v)[kFields]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int f = 0; f < FIELDS; ++f) lds[f][t] = v[f];
    __syncthreads();
#pragma unroll 1
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int f = 0; f < FIELDS; ++f) lds[f][t] += lds[f][t + s];
        }
        __syncthreads();
    }
}

// m_j / sqrt(d2) (fp32: one v_rsq_f32 per body, 1 ulp; fp64: seed + series)
template <typename T> __device__ __forceinline__ typename Lane<T>::vec inv_sqrt(typename Lane<T>::vec d2);
template <> __device__ __forceinline__ v2f inv_sqrt<float>(v2f d2) { return v2f{__builtin_amdgcn_rsqf(d2.x), __builtin_amdgcn_rsqf(d2.y)}; }
template <> __device__ __forceinline__ double inv_sqrt<double>(double d2) {
    const double y0 = __builtin_amdgcn_rsq(d2);
    const double r  = __builtin_fma(-d2, y0 * y0, 1.0);
    return __builtin_fma(y0 * r, __builtin_fma(r, 0.375, 0.5), y0);
}

// The bodies j of [j0, j1) against R vectors of the lane's bodies i: acc[r] += m_j / |p_i - p_j|_eps.  DIAG: only j > i counts.
template <typename T, bool DIAG, int R, typename Stream>
__device__ __forceinline__ void sweep(Stream bodies, unsigned j0, unsigned j1, const typename Lane<T>::vec (&px)[R], const typename Lane<T>::vec (&py)[R], const typename Lane<T>::vec (&pz)[R],
                                      const unsigned (&idx)[R * Lane<T>::W], typename Lane<T>::vec eps2, typename Lane<T>::vec (&acc)[R]) {
    using LT      = Lane<T>;
    using vec     = typename LT::vec;
    constexpr int W = LT::W;
#pragma unroll 4
    for (unsigned j = j0; j < j1; ++j) {
        const typename LT::raw4 b = bodies[j];
        const vec bx = LT::splat(b.x), by = LT::splat(b.y), bz = LT::splat(b.z), bm = LT::splat(b.w);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const vec dx = bx - px[r];
            const vec dy = by - py[r];
            const vec dz = bz - pz[r];
            vec       d2 = LT::fma(dx, dx, eps2);
            d2           = LT::fma(dy, dy, d2);
            d2           = LT::fma(dz, dz, d2);
            vec inv      = inv_sqrt<T>(d2);
            if constexpr (DIAG) {
#pragma unroll
                for (int w = 0; w < W; ++w) LT::set(inv, w, j > idx[r * W + w] ? LT::get(inv, w) : T(0));
            }
            acc[r] = LT::fma(bm, inv, acc[r]);
        }
    }
}
