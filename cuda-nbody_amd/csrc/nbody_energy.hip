// nbody_energy.hip -- diagnostics of the state the integrate kernels advance (nb_energy_*, include/nbody_hip.h).  gfx950 only.
//
// What it computes: the kinetic energy, the softened (Plummer) potential -sum_{i<j} m_i m_j / sqrt(|p_i - p_j|^2 + eps^2) -- the
// potential whose negative gradient is the force the integrate kernels apply --, the mass, the momentum, the angular momentum
// about the origin and the centre of mass.  How it is laid out:
//
//   * Every unordered pair once.  The bodies are cut into blocks of 64*I (I bodies i per lane: 4 packed pairs = 8 bodies fp32,
//     4 bodies fp64).  Block a meets blocks a + d (mod NB) for d = 0 .. NB/2 -- the tournament order of nbody_pair.hip; for an
//     even NB the partners at distance NB/2 meet once, from the lower block.  d = 0 is the diagonal block, where only j > i
//     counts (the i = j term would be m^2/eps, or inf when eps = 0: it is masked, not subtracted).  The potential is symmetric,
//     so there are no reaction sums to carry: half the arithmetic of a one-sided sweep and no N^2 workspace.
//   * Work units.  A unit is one partner block's chunk of kChunk consecutive bodies j.  The units of block a are split over
//     C workgroups (a function of N and the precision only, never of the device: same geometry, same bits everywhere), and
//     over the kWaves waves of a workgroup by a fixed stride.  Every wave holds its block's bodies i in registers and streams
//     the bodies j of a unit through SCALAR loads (wave-uniform addresses, the constant address space: positions are
//     read-only), as nbody_fast.hip does.
//   * fp32 hot loop: per body j and packed pair of bodies i, 3 v_pk_add_f32 (d), 3 v_pk_fma_f32 (d^2 + eps^2), 2 v_rsq_f32 and
//     1 v_pk_fma_f32 (acc += m_j * r^-1).  The fp32 sums run over one unit (kChunk = 128 bodies j) only; each is then multiplied
//     by m_i and folded into the lane's fp64 sum.  Everything after that is fp64.
//   * fp64: d^(-1/2) from the v_rsq_f64 seed y0 (relative error <= 2^-22) by a series in r = 1 - d^2 y0^2:
//     y0 (1 + r/2 + 3/8 r^2), truncation 5/16 r^3 < 2^-66 -- a few ulp, in the style of Lane<double>::coupling.
//   * O(N) terms (kinetic energy, mass, momentum, angular momentum, sum m p) in fp64 by the first workgroup of each block.
//   * Reduction: a fixed LDS tree per workgroup into one fp64 record in the workspace; a second kernel of one workgroup adds the
//     records, each thread a contiguous run of them in index order, then the same fixed tree.  No atomics: the result is a
//     function of the inputs alone, bit for bit.
//
// Compiled with FMA contraction ON (default).
#include "../../include/nbody_hip.h"
#include "nbody_kernels.h"

namespace nb {
namespace {

#include "nbody_lane.h"

constexpr int      kWaves   = 4;            // waves per workgroup
constexpr int      kThreads = 64 * kWaves;
constexpr unsigned kChunk   = 128;          // bodies j per unit: the longest fp32 sum
constexpr int      kR       = 4;            // vectors of bodies i per lane (I = kR * W)
constexpr unsigned kTargetWorkgroups = 2048;

template <typename T> constexpr unsigned block_bodies() { return 64u * kR * Lane<T>::W; }

template <typename T> struct EnergyArgs {
    const T* pos;
    const T* vel;
    double*  records;
    unsigned n, blocks, splits, units;  // NB, C, units per block ((NB/2 + 1) * block / kChunk)
    T        eps2;
};

#include "energy_pair.inc"  // kFields, kRecord, tree_sum, inv_sqrt, sweep: shared with energy_ensemble.hip

template <typename T> __global__ __launch_bounds__(kThreads) void energy_pairs(EnergyArgs<T> e) {
    using LT              = Lane<T>;
    using vec             = typename LT::vec;
    using vec4            = typename LT::vec4;
    using raw4            = typename LT::raw4;
    constexpr int      W  = LT::W;
    constexpr int      I  = kR * W;
    constexpr unsigned B  = block_bodies<T>();
    constexpr unsigned K  = B / kChunk;  // units per partner block
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx4/x8
    const stream_ptr   bodies = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(e.pos));
    const vec4* const  pos4   = reinterpret_cast<const vec4*>(e.pos);
    const vec4* const  vel4   = reinterpret_cast<const vec4*>(e.vel);

    const int      tid  = threadIdx.x;
    const int      wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int      lane = tid & 63;
    const unsigned a    = blockIdx.x / e.splits;
    const unsigned c    = blockIdx.x % e.splits;

    // bodies i of this lane: a*B + k*64 + lane (k = r*W + w); a body past the end has mass 0 and is never folded
    vec      px[kR], py[kR], pz[kR];
    T        mi[I];
    unsigned idx[I];
#pragma unroll
    for (int k = 0; k < I; ++k) {
        idx[k]           = a * B + k * 64 + lane;
        const bool  live = idx[k] < e.n;
        const vec4  p    = live ? pos4[idx[k]] : vec4{};
        LT::set(px[k / W], k % W, p.x);
        LT::set(py[k / W], k % W, p.y);
        LT::set(pz[k / W], k % W, p.z);
        mi[k] = live ? p.w : T(0);
    }
    vec eps2 = LT::splat(e.eps2);
    LT::keep_in_vgpr(eps2);

    double pot = 0;
    const unsigned u_begin = static_cast<unsigned>(static_cast<unsigned long long>(e.units) * c / e.splits);
    const unsigned u_end   = static_cast<unsigned>(static_cast<unsigned long long>(e.units) * (c + 1) / e.splits);
    const unsigned half    = e.blocks / 2;
#pragma unroll 1
    for (unsigned u = u_begin + wave; u < u_end; u += kWaves) {
        const unsigned d = u / K;
        if ((e.blocks & 1u) == 0 && d == half && d != 0 && a >= half) continue;  // (even NB: the pair at distance NB/2 is the lower block's)
        const unsigned b  = a + d < e.blocks ? a + d : a + d - e.blocks;
        const unsigned j0 = b * B + (u % K) * kChunk;
        if (j0 >= e.n) continue;
        const unsigned j1 = j0 + kChunk < e.n ? j0 + kChunk : e.n;
        vec acc[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) acc[r] = LT::splat(0);
        if (d == 0) sweep<T, true, kR>(bodies, j0, j1, px, py, pz, idx, eps2, acc);
        else        sweep<T, false, kR>(bodies, j0, j1, px, py, pz, idx, eps2, acc);
#pragma unroll
        for (int k = 0; k < I; ++k) {
            if (idx[k] < e.n) pot = __builtin_fma(static_cast<double>(mi[k]), static_cast<double>(LT::get(acc[k / W], k % W)), pot);
        }
    }

    double v[kFields] = {};
    v[0] = pot;
    if (c == 0) {  // the O(N) terms of block a, in fp64
#pragma unroll
        for (unsigned s = 0; s < B / kThreads; ++s) {
            const unsigned i = a * B + s * kThreads + tid;
            if (i >= e.n) continue;
            const vec4   p = pos4[i], q = vel4[i];
            const double m = p.w, x = p.x, y = p.y, z = p.z, vx = q.x, vy = q.y, vz = q.z;
            v[1] += m * (vx * vx + vy * vy + vz * vz);
            v[2] += m;
            v[3] += m * vx, v[4] += m * vy, v[5] += m * vz;
            v[6] += m * (y * vz - z * vy), v[7] += m * (z * vx - x * vz), v[8] += m * (x * vy - y * vx);
            v[9] += m * x, v[10] += m * y, v[11] += m * z;
        }
    }
    __shared__ double lds[kFields][kThreads];
    tree_sum(lds, v);
    if (tid < kFields) e.records[static_cast<size_t>(blockIdx.x) * kRecord + tid] = lds[tid][0];
}

// One workgroup: thread t adds a contiguous run of records in index order, then the fixed tree; thread 0 writes the result.
__global__ __launch_bounds__(kThreads) void energy_finish(const double* records, unsigned count, nb_energy_t* out) {
    const int      t     = threadIdx.x;
    const unsigned per   = (count + kThreads - 1) / kThreads;
    const unsigned first = t * per < count ? t * per : count;
    const unsigned last  = first + per < count ? first + per : count;
    double v[kFields] = {};
#pragma unroll 1
    for (unsigned r = first; r < last; ++r) {
#pragma unroll
        for (int f = 0; f < kFields; ++f) v[f] += records[static_cast<size_t>(r) * kRecord + f];
    }
    __shared__ double lds[kFields][kThreads];
    tree_sum(lds, v);
    if (t == 0) {
        const double mass = lds[2][0];
        nb_energy_t  res;
        res.kinetic   = 0.5 * lds[1][0];
        res.potential = -lds[0][0];
        res.total     = res.kinetic + res.potential;
        res.mass      = mass;
        for (int k = 0; k < 3; ++k) {
            res.momentum[k]         = lds[3 + k][0];
            res.angular_momentum[k] = lds[6 + k][0];
            res.center_of_mass[k]   = mass != 0 ? lds[9 + k][0] / mass : 0.0;
        }
        *out = res;
    }
}

}  // namespace

template <typename T> EnergyPlan plan_energy(unsigned n) {
    EnergyPlan p{};
    if (n == 0) return p;
    constexpr unsigned B = block_bodies<T>();
    p.block_bodies = B;
    p.blocks       = (n + B - 1) / B;
    p.units        = (p.blocks / 2 + 1) * (B / kChunk);
    // about kTargetWorkgroups workgroups in all, every wave with two units or more
    const unsigned want  = (kTargetWorkgroups + p.blocks - 1) / p.blocks;
    const unsigned most  = p.units / (2 * kWaves) > 0 ? p.units / (2 * kWaves) : 1;
    p.splits             = want < most ? want : most;
    p.records            = p.blocks * p.splits;
    p.workspace_bytes    = static_cast<size_t>(p.records) * kRecord * sizeof(double);
    return p;
}

template <typename T> hipError_t launch_energy(const T* pos, const T* vel, unsigned n, T eps2, const EnergyPlan& p, void* workspace, nb_energy_t* out, hipStream_t stream) {
    EnergyArgs<T> e{};
    e.pos = pos, e.vel = vel, e.records = static_cast<double*>(workspace);
    e.n = n, e.blocks = p.blocks, e.splits = p.splits, e.units = p.units, e.eps2 = eps2;
    (void)hipGetLastError();  // (a launch reports its own error)
    hipLaunchKernelGGL(energy_pairs<T>, dim3(p.records), dim3(kThreads), 0, stream, e);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL(energy_finish, dim3(1), dim3(kThreads), 0, stream, static_cast<const double*>(workspace), p.records, out);
    return hipGetLastError();
}

template EnergyPlan plan_energy<float>(unsigned);
template EnergyPlan plan_energy<double>(unsigned);
template hipError_t launch_energy<float>(const float*, const float*, unsigned, float, const EnergyPlan&, void*, nb_energy_t*, hipStream_t);
template hipError_t launch_energy<double>(const double*, const double*, unsigned, double, const EnergyPlan&, void*, nb_energy_t*, hipStream_t);

}  // namespace nb
