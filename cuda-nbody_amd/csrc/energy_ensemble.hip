// energy_ensemble.hip -- the kernels of libnbody_hip_energy_ensemble.so (nb_energy_ensemble_*, include/nbody_hip_energy_ensemble.h): the
// nb_energy_t of every system of an ensemble in two launches, and the drift between two measurements in one.  gfx950 only.
//
// What a system's record holds and how a pair is computed is nbody_energy.hip's, taken as text (energy_pair.inc): every unordered pair
// once, bodies i in registers (packed pairs in fp32), bodies j through SCALAR loads from the constant address space, fp32 sums over
// one chunk only and then multiplied by m_i and folded into fp64, the O(N) terms in fp64, a fixed LDS tree per workgroup into one
// 128-byte record, a second kernel that adds a system's records in index order.  No atomics, no scratch.  What is new is the geometry:
//
//   * A workgroup belongs to ONE system; blockIdx.x = (system, block a of bodies i, split c).  The geometry is a function of
//     (N, precision) alone, so a system's bits do not depend on the batch.
//   * Bodies per lane I and waves per workgroup S follow the system's size (plan_energy_ensemble below), so that a 256-body system
//     fills its lanes' slots: a block is 64 * I bodies, and a chunk of bodies j -- a unit of work -- is 64 of them, never more.
//   * The diagonal block.  Slot k of the bodies i holds indices k*64 + lane of the block, a chunk holds 64 consecutive bodies j
//     starting at a multiple of 64: chunk q lies wholly above slots k < q (those run unmasked), wholly at or below slots k > q (those
//     are skipped), and straddles slot q alone (that one runs masked, j > i).  All three decisions are wave-uniform.  In fp32 a vector
//     holds two slots: the vectors below q / 2 run unmasked, vector q / 2 masked (its other slot is all-pass or all-fail under the
//     same mask), the vectors above it are skipped.
//   * Above one block per system: the solo tournament (block a meets a .. a + NB/2 mod NB) inside the system.
//
// Compiled with FMA contraction ON (default).
#include "../../include/nbody_hip_energy_ensemble.h"
#include "energy_ensemble_kernels.h"

namespace nb {
namespace {

#include "nbody_lane.h"
#include "energy_pair.inc"  // kFields, kRecord, tree_sum, inv_sqrt, sweep: shared with nbody_energy.hip

constexpr unsigned kUnit          = 64;   // bodies j per unit: the longest fp32 sum (the rule allows 128)
constexpr int      kMaxWaves      = 4;    // waves per workgroup at most
constexpr int      kMaxVectors    = 4;    // vectors of bodies i per lane at most (fp32: 8 bodies, fp64: 4)
constexpr int      kFinishThreads = 64;   // energy_ensemble_finish: one wave per system
constexpr int      kDriftThreads  = 256;  // energy_ensemble_drift_summary: one workgroup

// Chunk q of the diagonal block with NU = q / W: vectors [0, NU) unmasked, vector NU masked, the rest skipped.
template <typename T, int R, int NU, typename Stream>
__device__ __forceinline__ void diagonal_unit(Stream bodies, unsigned j0, unsigned j1, const typename Lane<T>::vec (&px)[R], const typename Lane<T>::vec (&py)[R],
                                              const typename Lane<T>::vec (&pz)[R], const unsigned (&idx)[R * Lane<T>::W], typename Lane<T>::vec eps2, typename Lane<T>::vec (&acc)[R]) {
    using vec       = typename Lane<T>::vec;
    constexpr int W = Lane<T>::W;
    if constexpr (NU > 0) {
        vec      qx[NU], qy[NU], qz[NU], qa[NU];
        unsigned qi[NU * W];
#pragma unroll
        for (int r = 0; r < NU; ++r) qx[r] = px[r], qy[r] = py[r], qz[r] = pz[r], qa[r] = acc[r];
#pragma unroll
        for (int k = 0; k < NU * W; ++k) qi[k] = idx[k];
        sweep<T, false, NU>(bodies, j0, j1, qx, qy, qz, qi, eps2, qa);
#pragma unroll
        for (int r = 0; r < NU; ++r) acc[r] = qa[r];
    }
    vec      qx[1] = {px[NU]}, qy[1] = {py[NU]}, qz[1] = {pz[NU]}, qa[1] = {acc[NU]};
    unsigned qi[W];
#pragma unroll
    for (int w = 0; w < W; ++w) qi[w] = idx[NU * W + w];
    sweep<T, true, 1>(bodies, j0, j1, qx, qy, qz, qi, eps2, qa);
    acc[NU] = qa[0];
}

// ... chosen by the wave-uniform nu = q / W
template <typename T, int R, int NU = 0, typename Stream>
__device__ __forceinline__ void diagonal(Stream bodies, unsigned nu, unsigned j0, unsigned j1, const typename Lane<T>::vec (&px)[R], const typename Lane<T>::vec (&py)[R],
                                         const typename Lane<T>::vec (&pz)[R], const unsigned (&idx)[R * Lane<T>::W], typename Lane<T>::vec eps2, typename Lane<T>::vec (&acc)[R]) {
    if (nu == NU) {
        diagonal_unit<T, R, NU>(bodies, j0, j1, px, py, pz, idx, eps2, acc);
    } else if constexpr (NU + 1 < R) {
        diagonal<T, R, NU + 1>(bodies, nu, j0, j1, px, py, pz, idx, eps2, acc);
    }
}

template <typename T, int R, int S> __global__ __launch_bounds__(64 * S) void energy_ensemble_pairs(EnergyEnsembleArgs<T> e) {
    using LT                  = Lane<T>;
    using vec                 = typename LT::vec;
    using vec4                = typename LT::vec4;
    using raw4                = typename LT::raw4;
    constexpr int      W      = LT::W;
    constexpr int      I      = R * W;
    constexpr unsigned B      = 64u * I;  // bodies of a block
    constexpr int      kThreads = 64 * S;
    static_assert(I % S == 0, "the O(N) terms of a block are whole passes of the workgroup");
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx4/x8

    const int      tid  = threadIdx.x;
    const int      wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int      lane = tid & 63;
    // consecutive workgroups go to different XCDs, and a group's work depends on (a, c): the groups of system `local` are taken in an
    // order rotated by `local`, so that no XCD is dealt the heavy groups of every system
    const unsigned local = blockIdx.x / e.groups;
    const unsigned turn  = blockIdx.x - local * e.groups + local % e.groups;
    const unsigned g     = turn < e.groups ? turn : turn - e.groups;
    const unsigned a     = g / e.splits;
    const unsigned c     = g - a * e.splits;
    const unsigned long long system = e.first_system + local;
    const size_t       off    = static_cast<size_t>(system) * 4 * e.n;  // (64-bit: 2^28 fp32 bodies are 4 GiB)
    const stream_ptr   bodies = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(e.pos + off));
    const vec4* const  pos4   = reinterpret_cast<const vec4*>(e.pos + off);
    const vec4* const  vel4   = reinterpret_cast<const vec4*>(e.vel + off);

    // bodies i of this lane: a*B + k*64 + lane of the system (k = r*W + w); a body past the end has mass 0 and is never folded
    vec      px[R], py[R], pz[R];
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
    vec eps2 = LT::splat(e.system_eps2 != nullptr ? e.system_eps2[static_cast<size_t>(system) * e.eps2_stride] : e.eps2);
    LT::keep_in_vgpr(eps2);

    double pot = 0;
    const unsigned half    = e.blocks / 2;
    // the units of block a are dealt out one by one, first over the C workgroups that share the block, then over their waves: the cheap
    // units (the low chunks of the diagonal) and the full ones are spread evenly
#pragma unroll 1
    for (unsigned u = c + e.splits * wave; u < e.units; u += e.splits * S) {
        const unsigned d = u / I, q = u % I;  // partner at distance d, its chunk q (a block is I units)
        if ((e.blocks & 1u) == 0 && d == half && d != 0 && a >= half) continue;  // (even NB: the pair at distance NB/2 is the lower block's)
        const unsigned b  = a + d < e.blocks ? a + d : a + d - e.blocks;
        const unsigned j0 = b * B + q * kUnit;
        if (j0 >= e.n) continue;
        const unsigned j1 = j0 + kUnit < e.n ? j0 + kUnit : e.n;
        vec acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = LT::splat(0);
        if (d == 0) diagonal<T, R>(bodies, q / W, j0, j1, px, py, pz, idx, eps2, acc);
        else        sweep<T, false, R>(bodies, j0, j1, px, py, pz, idx, eps2, acc);
#pragma unroll
        for (int k = 0; k < I; ++k) {
            if (idx[k] < e.n) pot = __builtin_fma(static_cast<double>(mi[k]), static_cast<double>(LT::get(acc[k / W], k % W)), pot);
        }
    }

    double v[kFields] = {};
    v[0] = pot;
    __shared__ double lds[kFields][kThreads];
    double* const record = e.records + (static_cast<size_t>(system) * e.groups + g) * kRecord;
    if (c == 0) {  // the O(N) terms of block a, in fp64
#pragma unroll
        for (unsigned s = 0; s < B / kThreads; ++s) {
            const unsigned i = a * B + s * kThreads + tid;
            if (i >= e.n) continue;
            const vec4   p = pos4[i], w = vel4[i];
            const double m = p.w, x = p.x, y = p.y, z = p.z, vx = w.x, vy = w.y, vz = w.z;
            v[1] += m * (vx * vx + vy * vy + vz * vz);
            v[2] += m;
            v[3] += m * vx, v[4] += m * vy, v[5] += m * vz;
            v[6] += m * (y * vz - z * vy), v[7] += m * (z * vx - x * vz), v[8] += m * (x * vy - y * vx);
            v[9] += m * x, v[10] += m * y, v[11] += m * z;
        }
        tree_sum(lds, v);
        if (tid < kFields) record[tid] = lds[tid][0];
    } else {  // the other workgroups of the block hold a potential sum and eleven zeros
        tree_sum<1>(lds, v);
        if (tid < kFields) record[tid] = tid == 0 ? lds[0][0] : 0.0;
    }
}

// One wave per system: thread t adds a contiguous run of the system's records in index order, then the fixed tree; thread 0 writes the result.
__global__ __launch_bounds__(kFinishThreads) void energy_ensemble_finish(const double* records, unsigned count, unsigned long long first_system, nb_energy_t* results) {
    const int                t      = threadIdx.x;
    const unsigned long long system = first_system + blockIdx.x;
    const double* const      mine   = records + static_cast<size_t>(system) * count * kRecord;
    const unsigned per   = (count + kFinishThreads - 1) / kFinishThreads;
    const unsigned first = t * per < count ? t * per : count;
    const unsigned last  = first + per < count ? first + per : count;
    double v[kFields] = {};
#pragma unroll 1
    for (unsigned r = first; r < last; ++r) {
#pragma unroll
        for (int f = 0; f < kFields; ++f) v[f] += mine[static_cast<size_t>(r) * kRecord + f];
    }
    __shared__ double lds[kFields][kFinishThreads];
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
        results[system] = res;
    }
}

// What a run of systems says about the drift; `lower` holds the lower indices, so a tie stays with it.
struct Drift {
    double   worst, sum_sq, momentum;  // worst / momentum < 0: none yet
    unsigned worst_system, momentum_system, finite, not_finite;
};
__device__ __forceinline__ Drift merged(const Drift& lower, const Drift& upper) {
    Drift r = lower;
    if (upper.worst > r.worst) r.worst = upper.worst, r.worst_system = upper.worst_system;
    if (upper.momentum > r.momentum) r.momentum = upper.momentum, r.momentum_system = upper.momentum_system;
    r.sum_sq += upper.sum_sq, r.finite += upper.finite, r.not_finite += upper.not_finite;
    return r;
}

// One workgroup: thread t takes a contiguous run of systems in index order, then a fixed tree of merges; thread 0 writes the 64 bytes.
__global__ __launch_bounds__(kDriftThreads) void energy_ensemble_drift_summary(const nb_energy_t* start, const nb_energy_t* end, unsigned systems, nb_energy_ensemble_drift_t* out) {
    const int      t     = threadIdx.x;
    const unsigned per   = (systems + kDriftThreads - 1) / kDriftThreads;
    const unsigned first = static_cast<unsigned long long>(t) * per < systems ? t * per : systems;
    const unsigned last  = per < systems - first ? first + per : systems;
    constexpr double inf = __builtin_huge_val();
    Drift mine{-1.0, 0.0, -1.0, 0u, 0u, 0u, 0u};
#pragma unroll 1
    for (unsigned s = first; s < last; ++s) {
        const double e0 = start[s].total, e1 = end[s].total;
        double       rel = __builtin_fabs(e1 - e0) / __builtin_fabs(e0);  // (0 / 0 and x / 0: not finite)
        const bool   finite = rel < inf;                                  // (false for a NaN too)
        if (finite) mine.sum_sq = __builtin_fma(rel, rel, mine.sum_sq), mine.finite += 1;
        else        rel = inf, mine.not_finite += 1;
        double mom = -1.0;
        for (int k = 0; k < 3; ++k) {
            const double dp = __builtin_fabs(end[s].momentum[k] - start[s].momentum[k]);
            if (dp > mom) mom = dp;
        }
        mine = merged(mine, Drift{rel, 0.0, mom, s, s, 0u, 0u});
    }
    __shared__ Drift lds[kDriftThreads];
    lds[t] = mine;
    __syncthreads();
#pragma unroll 1
    for (int s = 1; s < kDriftThreads; s <<= 1) {  // (neighbouring runs first: the lower run is always the left operand)
        if (t % (2 * s) == 0) lds[t] = merged(lds[t], lds[t + s]);
        __syncthreads();
    }
    if (t == 0) {
        const Drift all = lds[0];
        nb_energy_ensemble_drift_t r{};
        r.worst_relative_drift  = all.worst;
        r.rms_relative_drift    = all.finite != 0 ? __builtin_sqrt(all.sum_sq / static_cast<double>(all.finite)) : 0.0;
        r.worst_momentum_drift  = all.momentum < 0 ? 0.0 : all.momentum;
        r.systems               = systems;
        r.worst_system          = all.worst_system;
        r.worst_momentum_system = all.momentum_system;
        r.not_finite            = all.not_finite;
        *out = r;
    }
}

template <typename T, int R, int S> hipError_t launch_rs(const EnergyEnsembleArgs<T>& a, unsigned long long systems, hipStream_t stream) {
    if constexpr ((R * Lane<T>::W) % S != 0) {
        return hipErrorInvalidValue;
    } else {
        const unsigned long long per = ensemble_systems_per_launch(a.groups, 64 * S);
        for (unsigned long long first = 0; first < systems; first += per) {
            EnergyEnsembleArgs<T> part = a;
            part.first_system          = first;
            const unsigned long long count = systems - first < per ? systems - first : per;
            hipLaunchKernelGGL((energy_ensemble_pairs<T, R, S>), dim3(static_cast<unsigned>(count * a.groups)), dim3(64 * S), 0, stream, part);
            if (const auto err = hipGetLastError(); err != hipSuccess) return err;
        }
        return hipSuccess;
    }
}

}  // namespace

// Geometry.  I, the bodies i per lane: the largest power of two with 64 I <= N, so that a block has no empty slot, between one vector
// (fp32: a packed pair) and four (what nb_energy_* holds).  A block's work is (NB/2 + 1) I units of 64 bodies j.  S, the waves of a
// workgroup: the largest power of two up to 4 that leaves every wave two units.  C, the workgroups that share a block: a batch of
// 262 144 bodies in all has 4 096 / I blocks, and 4 096 waves put four on every SIMD (<= 128 VGPRs), so C S >= I -- as long as every
// wave keeps its two units.
template <typename T> EnergyEnsemblePlan plan_energy_ensemble(unsigned n) {
    constexpr int W = Lane<T>::W;
    int I = W;
    while (I < kMaxVectors * W && 64u * (2 * I) <= n) I *= 2;
    EnergyEnsemblePlan p{};
    p.bodies_per_lane = I;
    p.blocks          = (n + 64u * I - 1) / (64u * I);
    p.units           = (p.blocks / 2 + 1) * static_cast<unsigned>(I);
    int S = 1;
    while (S < kMaxWaves && static_cast<unsigned>(2 * S) * 2u <= p.units) S *= 2;
    p.waves           = S;
    const unsigned want = static_cast<unsigned>((I + S - 1) / S);
    const unsigned most = p.units / (2u * S) > 0 ? p.units / (2u * S) : 1;
    p.splits          = want < most ? want : most;
    p.groups          = p.blocks * p.splits;
    p.block_threads   = 64u * S;
    p.lds_bytes       = static_cast<unsigned>(kFields * sizeof(double)) * p.block_threads;
    return p;
}

template <typename T> hipError_t launch_energy_ensemble(const EnergyEnsembleArgs<T>& args, unsigned long long systems, const EnergyEnsemblePlan& p, hipStream_t stream) {
    constexpr int W = Lane<T>::W;
    if (p.groups > energy_ensemble_records(args.n)) return hipErrorInvalidValue;  // (the workspace holds that many records per system)
    EnergyEnsembleArgs<T> a = args;
    a.blocks = p.blocks, a.splits = p.splits, a.units = p.units, a.groups = p.groups;
    (void)hipGetLastError();  // (a launch reports its own error)
    hipError_t err;
    switch (p.waves * 16 + p.bodies_per_lane / W) {  // (S, R) of plan_energy_ensemble
        case 1 * 16 + 1: err = launch_rs<T, 1, 1>(a, systems, stream); break;
        case 2 * 16 + 1: err = launch_rs<T, 1, 2>(a, systems, stream); break;
        case 1 * 16 + 2: err = launch_rs<T, 2, 1>(a, systems, stream); break;
        case 2 * 16 + 2: err = launch_rs<T, 2, 2>(a, systems, stream); break;
        case 4 * 16 + 2: err = launch_rs<T, 2, 4>(a, systems, stream); break;
        case 2 * 16 + 4: err = launch_rs<T, 4, 2>(a, systems, stream); break;
        case 4 * 16 + 4: err = launch_rs<T, 4, 4>(a, systems, stream); break;
        default: return hipErrorInvalidValue;
    }
    if (err != hipSuccess) return err;
    const unsigned long long per = ensemble_systems_per_launch(1, kFinishThreads);
    for (unsigned long long first = 0; first < systems; first += per) {
        const unsigned long long count = systems - first < per ? systems - first : per;
        hipLaunchKernelGGL(energy_ensemble_finish, dim3(static_cast<unsigned>(count)), dim3(kFinishThreads), 0, stream, static_cast<const double*>(a.records), p.groups, first, a.results);
        if (err = hipGetLastError(); err != hipSuccess) return err;
    }
    return hipSuccess;
}

hipError_t launch_energy_ensemble_drift(const nb_energy_t* start, const nb_energy_t* end, unsigned systems, nb_energy_ensemble_drift_record* out, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(energy_ensemble_drift_summary, dim3(1), dim3(kDriftThreads), 0, stream, start, end, systems, out);
    return hipGetLastError();
}

template EnergyEnsemblePlan plan_energy_ensemble<float>(unsigned);
template EnergyEnsemblePlan plan_energy_ensemble<double>(unsigned);
template hipError_t launch_energy_ensemble<float>(const EnergyEnsembleArgs<float>&, unsigned long long, const EnergyEnsemblePlan&, hipStream_t);
template hipError_t launch_energy_ensemble<double>(const EnergyEnsembleArgs<double>&, unsigned long long, const EnergyEnsemblePlan&, hipStream_t);

}  // namespace nb
