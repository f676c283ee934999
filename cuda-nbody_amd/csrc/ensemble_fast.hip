// ensemble_fast.hip -- NB_MODE_FAST of libnbody_hip_ensemble.so: the one-sided wave-stream layout of nbody_fast.hip, one system per
// workgroup.  gfx950 only; compiled with FMA contraction on.
//
// The kernel body is the product's own (nbody_fast_stream.inc), handed the Shard of one system: the bodies i sit in packed pairs per
// lane (Lane<T>), the bodies j of the system are wave-uniform and come in through scalar loads, the S waves of a workgroup split j
// and fold their partial sums through LDS in a fixed order; no atomics on the sums, no scratch, <= 128 VGPRs.  Each system's sums are
// kept in units of its own first body's mass (reference_mass, within usable_unit's window), with the per-chunk unit, species and
// mixed forms of nbody_fast.hip.  The geometry is a function of (N, precision) alone, so a system's bits do not depend on the batch.
#include "ensemble_kernels.h"

namespace nb {
namespace {

constexpr int block_threads_for(int S) { return 64 * S; }

#include "nbody_lane.h"
#include "nbody_fast_stream.h"

constexpr int kEnsembleLpt = 2;  // 128 bodies j per wave and chunk

template <typename T, int R, int S> __global__ __launch_bounds__(block_threads_for(S)) __attribute__((amdgpu_waves_per_eu(4, 4))) void ensemble_fast(EnsembleArgs<T> a) {
    constexpr int LPT = kEnsembleLpt;
    unsigned       block;
    const Shard<T> s = ensemble_shard(a, block);
#include "nbody_fast_stream.inc"
}

template <typename T, int R, int S> hipError_t launch_rs(const EnsembleArgs<T>& a, unsigned long long systems, const EnsemblePlan& p, hipStream_t stream) {
    const unsigned long long per = ensemble_systems_per_launch(p.groups, p.block_threads);
    (void)hipGetLastError();  // a launch reports ITS OWN error
    for (unsigned long long first = 0; first < systems; first += per) {
        EnsembleArgs<T> part = a;
        part.groups          = p.groups;
        part.first_system    = first;
        const unsigned long long count = systems - first < per ? systems - first : per;
        hipLaunchKernelGGL((ensemble_fast<T, R, S>), dim3(static_cast<unsigned>(count * p.groups)), dim3(block_threads_for(S)), p.lds_bytes, stream, part);
        if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace

// Geometry.  The goal: a batch of 262 144 bodies in all puts at least 4 waves on every SIMD (256 CUs x 4 SIMDs x 4 = 4 096 waves at
// 128 VGPRs) for N from 256 to 16 384, while every wave still streams at least one chunk of 128 bodies j.  Such a batch has
// 262 144 / (64 I) workgroups of S waves, 4 096 S / I waves: S >= I.  Each wave streams N / S bodies j: S <= N / 128.  So S is the
// largest power of two up to 8 with S <= N / 128 (1 below 256 bodies), and I = min(S, 4) bodies i per lane, at least one vector
// (fp32: a packed pair).  From 1 024 bodies this is the product's production geometry (I = 4, S = 8).
template <typename T> EnsemblePlan plan_ensemble_fast(unsigned n) {
    constexpr int W = Lane<T>::W;
    int           S = 1;
    while (S < 8 && static_cast<unsigned>(2 * S) * 128u <= n) S *= 2;
    int I = S < 4 ? S : 4;
    if (I < W) I = W;
    EnsemblePlan p;
    p.bodies_per_lane = I;
    p.waves           = S;
    p.block_threads   = static_cast<unsigned>(block_threads_for(S));
    p.groups          = (n + 64u * I - 1) / (64u * I);
    const size_t red  = static_cast<size_t>(S - 1) * 3 * I * 64 * sizeof(T);  // the fold of the S partial sums
    p.lds_bytes       = static_cast<unsigned>(red) + 256u;                    // + the waves' progress words
    if (sizeof(T) == 4) p.lds_bytes += static_cast<unsigned>(S) * 3 * I * 64 * sizeof(T);  // + fp32: the lanes' second-level sums
    return p;
}

template <typename T> hipError_t launch_ensemble_fast(const EnsembleArgs<T>& a, unsigned long long systems, const EnsemblePlan& p, hipStream_t stream) {
    constexpr int W = Lane<T>::W;
    switch (p.waves * 16 + p.bodies_per_lane / W) {  // (S, R) of plan_ensemble_fast
        case 1 * 16 + 1: return launch_rs<T, 1, 1>(a, systems, p, stream);
        case 2 * 16 + 2 / W: return launch_rs<T, 2 / W, 2>(a, systems, p, stream);
        case 4 * 16 + 4 / W: return launch_rs<T, 4 / W, 4>(a, systems, p, stream);
        case 8 * 16 + 4 / W: return launch_rs<T, 4 / W, 8>(a, systems, p, stream);
        default: return hipErrorInvalidValue;
    }
}

template EnsemblePlan plan_ensemble_fast<float>(unsigned);
template EnsemblePlan plan_ensemble_fast<double>(unsigned);
template hipError_t   launch_ensemble_fast<float>(const EnsembleArgs<float>&, unsigned long long, const EnsemblePlan&, hipStream_t);
template hipError_t   launch_ensemble_fast<double>(const EnsembleArgs<double>&, unsigned long long, const EnsemblePlan&, hipStream_t);

}  // namespace nb
