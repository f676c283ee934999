// ensemble_kernels.h -- internal launch interface of libnbody_hip_ensemble.so (include/nbody_hip_ensemble.h) between its C-ABI unit
// (ensemble_capi.hip) and its two kernel units: ensemble_strict.hip (nbody_strict.o's flags: bit-reproduction of the CPU path) and
// ensemble_fast.hip (contraction on).  Each kernel unit includes the product's kernel body (nbody_strict_step.inc /
// nbody_fast_stream.inc) and hands it the Shard of one system.
#pragma once

#include "nbody_kernels.h"

namespace nb {

inline constexpr unsigned kEnsembleMaxBodies = 65536;             // N per system
inline constexpr unsigned long long kEnsembleMaxTotal = 1ull << 31;  // N * B

// One launch over systems [first_system, first_system + grid / groups): workgroup g steps workgroup g % groups of system
// first_system + g / groups.  (A call whose grid would pass 2^31 threads is cut into several launches.)
template <typename T> struct EnsembleArgs {
    T*                 new_pos;
    const T*           old_pos;
    T*                 vel;
    const T*           params;        // T[4*B] {dt, damping, eps2, -} per system, or null: the three below
    unsigned           n;             // bodies per system
    unsigned           groups;        // workgroups per system
    unsigned long long first_system;
    T                  dt, damping, eps2;
};

// The Shard of the system workgroup `blockIdx.x` belongs to (64-bit offsets: 2^28 fp32 bodies are 4 GiB) and the workgroup's index
// within that system's grid
template <typename T> __device__ __forceinline__ Shard<T> ensemble_shard(const EnsembleArgs<T>& a, unsigned& block) {
    const unsigned           local  = blockIdx.x / a.groups;
    const unsigned long long system = a.first_system + local;
    block                           = blockIdx.x - local * a.groups;
    const size_t off                = static_cast<size_t>(system) * 4 * a.n;
    Shard<T> s;
    s.new_pos = a.new_pos + off;
    s.old_pos = a.old_pos + off;
    s.vel     = a.vel + off;
    s.acc     = nullptr;
    s.i_begin = 0, s.i_count = a.n, s.j_begin = 0, s.j_count = a.n;
    s.acc_in = false, s.finalize = true;
    if (a.params != nullptr) {
        const T* p = a.params + 4 * system;
        s.dt = p[0], s.damping = p[1], s.eps2 = p[2];
    } else {
        s.dt = a.dt, s.damping = a.damping, s.eps2 = a.eps2;
    }
    return s;
}

// the FAST geometry: a function of (n, precision) alone
struct EnsemblePlan {
    int      bodies_per_lane;  // I
    int      waves;            // S
    unsigned groups;           // workgroups per system
    unsigned block_threads;
    unsigned lds_bytes;
};
template <typename T> EnsemblePlan plan_ensemble_fast(unsigned n);
template <typename T> hipError_t   launch_ensemble_fast(const EnsembleArgs<T>& a, unsigned long long systems, const EnsemblePlan& p, hipStream_t stream);
template <typename T> hipError_t   launch_ensemble_strict(const EnsembleArgs<T>& a, unsigned long long systems, hipStream_t stream);

// grid x of one launch holds at most 2^31 threads: systems per launch for workgroups of `threads` threads, `groups` per system
inline unsigned long long ensemble_systems_per_launch(unsigned groups, unsigned threads) {
    const unsigned long long blocks = (1ull << 31) / threads;
    const unsigned long long per    = blocks / groups;
    return per > 0 ? per : 1;
}

}  // namespace nb
