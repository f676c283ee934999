// ensemble_strict.hip -- NB_MODE_STRICT of libnbody_hip_ensemble.so: every system of the batch bit-identical to nb_integrate_*
// STRICT on that system alone.  gfx950 only.
//
// MUST be compiled with nbody_strict.o's flags (csrc/Makefile): the kernel body is the product's own
// (nbody_strict_step.inc), handed the Shard of one system.  Its results do not depend on the launch geometry (each lane streams
// every body j of its system in order), so the geometry is picked for occupancy alone; the operand-window checks of the fast forms
// see the system's own softening^2.
#include "ensemble_kernels.h"

namespace nb {
namespace {

#include "nbody_strict_body.h"

// A workgroup never holds bodies of two systems: workgroup g steps workgroup g % groups of its system (ensemble_shard).
template <typename T> __global__ __launch_bounds__(512, 4) void ensemble_strict(EnsembleArgs<T> a) {
    unsigned       block;
    const Shard<T> s = ensemble_shard(a, block);
#include "nbody_strict_step.inc"
}

}  // namespace

// Workgroups of 64 .. 256 threads, the smallest power of two that covers a system (fp64 rings of 256 threads stay within 64 KiB
// of LDS: no opt-in call on the launch path).
template <typename T> hipError_t launch_ensemble_strict(const EnsembleArgs<T>& a, unsigned long long systems, hipStream_t stream) {
    unsigned p = 64;
    while (p < 256 && p < a.n) p *= 2;
    const unsigned groups = (a.n + p - 1) / p;
    const size_t   smem   = static_cast<size_t>(p / 64) * 2 * kChunk * 4 * sizeof(T) + 256;  // the waves' rings + progress words
    const unsigned long long per = ensemble_systems_per_launch(groups, p);
    (void)hipGetLastError();  // a launch reports ITS OWN error
    for (unsigned long long first = 0; first < systems; first += per) {
        EnsembleArgs<T> part = a;
        part.groups          = groups;
        part.first_system    = first;
        const unsigned long long count = systems - first < per ? systems - first : per;
        hipLaunchKernelGGL(ensemble_strict<T>, dim3(static_cast<unsigned>(count * groups)), dim3(p), smem, stream, part);
        if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    }
    return hipSuccess;
}

template hipError_t launch_ensemble_strict<float>(const EnsembleArgs<float>&, unsigned long long, hipStream_t);
template hipError_t launch_ensemble_strict<double>(const EnsembleArgs<double>&, unsigned long long, hipStream_t);

}  // namespace nb
