// hermite6_ensemble_kernels.h -- internal launch interface of libnbody_hip_hermite6_ensemble.so (include/nbody_hip_hermite6_ensemble.h)
// between its C-ABI unit (hermite6_ensemble_boundary.hip) and its kernel unit (hermite6_ensemble.hip, contraction on).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hermite6_kernels.h"          // hermite6_unroll_for
#include "hermite_ensemble_kernels.h"  // for its types and constants alone: EnsembleClock, EnsembleStatus, EnsembleSource, the limits, the partials

namespace nb {

// What hermite6_ensemble_eval works on: Hermite6Args of hermite6_kernels.h for B systems.  Every array holds system s at [s N, (s + 1) N);
// state12 is T[12 N B], the predicted state (STEP) or a copy of the caller's.  dt and softening^2 are the system's own (src).
template <typename T> struct EnsembleHermite6Args {
    const T*          state12;
    T*                new_pos;  // STEP
    const T*          old_pos;  // STEP (may equal new_pos)
    T*                vel;      // STEP, in place
    T*                acc;      // STEP: in place; !STEP: out
    T*                jerk;     // STEP: in place; !STEP: out
    T*                snap;     // STEP: in place; !STEP: out
    T*                crackle;  // STEP, in place
    unsigned          n;        // bodies per system
    unsigned          groups_per_system;
    EnsembleSource<T> src;
};

// state12 <- {pos, vel, acc_in} of every system (acc_in == nullptr: zeros); `zero` (may be nullptr): T[4 N B] set to 0 by the same launch
template <typename T> hipError_t launch_ensemble6_pack(T* state12, const T* pos, const T* vel, const T* acc_in, T* zero, unsigned n, unsigned b, hipStream_t stream);
template <typename T> hipError_t launch_ensemble6_eval(const EnsembleHermite6Args<T>& a, unsigned b, hipStream_t stream);
template <typename T> hipError_t launch_ensemble6_step(const EnsembleHermite6Args<T>& a, unsigned b, T* state12, hipStream_t stream);
// partial minima of every system's Aarseth ratio -> partial[b * ensemble_partials(n)]; then per system: dt_out[s] = (T)(eta sqrt(min))
// (dt_out != nullptr), or the clock of the system begun (begin) / advanced by the rule of the header (src.clocks != nullptr), with one partial
// status record per kEnsembleClockSystems systems; then (status != nullptr) the records summed into status.
template <typename T>
hipError_t launch_ensemble6_clocks(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, unsigned b, T eta, T* dt_out, EnsembleClock* clocks, bool begin,
                                   const EnsembleSource<T>& src, double* partial, EnsembleStatus* block_status, EnsembleStatus* status, hipStream_t stream);

// launch_hermite6_start (hermite6_kernels.h) for every system, through `state12` (T[12 N B]); softening^2 is the system's own.
template <typename T>
inline hipError_t launch_ensemble6_start(T* acc, T* jerk, T* snap, T* crackle, const T* pos, const T* vel, T* state12, unsigned n, unsigned b, T eps2, const T* system_eps2,
                                         hipStream_t stream) {
    EnsembleHermite6Args<T> a{};
    a.state12 = state12, a.acc = acc, a.jerk = jerk, a.snap = snap, a.n = n, a.src.eps2 = eps2, a.src.system_eps2 = system_eps2;
    // a and jerk do not depend on the accelerations: a first pass with b = 0, a second with that a for the snap
    if (const auto err = launch_ensemble6_pack<T>(state12, pos, vel, nullptr, nullptr, n, b, stream); err != hipSuccess) return err;
    if (const auto err = launch_ensemble6_eval<T>(a, b, stream); err != hipSuccess) return err;
    if (const auto err = launch_ensemble6_pack<T>(state12, pos, vel, acc, crackle, n, b, stream); err != hipSuccess) return err;
    return launch_ensemble6_eval<T>(a, b, stream);
}

}  // namespace nb
