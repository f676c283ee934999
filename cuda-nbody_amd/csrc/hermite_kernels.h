// hermite_kernels.h -- internal launch interface of libnbody_hip_hermite.so (include/nbody_hip_hermite.h) between its C-ABI unit
// (hermite_capi.hip) and its kernel unit (hermite_eval.hip, contraction on).
#pragma once

#include <hip/hip_runtime.h>

#include "wave_stream.h"

namespace nb {

// Index arithmetic: body indices are `unsigned`, element offsets 64-bit; a launch holds N / (64 W) workgroups of at most 512
// threads (<= 2^31 threads up to 2^28 bodies).  2^26 bodies are a 4 GiB fp64 workspace; the library refuses beyond that.
inline constexpr unsigned kHermiteMaxBodies = 1u << 26;

// nb_hermite_timestep_*: the first stage leaves at most this many partial minima (doubles) in the caller's scratch
inline constexpr unsigned kTimestepPartials = 1024;

// What hermite_eval works on.  STEP (nb_hermite_step_*): the bodies j and the lane's own predicted state come from the workspace
// `state8` = T[8N] {x, y, z, m, vx, vy, vz, 0}; the stored state (old_pos, vel, acc, jerk) is read and written by the body's own
// lane only.  Otherwise (nb_hermite_eval_*): bodies come from `pos` and `vel_in`, acc and jerk are written, nothing else is touched.
template <typename T> struct HermiteArgs {
    const T* state8;   // STEP: predicted state
    const T* pos;      // !STEP: positions T[4N]
    const T* vel_in;   // !STEP: velocities T[4N]
    T*       new_pos;  // STEP
    const T* old_pos;  // STEP (may equal new_pos)
    T*       vel;      // STEP, in place
    T*       acc;      // STEP: in place; !STEP: out
    T*       jerk;     // STEP: in place; !STEP: out
    unsigned n;
    T        dt;       // STEP
    T        eps2;     // > 0 (the C boundary replaces 0 by the floor of nbody_hip_hermite.h)
};

inline constexpr int kHermiteSums = 6;  // ax ay az jx jy jz: the sums of plan_stream (wave_stream.h), with unroll_for<T>()

template <typename T> hipError_t launch_hermite_eval(const HermiteArgs<T>& a, hipStream_t stream);
template <typename T> hipError_t launch_hermite_step(const HermiteArgs<T>& a, T* workspace, hipStream_t stream);
template <typename T> hipError_t launch_hermite_timestep(const T* acc, const T* jerk, unsigned n, T eta, T* dt_out, double* scratch, hipStream_t stream);

}  // namespace nb
