// hermite6_kernels.h -- internal launch interface of libnbody_hip_hermite6.so (include/nbody_hip_hermite6.h) between its C-ABI unit
// (hermite6_capi.hip) and its kernel unit (hermite6_eval.hip, contraction on).
#pragma once

#include <hip/hip_runtime.h>

#include "wave_stream.h"

namespace nb {

// Index arithmetic as in hermite_kernels.h: body indices are `unsigned`, element offsets 64-bit.  2^26 bodies are a 6 GiB fp64 workspace.
inline constexpr unsigned kHermite6MaxBodies = 1u << 26;

// nb_hermite6_timestep_*: the first stage leaves at most this many partial minima (doubles) in the caller's scratch
inline constexpr unsigned kHermite6TimestepPartials = 1024;

// U of hermite6_eval: a body j is three vec4 -- 12 (fp32) / 24 (fp64) scalar registers --, and two register sets of U = 4 / 2 are 96 of
// the 102 a wave has.  Half that leaves the loop's addresses, counters and constants their registers.
template <typename T> constexpr int hermite6_unroll_for() { return sizeof(T) == 8 ? 1 : 2; }

// What hermite6_eval works on.  The bodies j AND the lane's own bodies i come from `state12` = T[12N] {x, y, z, m, vx, vy, vz, 0,
// ax, ay, az, 0}: the predicted state (STEP, nb_hermite6_step_*) or a copy of the caller's (nb_hermite6_eval_*, nb_hermite6_init_*).
// STEP: the stored state (old_pos, vel, acc, jerk, snap, crackle) is read and written by the body's own lane only.  Otherwise acc, jerk
// and snap are written and nothing else is touched.
template <typename T> struct Hermite6Args {
    const T* state12;
    T*       new_pos;  // STEP
    const T* old_pos;  // STEP (may equal new_pos)
    T*       vel;      // STEP, in place
    T*       acc;      // STEP: in place; !STEP: out
    T*       jerk;     // STEP: in place; !STEP: out
    T*       snap;     // STEP: in place; !STEP: out
    T*       crackle;  // STEP, in place
    unsigned n;
    T        dt;       // STEP
    T        eps2;     // > 0 (the C boundary replaces 0 by the floor of nbody_hip_hermite6.h)
};

inline constexpr int kHermite6Sums = 9;  // ax ay az jx jy jz sx sy sz: the sums of plan_stream (wave_stream.h), with hermite6_unroll_for<T>()

// workspace <- {pos, vel, acc_in} (acc_in == nullptr: zeros); `zero` (may be nullptr): T[4N] set to 0 by the same launch
template <typename T> hipError_t launch_hermite6_pack(T* workspace, const T* pos, const T* vel, const T* acc_in, T* zero, unsigned n, hipStream_t stream);
template <typename T> hipError_t launch_hermite6_eval(const Hermite6Args<T>& a, hipStream_t stream);
template <typename T> hipError_t launch_hermite6_step(const Hermite6Args<T>& a, T* workspace, hipStream_t stream);
template <typename T>
hipError_t launch_hermite6_timestep(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, T eta, T* dt_out, double* scratch, hipStream_t stream);

// The start of a 6th-order run, four launches: acc, jerk and snap of (pos, vel) and crackle = 0, through `state12` (T[12N]).
template <typename T> inline hipError_t launch_hermite6_start(T* acc, T* jerk, T* snap, T* crackle, const T* pos, const T* vel, T* state12, unsigned n, T eps2, hipStream_t stream) {
    Hermite6Args<T> a{};
    a.state12 = state12, a.acc = acc, a.jerk = jerk, a.snap = snap, a.n = n, a.eps2 = eps2;
    // a and jerk do not depend on the accelerations: a first pass with b = 0, a second with that a for the snap
    if (const auto err = launch_hermite6_pack<T>(state12, pos, vel, nullptr, nullptr, n, stream); err != hipSuccess) return err;
    if (const auto err = launch_hermite6_eval<T>(a, stream); err != hipSuccess) return err;
    if (const auto err = launch_hermite6_pack<T>(state12, pos, vel, acc, crackle, n, stream); err != hipSuccess) return err;
    return launch_hermite6_eval<T>(a, stream);
}

}  // namespace nb
