// hermite_ensemble_kernels.h -- internal launch interface of libnbody_hip_hermite_ensemble.so (include/nbody_hip_hermite_ensemble.h)
// between its C-ABI unit (hermite_ensemble_capi.hip) and its kernel unit (hermite_ensemble.hip, contraction on).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hermite_kernels.h"  // kHermiteSums

namespace nb {

inline constexpr unsigned kEnsembleHermiteMaxBodies = 65536;     // per system: above it one system fills the chip (nb_hermite_*)
inline constexpr unsigned kEnsembleHermiteMaxTotal  = 1u << 28;  // N * B
inline constexpr unsigned kEnsembleTimestepBodies   = 256;       // bodies behind one partial minimum
inline constexpr unsigned kEnsembleClockSystems     = 256;       // systems behind one partial status record

inline constexpr std::uint32_t kClockDone = 1, kClockStalled = 2;

// nb_hermite_ensemble_clock_t / nb_hermite_ensemble_status_t of the header, as the kernels see them
struct EnsembleClock {
    double        time, dt_next, dt_last;
    std::uint32_t steps, flags;
};
struct EnsembleStatus {
    std::uint32_t      systems, done, stalled, stepped;
    unsigned long long total_steps;
    double             min_time, min_dt_last;
    unsigned long long reserved[3];
};
static_assert(sizeof(EnsembleClock) == 32 && sizeof(EnsembleStatus) == 64, "the records of the header");

// Where a system's time step and softening^2 come from.  clocks != nullptr (nb_hermite_ensemble_advance_*): dt is derived from the system's
// clock, t_stop and dt_max (clock_decision); else params != nullptr: {dt, eps2, -, -} per system; else the scalars.  eps2 per system comes
// from params, else from system_eps2, else the scalar; 0 takes the floor of nbody_hip_hermite.h, per system, on the device.
template <typename T> struct EnsembleSource {
    const EnsembleClock* clocks;
    const T*             params;       // T[4B] or nullptr
    const T*             system_eps2;  // T[B] or nullptr
    double               t_stop, dt_max;
    T                    dt, eps2;
};

// What hermite_ensemble_eval works on: HermiteArgs of hermite_kernels.h for B systems.  Every array holds system s at [s N, (s + 1) N).
template <typename T> struct EnsembleHermiteArgs {
    const T*          state8;   // STEP: predicted state T[8 N B]
    const T*          pos;      // !STEP
    const T*          vel_in;   // !STEP
    T*                new_pos;  // STEP
    const T*          old_pos;  // STEP (may equal new_pos)
    T*                vel;      // STEP, in place
    T*                acc;
    T*                jerk;
    unsigned          n;        // bodies per system
    unsigned          groups_per_system;
    EnsembleSource<T> src;
};

// doubles of partial minima per system, and the layout of the workspace behind the predicted state
inline unsigned ensemble_partials(unsigned n) { return (n + kEnsembleTimestepBodies - 1) / kEnsembleTimestepBodies; }
inline unsigned ensemble_status_blocks(unsigned b) { return (b + kEnsembleClockSystems - 1) / kEnsembleClockSystems; }

// The geometry of one system is the solo call's, plan_stream (wave_stream.h) of (N, precision) alone; B only sets the grid, groups * B.
template <typename T> hipError_t launch_ensemble_eval(const EnsembleHermiteArgs<T>& a, unsigned b, hipStream_t stream);
template <typename T> hipError_t launch_ensemble_step(const EnsembleHermiteArgs<T>& a, unsigned b, T* state8, hipStream_t stream);
// partial minima of every system -> partial[b * ensemble_partials(n)]; then per system: dt_out[s] = eta (T)min (dt_out != nullptr),
// or the clock of the system begun (begin) / advanced by the rule of the header (src.clocks != nullptr), with one partial status record per
// kEnsembleClockSystems systems; then (status != nullptr) the records summed into status.
template <typename T>
hipError_t launch_ensemble_clocks(const T* acc, const T* jerk, unsigned n, unsigned b, T eta, T* dt_out, EnsembleClock* clocks, bool begin, const EnsembleSource<T>& src,
                                  double* partial, EnsembleStatus* block_status, EnsembleStatus* status, hipStream_t stream);

}  // namespace nb
