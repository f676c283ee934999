/*
 * nbody_hip_energy_ensemble.h -- energy, momentum and angular momentum of EVERY system of an ensemble in one call
 * (libnbody_hip_energy_ensemble.so), and the drift between two such measurements folded into 64 bytes.
 *
 * The ensemble libraries (nbody_hip_ensemble.h, the 4th- and 6th-order Hermite ensembles, each with shared and block time steps) step
 * B independent systems of N bodies in one launch.  nb_energy_* of nbody_hip.h measures one system per call, in two launches, with a
 * geometry made for large systems; B calls of it are launch-bound.  The calls below measure the whole batch in two launches and say
 * which system of it went wrong.
 *
 * This library links none of the others and has no process-global state: softening^2 is an argument.  It exports exactly the six entry
 * points below.  Error codes are the NB_ERR_* / hipError_t values of nbody_hip.h; nb_error_string() of libnbody_hip.so names them.
 *
 * Layout: the ensembles' own.  B systems of N bodies each; system s holds bodies [s*N, (s+1)*N) of
 *   positions  T[4*N*B] = {x, y, z, mass} per body
 *   velocities T[4*N*B] = {vx, vy, vz, w} per body (.w is ignored)
 * Both are only read, and nothing past element 4*N*B of either is read.  Zero-mass padding bodies contribute nothing when eps^2 > 0 or
 * when they coincide with no body (below: Operand range).
 *
 * What one call computes.  device_results[s] is exactly the nb_energy_t (104 bytes) nb_energy_* gives for system s alone, with the
 * same definitions: the Plummer potential -sum_{i<j} m_i m_j / sqrt(|p_i - p_j|^2 + eps^2) over the pairs of that system, the i = j
 * term masked (not subtracted), G = 1.  NO SOFTENING FLOOR: eps^2 is used as given.  The Hermite kernels replace a softening^2 of 0
 * by a floor of their own; this potential does not, so with eps^2 == 0 two bodies at one place give an infinite potential here.
 * fp32 sums never run over more than 64 bodies j before they are multiplied by m_i and folded into fp64; the O(N) terms are fp64.
 *
 * Operand range.  That of nb_energy_* (nbody_hip.h, "Operand range"), system by system.  One pair's term m_i m_j / sqrt(d^2 + eps^2)
 * is held (tests/test_fast_domain.py, tests/test_energy_domain.py) to 1e-6 (fp32) / 1e-14 (fp64) of its magnitude for
 * d^2 + eps^2 in [2^-83, 2^84] (fp32) / [2^-599, 2^601] (fp64), the range the tests cover; outside it nothing is clamped.  In every
 * geometry of nb_energy_ensemble_plan_* every unordered pair and every body's O(N) terms are counted exactly once: a system in
 * which only two bodies, or one, have a mass gives the bits of those bodies alone.  fp32 sums run over at most
 * 128 (nb_energy_f32) / 64 (nb_energy_ensemble_f32) bodies j.
 * Non-finite inputs are ordinary data, and no other system of the batch changes a bit.  A NaN coordinate makes its system's
 * potential, total, that component of the centre of mass and the other two components of the angular momentum NaN, and nothing
 * else.  An infinite mass makes the kinetic energy, the mass and every component of the momentum and the angular momentum infinite,
 * and the potential (its own masked i = j term is m * 0), the total and the centre of mass NaN.  A NaN velocity component reaches the
 * kinetic energy, the total, that component of the momentum and the other two of the angular momentum; the potential, the mass and
 * the centre of mass keep their bits.  Zero-mass bodies contribute nothing when eps^2 > 0 or when they coincide with no body; a
 * zero-mass body ON another body with eps^2 == 0 is 0 * inf = NaN in the potential and the total, so pad with bodies that lie apart,
 * or soften.
 *
 * Softening.  system_softening_sq == NULL: every system uses softening_sq.  Otherwise system s reads
 * system_softening_sq[s * softening_stride] (device memory, softening_stride >= 1) and the scalar is ignored.  Stride 1 is the
 * Hermite ensembles' T[B]; stride 4 with the pointer at system_params + 2 is nb_ensemble_integrate_*'s {dt, damping, eps^2, -}.
 *
 * Ownership.  The caller owns all memory.  A call allocates nothing, takes no lock, never synchronises and is asynchronous on
 * `stream`, so it may sit between steps or inside a caller's graph capture.  nb_energy_ensemble_workspace_bytes says how much device
 * scratch memory a call needs, for either precision (pure host logic; one 128-byte fp64 record per workgroup; it grows no faster
 * than N*B).  Nothing outside workspace[0, that many bytes) and the B results is written.
 *
 * Reproducibility.  The 104 bytes of system s depend on that system's bodies, N, the precision and eps^2 only -- not on B, on s, on
 * the other systems, on the stream, on what the workspace held before or on the device: the geometry (nb_energy_ensemble_plan_*) is a
 * function of (N, precision) alone but for the grid, and every sum has a fixed order (no atomics).
 *
 * Limits.  1 <= N <= 65 536, B >= 1, N*B <= 2^31.
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null pointer (system_softening_sq may be null); N, B or
 * softening_stride out of range; workspace_bytes below the query's answer; a body array not aligned to 4*sizeof(T), a workspace,
 * result or summary array not aligned to 8 bytes, a softening array not aligned to sizeof(T); the workspace, the results or the
 * softening array overlapping a body array or each other.  Otherwise the launch's hipError_t (0 on success).
 */
#ifndef NBODY_HIP_ENERGY_ENSEMBLE_H
#define NBODY_HIP_ENERGY_ENSEMBLE_H

#include "nbody_hip.h" /* nb_energy_t, nb_stream_t, NB_ERR_*; error names: nb_error_string */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nb_energy_ensemble_plan { /* the geometry of a measurement */
    int                bodies_per_lane;   /* bodies i a lane holds; a block of bodies i is 64 * bodies_per_lane of them             */
    int                waves_per_group;   /* waves of a workgroup: they share the bodies i and split the chunks of bodies j         */
    unsigned           groups_per_system; /* workgroups one system occupies: its blocks x the workgroups that share a block         */
    unsigned           block_threads;
    unsigned           lds_bytes;
    unsigned           reserved;
    unsigned long long grid_blocks;       /* groups_per_system * num_systems                                                        */
} nb_energy_ensemble_plan_t;

/* Every field but grid_blocks is a function of (num_bodies, precision) alone.  NB_ERR_INVALID_ARGUMENT for what the measurement
 * refuses: sizes out of range, plan == NULL. */
NB_API int nb_energy_ensemble_plan_f32(unsigned num_bodies, unsigned num_systems, nb_energy_ensemble_plan_t* plan);
NB_API int nb_energy_ensemble_plan_f64(unsigned num_bodies, unsigned num_systems, nb_energy_ensemble_plan_t* plan);

NB_API int nb_energy_ensemble_workspace_bytes(unsigned num_bodies, unsigned num_systems, size_t* bytes);

/* The nb_energy_t of every system into device_results[0 .. num_systems) (see above). */
NB_API int nb_energy_ensemble_f32(const float* positions, const float* velocities, unsigned num_bodies, unsigned num_systems,
                                  float softening_sq, const float* system_softening_sq, unsigned softening_stride,
                                  void* workspace, size_t workspace_bytes, nb_energy_t* device_results, nb_stream_t stream);
NB_API int nb_energy_ensemble_f64(const double* positions, const double* velocities, unsigned num_bodies, unsigned num_systems,
                                  double softening_sq, const double* system_softening_sq, unsigned softening_stride,
                                  void* workspace, size_t workspace_bytes, nb_energy_t* device_results, nb_stream_t stream);

/* What a batch did to its energy between two measurements, in 64 bytes of device memory: a host reads 64 bytes per check, not 104*B.
 * The relative drift of system s is |total_end - total_start| / |total_start|.  A system whose drift is not finite (a NaN or an
 * infinity in either total, or total_start == 0) counts as the worst and is counted in not_finite; worst_relative_drift is then
 * +infinity.  Ties go to the lowest index.  A momentum drift that is NaN takes no part in worst_momentum_drift. */
typedef struct nb_energy_ensemble_drift_record {
    double             worst_relative_drift;  /* max_s |dE_s| / |E0_s|                                                            */
    double             rms_relative_drift;    /* sqrt(mean of the squares) over the systems whose drift is finite; 0 without any   */
    double             worst_momentum_drift;  /* max_s max_k |momentum_end[k] - momentum_start[k]|                                 */
    unsigned           systems;
    unsigned           worst_system;          /* where worst_relative_drift is                                                     */
    unsigned           worst_momentum_system; /* where worst_momentum_drift is                                                     */
    unsigned           not_finite;            /* systems without a finite relative drift                                           */
    unsigned long long reserved[3];
} nb_energy_ensemble_drift_t;                 /* 64 bytes */

/* start, end: two device arrays of num_systems results (they may be the same array); device_summary: 64 bytes of device memory.  One
 * workgroup, a fixed order, no atomics: the same bytes on every call.  NB_ERR_INVALID_ARGUMENT: a null pointer, num_systems == 0, an
 * array not aligned to 8 bytes, device_summary overlapping start or end. */
NB_API int nb_energy_ensemble_drift(const nb_energy_t* start, const nb_energy_t* end, unsigned num_systems,
                                    nb_energy_ensemble_drift_t* device_summary, nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_ENERGY_ENSEMBLE_H */
