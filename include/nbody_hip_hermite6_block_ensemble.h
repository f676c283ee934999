/*
 * nbody_hip_hermite6_block_ensemble.h -- 6th-order Hermite steps with BLOCK TIME STEPS of many independent N-body systems of one size,
 * one launch per stage whatever the number of systems (libnbody_hip_hermite6_block_ensemble.so).
 *
 * nb_hermite6_block_* (nbody_hip_hermite6_block.h) needs a quarter of the 4th-order scheme's block steps at a sixth of its energy error,
 * but a block step with few active bodies is a handful of launches around very little arithmetic, and a study of many small systems
 * pays them one system after the other.  nb_hermite_block_ensemble_* (nbody_hip_hermite_block_ensemble.h) shares those launches among B
 * systems, but is 4th order.  Here B systems take 6th-order block steps together: it is nb_hermite6_block_* per system on
 * nb_hermite_block_ensemble_*'s terms.  Every system has its own time, its own active set and its own status record, and one call is five
 * launches for all of them.
 *
 * This library links none of the other libraries and has no process-global state.  Error codes are the NB_ERR_* / hipError_t values of
 * nbody_hip.h.  The parameter and status records are those of nbody_hip_hermite_block.h; the plan and summary records and the limits
 * NB_HERMITE_BLOCK_ENSEMBLE_MAX_BODIES and NB_HERMITE_BLOCK_ENSEMBLE_MAX_TOTAL are the types and constants of
 * nbody_hip_hermite_block_ensemble.h, which is included for them alone: no function of that library is needed, and no struct is declared here.
 *
 * Layout.  B systems of N bodies each, as nbody_hip_hermite_block_ensemble.h lays them out: system s owns bodies [s*N, (s+1)*N) of every
 * array, all caller-owned device arrays, T = float | double:
 *   positions, velocities, accelerations, jerks, snaps, crackles   T[4*N*B] each, the fields of nbody_hip_hermite6.h; velocities.w is preserved
 *   ticks      uint64[N*B]   the time of the body's stored state, in ticks
 *   levels     int32[N*B]    the body's level
 *   status     nb_hermite_block_status_t[B] (64 bytes each), one per system
 *   workspace  nb_hermite6_block_ensemble_workspace_bytes(N, B, sizeof T) = B * workspace_stride bytes; content before a call does not
 *              matter, nothing is kept in it between calls.  System s owns [s * workspace_stride, (s + 1) * workspace_stride): the
 *              predicted state {x, y, z, m, vx, vy, vz, 0, ax, ay, az, 0} of its bodies (its first 12*N T), the partial planes
 *              [J][9][slots] (at partial_offset), its active list, the schedule's counts and minima, one control record.  init alone
 *              uses the FRONT of the workspace as one contiguous T[12*N*B] for the packed state of its evaluation passes
 *              (B * workspace_stride >= 12*N*B*sizeof T); it is free, since nothing is kept in the workspace between calls.
 * One nb_hermite_block_params_t and one t_stop hold for all systems.  Softening: system_softening_sq == NULL: every system uses
 * softening_sq; otherwise it is a device array T[B] of softening^2 per system and the scalar is ignored.  A value of 0 takes the floor of
 * nbody_hip_hermite.h, per system, on the device.  Systems of different sizes: pad with bodies of mass +0 behind the real ones, as
 * nbody_hip_hermite_ensemble.h describes.
 *
 * The scheme is nbody_hip_hermite6_block.h's, unchanged ("THE SCHEME" there): levels, ticks, the 6th-order predictor to the crackle, the
 * corrector with h = dt_i, dt_A = sqrt(eta (|a||s| + |j|^2) / (|j||c| + |s|^2)) in fp64 from the stored T values with eta inside the root,
 * the level rule, t_stop; so are its "Operand range", with each system's own first body as its m_0, and its "Range of h": a tick or a
 * dt_max whose cube is not a normal T is refused by init, step and sync (fp32: dt_max = 2^-10 with max_level = 33).
 *
 * EACH SYSTEM TAKES EXACTLY THE SOLO 6TH-ORDER BLOCK STEP.  After k calls of nb_hermite6_block_ensemble_step_*, system s holds bit for bit
 * what k calls of nb_hermite6_block_step_* give on that system alone with the same parameters: positions, velocities, accelerations,
 * jerks, snaps, crackles, ticks, levels and its status record (now_ticks, block_steps, body_steps, last_active, deepest_level, flags).
 * The same holds for init (the bits of nb_hermite6_block_init_*) and sync (the 6th-order predictor to status[s].now_ticks, .w of the
 * velocity preserved).  What follows from it:
 *   - Every system has its own `now`, active set and n_act; the times of the systems drift apart from call to call.
 *   - The evaluation geometry of system s is the solo one of (N, n_act of s), stream geometry with the target of 512 workgroups on a
 *     per-system grid of launch_groups: tiles = ceil(n_act / tile), J = the smallest power of two with tiles * J >= 512, capped as
 *     nbody_hip_hermite_block.h describes, S from N.  (tiles, J) and with them the order of every sum are what the solo step uses.
 *     A B-DEPENDENT TARGET WOULD SAVE WORKGROUPS AND PARTIAL PLANES, BUT A SYSTEM'S BITS WOULD THEN DEPEND ON B: IT IS DELIBERATELY NOT
 *     TAKEN.
 *   - A system whose next block step would pass t_stop is left bit-identical except for NB_HERMITE_BLOCK_STOPPED in its own status (and
 *     deepest_level, as in the solo call).  Its workgroups leave after reading its control record; it does not hold the others back.  A
 *     later call with a larger t_stop resumes it.
 *   - A system's bits depend on its own inputs, N, the precision and the parameters only -- not on B, on its index, on the other systems,
 *     on the stream or on the workspace's prior content.  No workgroup ever touches two systems, so a system full of NaN harms no other.
 *
 * Geometry (nb_hermite6_block_ensemble_plan_*): the fields of nb_hermite6_block_plan_* for (N, num_active) -- nine sums: lds_bytes =
 * max(S - 1, 1) * 9 * tile * sizeof(T) + 128, partial_bytes = J * 9 * slots * sizeof(T), unroll = 2 (fp32) / 1 (fp64); partial_offset is
 * the solo plan's --, step_launches = 5, then what B adds: the evaluation launches groups_per_system = launch_groups workgroups per system,
 * the schedule stages blocks_per_system = ceil(N / 256); the grids are B times these.
 *
 * Summary.  nb_hermite6_block_ensemble_summary folds the B status records into one 64-byte record, in one launch of one workgroup: integer
 * sums and exact minima / maxima only.  Every system has reached t_stop when stopped == systems.
 *
 * Rules.  The caller owns all memory; a call allocates nothing, keeps no state, takes no lock, uses no atomics, never synchronises, never
 * prints and is asynchronous on `stream`, so it may sit inside a graph capture.  Every sum is formed in a fixed order and every word is
 * written by one lane.  init is 5 launches, a step 5, sync and summary 1.
 *
 * Limits.  1 <= N <= 65 536 (NB_HERMITE_BLOCK_ENSEMBLE_MAX_BODIES), B >= 1, N*B <= 2^28, and B * workgroups per system * threads per
 * workgroup <= 2^31 in every stage, init's evaluation included, so that every stage is one launch.  Above 65 536 bodies one system fills
 * the chip by itself: nb_hermite6_block_step_* is the call there.
 *
 * Not built: per-system body counts, parameters or t_stop; several tiny systems packed into one wave; a B-dependent evaluation geometry;
 * sharded forms.
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null pointer (but system_softening_sq); N, B, num_active or a
 * product out of range; an array not aligned to 4*sizeof(T) (ticks, status, summary: 8; levels: 4; system_softening_sq: sizeof(T);
 * workspace: 32); workspace_bytes too small; any two arrays of a call overlapping; a parameter nb_hermite6_block_* refuses, its cube rule
 * included; a NaN t_stop.  Otherwise the launch's hipError_t (0 on success).
 */
#ifndef NBODY_HIP_HERMITE6_BLOCK_ENSEMBLE_H
#define NBODY_HIP_HERMITE6_BLOCK_ENSEMBLE_H

#include <stddef.h>
#include <stdint.h>

#include "nbody_hip_hermite_block_ensemble.h" /* for its types and constants alone: _plan_t, _summary_t, _MAX_BODIES, _MAX_TOTAL */

#ifdef __cplusplus
extern "C" {
#endif

/* B * workspace_stride; workspace_stride = the sum, each term rounded up to 256 bytes, of 12*N*sizeof_T (predicted state),
 * G*9*tile*sizeof_T (partial planes; tile = 128 fp32, 64 fp64; G = launch_groups of N or, where that is larger, of 255, 511 or 1 023
 * bodies when N is above them: the size grows with N and with B, never shrinks), 4*N (active list), 4*ceil(N/256) (counts),
 * 8*ceil(N/256) and 4*ceil(N/256) (partial minima and levels), 64 (control record) */
NB_API int nb_hermite6_block_ensemble_workspace_bytes(unsigned num_bodies, unsigned num_systems, unsigned sizeof_T, size_t* bytes);

NB_API int nb_hermite6_block_ensemble_plan_f32(unsigned num_bodies, unsigned num_systems, unsigned num_active, nb_hermite_block_ensemble_plan_t* plan);
NB_API int nb_hermite6_block_ensemble_plan_f64(unsigned num_bodies, unsigned num_systems, unsigned num_active, nb_hermite_block_ensemble_plan_t* plan);

/* per system: accelerations, jerks, snaps, crackles, levels, ticks and the status record from positions and velocities */
NB_API int nb_hermite6_block_ensemble_init_f32(float* positions, float* velocities, float* accelerations, float* jerks, float* snaps, float* crackles,
                                               uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
                                               unsigned num_bodies, unsigned num_systems, float softening_sq, const float* system_softening_sq,
                                               const nb_hermite_block_params_t* params, nb_stream_t stream);
NB_API int nb_hermite6_block_ensemble_init_f64(double* positions, double* velocities, double* accelerations, double* jerks, double* snaps, double* crackles,
                                               uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
                                               unsigned num_bodies, unsigned num_systems, double softening_sq, const double* system_softening_sq,
                                               const nb_hermite_block_params_t* params, nb_stream_t stream);

/* one block step of every system whose next step does not pass t_stop; the others get the flag */
NB_API int nb_hermite6_block_ensemble_step_f32(float* positions, float* velocities, float* accelerations, float* jerks, float* snaps, float* crackles,
                                               uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
                                               unsigned num_bodies, unsigned num_systems, float softening_sq, const float* system_softening_sq,
                                               const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream);
NB_API int nb_hermite6_block_ensemble_step_f64(double* positions, double* velocities, double* accelerations, double* jerks, double* snaps, double* crackles,
                                               uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
                                               unsigned num_bodies, unsigned num_systems, double softening_sq, const double* system_softening_sq,
                                               const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream);

/* every body of system s predicted to status[s].now_ticks -> positions_out, velocities_out */
NB_API int nb_hermite6_block_ensemble_sync_f32(float* positions_out, float* velocities_out, const float* positions, const float* velocities,
                                               const float* accelerations, const float* jerks, const float* snaps, const float* crackles, const uint64_t* ticks,
                                               const nb_hermite_block_status_t* status, unsigned num_bodies, unsigned num_systems,
                                               const nb_hermite_block_params_t* params, nb_stream_t stream);
NB_API int nb_hermite6_block_ensemble_sync_f64(double* positions_out, double* velocities_out, const double* positions, const double* velocities,
                                               const double* accelerations, const double* jerks, const double* snaps, const double* crackles, const uint64_t* ticks,
                                               const nb_hermite_block_status_t* status, unsigned num_bodies, unsigned num_systems,
                                               const nb_hermite_block_params_t* params, nb_stream_t stream);

/* the B status records folded into one */
NB_API int nb_hermite6_block_ensemble_summary(const nb_hermite_block_status_t* status, unsigned num_systems, nb_hermite_block_ensemble_summary_t* summary,
                                              nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_HERMITE6_BLOCK_ENSEMBLE_H */
