/*
 * nbody_hip_hermite6_ensemble.h -- 6th-order Hermite steps of many independent N-body systems of one size, one launch per stage, each
 * system with a time step of its own (libnbody_hip_hermite6_ensemble.so).
 *
 * nb_hermite_ensemble_* (nbody_hip_hermite_ensemble.h) fills the chip with B small systems that take 4th-order steps; nb_hermite6_*
 * (nbody_hip_hermite6.h) takes the 6th-order step, which reaches a given error with a third to a quarter of the steps, but fills the chip
 * only from about 65 536 bodies.  Here B systems take 6th-order steps together, and in the adaptive form every system keeps its time and
 * its time step on the device, as in nbody_hip_hermite_ensemble.h.  That header is included for its types alone
 * (nb_hermite_ensemble_plan_t, nb_hermite_ensemble_clock_t, nb_hermite_ensemble_status_t, NB_HERMITE_ENSEMBLE_DONE / _STALLED and the
 * limits): this library links none of the other libraries and has no process-global state (softening^2 is an argument).  Error codes are
 * the NB_ERR_* / hipError_t values of nbody_hip.h; nb_error_string() of libnbody_hip.so names them.
 *
 * Layout.  B systems of N bodies each; system s holds bodies [s*N, (s+1)*N) of every array, all caller-owned device arrays of
 * T = float | double with the fields of nbody_hip_hermite6.h:
 *   positions     T[4*N*B] = {x, y, z, mass}
 *   velocities    T[4*N*B] = {vx, vy, vz, w}   (.w is preserved, never interpreted)
 *   accelerations T[4*N*B] = {ax, ay, az, 0}
 *   jerks         T[4*N*B] = {jx, jy, jz, 0}
 *   snaps         T[4*N*B] = {sx, sy, sz, 0}
 *   crackles      T[4*N*B] = {cx, cy, cz, 0}
 *   workspace     nb_hermite6_ensemble_workspace_bytes(N, B, sizeof(T)) bytes: the predicted state {x, y, z, m, vx, vy, vz, 0, ax, ay,
 *                 az, 0} per body (12*N*B*sizeof(T)), then ceil(N / 256) partial minima (doubles) per system and one 64-byte partial
 *                 status per 256 systems.  Its content before a call does not matter; nothing is kept in it between calls.
 * Systems of different sizes: pad every system to the largest N with bodies of mass +0 placed after its real bodies (softening^2
 * > 0, or no padding body on top of a real one), as nbody_hip_ensemble.h describes.  A zero-mass body pulls nothing.  THE PADDING
 * BODIES ARE STEPPED like any other body and move under the others' pull, AND THEY ENTER THE TIME-STEP MINIMUM of their system: a
 * padding body placed next to a real one shortens that system's steps.  Per-system body counts are not built.
 *
 * Each system takes exactly the solo step.  With the same dt and softening^2, system s after nb_hermite6_ensemble_step_* holds the
 * bits nb_hermite6_step_* gives on that system alone -- the predicted state in the workspace included --;
 * nb_hermite6_ensemble_eval_* likewise equals nb_hermite6_eval_*, nb_hermite6_ensemble_init_* equals nb_hermite6_init_*, and
 * nb_hermite6_ensemble_timestep_* equals nb_hermite6_timestep_*:
 *   dt_out[s] = eta * sqrt( min_i (|a||s| + |j|^2) / (|j||c| + |s|^2) )
 * over the bodies of system s with a positive denominator and a finite ratio; +inf if there is none.  Per-body arithmetic is fp64 for
 * either T, and eta sits outside the root.  The formulas, the floor that softening_sq == 0 takes (per system), the predictor, the
 * corrector and the new crackle are those of nbody_hip_hermite6.h, and so are the operand range the error bounds hold on ("Operand
 * range" there; the unit mass a system's unit chunks are recognised by is that system's own first body's) and the range of the time
 * step ("Time step" there).  Range of h: as in that header, |dt|^3 -- scalar or per system -- must be a normal T (the crackle divides
 * by it): 2^-42 <= |dt| <= 2^42 (fp32) / 2^-340 <= |dt| <= 2^341 (fp64); it is not checked, and outside that range c1 is what that
 * header says.  The adaptive form chooses dt itself and does not hold it to this range: a system whose dt_next falls below it takes
 * that step, its crackles are then without bound or infinite (dt_next = 0: the system ends STALLED) or NaN (bodies the criterion leaves
 * out), and dt_max is the caller's to keep inside the range.
 *
 * Geometry (nb_hermite6_ensemble_plan_*).  Per system it is nb_hermite6_plan_*'s, a function of (N, precision) alone: a workgroup
 * owns 64 * bodies_per_lane bodies i of ONE system, workgroup g works on tile g mod groups_per_system of system g / groups_per_system,
 * and B only sets the grid.  lds_bytes counts 9 sums.  A workgroup never touches two systems, so a system of NaN and inf harms no other.
 *
 * Reproducibility.  A system's bits depend only on its own inputs, N, the precision and its parameters -- not on B, on the system's
 * index, on the other systems, on the stream, on the workspace's earlier content or on the device.  No atomics anywhere.
 *
 * Parameters.
 *   nb_hermite6_ensemble_eval_*, _init_*, _begin_*, _advance_*: system_softening_sq == NULL: every system uses softening_sq; otherwise
 *     it is a device array T[B] of softening^2 per system and the scalar is ignored.
 *   nb_hermite6_ensemble_step_*: system_params == NULL: every system uses (delta_time, softening_sq); otherwise it is a device array
 *     T[4*B] of {dt, softening^2, ignored, ignored} per system and the two scalars are ignored.
 *
 * Overlaps.  new_positions == old_positions IS ALLOWED (and gives the bits of two separate arrays), and so is acc_out == acc_in of
 * nb_hermite6_ensemble_eval_* (the evaluation reads the workspace's copy).  Every other overlap between the arrays of a call -- the
 * clocks, the status, the parameter arrays and the workspace included -- is refused.
 *
 * The adaptive form.  nb_hermite6_ensemble_begin_* is nb_hermite6_ensemble_init_* and one 32-byte clock per system:
 * {time = 0, dt_next = the time step of that state, dt_last = 0, steps = 0, flags}; flags holds NB_HERMITE_ENSEMBLE_STALLED if dt_next
 * is not > 0, else 0.  (Crackles are 0 at the start, so dt_next = eta sqrt(min (|a||s| + |j|^2) / |s|^2) there.)
 * nb_hermite6_ensemble_advance_* then takes ONE step per system that can still move, with that system's own dt, in at most five
 * launches whatever B is.  The rule is that of nb_hermite_ensemble_advance_*, per system:
 *   - A system whose flags hold DONE or STALLED is left bit-identical.  Its workgroups leave after one scalar load.
 *   - Otherwise remaining = t_stop - time, in double.
 *   - If remaining is not > 0, or (T)remaining is 0: set DONE, time = t_stop, state untouched.
 *   - Else cand = min(dt_next, dt_max).  If cand >= remaining, then dt = (T)remaining and this is the system's last step.  Otherwise
 *     dt = (T)cand.
 *   - After the solo step with that dt: time = t_stop on a last step, else time + (double)dt; dt_last = dt; steps += 1; dt_next is set
 *     from the new a, j, s and c, as nb_hermite6_ensemble_timestep_* computes it; on a last step, set DONE.
 *   - If dt_next is not > 0 and DONE is not set, set STALLED.  +inf counts as > 0.
 * dt is a pure function of the clock record (and t_stop, dt_max), and only the call's clock stage, which runs after every stage that
 * reads the clocks, writes them: every workgroup of a system derives the same dt.  `status` is optional (NULL: not written): the
 * 64-byte record of nbody_hip_hermite_ensemble.h, written by the call's last stage.  It holds integer sums and exact minima only, so
 * its bits do not depend on order.  A caller enqueues a batch of calls and reads 64 bytes.
 * Precision.  The crackle the criterion reads comes out of the corrector as (60 D0 - 36 D1 + 9 D2) / h^3 and carries the rounding of
 * a1 - a0 times 60 / h^3.  In fp64 that is nothing.  IN FP32 IT CAN RULE THE DENOMINATOR |j||c| + |s|^2: a shorter step then makes more
 * noise and a still shorter step, and the system ends STALLED -- with the solo calls as here.  With h = eta * tau (tau a system's own
 * time scale) the steps hold while eta^3 is well above 60 * 2^-24; eta = 0.2 is, eta = 0.025 (which suits fp64) is not, and a system
 * whose steps dt_max keeps far below tau can stall at any eta.  Steps of a given dt (nb_hermite6_ensemble_step_*) are not affected.
 *
 * Rules.  The caller owns all memory; a call allocates nothing, keeps no state, takes no lock, uses no atomics, never synchronises,
 * never prints and is asynchronous on `stream`, so it may sit inside a graph capture.
 *
 * Limits.  Those of nbody_hip_hermite_ensemble.h: 1 <= N <= 65 536 (NB_HERMITE_ENSEMBLE_MAX_BODIES), B >= 1, N*B <= 2^28
 * (NB_HERMITE_ENSEMBLE_MAX_TOTAL), and B * groups_per_system * block_threads <= 2^31, so that a call is one launch per stage.  Above
 * 65 536 bodies one system fills the chip by itself: nb_hermite6_step_* is the call there.
 *
 * Not built here: 6th-order block ensembles (block time steps per system with this scheme) are nbody_hip_hermite6_block_ensemble.h, whose
 * initial evaluation is this library's.  Not built: per-system body counts; sharded forms; several tiny systems packed into one wave
 * (N < 64 * bodies_per_lane leaves lanes idle).
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null pointer (but the optional ones); N, B or their products
 * out of range; an array, a parameter array of step or the workspace not aligned to 4*sizeof(T) (system_softening_sq, dt_out:
 * sizeof(T); clocks, status: 8); workspace_bytes too small; t_stop NaN or dt_max not > 0; any two arrays of a call overlapping (but
 * new_positions == old_positions, and acc_out == acc_in).  Otherwise the launch's hipError_t (0 on success).
 */
#ifndef NBODY_HIP_HERMITE6_ENSEMBLE_H
#define NBODY_HIP_HERMITE6_ENSEMBLE_H

#include <stddef.h>
#include <stdint.h>

#include "nbody_hip_hermite_ensemble.h" /* for its types alone: the plan, the clock, the status record, the flags, the limits */

#ifdef __cplusplus
extern "C" {
#endif

/* 12 * N * B * sizeof_T + 8 * B * ceil(N / 256) + 64 * ceil(B / 256) (sizeof_T: 4 or 8) */
NB_API int nb_hermite6_ensemble_workspace_bytes(unsigned num_bodies, unsigned num_systems, unsigned sizeof_T, size_t* bytes);

NB_API int nb_hermite6_ensemble_plan_f32(unsigned num_bodies, unsigned num_systems, nb_hermite_ensemble_plan_t* plan);
NB_API int nb_hermite6_ensemble_plan_f64(unsigned num_bodies, unsigned num_systems, nb_hermite_ensemble_plan_t* plan);

/* accelerations, jerks and snaps of every system's state; nothing is integrated -- two launches */
NB_API int nb_hermite6_ensemble_eval_f32(float* acc_out, float* jerk_out, float* snap_out, const float* positions, const float* velocities,
                                         const float* acc_in, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                         unsigned num_systems, float softening_sq, const float* system_softening_sq, nb_stream_t stream);
NB_API int nb_hermite6_ensemble_eval_f64(double* acc_out, double* jerk_out, double* snap_out, const double* positions, const double* velocities,
                                         const double* acc_in, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                         unsigned num_systems, double softening_sq, const double* system_softening_sq, nb_stream_t stream);

/* the start of a run: a, jerk, snap of every system's state, crackle = 0 -- four launches */
NB_API int nb_hermite6_ensemble_init_f32(float* accelerations, float* jerks, float* snaps, float* crackles, const float* positions,
                                         const float* velocities, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                         unsigned num_systems, float softening_sq, const float* system_softening_sq, nb_stream_t stream);
NB_API int nb_hermite6_ensemble_init_f64(double* accelerations, double* jerks, double* snaps, double* crackles, const double* positions,
                                         const double* velocities, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                         unsigned num_systems, double softening_sq, const double* system_softening_sq, nb_stream_t stream);

/* one 6th-order Hermite step of every system -- two launches */
NB_API int nb_hermite6_ensemble_step_f32(float* new_positions, const float* old_positions, float* velocities, float* accelerations, float* jerks,
                                         float* snaps, float* crackles, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                         unsigned num_systems, float delta_time, float softening_sq, const float* system_params,
                                         nb_stream_t stream);
NB_API int nb_hermite6_ensemble_step_f64(double* new_positions, const double* old_positions, double* velocities, double* accelerations, double* jerks,
                                         double* snaps, double* crackles, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                         unsigned num_systems, double delta_time, double softening_sq, const double* system_params,
                                         nb_stream_t stream);

/* dt_out[s] (device, T[B]) = eta * sqrt(min (|a||s| + |j|^2) / (|j||c| + |s|^2)) over system s -- two launches */
NB_API int nb_hermite6_ensemble_timestep_f32(const float* accelerations, const float* jerks, const float* snaps, const float* crackles,
                                             unsigned num_bodies, unsigned num_systems, float eta, float* dt_out, void* workspace,
                                             size_t workspace_bytes, nb_stream_t stream);
NB_API int nb_hermite6_ensemble_timestep_f64(const double* accelerations, const double* jerks, const double* snaps, const double* crackles,
                                             unsigned num_bodies, unsigned num_systems, double eta, double* dt_out, void* workspace,
                                             size_t workspace_bytes, nb_stream_t stream);

/* the start of an adaptive run: nb_hermite6_ensemble_init_* and the clocks of every system -- six launches */
NB_API int nb_hermite6_ensemble_begin_f32(float* accelerations, float* jerks, float* snaps, float* crackles, const float* positions,
                                          const float* velocities, nb_hermite_ensemble_clock_t* clocks, unsigned num_bodies,
                                          unsigned num_systems, float softening_sq, const float* system_softening_sq, float eta,
                                          void* workspace, size_t workspace_bytes, nb_stream_t stream);
NB_API int nb_hermite6_ensemble_begin_f64(double* accelerations, double* jerks, double* snaps, double* crackles, const double* positions,
                                          const double* velocities, nb_hermite_ensemble_clock_t* clocks, unsigned num_bodies,
                                          unsigned num_systems, double softening_sq, const double* system_softening_sq, double eta,
                                          void* workspace, size_t workspace_bytes, nb_stream_t stream);

/* one step of every system that can still move, each with its own dt (the rule above) -- at most five launches */
NB_API int nb_hermite6_ensemble_advance_f32(float* new_positions, const float* old_positions, float* velocities, float* accelerations,
                                            float* jerks, float* snaps, float* crackles, nb_hermite_ensemble_clock_t* clocks,
                                            nb_hermite_ensemble_status_t* status, void* workspace, size_t workspace_bytes,
                                            unsigned num_bodies, unsigned num_systems, double t_stop, double dt_max, float eta,
                                            float softening_sq, const float* system_softening_sq, nb_stream_t stream);
NB_API int nb_hermite6_ensemble_advance_f64(double* new_positions, const double* old_positions, double* velocities, double* accelerations,
                                            double* jerks, double* snaps, double* crackles, nb_hermite_ensemble_clock_t* clocks,
                                            nb_hermite_ensemble_status_t* status, void* workspace, size_t workspace_bytes,
                                            unsigned num_bodies, unsigned num_systems, double t_stop, double dt_max, double eta,
                                            double softening_sq, const double* system_softening_sq, nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_HERMITE6_ENSEMBLE_H */
