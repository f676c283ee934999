/*
 * nbody_hip_hermite_ensemble.h -- 4th-order Hermite steps of many independent N-body systems of one size, one launch per stage, each
 * system with a time step of its own (libnbody_hip_hermite_ensemble.so).
 *
 * nb_ensemble_* (nbody_hip_ensemble.h) fills the chip with B small systems, but with the reference's first-order step; nb_hermite_*
 * (nbody_hip_hermite.h) takes the 4th-order step a user of small systems wants, but fills the chip only from about 65 536 bodies, and
 * its adaptive time step costs a host read per step and system.  Here B systems take Hermite steps together, and in the adaptive
 * form every system keeps its time and its time step on the device: a stiff system does not set the step of the calm ones, and the
 * host never reads a dt.
 *
 * This library links none of the other libraries and has no process-global state (softening^2 is an argument).  Error codes are the
 * NB_ERR_* / hipError_t values of nbody_hip.h; nb_error_string() of libnbody_hip.so names them.
 *
 * Layout.  B systems of N bodies each; system s holds bodies [s*N, (s+1)*N) of every array, all caller-owned device arrays of
 * T = float | double with the fields of nbody_hip_hermite.h:
 *   positions     T[4*N*B] = {x, y, z, mass}
 *   velocities    T[4*N*B] = {vx, vy, vz, w}   (.w is preserved, never interpreted)
 *   accelerations T[4*N*B] = {ax, ay, az, 0}
 *   jerks         T[4*N*B] = {jx, jy, jz, 0}
 *   workspace     nb_hermite_ensemble_workspace_bytes(N, B, sizeof(T)) bytes: the predicted state {x, y, z, m, vx, vy, vz, 0} per
 *                 body (8*N*B*sizeof(T)), then ceil(N / 256) partial minima (doubles) per system and one 64-byte partial status per
 *                 256 systems.  Its content before a call does not matter; nothing is kept in it between calls.
 * Systems of different sizes: pad every system to the largest N with bodies of mass +0 placed after its real bodies (softening^2
 * > 0, or no padding body on top of a real one), as nbody_hip_ensemble.h describes.  A zero-mass body pulls nothing.  THE PADDING
 * BODIES ARE STEPPED like any other body and move under the others' pull, AND THEY ENTER THE TIME-STEP MINIMUM of their system: a
 * padding body placed next to a real one shortens that system's steps.  Per-system body counts are not built.
 *
 * Each system takes exactly the solo step.  With the same dt and softening^2, system s after nb_hermite_ensemble_step_* holds the
 * bits nb_hermite_step_* gives on that system alone; nb_hermite_ensemble_eval_* likewise equals nb_hermite_eval_*, and
 * nb_hermite_ensemble_timestep_* equals nb_hermite_timestep_* (dt_out[s] = eta * (T)min_i |a_i| / |jerk_i| over the bodies of
 * system s with |jerk_i| > 0 and a finite ratio; +inf if there is none).  The formulas, the floor that softening_sq == 0 takes (per
 * system) and the predictor-corrector are those of nbody_hip_hermite.h, and so is the operand range the error bounds hold on
 * ("Operand range" there; the unit mass a system's unit chunks are recognised by is that system's own first body's).
 *
 * Geometry (nb_hermite_ensemble_plan_*).  Per system it is nb_hermite_plan_*'s, a function of (N, precision) alone: a workgroup owns
 * 64 * bodies_per_lane bodies i of ONE system, workgroup g works on tile g mod groups_per_system of system g / groups_per_system, and
 * B only sets the grid.  A workgroup never touches two systems, so a system of NaN and inf harms no other.
 *
 * Reproducibility.  A system's bits depend only on its own inputs, N, the precision and its parameters -- not on B, on the system's
 * index, on the other systems, on the stream or on the device.  No atomics anywhere.
 *
 * Parameters.
 *   nb_hermite_ensemble_eval_*, _begin_*, _advance_*: system_softening_sq == NULL: every system uses softening_sq; otherwise it is a
 *     device array T[B] of softening^2 per system and the scalar is ignored.
 *   nb_hermite_ensemble_step_*: system_params == NULL: every system uses (delta_time, softening_sq); otherwise it is a device array
 *     T[4*B] of {dt, softening^2, ignored, ignored} per system and the two scalars are ignored.
 *
 * Overlaps.  new_positions == old_positions IS ALLOWED (and gives the bits of two separate arrays).  Every other overlap between the
 * arrays of a call -- the clocks, the status, the parameter arrays and the workspace included -- is refused.
 *
 * The adaptive form.  nb_hermite_ensemble_begin_* evaluates the initial state (accelerations and jerks, as nb_hermite_ensemble_eval_*)
 * and writes one 32-byte clock per system: {time = 0, dt_next = eta * (T)min of that state, dt_last = 0, steps = 0, flags};
 * flags holds NB_HERMITE_ENSEMBLE_STALLED if dt_next is not > 0, else 0.  nb_hermite_ensemble_advance_* then takes ONE step per system
 * that can still move, with that system's own dt, in at most five launches whatever B is.  The rule, per system:
 *   - A system whose flags hold DONE or STALLED is left bit-identical.  Its workgroups leave after one scalar load.
 *   - Otherwise remaining = t_stop - time, in double.
 *   - If remaining is not > 0, or (T)remaining is 0: set DONE, time = t_stop, state untouched.
 *   - Else cand = min(dt_next, dt_max).  If cand >= remaining, then dt = (T)remaining and this is the system's last step.  Otherwise
 *     dt = (T)cand.
 *   - After the solo step with that dt: time = t_stop on a last step, else time + (double)dt; dt_last = dt; steps += 1; dt_next is set
 *     from the new a and j, as nb_hermite_ensemble_timestep_* computes it; on a last step, set DONE.
 *   - If dt_next is not > 0 and DONE is not set, set STALLED.  +inf counts as > 0.
 * dt is a pure function of the clock record (and t_stop, dt_max), and only the call's clock stage, which runs after every stage that
 * reads the clocks, writes them: every workgroup of a system derives the same dt.  `status` is optional (NULL: not written): a
 * 64-byte record written by the call's last stage -- the systems, how many are done, how many stalled, how many this call stepped,
 * the total of `steps` over all systems, the smallest `time`, and the smallest dt_last among the systems this call stepped (+inf if it
 * stepped none).  It holds integer sums and exact minima only, so its bits do not depend on order.  A caller enqueues a batch of calls
 * and reads 64 bytes.
 *
 * Rules.  The caller owns all memory; a call allocates nothing, keeps no state, takes no lock, uses no atomics, never synchronises,
 * never prints and is asynchronous on `stream`, so it may sit inside a graph capture.
 *
 * Limits.  1 <= N <= 65 536 (NB_HERMITE_ENSEMBLE_MAX_BODIES), B >= 1, N*B <= 2^28, and B * groups_per_system * block_threads <= 2^31, so
 * that a call is one launch per stage.  Above 65 536 bodies one system fills the chip by itself: nb_hermite_step_* is the call there.
 *
 * Not built: several tiny systems packed into one wave (N < 64 * bodies_per_lane leaves lanes idle); per-system body counts; sharded
 * forms.  (Block time steps per system are nbody_hip_hermite_block_ensemble.h.)
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null pointer (but the optional ones); N, B or their products
 * out of range; an array, a parameter array of step or the workspace not aligned to 4*sizeof(T) (system_softening_sq, dt_out:
 * sizeof(T); clocks, status: 8); workspace_bytes too small; t_stop NaN or dt_max not > 0; any two arrays of a call overlapping (but
 * new_positions == old_positions).  Otherwise the launch's hipError_t (0 on success).
 */
#ifndef NBODY_HIP_HERMITE_ENSEMBLE_H
#define NBODY_HIP_HERMITE_ENSEMBLE_H

#include <stddef.h>
#include <stdint.h>

#include "nbody_hip.h" /* nb_stream_t, NB_ERR_*; error names: nb_error_string */

#ifdef __cplusplus
extern "C" {
#endif

#define NB_HERMITE_ENSEMBLE_MAX_BODIES 65536u
#define NB_HERMITE_ENSEMBLE_MAX_TOTAL (1u << 28) /* N * B */
#define NB_HERMITE_ENSEMBLE_DONE 1u    /* clock flags: the system has reached t_stop */
#define NB_HERMITE_ENSEMBLE_STALLED 2u /* clock flags: dt_next is not > 0; the system is not stepped any more */

typedef struct nb_hermite_ensemble_plan { /* nb_hermite_plan_t per system, and the grid */
    int                bodies_per_lane;   /* bodies i a lane holds (fp32: one packed pair, fp64: one)                         */
    int                waves_per_group;   /* waves of a workgroup: they share the bodies i and split the bodies j            */
    int                unroll;            /* bodies j per scalar load group                                                  */
    unsigned           groups;            /* = groups_per_system (the name of nb_hermite_plan_t)                             */
    unsigned           block_threads;
    unsigned           lds_bytes;
    unsigned           groups_per_system; /* workgroups one system occupies                                                  */
    unsigned           reserved;
    unsigned long long grid_blocks;       /* groups_per_system * num_systems                                                 */
} nb_hermite_ensemble_plan_t;

typedef struct nb_hermite_ensemble_clock { /* 32 bytes of device memory per system */
    double   time;
    double   dt_next; /* the step the system would take next, before dt_max and t_stop */
    double   dt_last; /* the step it took last */
    uint32_t steps;
    uint32_t flags;   /* NB_HERMITE_ENSEMBLE_DONE | NB_HERMITE_ENSEMBLE_STALLED */
} nb_hermite_ensemble_clock_t;

typedef struct nb_hermite_ensemble_status { /* 64 bytes of device memory, written by nb_hermite_ensemble_advance_* */
    uint32_t systems;
    uint32_t done;
    uint32_t stalled;
    uint32_t stepped;     /* systems this call stepped */
    uint64_t total_steps; /* sum of `steps` over all systems */
    double   min_time;
    double   min_dt_last; /* over the systems this call stepped; +inf if none */
    uint64_t reserved[3]; /* 0 */
} nb_hermite_ensemble_status_t;

/* 8 * N * B * sizeof_T + 8 * B * ceil(N / 256) + 64 * ceil(B / 256) (sizeof_T: 4 or 8) */
NB_API int nb_hermite_ensemble_workspace_bytes(unsigned num_bodies, unsigned num_systems, unsigned sizeof_T, size_t* bytes);

NB_API int nb_hermite_ensemble_plan_f32(unsigned num_bodies, unsigned num_systems, nb_hermite_ensemble_plan_t* plan);
NB_API int nb_hermite_ensemble_plan_f64(unsigned num_bodies, unsigned num_systems, nb_hermite_ensemble_plan_t* plan);

/* accelerations and jerks of every system's state; nothing is integrated, positions and velocities are only read */
NB_API int nb_hermite_ensemble_eval_f32(float* accelerations, float* jerks, const float* positions, const float* velocities,
                                        unsigned num_bodies, unsigned num_systems, float softening_sq, const float* system_softening_sq,
                                        nb_stream_t stream);
NB_API int nb_hermite_ensemble_eval_f64(double* accelerations, double* jerks, const double* positions, const double* velocities,
                                        unsigned num_bodies, unsigned num_systems, double softening_sq, const double* system_softening_sq,
                                        nb_stream_t stream);

/* one Hermite step of every system -- two launches */
NB_API int nb_hermite_ensemble_step_f32(float* new_positions, const float* old_positions, float* velocities, float* accelerations, float* jerks,
                                        void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems,
                                        float delta_time, float softening_sq, const float* system_params, nb_stream_t stream);
NB_API int nb_hermite_ensemble_step_f64(double* new_positions, const double* old_positions, double* velocities, double* accelerations, double* jerks,
                                        void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems,
                                        double delta_time, double softening_sq, const double* system_params, nb_stream_t stream);

/* dt_out[s] (device, T[B]) = eta * min |a| / |jerk| over system s -- two launches */
NB_API int nb_hermite_ensemble_timestep_f32(const float* accelerations, const float* jerks, unsigned num_bodies, unsigned num_systems, float eta,
                                            float* dt_out, void* workspace, size_t workspace_bytes, nb_stream_t stream);
NB_API int nb_hermite_ensemble_timestep_f64(const double* accelerations, const double* jerks, unsigned num_bodies, unsigned num_systems, double eta,
                                            double* dt_out, void* workspace, size_t workspace_bytes, nb_stream_t stream);

/* the start of an adaptive run: accelerations, jerks and the clocks of every system -- three launches */
NB_API int nb_hermite_ensemble_begin_f32(float* accelerations, float* jerks, const float* positions, const float* velocities,
                                         nb_hermite_ensemble_clock_t* clocks, unsigned num_bodies, unsigned num_systems,
                                         float softening_sq, const float* system_softening_sq, float eta,
                                         void* workspace, size_t workspace_bytes, nb_stream_t stream);
NB_API int nb_hermite_ensemble_begin_f64(double* accelerations, double* jerks, const double* positions, const double* velocities,
                                         nb_hermite_ensemble_clock_t* clocks, unsigned num_bodies, unsigned num_systems,
                                         double softening_sq, const double* system_softening_sq, double eta,
                                         void* workspace, size_t workspace_bytes, nb_stream_t stream);

/* one step of every system that can still move, each with its own dt (the rule above) -- at most five launches */
NB_API int nb_hermite_ensemble_advance_f32(float* new_positions, const float* old_positions, float* velocities, float* accelerations, float* jerks,
                                           nb_hermite_ensemble_clock_t* clocks, nb_hermite_ensemble_status_t* status,
                                           void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems,
                                           double t_stop, double dt_max, float eta, float softening_sq, const float* system_softening_sq,
                                           nb_stream_t stream);
NB_API int nb_hermite_ensemble_advance_f64(double* new_positions, const double* old_positions, double* velocities, double* accelerations, double* jerks,
                                           nb_hermite_ensemble_clock_t* clocks, nb_hermite_ensemble_status_t* status,
                                           void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems,
                                           double t_stop, double dt_max, double eta, double softening_sq, const double* system_softening_sq,
                                           nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_HERMITE_ENSEMBLE_H */
