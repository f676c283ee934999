/*
 * nbody_hip_ensemble.h -- many independent N-body systems of one size stepped in ONE launch (libnbody_hip_ensemble.so).
 *
 * Below ~65 536 bodies a single system cannot fill the MI355X: a 1 024-body FAST step is a few microseconds of launch latency
 * for 1e6 interactions.  A caller with many small systems -- seeds of one configuration, a sweep over dt and softening, the demo
 * rows side by side -- hands them over here as one batch, and the chip is filled by the number of systems instead of their size.
 *
 * This library links neither libnbody_hip.so nor its state: it reads no process-global setting (softening^2 is an argument) and
 * exports exactly the four entry points below.  Error codes are the NB_ERR_* / hipError_t values of nbody_hip.h; nb_error_string()
 * of libnbody_hip.so names them.
 *
 * Layout.  B systems of N bodies each; system s holds bodies [s*N, (s+1)*N) of every array.
 *   positions  T[4*N*B] = {x, y, z, mass} per body
 *   velocities T[4*N*B] = {vx, vy, vz, w} per body (.w is preserved, never interpreted)
 * Systems of different sizes: pad every system to the largest N with bodies of mass +0 placed after its real bodies (softening^2
 * > 0, or no padding body on top of a real one).  A zero-mass body pulls nothing; in NB_MODE_STRICT the real bodies of a padded
 * system are bit-identical to the same system unpadded.  The padding is stepped too and moves under the others' pull.
 *
 * What one call does.  Each system takes exactly the step nb_integrate_* takes on it alone: a_i sums over the bodies of its own
 * system only, v = (v + a*dt)*damping, p += v*dt.  New positions go to new_positions; velocities are updated in place.
 * Ownership is the reference's: the caller owns all memory.  A call allocates nothing, takes no lock, never synchronises and is
 * asynchronous on `stream`, so it may sit inside a caller's graph capture.
 *
 * Parameters.  system_params == NULL: every system uses (delta_time, damping, softening_sq).  Otherwise system_params is a device
 * array T[4*B] of {dt, damping, softening^2, ignored} per system, and the three scalar arguments are ignored.
 *
 * Modes.
 *   NB_MODE_STRICT : every system is bit-identical to nb_integrate_* STRICT on that system alone (the reference's CPU path).
 *   NB_MODE_FAST   : the FAST arithmetic (v_rsq, FMA) of nb_integrate_*, one-sided (every directed interaction once).  Sums are
 *                    kept in units of the system's first body's mass when that mass lies within 2^+-20 (fp32) / 2^+-60 (fp64).
 *
 * Reproducibility.  A system's output bits depend only on its own inputs, N, the precision, the mode and its parameters -- not on
 * B, on the system's index, on the other systems, on the stream or on the device.  The FAST geometry (nb_ensemble_plan_*) is a
 * function of (N, precision) alone; B only sets the grid.
 *
 * Limits.  1 <= N <= 65 536, B >= 1, N*B <= 2^31.  Above 65 536 bodies one system fills the chip by itself: nb_integrate_ws_*
 * (pairwise, every pair once) is the right call there.
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null body pointer; N or B out of range; an unknown mode;
 * a body array or system_params not aligned to 4*sizeof(T); new_positions overlapping old_positions or velocities; velocities
 * overlapping old_positions; system_params overlapping any body array.  Otherwise the launch's hipError_t (0 on success).
 */
#ifndef NBODY_HIP_ENSEMBLE_H
#define NBODY_HIP_ENSEMBLE_H

#include "nbody_hip.h" /* nb_stream_t, NB_MODE_*, NB_ERR_*; error names: nb_error_string */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nb_ensemble_plan { /* the FAST geometry */
    int                bodies_per_lane;   /* bodies i a lane holds                                                            */
    int                waves_per_group;   /* waves of a workgroup: they share the bodies i and split the bodies j            */
    unsigned           groups_per_system; /* workgroups one system occupies                                                  */
    unsigned           block_threads;
    unsigned           lds_bytes;
    unsigned long long grid_blocks;       /* groups_per_system * num_systems                                                 */
} nb_ensemble_plan_t;

/* The FAST geometry of an ensemble of num_systems systems of num_bodies bodies (NB_ERR_INVALID_ARGUMENT for what the step refuses:
 * sizes out of range, plan == NULL).  Every field but grid_blocks is a function of (num_bodies, precision) alone. */
NB_API int nb_ensemble_plan_f32(unsigned num_bodies, unsigned num_systems, nb_ensemble_plan_t* plan);
NB_API int nb_ensemble_plan_f64(unsigned num_bodies, unsigned num_systems, nb_ensemble_plan_t* plan);

/* One step of every system (see above). */
NB_API int nb_ensemble_integrate_f32(float* new_positions, const float* old_positions, float* velocities,
                                     unsigned num_bodies, unsigned num_systems,
                                     float delta_time, float damping, float softening_sq,
                                     const float* system_params, int mode, nb_stream_t stream);
NB_API int nb_ensemble_integrate_f64(double* new_positions, const double* old_positions, double* velocities,
                                     unsigned num_bodies, unsigned num_systems,
                                     double delta_time, double damping, double softening_sq,
                                     const double* system_params, int mode, nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_ENSEMBLE_H */
