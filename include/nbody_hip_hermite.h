/*
 * nbody_hip_hermite.h -- 4th-order Hermite steps of one N-body system (libnbody_hip_hermite.so).
 *
 * nb_integrate_* takes the reference's first-order step.  The scheme here (Makino & Aarseth 1992) also costs one evaluation of all
 * N^2 interactions per step, but the evaluation returns the JERK (the time derivative of the acceleration) besides the
 * acceleration, and a predictor-corrector built on both has a local error that falls with dt^5, a global one with dt^4.
 *
 * This library links neither libnbody_hip.so nor its state: it reads no process-global setting (softening^2 is an argument).
 * Error codes are the NB_ERR_* / hipError_t values of nbody_hip.h; nb_error_string() of libnbody_hip.so names them.
 *
 * State of a system of N bodies, all caller-owned device arrays of T = float | double:
 *   positions     T[4*N] = {x, y, z, mass}
 *   velocities    T[4*N] = {vx, vy, vz, w}   (.w is preserved, never interpreted)
 *   accelerations T[4*N] = {ax, ay, az, 0}
 *   jerks         T[4*N] = {jx, jy, jz, 0}
 *   workspace     8*N*sizeof(T) bytes (nb_hermite_workspace_bytes): the predicted state {x, y, z, m, vx, vy, vz, 0} per body.
 *                 Its content before a call does not matter; nothing is kept in it between calls.
 *
 * Evaluation (nb_hermite_eval_*).  With r = x_j - x_i, w = v_j - v_i, s^2 = r.r + softening_sq, over all j:
 *   a_i    = sum m_j s^-3 r
 *   jerk_i = sum m_j s^-3 (w - 3 (r.w) s^-2 r)
 * softening_sq == 0 is evaluated with the floor s^2 = r.r + 2^-60 (fp32) / 2^-300 (fp64): the i = j term and any pair of coincident
 * bodies with one velocity then contribute exactly 0 instead of NaN, and a pair further apart than 2^-18 (fp32; 2^-124 fp64) is not changed by more
 * than an ulp of s^2.  (With softening_sq > 0 a coincident pair contributes a = 0, jerk = m w / softening^3, as the formulas say.)
 *
 * Operand range.  The evaluation is held (tests/test_hermite_domain.py) to 5e-6 (fp32) / 1e-14 (fp64) times a body's sums of term
 * magnitudes, A_i = sum |m| s^-3 |r| and J_i = sum |m| s^-3 (|w| + 3 |r.w| s^-2 |r|), and a single
 * term to 1e-6 / 1e-14 (a) and 5e-6 / 1e-14 (jerk) of its magnitude, for
 *   s^2 = r.r + softening_sq of every pair in [2^-84, 2^84] (fp32) / [2^-600, 2^600] (fp64);
 *   masses 0 or of magnitude in [2^-40, 2^40] (fp32) / [2^-100, 2^100] (fp64), any sign;
 *   velocities with |r| |w| of every pair, and the sums A_i and J_i, at most 2^126 (fp32) / 2^1022 (fp64).  At the corner of the
 *   ranges that go together -- masses of 2^40 at softening_sq = 2^-39 (fp32); 2^100 at 2^-100 (fp64) -- a jerk term is
 *   2^98.5 |w|, so 500 coherent ones admit |w| up to 2^17.
 * Inside this range no intermediate of the kernel leaves T's normal range before the result does: sums kept in units of a light
 * first body's mass go over to plain units before they outgrow T.  Outside it nothing is clamped.  fp32: below s^2 = 2^-85.4, s^-3 overflows and the body's
 * sums are infinite or NaN; above s^2 = 2^84, s^-3 = s^-1 s^-2 is subnormal and the term is off by up to two units of 2^-149 in
 * s^-3 -- a bit of precision per 2/3 of a binade -- until it is 0.  fp64 has room on either side of its range (s^-3 leaves it at
 * s^2 = 2^+-682); the range is what the tests cover.  A sum beyond 2^126 / 2^1022 may overflow to an infinity before the cancelling
 * terms arrive.
 * Non-finite inputs are ordinary data: a NaN coordinate or a NaN / infinite mass reaches a and jerk of every body, a NaN velocity
 * every jerk and no acceleration; masses and velocity .w are never written.
 *
 * Step (nb_hermite_step_*), shared time step dt, P(EC)^1 -- two launches:
 *   predict   x_p = x + v dt + a dt^2/2 + j dt^3/6,   v_p = v + a dt + j dt^2/2                     -> workspace
 *   evaluate  a1, j1 = eval(x_p, v_p)
 *   correct   v1 = v + (a + a1) dt/2 + (j - j1) dt^2/12,   x1 = x + (v + v1) dt/2 + (a - a1) dt^2/12
 *   store     x1 -> new_positions; v1, a1, j1 in place.
 * A run starts with nb_hermite_eval_* of the initial state (a0, j0).  There is no damping.  The bodies j are read from the
 * workspace, so a lane reads and writes its own body's stored state only: new_positions == old_positions IS ALLOWED (and gives the
 * bits of two separate arrays).  Every other overlap between the arrays of a call is refused.
 *
 * Time step (nb_hermite_timestep_*).  dt_out[0] = eta * min_i |a_i| / |jerk_i| over the bodies with |jerk_i| > 0 and a finite ratio;
 * +inf if there is none.  The result stays on the device: a caller that adapts dt reads one scalar when it wants to.  The rule holds
 * for every finite a and jerk, subnormal ones included, whose ratio is a finite double and, rounded to T, a normal number or 0:
 * the two norms are formed from components scaled by a power of two each, so neither |a|^2 nor |jerk|^2 can leave fp64's range.
 *
 * Rules.  The caller owns all memory; a call allocates nothing, keeps no state, takes no lock, never synchronises, never prints and
 * is asynchronous on `stream`, so it may sit inside a graph capture.  No atomics: results are bit-identical from call to call.
 * The geometry (nb_hermite_plan_*) is a function of (N, precision) alone.
 *
 * Limits.  1 <= N <= 2^26 (NB_HERMITE_MAX_BODIES; a 4 GiB fp64 workspace).  Body indices are 32-bit, byte offsets 64-bit.
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null pointer; N out of range; an array or the workspace
 * not aligned to 4*sizeof(T) (dt_out: sizeof(T), scratch: 8); workspace_bytes / scratch_bytes too small; any two arrays of a call
 * overlapping (but new_positions == old_positions).  Otherwise the launch's hipError_t (0 on success).
 */
#ifndef NBODY_HIP_HERMITE_H
#define NBODY_HIP_HERMITE_H

#include <stddef.h>

#include "nbody_hip.h" /* nb_stream_t, NB_ERR_*; error names: nb_error_string */

#ifdef __cplusplus
extern "C" {
#endif

#define NB_HERMITE_MAX_BODIES (1u << 26)
#define NB_HERMITE_TIMESTEP_SCRATCH_BYTES 8192 /* nb_hermite_timestep_*: partial minima, any content before the call */

typedef struct nb_hermite_plan { /* the geometry of the evaluation kernel */
    int      bodies_per_lane; /* bodies i a lane holds (fp32: one packed pair, fp64: one)                          */
    int      waves_per_group; /* waves of a workgroup: they share the bodies i and split the bodies j             */
    int      unroll;          /* bodies j per scalar load group                                                   */
    unsigned groups;          /* workgroups                                                                       */
    unsigned block_threads;
    unsigned lds_bytes;
} nb_hermite_plan_t;

/* 8 * num_bodies * sizeof_T (sizeof_T: 4 or 8) */
NB_API int nb_hermite_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes);

NB_API int nb_hermite_plan_f32(unsigned num_bodies, nb_hermite_plan_t* plan);
NB_API int nb_hermite_plan_f64(unsigned num_bodies, nb_hermite_plan_t* plan);

/* accelerations and jerks of a state; nothing is integrated, positions and velocities are only read */
NB_API int nb_hermite_eval_f32(float* accelerations, float* jerks, const float* positions, const float* velocities,
                               unsigned num_bodies, float softening_sq, nb_stream_t stream);
NB_API int nb_hermite_eval_f64(double* accelerations, double* jerks, const double* positions, const double* velocities,
                               unsigned num_bodies, double softening_sq, nb_stream_t stream);

/* one Hermite step (see above) */
NB_API int nb_hermite_step_f32(float* new_positions, const float* old_positions, float* velocities, float* accelerations, float* jerks,
                               void* workspace, size_t workspace_bytes, unsigned num_bodies, float delta_time, float softening_sq,
                               nb_stream_t stream);
NB_API int nb_hermite_step_f64(double* new_positions, const double* old_positions, double* velocities, double* accelerations, double* jerks,
                               void* workspace, size_t workspace_bytes, unsigned num_bodies, double delta_time, double softening_sq,
                               nb_stream_t stream);

/* dt_out[0] (device) = eta * min |a| / |jerk|; scratch: NB_HERMITE_TIMESTEP_SCRATCH_BYTES device bytes */
NB_API int nb_hermite_timestep_f32(const float* accelerations, const float* jerks, unsigned num_bodies, float eta, float* dt_out,
                                   void* scratch, size_t scratch_bytes, nb_stream_t stream);
NB_API int nb_hermite_timestep_f64(const double* accelerations, const double* jerks, unsigned num_bodies, double eta, double* dt_out,
                                   void* scratch, size_t scratch_bytes, nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_HERMITE_H */
