/*
 * nbody_hip_hermite6.h -- 6th-order Hermite steps of one N-body system (libnbody_hip_hermite6.so).
 *
 * nb_hermite_* (nbody_hip_hermite.h) is the 4th-order scheme.  The scheme here (Nitadori & Makino 2008) also costs one evaluation of
 * all N^2 interactions per step, but the evaluation returns the SNAP (the second time derivative of the acceleration) besides the
 * acceleration and the jerk, and a predictor-corrector built on all three has a global error that falls with dt^6.
 *
 * This library links none of the others and reads no process-global setting (softening^2 is an argument).  Error codes are the
 * NB_ERR_* / hipError_t values of nbody_hip.h; nb_error_string() of libnbody_hip.so names them.
 *
 * State of a system of N bodies, all caller-owned device arrays of T = float | double:
 *   positions     T[4*N] = {x, y, z, mass}
 *   velocities    T[4*N] = {vx, vy, vz, w}   (.w is preserved, never interpreted)
 *   accelerations T[4*N] = {ax, ay, az, 0}
 *   jerks         T[4*N] = {jx, jy, jz, 0}
 *   snaps         T[4*N] = {sx, sy, sz, 0}
 *   crackles      T[4*N] = {cx, cy, cz, 0}   (the third derivative of the acceleration, from the corrector's interpolation)
 *   workspace     12*N*sizeof(T) bytes (nb_hermite6_workspace_bytes): {x, y, z, m, vx, vy, vz, 0, ax, ay, az, 0} per body.
 *                 Its content before a call does not matter; nothing is kept in it between calls.
 *
 * Evaluation (nb_hermite6_eval_*).  With r = x_j - x_i, w = v_j - v_i, b = a_j - a_i, s^2 = r.r + softening_sq, k = m_j s^-3, over all j:
 *   alpha = (r.w) / s^2             beta = (w.w + r.b) / s^2 + alpha^2
 *   a_i    = sum k r
 *   jerk_i = sum k (w - 3 alpha r)                  =: sum k J'
 *   snap_i = sum k (b - 6 alpha J' - 3 beta r)
 * One launch copies positions, velocities and acc_in to the workspace, one evaluates; the bodies are read from the workspace only,
 * so acc_out == acc_in IS ALLOWED.  acc_in is arbitrary data: the snap is the formula's value for it (a and jerk do not depend on it).
 * softening_sq == 0 is evaluated with the floor s^2 = r.r + 2^-60 (fp32) / 2^-300 (fp64), as nb_hermite_eval_*: the i = j term then
 * contributes exactly 0 to all three sums instead of NaN, and so does a pair of coincident bodies with the same velocity and acc_in.
 *
 * Operand range.  That of nb_hermite_eval_* (nbody_hip_hermite.h, "Operand range") with the snap beside the jerk: the evaluation is
 * held to 5e-6 (fp32) / 1e-14 (fp64) times a body's sums of term magnitudes A_i, J_i and
 * S_i = sum |m| s^-3 (|b| + 6 |alpha| |J'| + 3 |beta| |r|) (every operand's magnitude, + for every -), for
 *   s^2 of every pair in [2^-84, 2^84] (fp32) / [2^-600, 2^600] (fp64);
 *   masses 0 or of magnitude in [2^-40, 2^40] (fp32) / [2^-100, 2^100] (fp64), any sign;
 *   velocities and acc_in with |r| |w|, |w|^2, |r| |b|, alpha^2 and |beta| of every pair, and the sums A_i, J_i and S_i, at most
 *   2^126 (fp32) / 2^1022 (fp64).  The snap is the first to get there: at masses of 2^40 and softening_sq = 2^-39 a snap term is of
 *   the order 2^118 |w|^2.
 * Outside the range nothing is clamped: what nbody_hip_hermite.h says of s^2, of sums beyond the range and of non-finite inputs
 * holds here, and a NaN in acc_in reaches every snap and nothing else.
 *
 * Start of a run (nb_hermite6_init_*).  Evaluates with b = 0 for a and jerk, evaluates again with that a for the snap -- a and jerk of
 * the second pass are the first pass's bits, the sums do not depend on b --, and sets the crackles to 0.  Four launches.
 *
 * Step (nb_hermite6_step_*), shared time step h = delta_time, P(EC)^1 -- two launches:
 *   predict   x_p = x + v h + a h^2/2 + j h^3/6 + s h^4/24 + c h^5/120
 *             v_p = v + a h + j h^2/2 + s h^3/6 + c h^4/24
 *             a_p = a + j h + s h^2/2 + c h^3/6                                                     -> workspace
 *   evaluate  a1, j1, s1 = eval(x_p, v_p, a_p)
 *   correct   v1 = v + (a + a1) h/2 - (j1 - j) h^2/10 + (s + s1) h^3/120
 *             x1 = x + (v + v1) h/2 - (a1 - a) h^2/10 + (j + j1) h^3/120
 *   crackle   D0 = a1 - a - j h - s h^2/2,  D1 = (j1 - j - s h) h,  D2 = (s1 - s) h^2,   c1 = (60 D0 - 36 D1 + 9 D2) / h^3
 *             (the third derivative, at the step's end, of the quintic through a, j, s at both ends)
 *   store     x1 -> new_positions; v1, a1, j1, s1, c1 in place.
 * There is no damping.  Range of h: |delta_time|^3, formed in T as (h h) h, must be a normal T (c1 divides by it):
 * 2^-42 <= |h| <= 2^42 (fp32) / 2^-340 <= |h| <= 2^341 (fp64).  The call does not check it.  Below that range the cube is subnormal and
 * c1 has no bound, and where it rounds to 0 (|h| <= 2^-50 / 2^-359, and h = 0) c1 is infinite or NaN: the next step's predictor then
 * makes positions NaN.  Above it h^3 is infinite: v1 and x1 are infinite or NaN.  The bodies j are read from the workspace, so a lane reads
 * and writes its own body's stored state only: new_positions == old_positions IS ALLOWED (and gives the bits of two separate arrays).
 * Every other overlap between the arrays of a call is refused.
 *
 * Time step (nb_hermite6_timestep_*).  Aarseth's criterion with the derivatives the scheme holds:
 *   dt_out[0] = eta * sqrt( min_i (|a||s| + |j|^2) / (|j||c| + |s|^2) )
 * over the bodies with a positive denominator and a finite ratio; +inf if there is none.  Per-body arithmetic is fp64 for either T:
 * plain products of two norms, so the rule holds while |a|^2, |j|^2, |s|^2, |c|^2 and their pairwise products are normal doubles --
 * always for fp32 inputs, for fp64 inputs with every nonzero norm in [2^-250, 2^250].  Beyond that range THE STEP CAN COME OUT TOO
 * LARGE: a body whose numerator or denominator overflows is left out of the minimum, and so is one whose denominator underflows to 0;
 * products that underflow to 0 beside ones that do not count as 0, and the body gives the step the surviving products give.
 * The result stays on the device: a caller that adapts dt reads one scalar when it wants to.
 *
 * Rules.  The caller owns all memory; a call allocates nothing, keeps no state, takes no lock, never synchronises, never prints and
 * is asynchronous on `stream`, so it may sit inside a graph capture.  No atomics: results are bit-identical from call to call.
 * The geometry (nb_hermite6_plan_*) is a function of (N, precision) alone.
 *
 * Limits.  1 <= N <= 2^26 (NB_HERMITE6_MAX_BODIES).  Body indices are 32-bit, byte offsets 64-bit.
 *
 * Not built here: block time steps are nbody_hip_hermite6_block.h, many small systems in one launch nbody_hip_hermite6_ensemble.h;
 * block time steps of many systems with this scheme, a pairwise or sharded form and the 8th-order scheme are not built.
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null pointer; N out of range; an array or the workspace
 * not aligned to 4*sizeof(T) (dt_out: sizeof(T), scratch: 8); workspace_bytes / scratch_bytes too small; any two arrays of a call
 * overlapping (but new_positions == old_positions, and acc_out == acc_in).  Otherwise the launch's hipError_t (0 on success).
 */
#ifndef NBODY_HIP_HERMITE6_H
#define NBODY_HIP_HERMITE6_H

#include <stddef.h>

#include "nbody_hip.h" /* nb_stream_t, NB_ERR_*; error names: nb_error_string */

#ifdef __cplusplus
extern "C" {
#endif

#define NB_HERMITE6_MAX_BODIES (1u << 26)
#define NB_HERMITE6_TIMESTEP_SCRATCH_BYTES 8192 /* = NB_HERMITE_TIMESTEP_SCRATCH_BYTES: partial minima, any content before the call */

typedef struct nb_hermite6_plan { /* the geometry of the evaluation kernel: the fields of nb_hermite_plan_t */
    int      bodies_per_lane; /* bodies i a lane holds (fp32: one packed pair, fp64: one)                          */
    int      waves_per_group; /* waves of a workgroup: they share the bodies i and split the bodies j             */
    int      unroll;          /* bodies j per scalar load group                                                   */
    unsigned groups;          /* workgroups                                                                       */
    unsigned block_threads;
    unsigned lds_bytes;
} nb_hermite6_plan_t;

/* 12 * num_bodies * sizeof_T (sizeof_T: 4 or 8) */
NB_API int nb_hermite6_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes);

NB_API int nb_hermite6_plan_f32(unsigned num_bodies, nb_hermite6_plan_t* plan);
NB_API int nb_hermite6_plan_f64(unsigned num_bodies, nb_hermite6_plan_t* plan);

/* accelerations, jerks and snaps of a state; nothing is integrated, positions, velocities and acc_in are only read */
NB_API int nb_hermite6_eval_f32(float* acc_out, float* jerk_out, float* snap_out, const float* positions, const float* velocities,
                                const float* acc_in, void* workspace, size_t workspace_bytes, unsigned num_bodies, float softening_sq,
                                nb_stream_t stream);
NB_API int nb_hermite6_eval_f64(double* acc_out, double* jerk_out, double* snap_out, const double* positions, const double* velocities,
                                const double* acc_in, void* workspace, size_t workspace_bytes, unsigned num_bodies, double softening_sq,
                                nb_stream_t stream);

/* the start of a run: a, jerk, snap of the state, crackle = 0 */
NB_API int nb_hermite6_init_f32(float* accelerations, float* jerks, float* snaps, float* crackles, const float* positions,
                                const float* velocities, void* workspace, size_t workspace_bytes, unsigned num_bodies, float softening_sq,
                                nb_stream_t stream);
NB_API int nb_hermite6_init_f64(double* accelerations, double* jerks, double* snaps, double* crackles, const double* positions,
                                const double* velocities, void* workspace, size_t workspace_bytes, unsigned num_bodies, double softening_sq,
                                nb_stream_t stream);

/* one 6th-order Hermite step (see above) */
NB_API int nb_hermite6_step_f32(float* new_positions, const float* old_positions, float* velocities, float* accelerations, float* jerks,
                                float* snaps, float* crackles, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                float delta_time, float softening_sq, nb_stream_t stream);
NB_API int nb_hermite6_step_f64(double* new_positions, const double* old_positions, double* velocities, double* accelerations, double* jerks,
                                double* snaps, double* crackles, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                double delta_time, double softening_sq, nb_stream_t stream);

/* dt_out[0] (device) = eta * sqrt(min (|a||s| + |j|^2) / (|j||c| + |s|^2)); scratch: NB_HERMITE6_TIMESTEP_SCRATCH_BYTES device bytes */
NB_API int nb_hermite6_timestep_f32(const float* accelerations, const float* jerks, const float* snaps, const float* crackles,
                                    unsigned num_bodies, float eta, float* dt_out, void* scratch, size_t scratch_bytes, nb_stream_t stream);
NB_API int nb_hermite6_timestep_f64(const double* accelerations, const double* jerks, const double* snaps, const double* crackles,
                                    unsigned num_bodies, double eta, double* dt_out, void* scratch, size_t scratch_bytes, nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_HERMITE6_H */
