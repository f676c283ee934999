/*
 * nbody_hip_hermite6_block.h -- 6th-order Hermite steps with BLOCK TIME STEPS (libnbody_hip_hermite6_block.so).
 *
 * nb_hermite6_step_* (nbody_hip_hermite6.h) moves every body by one shared dt, so one hard binary sets the price of all N^2
 * interactions; nb_hermite_block_* (nbody_hip_hermite_block.h) gives every body a step of its own but is 4th order, and its runs are
 * bound by the NUMBER of block steps.  Here the 6th-order scheme (Nitadori & Makino 2008) runs on the block schedule: every body has
 * a power-of-two fraction of dt_max for a step, one block step evaluates the n_act bodies that are due against all N, and the higher
 * order takes longer steps at the same error -- fewer block steps.
 *
 * This library links none of the other libraries and reads no process-global setting.  Error codes are the NB_ERR_* / hipError_t
 * values of nbody_hip.h.  Parameters (nb_hermite_block_params_t), the status record (nb_hermite_block_status_t), the plan struct
 * (nb_hermite_block_plan_t), NB_HERMITE_BLOCK_MAX_BODIES, NB_HERMITE_BLOCK_MAX_LEVEL and the flag NB_HERMITE_BLOCK_STOPPED are the types
 * and constants of nbody_hip_hermite_block.h, which is included for them alone: no function of that library is needed.
 *
 * State of a system of N bodies, all caller-owned device arrays, T = float | double:
 *   positions, velocities, accelerations, jerks, snaps, crackles   T[4*N] each, in the layouts of nbody_hip_hermite6.h
 *                                                                  ({x, y, z, m}, {vx, vy, vz, w}, {.., 0}); velocities.w is preserved
 *   ticks   uint64[N]  the time of the body's stored state, in ticks
 *   levels  int32[N]   the body's level k_i
 *   status  one nb_hermite_block_status_t (64 bytes)
 *   workspace  nb_hermite6_block_workspace_bytes(N, sizeof T) bytes; content before a call does not matter, nothing is kept in it
 *              between calls.  Its first 12*N T hold the predicted state {x, y, z, m, vx, vy, vz, 0, ax, ay, az, 0} per body; behind
 *              that the partial planes [J][9][slots], the active list, the schedule's counts and partial minima, one control record,
 *              each section on a 256-byte boundary.
 *
 * THE SCHEME.  Ticks, levels, t_stop, the level-change rule and the status counters are exactly those of nbody_hip_hermite_block.h:
 * parameters {eta, eta_start, dt_max, max_level} (doubles > 0; 0 <= max_level <= 40); one tick is q = dt_max * 2^-max_level; body i's
 * step is dt_i = dt_max * 2^-k_i = ticks(k_i) = 2^(max_level - k_i) ticks; a real interval is ticks * q, formed in fp64 and rounded to
 * T once.
 *
 *  init        1. a, jerk, snap, crackle are the bits nb_hermite6_init_* gives: two passes of pack and evaluate (the second with the
 *                 first's a for the snap), then crackle = 0; softening_sq == 0 takes the same floor.
 *              2. want = eta_start * |a| / |jerk|; dt_max when the ratio is not finite and positive.
 *              3. k_i = the smallest level k with dt_max * 2^-k <= want, clamped to [0, max_level].
 *              4. tick_i = 0; the status record is cleared.
 *  block step  1. now = min_i (tick_i + ticks(k_i));  active = {i : tick_i + ticks(k_i) == now}.
 *              2. Predict EVERY body to `now` with its own tau_j = (now - tick_j) * q into the workspace, by the 6th-order predictor
 *                 of nb_hermite6_step_* (Horner form to the crackle, the expressions of that library's predictor):
 *                    x_p = x + v h + a h^2/2 + j h^3/6 + s h^4/24 + c h^5/120
 *                    v_p = v + a h + j h^2/2 + s h^3/6 + c h^4/24
 *                    a_p = a + j h + s h^2/2 + c h^3/6                                  (h = tau_j; tau_j = 0 gives the stored bits)
 *              3. For the active bodies only: a1, j1, s1 = the sums of nbody_hip_hermite6.h over all predicted j; the body's own
 *                 a_p is its a_i.
 *              4. The corrector of nb_hermite6_step_* with h = dt_i, and the new crackle:
 *                    v1 = v + (a + a1) h/2 - (j1 - j) h^2/10 + (s + s1) h^3/120
 *                    x1 = x + (v + v1) h/2 - (a1 - a) h^2/10 + (j + j1) h^3/120
 *                    D0 = a1 - a - j h - s h^2/2,  D1 = (j1 - j - s h) h,  D2 = (s1 - s) h^2,   c1 = (60 D0 - 36 D1 + 9 D2) / h^3
 *                 in that library's expressions, the small terms summed first.
 *              5. The body's step, in fp64 from the STORED T-typed a1, j1, s1, c1 in both precisions:
 *                    dt_A = sqrt(eta (|a1| |s1| + |j1|^2) / (|j1| |c1| + |s1|^2))          (dt_max when not finite)
 *                 with |.| = sqrt(x^2 + y^2 + z^2): Aarseth's criterion with the derivatives the scheme holds, the ratio of
 *                 nb_hermite6_timestep_*.
 *              6. ETA SITS INSIDE THE ROOT HERE, as in nb_hermite_block_*; it sits OUTSIDE the root in nb_hermite6_timestep_*.
 *                 eta ~ 0.2 here matches eta ~ 0.02 of the 4th-order block library: on that library's binary test problem (256
 *                 bodies, one hard binary, to t = 1) it gives a sixth of the energy error with a quarter of the block steps and
 *                 0.37 of the interactions.
 *              7. New level by the 4th-order library's rule: if dt_A < dt_i, halve until <= dt_A or max_level; else if
 *                 dt_A >= 2 dt_i, k_i > 0 and `now` is a multiple of 2 ticks(k_i), double once; else keep.  tick_i = now.  Inactive
 *                 bodies' stored state is not touched.
 *  t_stop      a block step whose now * q (fp64) would exceed t_stop changes nothing but sets NB_HERMITE_BLOCK_STOPPED in
 *              status.flags (a step that runs clears it).
 *  consequence every tick_i is a multiple of ticks(k_i): at every multiple of dt_max all bodies are active and the state is
 *              synchronised.
 *  sync        nb_hermite6_block_sync_*: every body predicted to status.now_ticks into caller arrays ({x, y, z, m}, {vx, vy, vz, w})
 *              by the same 6th-order predictor; .w of the velocity is preserved; the stored state is only read.
 *
 * Operand range.  The sums a1, j1, s1 are those of nb_hermite6_eval_* and are held to the same bounds over the same range
 * (nbody_hip_hermite6.h, "Operand range"), with one difference: the partial planes are stored in units of the first body's mass m_0
 * when 2^-20 <= |m_0| <= 2^20 (fp32; 2^+-60 fp64), and there is no escape to plain units, so the sums of term magnitudes A_i, J_i and
 * S_i may reach 2^126 min(1, |m_0|) (fp32) / 2^1022 min(1, |m_0|) (fp64) only; beyond that a body's sums may be infinite or NaN.  dt_A
 * and init's want are plain fp64 expressions -- products of two norms: they follow the rule above while |a|^2, |j|^2, |s|^2, |c|^2
 * and their pairwise products are normal doubles -- always in fp32, in fp64 with every nonzero norm in [2^-250, 2^250].  Beyond that
 * range the result is what the fp64 expression gives: dt_max (a larger step) where it is infinite or NaN -- a square or product
 * overflowed, or the denominator underflowed to 0; init: also where want is 0 -- and for dt_A a finite value that can be too small,
 * down to 0 (the deepest level), where the numerator underflowed over a denominator that did not.
 *
 * Range of h.  The corrector divides by h^3, formed in T as (h h) h, for every step a body can take, from dt_max down to one tick
 * q = dt_max 2^-max_level: both cubes must be normal in T -- 2^-42 <= q and dt_max <= 2^42 (fp32) / 2^-340 <= q and dt_max <= 2^341
 * (fp64) --, and init, step and sync refuse parameters outside that range (fp32: dt_max = 2^-10 with max_level = 33).  Inside it c1 is
 * held to the evaluation's bounds carried through 60/h^3, 36/h^2 and 9/h, and finite sums give a finite state.
 *
 * Status.  As nbody_hip_hermite_block.h: now_ticks, block_steps, body_steps = sum of n_act, last_active, deepest_level, flags.
 *
 * Geometry (nb_hermite6_block_plan_*): a function of (N, n_act, precision) alone.  The fields of nb_hermite_block_plan_t with the number
 * of partial sums (9) where that library's formulas use 6: tiles = ceil(n_act / tile), J = the smallest power of two with
 * tiles * J >= 512, capped at the largest power of two <= chunks / S; unroll = 2 (fp32) / 1 (fp64);
 * lds_bytes = max(S - 1, 1) * 9 * tile * sizeof(T) + 128; partial planes [J][9][slots] at partial_offset,
 * partial_bytes = J * 9 * slots * sizeof(T).
 *
 * Rules.  The caller owns all memory; a call allocates nothing, keeps no state, takes no lock, never synchronises, never prints and
 * is asynchronous on `stream`, so it may sit inside a graph capture.  No atomics, every sum in a fixed order: results are
 * bit-identical from call to call.  A block step is 6 launches, init is 5.
 *
 * Limits.  1 <= N <= 2^24 (NB_HERMITE_BLOCK_MAX_BODIES).  Body indices are 32-bit, byte offsets 64-bit.
 *
 * Not built here: block time steps of many systems with this scheme are nbody_hip_hermite6_block_ensemble.h, which takes this library's
 * step per system, bit for bit.  Not built: a pairwise or sharded form.
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null pointer; N (or num_active) out of range; an array not
 * aligned to 4*sizeof(T) (ticks, status: 8; levels: 4; workspace: 32); workspace_bytes too small; any two arrays of a call
 * overlapping; a parameter that is not finite and positive, max_level outside [0, 40], a tick that is not a normal double, a tick or a
 * dt_max whose cube is not a normal T ("Range of h"); a NaN t_stop.  Otherwise the launch's hipError_t (0 on success).
 */
#ifndef NBODY_HIP_HERMITE6_BLOCK_H
#define NBODY_HIP_HERMITE6_BLOCK_H

#include <stddef.h>
#include <stdint.h>

#include "nbody_hip_hermite_block.h" /* for its types alone: nb_hermite_block_params_t, _status_t, _plan_t, NB_HERMITE_BLOCK_* */

#ifdef __cplusplus
extern "C" {
#endif

NB_API int nb_hermite6_block_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes);

NB_API int nb_hermite6_block_plan_f32(unsigned num_bodies, unsigned num_active, nb_hermite_block_plan_t* plan);
NB_API int nb_hermite6_block_plan_f64(unsigned num_bodies, unsigned num_active, nb_hermite_block_plan_t* plan);

/* accelerations, jerks, snaps, crackles, levels, ticks and the status record from positions and velocities */
NB_API int nb_hermite6_block_init_f32(float* positions, float* velocities, float* accelerations, float* jerks, float* snaps, float* crackles, uint64_t* ticks,
                                      int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                      float softening_sq, const nb_hermite_block_params_t* params, nb_stream_t stream);
NB_API int nb_hermite6_block_init_f64(double* positions, double* velocities, double* accelerations, double* jerks, double* snaps, double* crackles, uint64_t* ticks,
                                      int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                      double softening_sq, const nb_hermite_block_params_t* params, nb_stream_t stream);

/* one block step (see above), or nothing but the flag when it would pass t_stop */
NB_API int nb_hermite6_block_step_f32(float* positions, float* velocities, float* accelerations, float* jerks, float* snaps, float* crackles, uint64_t* ticks,
                                      int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                      float softening_sq, const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream);
NB_API int nb_hermite6_block_step_f64(double* positions, double* velocities, double* accelerations, double* jerks, double* snaps, double* crackles, uint64_t* ticks,
                                      int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                      double softening_sq, const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream);

/* every body predicted to status.now_ticks -> positions_out, velocities_out */
NB_API int nb_hermite6_block_sync_f32(float* positions_out, float* velocities_out, const float* positions, const float* velocities, const float* accelerations,
                                      const float* jerks, const float* snaps, const float* crackles, const uint64_t* ticks,
                                      const nb_hermite_block_status_t* status, unsigned num_bodies, const nb_hermite_block_params_t* params, nb_stream_t stream);
NB_API int nb_hermite6_block_sync_f64(double* positions_out, double* velocities_out, const double* positions, const double* velocities, const double* accelerations,
                                      const double* jerks, const double* snaps, const double* crackles, const uint64_t* ticks,
                                      const nb_hermite_block_status_t* status, unsigned num_bodies, const nb_hermite_block_params_t* params, nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_HERMITE6_BLOCK_H */
