/*
 * nbody_hip_hermite_block.h -- 4th-order Hermite steps with BLOCK TIME STEPS (libnbody_hip_hermite_block.so).
 *
 * nb_hermite_step_* (nbody_hip_hermite.h) moves every body by the same dt, so one hard binary sets the price of all N^2 interactions.
 * Here every body has a step of its own, a power-of-two fraction of dt_max (Makino 1991; Makino & Aarseth 1992), and one block step
 * evaluates only the n_act bodies that are due against all N: n_act * N interactions.
 *
 * This library links none of the other libraries and reads no process-global setting.  Error codes are the NB_ERR_* / hipError_t
 * values of nbody_hip.h.  Arrays are those of nbody_hip_hermite.h (positions {x, y, z, m}, velocities {vx, vy, vz, w}, accelerations,
 * jerks: T[4*N] each, T = float | double) and, per body, all caller-owned device arrays:
 *   ticks   uint64[N]  the time of the body's stored state, in ticks
 *   levels  int32[N]   the body's level k_i
 *   status  one nb_hermite_block_status_t (64 bytes)
 *   workspace  nb_hermite_block_workspace_bytes(N, sizeof T) bytes; content before a call does not matter, nothing is kept in it
 *              between calls: the predicted state {x, y, z, m, vx, vy, vz, 0} of every body, the partial sums, the active list,
 *              the schedule's counts and minima, one control record.  The predicted state is its first 8*N T.
 *
 * THE SCHEME.  Parameters {eta, eta_start, dt_max, max_level} (doubles > 0; 0 <= max_level <= 40).  One tick is
 * q = dt_max * 2^-max_level; body i's step is dt_i = dt_max * 2^-k_i = ticks(k_i) = 2^(max_level - k_i) ticks.  Times are integers,
 * so any dt_max gives exact comparisons; a real interval is ticks * q, formed in fp64 and rounded to T once.
 *
 *  init        a, jerk = eval(x, v) (nb_hermite_eval_*, same floor for softening_sq == 0); want = eta_start * |a| / |jerk| (dt_max when
 *              the ratio is not finite and positive); k_i = the smallest level with dt_max * 2^-k <= want, clamped to
 *              [0, max_level]; tick_i = 0.  The status record is cleared.
 *  block step  now = min_i (tick_i + ticks(k_i));  active = {i : tick_i + ticks(k_i) == now}.
 *              Predict EVERY body to `now` with its own tau_j = (now - tick_j) * q (the predictor of nb_hermite_step_*) into the
 *              workspace.  For the active bodies only: a1, j1 = the sums of nbody_hip_hermite.h over all predicted j; the
 *              corrector of nb_hermite_step_* with dt = dt_i; then, with h = dt_i,
 *                  a2  = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2,   a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3,   a2' = a2 + h a3,
 *                  dt_A = sqrt(eta (|a1| |a2'| + |j1|^2) / (|j1| |a3| + |a2'|^2))      (dt_max when not finite).
 *              New level: if dt_A < dt_i, halve until <= dt_A or max_level; else if dt_A >= 2 dt_i, k_i > 0 and `now` is a multiple
 *              of 2 ticks(k_i), double once; else keep.  tick_i = now.  Inactive bodies' stored state is not touched.
 *              dt_A is computed in fp64 from the STORED T-typed a0, j0, a1, j1 in both precisions, with h = ticks(k_i) * q in fp64.
 *  t_stop      a block step whose now * q (fp64) would exceed t_stop changes nothing but sets NB_HERMITE_BLOCK_STOPPED in
 *              status.flags (a step that runs clears it).  So a caller enqueues calls in batches and reads 64 bytes when it likes.
 *  consequence every tick_i is a multiple of ticks(k_i): at every multiple of dt_max all bodies are active and the state is
 *              synchronised.
 *  sync        nb_hermite_block_sync_*: every body predicted to status.now_ticks into caller arrays ({x, y, z, m}, {vx, vy, vz, w}):
 *              a synchronised snapshot for output and nb_energy_*; the stored state is only read.
 *
 * Operand range.  The sums a1, j1 are those of nb_hermite_eval_* and are held to the same bounds over the same range of s^2, masses
 * and velocities (nbody_hip_hermite.h, "Operand range": s^2 in [2^-84, 2^84] (fp32) / [2^-600, 2^600] (fp64), masses 0 or of magnitude
 * in [2^-40, 2^40] / [2^-100, 2^100]), with one difference: the partial planes are stored in units of the first body's mass m_0 when
 * 2^-20 <= |m_0| <= 2^20 (fp32; 2^+-60 fp64), so the sums of term magnitudes A_i and J_i may reach 2^126 min(1, |m_0|) (fp32) /
 * 2^1022 min(1, |m_0|) (fp64) only: 2^106 behind a first body of 2^-20; beyond that a body's sums may be infinite or NaN.  dt_A and
 * init's want are plain fp64 expressions -- squares and products of two norms: they follow the rule above while |a|^2, |j|^2,
 * |a2'|^2, |a3|^2 and their pairwise products are normal doubles -- always in fp32, in fp64 with every nonzero norm in
 * [2^-250, 2^250].  Beyond that range the result is what the fp64 expression gives: dt_max (a larger step) where it is infinite or
 * NaN -- a square or product overflowed, or the denominator underflowed to 0; init: also where want is 0 -- and for dt_A a finite
 * value that can be too small, down to 0 (the deepest level), where the numerator underflowed over a denominator that did not.
 *
 * Status.  now_ticks: the time of the last block step taken; block_steps; body_steps = sum of n_act; last_active = n_act of the
 * last block step; deepest_level: the deepest level any body held when a block step began; flags.  Written by single lanes with
 * ordinary stores, read by the caller after synchronising the stream.
 *
 * Geometry (nb_hermite_block_plan_*): a function of (N, n_act, precision) alone, never of the device or the stream.  The evaluation's
 * workgroups own one tile of 64 * bodies_per_lane active bodies and one of `ranges` (J) contiguous ranges of the chunks of 128 bodies
 * j: S = waves_per_group from N as nb_hermite_plan_*, tiles = ceil(n_act / tile), J = the smallest power of two with tiles * J >= 512,
 * capped at the largest power of two <= chunks / S.  The launch holds `launch_groups` workgroups whatever n_act is (it is read on
 * the device); the tiles * J first ones work.  Partial sums: planes [J][6][slots], slots = tiles * tile, at partial_offset.
 *
 * Rules.  The caller owns all memory; a call allocates nothing, keeps no state, takes no lock, never synchronises, never prints and
 * is asynchronous on `stream`, so it may sit inside a graph capture.  No atomics, every sum in a fixed order: results are
 * bit-identical from call to call.  A block step is 6 launches.
 *
 * Limits.  1 <= N <= 2^24 (NB_HERMITE_BLOCK_MAX_BODIES): the scan of the per-workgroup active counts is one workgroup whose lanes
 * fold N / 2^18 counts each.  Body indices are 32-bit, byte offsets 64-bit.
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null pointer; N (or num_active) out of range; an array not
 * aligned to 4*sizeof(T) (ticks, status: 8; levels: 4; workspace: 32); workspace_bytes too small; any two arrays of a call
 * overlapping; a parameter that is not finite and positive, max_level outside [0, 40], a tick that is not a normal double; a NaN
 * t_stop.  Otherwise the launch's hipError_t (0 on success).
 */
#ifndef NBODY_HIP_HERMITE_BLOCK_H
#define NBODY_HIP_HERMITE_BLOCK_H

#include <stddef.h>
#include <stdint.h>

#include "nbody_hip.h" /* nb_stream_t, NB_ERR_*; error names: nb_error_string */

#ifdef __cplusplus
extern "C" {
#endif

#define NB_HERMITE_BLOCK_MAX_BODIES (1u << 24)
#define NB_HERMITE_BLOCK_MAX_LEVEL 40
#define NB_HERMITE_BLOCK_STOPPED 1u /* status.flags: the last call would have passed t_stop and did nothing */

typedef struct nb_hermite_block_params {
    double eta;       /* accuracy parameter of dt_A                                  */
    double eta_start; /* ... of the first step, from |a| / |jerk|                    */
    double dt_max;    /* the step of level 0                                         */
    int    max_level; /* the deepest level: steps down to dt_max * 2^-max_level      */
    int    reserved;
} nb_hermite_block_params_t;

typedef struct nb_hermite_block_status { /* 64 bytes, device memory */
    uint64_t now_ticks;
    uint64_t block_steps;
    uint64_t body_steps;
    uint32_t last_active;
    int32_t  deepest_level;
    uint32_t flags;
    uint32_t reserved[7];
} nb_hermite_block_status_t;

typedef struct nb_hermite_block_plan { /* the geometry of the evaluation of one block step */
    int                bodies_per_lane; /* active bodies a lane holds (fp32: one packed pair, fp64: one)       */
    int                waves_per_group; /* S: waves of a workgroup; they share the tile and split the range    */
    int                unroll;          /* bodies j per scalar load group                                      */
    unsigned           tiles;           /* ceil(num_active / (64 * bodies_per_lane))                           */
    unsigned           ranges;          /* J                                                                   */
    unsigned           groups;          /* tiles * ranges: the workgroups that work                            */
    unsigned           launch_groups;   /* the workgroups launched: >= groups for every num_active <= N        */
    unsigned           block_threads;
    unsigned           lds_bytes;
    unsigned           slots;           /* tiles * 64 * bodies_per_lane: the stride of a partial plane         */
    unsigned           chunks;          /* ceil(N / 128)                                                       */
    unsigned           launches;        /* kernel launches of one block step                                   */
    unsigned long long partial_offset;  /* byte offset of the partial planes in the workspace                  */
    unsigned long long partial_bytes;   /* ranges * 6 * slots * sizeof(T)                                      */
} nb_hermite_block_plan_t;

NB_API int nb_hermite_block_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes);

NB_API int nb_hermite_block_plan_f32(unsigned num_bodies, unsigned num_active, nb_hermite_block_plan_t* plan);
NB_API int nb_hermite_block_plan_f64(unsigned num_bodies, unsigned num_active, nb_hermite_block_plan_t* plan);

/* accelerations, jerks, levels, ticks and the status record from positions and velocities */
NB_API int nb_hermite_block_init_f32(float* positions, float* velocities, float* accelerations, float* jerks, uint64_t* ticks, int32_t* levels,
                                     nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                     float softening_sq, const nb_hermite_block_params_t* params, nb_stream_t stream);
NB_API int nb_hermite_block_init_f64(double* positions, double* velocities, double* accelerations, double* jerks, uint64_t* ticks, int32_t* levels,
                                     nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                     double softening_sq, const nb_hermite_block_params_t* params, nb_stream_t stream);

/* one block step (see above), or nothing but the flag when it would pass t_stop */
NB_API int nb_hermite_block_step_f32(float* positions, float* velocities, float* accelerations, float* jerks, uint64_t* ticks, int32_t* levels,
                                     nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                     float softening_sq, const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream);
NB_API int nb_hermite_block_step_f64(double* positions, double* velocities, double* accelerations, double* jerks, uint64_t* ticks, int32_t* levels,
                                     nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies,
                                     double softening_sq, const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream);

/* every body predicted to status.now_ticks -> positions_out, velocities_out */
NB_API int nb_hermite_block_sync_f32(float* positions_out, float* velocities_out, const float* positions, const float* velocities,
                                     const float* accelerations, const float* jerks, const uint64_t* ticks, const nb_hermite_block_status_t* status,
                                     unsigned num_bodies, const nb_hermite_block_params_t* params, nb_stream_t stream);
NB_API int nb_hermite_block_sync_f64(double* positions_out, double* velocities_out, const double* positions, const double* velocities,
                                     const double* accelerations, const double* jerks, const uint64_t* ticks, const nb_hermite_block_status_t* status,
                                     unsigned num_bodies, const nb_hermite_block_params_t* params, nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_HERMITE_BLOCK_H */
