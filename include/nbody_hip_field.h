/*
 * nbody_hip_field.h -- acceleration, jerk and potential of N sources at M points of the caller's own (libnbody_hip_field.so).
 *
 * Every other force call of the project evaluates a state on itself.  This one is the interface of the GRAPE-6 family of force
 * libraries: j-particles in, i-particles in, acceleration + jerk + potential out.  It serves massless tracers, potential and force
 * maps, callers who keep their own integrator or regularise their own binaries, and callers who shard the sources over devices
 * themselves and add the partial sums.
 *
 * This library links none of the other libraries and reads no process-global setting.  Error codes are the NB_ERR_* / hipError_t
 * values of nbody_hip.h.  T = float | double; all arrays are caller-owned device memory.
 *
 * Inputs.
 *   sources            T[4*N] = {x, y, z, mass}
 *   source_velocities  T[4*N] = {vx, vy, vz, -}, or NULL
 *   targets            T[4*M] = {x, y, z, -}; .w is ignored, so a positions array or a slice of one can be passed as it is
 *   target_velocities  T[4*M] = {ux, uy, uz, -}, or NULL
 *   self_index         unsigned[M], or NULL
 *
 * Definition.  With r = x_j - p_k, w = v_j - u_k and s^2 = r.r + softening_sq, over all j in [0, N):
 *   a_k    =  sum m s^-3 r
 *   jerk_k =  sum m s^-3 (w - 3 (r.w) s^-2 r)
 *   phi_k  = -sum m s^-1
 * softening_sq == 0 is evaluated with the floor of nbody_hip_hermite.h: s^2 = r.r + 2^-60 (fp32) / 2^-300 (fp64).  A coincident pair
 * (r = 0) then contributes exactly 0 to a, and exactly 0 to the jerk when w = 0 as well (a body met as its own source); with w != 0 the
 * jerk term is m w / s^3 with s at the floor, as the formula says.  The potential uses the same s^2: a coincident pair that is NOT
 * excluded contributes -m * 2^30 (fp32) / -m * 2^150 (fp64) at softening 0.  Callers exclude such a pair by index.
 *
 * Operand range.  That of nb_hermite_eval_* (nbody_hip_hermite.h, "Operand range"): the sums are held to 5e-6 (fp32) / 1e-14 (fp64)
 * times a target's sums of term magnitudes A_k, J_k and P_k = sum |m| s^-1, and a single term to 1e-6 / 1e-14 (a, phi) and
 * 5e-6 / 1e-14 (jerk) of its magnitude, for
 *   s^2 of every pair in [2^-84, 2^84] (fp32) / [2^-600, 2^600] (fp64);
 *   masses 0 or of magnitude in [2^-40, 2^40] (fp32) / [2^-100, 2^100] (fp64), any sign;
 *   velocities with |r| |w| of every pair, and the sums A_k, J_k and P_k, at most 2^126 (fp32) / 2^1022 (fp64).
 * The sums are in plain units: no source's mass is a unit, and a source's term has the same bits whatever the other sources of its
 * chunk weigh.  Outside the range nothing is clamped (nbody_hip_hermite.h says what s^-3 does); non-finite inputs are ordinary data,
 * and exclusion is "mass 0": an excluded source with a NaN or infinite MASS reaches no result of the targets that exclude it, one with
 * a non-finite coordinate or velocity reaches them as 0 * NaN does.
 *
 * Exclusion is by INDEX, never by distance.  In the sums of target k, m is m_j, except that it is taken as 0 when j == self_index[k].
 * NB_FIELD_NONE (0xFFFFFFFF), or a NULL array, excludes nobody.  Because exclusion is defined as "mass 0" it is exact: excluding j gives
 * the bits of the same call with m_j = 0 and no exclusion.
 *
 * Outputs.  Each may be NULL and is then not stored; at least one must be given; jerks != NULL requires both velocity arrays.
 *   accelerations  T[4*M] = {ax, ay, az, 0}
 *   jerks          T[4*M] = {jx, jy, jz, 0}
 *   potentials     T[M]
 * Which outputs are stored changes no bit of the others.
 *
 * Aliasing.  Inputs are only read and may alias each other; targets == sources is the common case.  An output overlapping any other
 * array of the call is refused.
 *
 * A target's results depend on its own data (position, velocity, self_index), on the sources and on (N, M, precision), and on nothing
 * else: not on the targets beside it, not on its slot in the array, not on which other targets carry a self_index.  Permuting the
 * targets permutes the outputs bit for bit.
 *
 * Geometry (nb_field_plan_*): a function of (N, M, precision) alone.  A workgroup owns one tile of 64 * bodies_per_lane targets and one
 * of `ranges` (J) contiguous ranges of the chunks of 128 sources; its S = waves_per_group waves split the range's chunks and fold
 * through LDS in wave order.  S is nb_hermite_plan_*'s for N; tiles = ceil(M / (64 * bodies_per_lane)); J is the smallest power of two
 * with tiles * J >= 512, capped at the largest power of two <= chunks / S; groups = tiles * J.  With J = 1 the evaluation stores the
 * outputs itself (one launch); with J > 1 it stores partial planes [J][4 or 7][tiles * 64 * bodies_per_lane] of T into the workspace and
 * a second kernel, one lane per target, adds them in range order (two launches).
 *
 * Rules.  The caller owns all memory; a call allocates nothing, keeps no state, takes no lock, never synchronises, never prints and is
 * asynchronous on `stream`, so it may sit inside a graph capture.  No atomics, every sum in an order fixed by the geometry: results
 * are bit-identical from call to call.  The workspace (nb_field_workspace_bytes; 0 bytes when J = 1, and then it may be NULL) is
 * caller-owned; its content before a call does not matter and nothing is kept in it between calls.
 *
 * Limits.  1 <= N <= 2^26 (NB_FIELD_MAX_SOURCES), 1 <= M <= 2^24 (NB_FIELD_MAX_TARGETS).  Indices are 32-bit, byte offsets 64-bit.
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null sources or targets (or a null workspace when
 * nb_field_workspace_bytes is not 0); N or M out of range; a 4-vector array not aligned to 4*sizeof(T), potentials to sizeof(T),
 * self_index to 4, the workspace to 32; workspace_bytes too small; an output (or the workspace) overlapping any other array of the
 * call; a negative or NaN softening_sq; jerks given without both velocity arrays; no output at all.  Otherwise the launch's hipError_t
 * (0 on success).
 */
#ifndef NBODY_HIP_FIELD_H
#define NBODY_HIP_FIELD_H

#include <stddef.h>

#include "nbody_hip.h" /* nb_stream_t, NB_ERR_*; error names: nb_error_string */

#ifdef __cplusplus
extern "C" {
#endif

#define NB_FIELD_MAX_SOURCES (1u << 26)
#define NB_FIELD_MAX_TARGETS (1u << 24)
#define NB_FIELD_NONE 0xFFFFFFFFu

typedef struct nb_field_plan {
    int                bodies_per_lane; /* targets a lane holds (fp32: one packed pair, fp64: one)                          */
    int                waves_per_group; /* S: waves of a workgroup; they share the tile, split the range's chunks           */
    int                unroll;          /* sources per scalar load group                                                    */
    unsigned           tiles;           /* ceil(M / (64 * bodies_per_lane))                                                 */
    unsigned           ranges;          /* J                                                                                */
    unsigned           groups;          /* tiles * J: the evaluation's workgroups                                           */
    unsigned           block_threads;   /* 64 * S                                                                           */
    unsigned           lds_bytes;       /* of an evaluation workgroup that computes the jerk (the larger form)              */
    unsigned           launches;        /* kernel launches of one call: 1 (J = 1) or 2                                      */
    unsigned           reserved;
    unsigned long long partial_offset;  /* byte offset of the partial planes in the workspace                               */
    unsigned long long partial_bytes;   /* J * 7 * tiles * 64 * bodies_per_lane * sizeof(T); 0 when J = 1                   */
} nb_field_plan_t;

NB_API int nb_field_workspace_bytes(unsigned num_sources, unsigned num_targets, unsigned sizeof_T, size_t* bytes);

NB_API int nb_field_plan_f32(unsigned num_sources, unsigned num_targets, nb_field_plan_t* plan);
NB_API int nb_field_plan_f64(unsigned num_sources, unsigned num_targets, nb_field_plan_t* plan);

NB_API int nb_field_eval_f32(const float* sources, const float* source_velocities, unsigned num_sources, const float* targets,
                             const float* target_velocities, const unsigned* self_index, unsigned num_targets, float softening_sq,
                             float* accelerations, float* jerks, float* potentials, void* workspace, size_t workspace_bytes,
                             nb_stream_t stream);
NB_API int nb_field_eval_f64(const double* sources, const double* source_velocities, unsigned num_sources, const double* targets,
                             const double* target_velocities, const unsigned* self_index, unsigned num_targets, double softening_sq,
                             double* accelerations, double* jerks, double* potentials, void* workspace, size_t workspace_bytes,
                             nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_FIELD_H */
