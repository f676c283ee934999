/*
 * nbody_hip_neighbour.h -- nearest neighbours, potentials and neighbour lists of a state (libnbody_hip_neighbour.so).
 *
 * Three questions about every body i of a state, answered exactly, over all pairs, in one asynchronous call: which body is closest
 * and how close; how many (and which) bodies lie within a radius; what the potential is at the body.  They are what the users of
 * nb_hermite_block_* (nbody_hip_hermite_block.h) start from when they look for hard binaries or keep Ahmad-Cohen neighbour lists.
 *
 * This library links none of the other libraries and reads no process-global setting.  Error codes are the NB_ERR_* / hipError_t
 * values of nbody_hip.h.  T = float | double; positions are T[4*N] = {x, y, z, mass}.
 *
 * THE DISTANCE.  With dx = x_j - x_i, dy = y_j - y_i, dz = z_j - z_i, each one rounding in T,
 *
 *                d2(i, j) = fma(dx, dx, fma(dy, dy, dz * dz))                                  (NB_NEIGHBOUR_DIST_SQ below)
 *
 * in T: one product and two fused multiply-adds, three roundings.  Every kernel of the library computes d2 by this expression and no
 * other, so d2(i, j) and d2(j, i) are the same bits (negating dx, dy, dz changes no product), and the survey and the lists agree with
 * each other exactly.  "Self" means j == i by INDEX, never by distance: a distinct body at the same place is a neighbour at distance
 * 0.  A NaN d2 never compares less, so such a pair is never a neighbour; neither is a d2 that is not less than +inf.
 *
 * nb_neighbour_survey_*  for every body i; each output array may be NULL and is then not stored (at least one must be given):
 *   nearest_index[i]    unsigned  the j != i of smallest d2(i, j), the LOWEST such j on equal bits; NB_NEIGHBOUR_NONE if there is none
 *                                 (N = 1, or no d2 that compares less than +inf)
 *   nearest_dist_sq[i]  T         that d2; +inf if there is none
 *   counts[i]           unsigned  the number of j != i with d2(i, j) < r2_i (strict)
 *   potentials[i]       T         -sum_{j != i} m_j / sqrt(d2(i, j) + softening_sq); NULL: no v_rsq is spent.  At softening_sq = 0 a
 *                                 coincident distinct pair gives -inf, as the formula says; so does a pair whose d2 + softening_sq is
 *                                 SUBNORMAL (below: Operand range).  The order of the sum is fixed by the
 *                                 geometry (nb_neighbour_plan_*), so the bits repeat from call to call.
 *   r2_i is `radius_sq`, or radii_sq[i] when radii_sq != NULL (a device array T[N]: one-sided "gather" lists).  The caller passes
 *   SQUARED radii, so no rounding of a square is left undefined.  A NaN or negative r2_i in the array counts nobody.
 *
 * nb_neighbour_lists_*   the same relation {(i, j) : j != i, d2(i, j) < r2_i} as lists in CSR form:
 *   offsets[N + 1]      unsigned long long  the exclusive prefix of the counts; offsets[N] is their total
 *   indices[capacity]   unsigned            the list of body i is indices[offsets[i] .. offsets[i + 1]), ASCENDING in j
 *   The call is self-contained (count, scan, fill: 5 launches); it trusts no counts of an earlier survey.  When the total exceeds
 *   `capacity`, offsets is still complete and right, indices is left untouched, and the status record carries NB_NEIGHBOUR_OVERFLOW
 *   and the total needed: the fill kernel reads that decision on the device and returns at once; the host never synchronises and never
 *   learns the total unless it reads the record.  capacity may be 0 (indices may then be NULL): a call that only sizes the lists.
 *
 * Status (64 bytes of device memory, written by every call with ordinary stores of single lanes; read it after synchronising):
 *   total_neighbours   the sum of the counts (the capacity a lists call needs)
 *   closest_i < closest_j, closest_dist_sq   the pair of smallest d2, as a double (exact: T widened); on equal bits the lowest i, then the
 *                      lowest j.  NB_NEIGHBOUR_NONE, NB_NEIGHBOUR_NONE, +inf if no body has a nearest neighbour, and after a lists call,
 *                      which does not look for it.
 *   max_count, max_count_body   the largest count and the LOWEST body that has it (0, 0 when all counts are 0)
 *   flags              NB_NEIGHBOUR_OVERFLOW or 0
 * So a caller finds the hardest encounter of a 262 144-body state by reading 64 bytes.
 *
 * Operand range.  The exact outputs -- nearest_index, nearest_dist_sq, counts, the lists, the status record -- hold for EVERY input:
 * d2 is IEEE arithmetic in T with subnormals kept, in fp32 too, and every comparison sees it as it is.  So a subnormal d2 is not 0 (it is
 * less than a larger subnormal radius and not less than one equal to it), a d2 that overflows is +inf and nobody's neighbour, even at a
 * radius of +inf, and a NaN d2 (a NaN coordinate; two bodies at the same infinity) is nobody's neighbour either.  A body at an infinity
 * has no nearest neighbour and is in no list; -0.0 and +0.0 are one place.  The masses take no part in any of these.
 * The potentials are held to the formula while s2 = d2 + softening_sq is in [2^-126, 2^128) (fp32) / [2^-1022, 2^1021) (fp64): the
 * normal range of T, less the three binades at the top of fp64 in which the square of the v_rsq_f64 seed is subnormal.  One term is
 * then within 1e-6 (fp32) / 1e-14 (fp64) of -m_j / sqrt(s2) rounded to T (measured: 1.5e-7 / 3.0e-16); the measured
 * error in those three binades of fp64 is no larger.  A SUBNORMAL s2 is outside the range in both precisions:
 * v_rsq_f32 takes a subnormal operand as 0, and in fp64 the square of the seed is infinite below s2 = 2^-1024.  The term is then
 * -m_j * inf: -inf, as for a coincident pair at softening_sq = 0, and NaN where m_j is 0 (fp64 is still finite and within the bound
 * for a subnormal s2 above 2^-1024).  A pair with s2 = +inf adds m_j * 0, and so does the body's own slot, j = i: 0 for a finite mass.  So
 * a NaN or infinite mass makes every potential non-finite, its body's own included (-inf or NaN from the other bodies', NaN where s2 is
 * +inf and at its own), and reaches nothing else.
 *
 * Geometry (nb_neighbour_plan_*): a function of (N, precision) alone, never of the device, the stream or the outputs asked for.  The
 * survey's workgroups own one tile of 64 * bodies_per_lane bodies i (an aligned chunk of bodies j, or half of one in fp64); their S
 * waves split the chunks of 128 bodies j (chunk c -> wave c mod S) and fold through LDS in wave order.  The lists' count and fill
 * passes run one wave per (tile, range) over `list_ranges` (J) contiguous ranges of the chunks: J = the smallest power of two with
 * tiles * J >= 2048, capped at the largest power of two <= chunks.  Counts per range: planes [J][N] of unsigned in the workspace.
 *
 * Rules.  The caller owns all memory; a call allocates nothing, keeps no state, takes no lock, never synchronises, never prints and is
 * asynchronous on `stream`, so it may sit inside a graph capture.  No atomics, every sum in a fixed order: results are bit-identical
 * from call to call.  The workspace (nb_neighbour_workspace_bytes) is caller-owned; its content before a call does not matter and
 * nothing is kept in it between calls.  Inputs are only read.
 *
 * Limits.  1 <= N <= 2^24 (NB_NEIGHBOUR_MAX_BODIES).  Body indices are 32-bit, byte offsets and list offsets 64-bit.
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null positions, status or workspace (or offsets; or indices with
 * capacity > 0); no output array at all; N out of range; positions not aligned to 4*sizeof(T), radii_sq / nearest_dist_sq / potentials
 * to sizeof(T), the unsigned arrays to 4, offsets and status to 8, the workspace to 32; workspace_bytes too small; any two arrays of a
 * call overlapping; a negative or NaN radius_sq (when radii_sq == NULL) or softening_sq.  Otherwise the launch's hipError_t (0 on
 * success).
 */
#ifndef NBODY_HIP_NEIGHBOUR_H
#define NBODY_HIP_NEIGHBOUR_H

#include <stddef.h>
#include <stdint.h>

#include "nbody_hip.h" /* nb_stream_t, NB_ERR_*; error names: nb_error_string */

#ifdef __cplusplus
extern "C" {
#endif

#define NB_NEIGHBOUR_MAX_BODIES (1u << 24)
#define NB_NEIGHBOUR_NONE 0xFFFFFFFFu
#define NB_NEIGHBOUR_OVERFLOW 1u /* status.flags: the lists need more than `capacity` entries; indices was not written */

/* the one expression of d2; dx, dy, dz = the differences x_j - x_i ... in T; FMA = fmaf | fma */
#define NB_NEIGHBOUR_DIST_SQ(FMA, dx, dy, dz) FMA((dx), (dx), FMA((dy), (dy), (dz) * (dz)))

typedef struct nb_neighbour_status { /* 64 bytes, device memory */
    uint64_t total_neighbours;
    double   closest_dist_sq;
    uint32_t closest_i;
    uint32_t closest_j;
    uint32_t max_count;
    uint32_t max_count_body;
    uint32_t flags;
    uint32_t reserved[7];
} nb_neighbour_status_t;

typedef struct nb_neighbour_plan {
    int                bodies_per_lane; /* bodies i a lane holds (fp32: one packed pair, fp64: one)            */
    int                waves_per_group; /* S: waves of a survey workgroup; they share the tile, split the chunks */
    int                unroll;          /* bodies j per scalar load group                                      */
    unsigned           tiles;           /* ceil(N / (64 * bodies_per_lane)): the survey's workgroups           */
    unsigned           block_threads;   /* 64 * S                                                              */
    unsigned           lds_bytes;       /* of a survey workgroup                                               */
    unsigned           chunks;          /* ceil(N / 128)                                                       */
    unsigned           list_ranges;     /* J                                                                   */
    unsigned           list_groups;     /* tiles * J: one-wave workgroups of the count and the fill pass       */
    unsigned           survey_launches; /* kernel launches of one survey call                                  */
    unsigned           list_launches;   /* ... of one lists call                                               */
    unsigned           reserved;
    unsigned long long planes_offset;   /* byte offset of the count planes in the workspace                    */
    unsigned long long planes_bytes;    /* J * N * 4                                                           */
} nb_neighbour_plan_t;

NB_API int nb_neighbour_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes);

NB_API int nb_neighbour_plan_f32(unsigned num_bodies, nb_neighbour_plan_t* plan);
NB_API int nb_neighbour_plan_f64(unsigned num_bodies, nb_neighbour_plan_t* plan);

/* nearest neighbour, counts within the radius and potentials of every body; the status record */
NB_API int nb_neighbour_survey_f32(const float* positions, unsigned num_bodies, float radius_sq, const float* radii_sq, float softening_sq,
                                   unsigned* nearest_index, float* nearest_dist_sq, unsigned* counts, float* potentials,
                                   nb_neighbour_status_t* status, void* workspace, size_t workspace_bytes, nb_stream_t stream);
NB_API int nb_neighbour_survey_f64(const double* positions, unsigned num_bodies, double radius_sq, const double* radii_sq, double softening_sq,
                                   unsigned* nearest_index, double* nearest_dist_sq, unsigned* counts, double* potentials,
                                   nb_neighbour_status_t* status, void* workspace, size_t workspace_bytes, nb_stream_t stream);

/* the neighbours within the radius as CSR lists, or nothing but offsets and the status record when they exceed `capacity` */
NB_API int nb_neighbour_lists_f32(const float* positions, unsigned num_bodies, float radius_sq, const float* radii_sq,
                                  unsigned long long* offsets, unsigned* indices, unsigned long long capacity,
                                  nb_neighbour_status_t* status, void* workspace, size_t workspace_bytes, nb_stream_t stream);
NB_API int nb_neighbour_lists_f64(const double* positions, unsigned num_bodies, double radius_sq, const double* radii_sq,
                                  unsigned long long* offsets, unsigned* indices, unsigned long long capacity,
                                  nb_neighbour_status_t* status, void* workspace, size_t workspace_bytes, nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_NEIGHBOUR_H */
