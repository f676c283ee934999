/*
 * nbody_hip_knn.h -- the K nearest neighbours of every body, local densities and the density centre (libnbody_hip_knn.so).
 *
 * For every body i of a state: its K nearest neighbours by rank and the distance to each; from them the local density of
 * Casertano & Hut's kind; and from the densities one 128-byte record with the density centre, the density radius, the core radius and
 * the radius that gives every body at least K list entries.  They are what the users of nb_hermite_block_* read a cluster by, what an
 * SPH-style density starts from, and the radius an Ahmad-Cohen neighbour list (nb_neighbour_lists_*) is sized with.
 *
 * This library links none of the other libraries and reads no process-global setting.  Error codes are the NB_ERR_* / hipError_t
 * values of nbody_hip.h.  T = float | double; positions are T[4*N] = {x, y, z, mass}.
 *
 * THE NEIGHBOUR LIST OF BODY i is the first K entries of all pairs (d2(i, j), j) with j != i BY INDEX, sorted lexicographically:
 * d2 ascending, the lowest j first on equal bits.  d2 is NB_NEIGHBOUR_DIST_SQ of nbody_hip_neighbour.h in T (the one expression of d2
 * in the project), so rank 0 agrees bit for bit with nb_neighbour_survey_*'s nearest_index / nearest_dist_sq.  A distinct body at the
 * same place is a neighbour at 0.  A NaN d2 is never a neighbour; neither is a d2 that is not less than +inf.  With fewer than K
 * candidates the remaining ranks hold NB_NEIGHBOUR_NONE and +inf.  1 <= K <= 16 (NB_KNN_MAX_K), 1 <= N <= 2^24.  The lists are a
 * function of the positions alone: they do not depend on the geometry, the outputs asked for, or a body's slot in a tile.
 *
 * nb_knn_survey_*  each output may be NULL and is then not stored; at least one output, or the structure record, must be asked for:
 *   knn_index     unsigned[N][K], row-major   the neighbour indices by rank
 *   knn_dist_sq   T[N][K], row-major          their d2 by rank
 *   densities     T[N]                        the local density rho_i, rounded once from double
 *   structure     nb_knn_structure_t          128 bytes of device memory, below
 * Alignment and overlap rules are those of nbody_hip_neighbour.h: positions to 4*sizeof(T), knn_dist_sq and densities to sizeof(T),
 * knn_index to 4, the record to 8, the workspace to 32; no two arrays of a call overlap.
 *
 * THE DENSITY.  All density arithmetic is in double.  M_i is the sum, in rank order, of the masses of the K - 1 inner neighbours
 * (ranks 0 .. K-2); d_K^2 is the K-th d2 (rank K-1), widened to double;
 *
 *                rho_i = M_i / (c * (d_K^2 * sqrt(d_K^2))),    c = 4.188790204786391 (NB_KNN_SPHERE, the double nearest 4 pi / 3)
 *
 * rho_i is DEFINED AS 0 when d_K^2 is 0, +inf or missing (fewer than K neighbours), or when the cube d_K^2 * sqrt(d_K^2) is not a
 * positive normal double or c times it is not finite (fp64 only: below).  Such bodies are counted in the record (`degenerate`), and NB_KNN_DEGENERATE says there
 * were any.  Densities and the record need K >= 2; with K = 1 they are refused.
 *
 * THE STRUCTURE RECORD (doubles and 32-bit counts; every sum in an order fixed by the plan, so the bits repeat from call to call):
 *   sum_density      sum rho_i
 *   centre[3]        the density centre x_d = sum rho_i x_i / sum rho_i
 *   density_radius   sum rho_i |x_i - x_d| / sum rho_i
 *   core_radius      sqrt(sum rho_i^2 |x_i - x_d|^2 / sum rho_i^2)
 *   max_density, max_density_body   the largest rho_i and the LOWEST body that has it
 *   min_kth_dist_sq, max_kth_dist_sq   the smallest and the largest FINITE d_K^2 (+inf and -inf when no body has one).  The largest is
 *                    the squared radius at which every body with K neighbours has >= K entries in a list of d2 <= that radius.
 *   defined, degenerate   bodies whose density is given by the formula / defined as 0; defined + degenerate = N
 *   flags            NB_KNN_DEGENERATE: degenerate > 0.  NB_KNN_NO_DENSITY: sum_density is not greater than 0; the centre and the two
 *                    radii are then NaN.
 * The density radius and the core radius are the two definitions of a "core radius" in use: the density-weighted mean distance
 * and the density-squared-weighted rms distance from the density centre.
 *
 * Operand range.  The lists hold for EVERY input, subnormal and overflowed d2 included: the "Operand range" of nbody_hip_neighbour.h,
 * which is about the same d2.  Ranks past the candidates with a d2 below +inf hold NB_NEIGHBOUR_NONE and +inf.  The masses take no part
 * in the lists.
 * The density is given by the formula for d_K^2 in [2^-681, 2^681), where the cube is a normal double and c times it finite whatever
 * the mantissa (the rule itself is the one above, on the cube and the product as computed).  In fp32 that is every d_K^2 from the
 * smallest subnormal to the largest finite float.  In fp64 a smaller d_K^2 (its cube is subnormal, or 0 below 2^-716) or a larger one
 * (c times its cube is +inf, from 2^683 the cube itself) is `degenerate` and has the density 0 -- never +inf, and never a 0 that the
 * formula's own overflow made and that is counted as `defined`.  A defined rho_i is a normal double unless M_i / (c * cube) leaves
 * the range: M_i > 16 at the lower edge, M_i < 4 at the upper one; a NaN or infinite mass reaches the densities of the bodies that
 * have it among their K - 1 inner neighbours, and through them the record's sums.  `densities` in fp32 is the double rounded once:
 * +inf above FLT_MAX (unit masses: d_K^2 below about 2^-87), subnormal or 0 below FLT_MIN; the double is what the record is made of.
 * The record squares rho_i.  Its sums are what the formulas say while every nonzero rho_i, rho_i |x_i|, rho_i |x_i - x_d|, rho_i^2 and
 * rho_i^2 |x_i - x_d|^2, and the sum of each, is a normal double: rho_i within [2^-511, 2^511] less the room the sums need, which for
 * unit masses and a state of the size of d_K is d_K^2 in [2^-342, 2^339).  In fp32, with masses within 2^+-100, that is always so.
 * Outside it nothing is clamped: the counts, the extremes, the densest body and the flags stay exact, the sums and the two radii are
 * what IEEE arithmetic gives (+inf, or NaN from inf / inf and 0 / 0).
 *
 * Geometry (nb_knn_plan_*) and workspace (nb_knn_workspace_bytes): functions of (N, K, precision) alone.  A workgroup of the search
 * owns one tile of 64 * bodies_per_lane bodies i; its S waves split the chunks of 128 bodies j (chunk c -> wave c mod S), each keeps
 * a sorted list of `capacity` >= K entries per body in registers, and the waves' lists merge pairwise through LDS by (d2, j).  The
 * workspace holds the double rho[N], the tiles' records and the partial sums of the radii; its content before a call does not matter.
 *
 * Rules.  The caller owns all memory; a call allocates nothing, keeps no state, takes no lock, never synchronises, never prints and is
 * asynchronous on `stream`, so it may sit inside a graph capture.  No atomics, every word written by one lane.  Inputs are only read.
 *
 * Errors.  NB_ERR_INVALID_ARGUMENT, returned before any HIP call, for: a null positions or workspace; no output and no record at all;
 * N or K out of range; densities or the record with K = 1; a misaligned array; workspace_bytes too small; any two arrays of a call
 * overlapping.  Otherwise the launch's hipError_t (0 on success).
 */
#ifndef NBODY_HIP_KNN_H
#define NBODY_HIP_KNN_H

#include <stddef.h>
#include <stdint.h>

#include "nbody_hip_neighbour.h" /* NB_NEIGHBOUR_DIST_SQ, NB_NEIGHBOUR_NONE, NB_NEIGHBOUR_MAX_BODIES; nb_stream_t, NB_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define NB_KNN_MAX_K 16u
#define NB_KNN_SPHERE 4.188790204786391 /* the double nearest 4 pi / 3 */
#define NB_KNN_DEGENERATE 1u /* flags: some body's density is defined as 0 */
#define NB_KNN_NO_DENSITY 2u /* flags: sum_density is not > 0; centre, density_radius and core_radius are NaN */

typedef struct nb_knn_structure { /* 128 bytes, device memory */
    double   sum_density;
    double   centre[3];
    double   density_radius;
    double   core_radius;
    double   max_density;
    double   min_kth_dist_sq;
    double   max_kth_dist_sq;
    uint32_t max_density_body;
    uint32_t defined;
    uint32_t degenerate;
    uint32_t flags;
    uint32_t reserved[10];
} nb_knn_structure_t;

typedef struct nb_knn_plan {
    int                bodies_per_lane;    /* W: bodies i a lane holds (fp32: one packed pair, fp64: one)              */
    int                waves_per_group;    /* S: waves of a search workgroup; they share the tile, split the chunks    */
    int                unroll;             /* U: bodies j per scalar load group                                        */
    int                capacity;           /* list entries a lane keeps per body: the compiled 4, 8 or 16 that holds K */
    unsigned           ranges;             /* J: ranges the chunks are cut into (1: no partial lists)                  */
    unsigned           tiles;              /* ceil(N / (64 * W)): the search's workgroups                              */
    unsigned           block_threads;      /* 64 * S                                                                   */
    unsigned           lds_bytes;          /* of a search workgroup                                                    */
    unsigned           chunks;             /* ceil(N / 128)                                                            */
    unsigned           blocks;             /* ceil(N / 256): workgroups of the pass for the two radii                  */
    unsigned           search_launches;    /* kernel launches of a call without the record                             */
    unsigned           structure_launches; /* further launches of a call with the record (0 when K = 1)                */
    unsigned long long density_offset;     /* byte offset of the double rho[N] in the workspace                        */
    unsigned long long density_bytes;      /* N * 8                                                                    */
} nb_knn_plan_t;

NB_API int nb_knn_workspace_bytes(unsigned num_bodies, unsigned k, unsigned sizeof_T, size_t* bytes);

NB_API int nb_knn_plan_f32(unsigned num_bodies, unsigned k, nb_knn_plan_t* plan);
NB_API int nb_knn_plan_f64(unsigned num_bodies, unsigned k, nb_knn_plan_t* plan);

/* the K nearest neighbours of every body, the local densities and the structure record */
NB_API int nb_knn_survey_f32(const float* positions, unsigned num_bodies, unsigned k, unsigned* knn_index, float* knn_dist_sq, float* densities,
                             nb_knn_structure_t* structure, void* workspace, size_t workspace_bytes, nb_stream_t stream);
NB_API int nb_knn_survey_f64(const double* positions, unsigned num_bodies, unsigned k, unsigned* knn_index, double* knn_dist_sq, double* densities,
                             nb_knn_structure_t* structure, void* workspace, size_t workspace_bytes, nb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_HIP_KNN_H */
