// hermite_block_boundary.h -- what the extern "C" boundaries of the four block-step libraries (hermite_block_capi.hip,
// hermite6_block_boundary.hip, hermite_block_ensemble_capi.hip, hermite6_block_ensemble_boundary.hip) share: the header's constants and records held against the kernels',
// the checks of N and of the parameters, and the part of a plan that (N, num_active, precision) alone decide.  Host only.
#pragma once

#include "../../include/nbody_hip_hermite_block.h"
#include "hermite_block_kernels.h"

#include <cmath>

namespace nb {

static_assert(NB_HERMITE_BLOCK_MAX_BODIES == kBlockMaxBodies, "the header's limit is the kernels'");
static_assert(NB_HERMITE_BLOCK_MAX_LEVEL == kBlockMaxLevel, "the header's deepest level is the kernels'");
static_assert(NB_HERMITE_BLOCK_STOPPED == kBlockStopped, "the header's flag is the kernels'");
static_assert(sizeof(nb_hermite_block_status_t) == 64 && sizeof(BlockStatus) == 64, "the status record is 64 bytes");
static_assert(sizeof(nb_hermite_block_params_t) == sizeof(BlockParams), "the parameters cross by value");
static_assert(sizeof(BlockCtrl) == 64, "the control record is 64 bytes");

// N of a system that steps alone (the ensemble has limits of its own)
inline bool block_size_ok(unsigned n) { return n >= 1 && n <= kBlockMaxBodies; }

inline bool block_params_ok(const nb_hermite_block_params_t* p) {
    if (p == nullptr) return false;
    const auto positive = [](double v) { return std::isfinite(v) && v > 0; };
    return positive(p->eta) && positive(p->eta_start) && positive(p->dt_max) && p->max_level >= 0 && p->max_level <= kBlockMaxLevel &&
           std::isnormal(std::ldexp(p->dt_max, -p->max_level));
}

inline BlockParams block_params_of(const nb_hermite_block_params_t* p) { return BlockParams{p->eta, p->eta_start, p->dt_max, p->max_level, 0}; }

// The fields nb_hermite_block_plan_t and nb_hermite_block_ensemble_plan_t have in common, of one system of n bodies with n_active of them
// active, with `sums` partial planes.  The caller adds its launches and where the planes lie.
template <typename Plan> void block_plan_fill(Plan* out, unsigned n, unsigned n_active, size_t size_t_of, unsigned sums, int unroll) {
    const unsigned  per_tile = size_t_of == 4 ? 128 : 64;
    const BlockGeom g        = block_geometry(n, n_active, per_tile);
    const unsigned  S        = block_waves(n);
    out->bodies_per_lane = per_tile / 64;
    out->waves_per_group = static_cast<int>(S);
    out->unroll          = unroll;
    out->tiles           = g.tiles;
    out->ranges          = g.ranges;
    out->groups          = g.tiles * g.ranges;
    out->launch_groups   = block_launch_groups(n, per_tile);
    out->block_threads   = 64 * S;
    out->lds_bytes       = static_cast<unsigned>((S > 1 ? S - 1 : 1) * sums * per_tile * size_t_of) + 128;
    out->slots           = g.tiles * per_tile;
    out->chunks          = block_chunks(n);
    out->partial_bytes   = static_cast<unsigned long long>(g.ranges) * sums * out->slots * size_t_of;
}

}  // namespace nb
