// hermite_block_boundary.h -- the extern "C" boundary of the Hermite libraries that step one system with block time steps
// (hermite_block_capi.hip, hermite6_block_boundary.hip), one text for both orders, templated on <T, Order> as hermite_boundary.h: the
// workspace layout, the plan query and every call's argument check and launch sequence.  Ahead of that, what the boundaries of all four
// block-step libraries (these two and hermite_block_ensemble_boundary.h's) share: the header's constants and records held against the
// kernels', the checks of N and of the parameters, and the part of a plan that (N, num_active, precision) alone decide.  Host only.
//
// Every argument is checked on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never waits
// for the device.  The initial evaluation is hermite_eval.o's or hermite6_eval.o's (linked in; those objects export nothing).
#pragma once

#include "../../include/nbody_hip_hermite_block.h"
#include "capi_check.h"
#include "hermite6_block_kernels.h"
#include "hermite_block_kernels.h"
#include "hermite_boundary.h"  // what the order decides
#include "softening_floor.h"

#include <cmath>

namespace nb {

static_assert(NB_HERMITE_BLOCK_MAX_BODIES == kBlockMaxBodies, "the header's limit is the kernels'");
static_assert(NB_HERMITE_BLOCK_MAX_LEVEL == kBlockMaxLevel, "the header's deepest level is the kernels'");
static_assert(NB_HERMITE_BLOCK_STOPPED == kBlockStopped, "the header's flag is the kernels'");
static_assert(sizeof(nb_hermite_block_status_t) == 64 && sizeof(BlockStatus) == 64, "the status record is 64 bytes");
static_assert(sizeof(nb_hermite_block_params_t) == sizeof(BlockParams), "the parameters cross by value");
static_assert(sizeof(BlockCtrl) == 64, "the control record is 64 bytes");
static_assert(kBlockSums == kOrderSums<4> && kBlock6Sums == kOrderSums<6>, "a partial plane per sum of the evaluation");
static_assert(kBlockMaxBodies <= kHermiteMaxBodies && kBlockMaxBodies <= kHermite6MaxBodies, "the initial evaluation takes every N the block steps take");

// N of a system that steps alone (the ensemble has limits of its own)
inline bool block_size_ok(unsigned n) { return n >= 1 && n <= kBlockMaxBodies; }

// the cube of a step, as the 6th-order corrector forms it in T (hh = h * h, h3 = hh * h): c1 divides by it
template <typename T> bool cube_is_normal(double step) {
    const T h = static_cast<T>(step), hh = h * h, h3 = hh * h;
    return std::isnormal(h3);
}

// T: the corrector's precision.  At order 6 the longest step (dt_max) and the shortest (one tick) must have normal cubes in T: the "Range
// of h" of include/nbody_hip_hermite6_block.h.
template <typename T, int Order> bool block_params_ok(const nb_hermite_block_params_t* p) {
    if (p == nullptr) return false;
    const auto positive = [](double v) { return std::isfinite(v) && v > 0; };
    if (!positive(p->eta) || !positive(p->eta_start) || !positive(p->dt_max) || p->max_level < 0 || p->max_level > kBlockMaxLevel) return false;
    const double tick = std::ldexp(p->dt_max, -p->max_level);
    return std::isnormal(tick) && (Order != 6 || (cube_is_normal<T>(tick) && cube_is_normal<T>(p->dt_max)));
}

inline BlockParams block_params_of(const nb_hermite_block_params_t* p) { return BlockParams{p->eta, p->eta_start, p->dt_max, p->max_level, 0}; }

// The fields nb_hermite_block_plan_t and nb_hermite_block_ensemble_plan_t have in common, of one system of n bodies with n_active of them
// active.  The caller adds its launches and where the planes lie.
template <typename T, int Order, typename Plan> void block_plan_fill(Plan* out, unsigned n, unsigned n_active) {
    const unsigned  per_tile = 64 * stream_lane_bodies<T>(), sums = kOrderSums<Order>;
    const BlockGeom g        = block_geometry(n, n_active, per_tile);
    const unsigned  S        = block_waves(n);
    out->bodies_per_lane = per_tile / 64;
    out->waves_per_group = static_cast<int>(S);
    out->unroll          = order_unroll<T, Order>();
    out->tiles           = g.tiles;
    out->ranges          = g.ranges;
    out->groups          = g.tiles * g.ranges;
    out->launch_groups   = block_launch_groups(n, per_tile);
    out->block_threads   = 64 * S;
    out->lds_bytes       = static_cast<unsigned>((S > 1 ? S - 1 : 1) * sums * per_tile * sizeof(T)) + 128;
    out->slots           = g.tiles * per_tile;
    out->chunks          = block_chunks(n);
    out->partial_bytes   = static_cast<unsigned long long>(g.ranges) * sums * out->slots * sizeof(T);
}

namespace block {

template <int Order> BlockLayout layout(unsigned n, size_t size_t_of) { return block_layout(n, size_t_of, kBodyVec4<Order>, kOrderSums<Order>); }

template <int Order> int workspace_bytes(unsigned n, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !block_size_ok(n) || !element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = layout<Order>(n, sizeof_T).bytes;
    return 0;
}

template <typename T, int Order> int plan_query(unsigned n, unsigned n_active, nb_hermite_block_plan_t* out) {
    if (out == nullptr || !block_size_ok(n) || n_active < 1 || n_active > n) return NB_ERR_INVALID_ARGUMENT;
    block_plan_fill<T, Order>(out, n, n_active);
    out->launches       = 6;
    out->partial_offset = layout<Order>(n, sizeof(T)).partial;
    return 0;
}

template <typename T, int Order> using Args = std::conditional_t<Order == 6, Block6Args<T>, BlockArgs<T>>;

// the arrays of a system and the workspace, checked; fills `a`
template <typename T, int Order>
bool bind(Args<T, Order>& a, T* pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace,
          size_t workspace_bytes, unsigned n, const nb_hermite_block_params_t* params) {
    if (!block_size_ok(n) || !block_params_ok<T, Order>(params)) return false;
    const BlockLayout l = layout<Order>(n, sizeof(T));
    if (workspace_bytes < l.bytes) return false;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al, kHigher<Order>}, {crackle, bodies, al, kHigher<Order>},
                   {ticks, static_cast<std::uintptr_t>(n) * 8, 8}, {levels, static_cast<std::uintptr_t>(n) * 4, 4}, {status, 64, 8}, {workspace, l.bytes, 32}})) {
        return false;
    }
    char* const ws = static_cast<char*>(workspace);
    a.pos = pos, a.vel = vel, a.acc = acc, a.jerk = jerk;
    if constexpr (Order == 6) {
        a.snap = snap, a.crackle = crackle, a.state12 = reinterpret_cast<T*>(ws + l.state);
    } else {
        a.state8 = reinterpret_cast<T*>(ws + l.state);
    }
    a.ticks    = reinterpret_cast<unsigned long long*>(ticks);
    a.levels   = levels;
    a.status   = reinterpret_cast<BlockStatus*>(status);
    a.partial  = reinterpret_cast<T*>(ws + l.partial);
    a.active   = reinterpret_cast<unsigned*>(ws + l.active);
    a.counts   = reinterpret_cast<unsigned*>(ws + l.counts);
    a.min_part = reinterpret_cast<unsigned long long*>(ws + l.min_part);
    a.lvl_part = reinterpret_cast<int*>(ws + l.lvl_part);
    a.ctrl     = reinterpret_cast<BlockCtrl*>(ws + l.ctrl);
    a.n        = n;
    a.p        = block_params_of(params);
    a.t_stop   = 0;
    return true;
}

template <typename T, int Order>
int init(T* pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
         unsigned n, T eps2, const nb_hermite_block_params_t* params, nb_stream_t stream) {
    Args<T, Order> a{};
    if (!bind<T, Order>(a, pos, vel, acc, jerk, snap, crackle, ticks, levels, status, workspace, workspace_bytes, n, params)) return NB_ERR_INVALID_ARGUMENT;
    a.eps2       = floored(eps2);
    const auto s = static_cast<hipStream_t>(stream);
    if constexpr (Order == 6) {
        if (const auto err = launch_hermite6_start<T>(acc, jerk, snap, crackle, pos, vel, a.state12, n, a.eps2, s); err != hipSuccess) return static_cast<int>(err);
        return static_cast<int>(launch_block6_init<T>(a, s));
    } else {
        HermiteArgs<T> e{};
        e.pos = pos, e.vel_in = vel, e.acc = acc, e.jerk = jerk, e.n = n, e.eps2 = a.eps2;
        if (const auto err = launch_hermite_eval<T>(e, s); err != hipSuccess) return static_cast<int>(err);
        return static_cast<int>(launch_block_init<T>(a, s));
    }
}

template <typename T, int Order>
int step(T* pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
         unsigned n, T eps2, const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream) {
    Args<T, Order> a{};
    if (std::isnan(t_stop)) return NB_ERR_INVALID_ARGUMENT;
    if (!bind<T, Order>(a, pos, vel, acc, jerk, snap, crackle, ticks, levels, status, workspace, workspace_bytes, n, params)) return NB_ERR_INVALID_ARGUMENT;
    a.eps2   = floored(eps2);
    a.t_stop = t_stop;
    if constexpr (Order == 6) {
        return static_cast<int>(launch_block6_step<T>(a, static_cast<hipStream_t>(stream)));
    } else {
        return static_cast<int>(launch_block_step<T>(a, static_cast<hipStream_t>(stream)));
    }
}

template <typename T, int Order>
int sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const T* snap, const T* crackle, const uint64_t* ticks,
         const nb_hermite_block_status_t* status, unsigned n, const nb_hermite_block_params_t* params, nb_stream_t stream) {
    if (!block_size_ok(n) || !block_params_ok<T, Order>(params)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{pos_out, bodies, al}, {vel_out, bodies, al}, {pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al, kHigher<Order>},
                   {crackle, bodies, al, kHigher<Order>}, {ticks, static_cast<std::uintptr_t>(n) * 8, 8}, {status, 64, 8}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    const auto* const t  = reinterpret_cast<const unsigned long long*>(ticks);
    const auto* const st = reinterpret_cast<const BlockStatus*>(status);
    if constexpr (Order == 6) {
        return static_cast<int>(launch_block6_sync<T>(pos_out, vel_out, pos, vel, acc, jerk, snap, crackle, t, st, n, block_params_of(params), static_cast<hipStream_t>(stream)));
    } else {
        return static_cast<int>(launch_block_sync<T>(pos_out, vel_out, pos, vel, acc, jerk, t, st, n, block_params_of(params), static_cast<hipStream_t>(stream)));
    }
}

}  // namespace block
}  // namespace nb
