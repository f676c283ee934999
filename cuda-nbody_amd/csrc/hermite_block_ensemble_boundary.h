// hermite_block_ensemble_boundary.h -- the extern "C" boundary of the Hermite libraries that step many independent systems with block time
// steps (hermite_block_ensemble_capi.hip, hermite6_block_ensemble_boundary.hip), one text for both orders, templated on <T, Order> as
// hermite_boundary.h: the size check, the per-system workspace layout, the plan query and every call's argument check and launch sequence.
// Host only.
//
// Every argument is checked on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never waits
// for the device.  The initial evaluation is hermite_ensemble.o's or hermite6_ensemble.o's (linked in; those objects export nothing).
// softening^2 == 0 takes its floor per system, on the device.
#pragma once

#include "../../include/nbody_hip_hermite_block_ensemble.h"
#include "capi_check.h"
#include "hermite6_block_ensemble_kernels.h"
#include "hermite_block_boundary.h"  // the parameters' check, block_plan_fill
#include "hermite_block_ensemble_kernels.h"
#include "hermite_ensemble_boundary.h"  // grid_ok of init's evaluation

namespace nb::block_ensemble {

static_assert(NB_HERMITE_BLOCK_ENSEMBLE_MAX_BODIES == kBlockEnsembleMaxBodies && NB_HERMITE_BLOCK_ENSEMBLE_MAX_TOTAL == kBlockEnsembleMaxTotal,
              "the header's limits are the kernels'");
static_assert(NB_HERMITE_BLOCK_ENSEMBLE_MAX_BODIES == kEnsembleHermiteMaxBodies && NB_HERMITE_BLOCK_ENSEMBLE_MAX_TOTAL == kEnsembleHermiteMaxTotal,
              "... and those of the ensemble evaluation init runs");
static_assert(kBlockEnsembleMaxBodies <= 256 * kBlockThreads, "a system's counts and partial minima: one per lane of a workgroup of 256");
static_assert(sizeof(nb_hermite_block_ensemble_summary_t) == 64 && sizeof(BlockEnsembleSummary) == 64, "the summary record is 64 bytes");

template <int Order> BlockEnsembleLayout layout(unsigned n, size_t size_t_of) { return block_ensemble_layout(n, size_t_of, kBodyVec4<Order>, kOrderSums<Order>); }

// N, B and their products: every stage of every call is one launch
template <typename T, int Order> bool size_ok(unsigned n, unsigned b) {
    if (n < 1 || n > kBlockEnsembleMaxBodies || b < 1 || static_cast<unsigned long long>(n) * b > kBlockEnsembleMaxTotal) return false;
    constexpr unsigned       per_tile = 64 * stream_lane_bodies<T>();
    const unsigned long long limit    = 1ull << 31;
    const unsigned long long eval     = static_cast<unsigned long long>(b) * block_launch_groups(n, per_tile) * (64 * block_waves(n));
    const unsigned long long schedule = static_cast<unsigned long long>(b) * block_ensemble_blocks(n) * kBlockThreads;
    return eval <= limit && schedule <= limit && ensemble::grid_ok<T, Order>(n, b);  // (the last: init's evaluation)
}

template <typename T, int Order> int workspace_bytes_of(unsigned n, unsigned b, size_t* bytes) {
    if (!size_ok<T, Order>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = layout<Order>(n, sizeof(T)).stride * b;
    return 0;
}
template <int Order> int workspace_bytes(unsigned n, unsigned b, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    return sizeof_T == 4 ? workspace_bytes_of<float, Order>(n, b, bytes) : workspace_bytes_of<double, Order>(n, b, bytes);
}

template <typename T, int Order> int plan_query(unsigned n, unsigned b, unsigned n_active, nb_hermite_block_ensemble_plan_t* out) {
    if (out == nullptr || !size_ok<T, Order>(n, b) || n_active < 1 || n_active > n) return NB_ERR_INVALID_ARGUMENT;
    const BlockEnsembleLayout l = layout<Order>(n, sizeof(T));
    block_plan_fill<T, Order>(out, n, n_active);
    out->step_launches     = 5;
    out->partial_offset    = l.partial;
    out->groups_per_system = out->launch_groups;
    out->blocks_per_system = block_ensemble_blocks(n);
    out->eval_grid         = static_cast<unsigned long long>(b) * out->groups_per_system;
    out->schedule_grid     = static_cast<unsigned long long>(b) * out->blocks_per_system;
    out->workspace_stride  = l.stride;
    return 0;
}

template <typename T, int Order> using Args = std::conditional_t<Order == 6, Block6EnsembleArgs<T>, BlockEnsembleArgs<T>>;

// the arrays of the B systems and the workspace, checked; fills `a`
template <typename T, int Order>
bool bind(Args<T, Order>& a, T* pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace,
          size_t workspace_bytes, unsigned n, unsigned b, T eps2, const T* system_eps2, const nb_hermite_block_params_t* params) {
    if (!size_ok<T, Order>(n, b) || !block_params_ok<T, Order>(params)) return false;
    const BlockEnsembleLayout l     = layout<Order>(n, sizeof(T));
    const std::uintptr_t      total = static_cast<std::uintptr_t>(l.stride) * b;
    if (workspace_bytes < total) return false;
    const std::uintptr_t count = static_cast<std::uintptr_t>(n) * b, bodies = count * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al, kHigher<Order>}, {crackle, bodies, al, kHigher<Order>},
                   {ticks, count * 8, 8}, {levels, count * 4, 4}, {status, static_cast<std::uintptr_t>(b) * 64, 8}, {workspace, total, 32},
                   {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
        return false;
    }
    a.pos = pos, a.vel = vel, a.acc = acc, a.jerk = jerk;
    if constexpr (Order == 6) a.snap = snap, a.crackle = crackle;
    a.ticks             = reinterpret_cast<unsigned long long*>(ticks);
    a.levels            = levels;
    a.status            = reinterpret_cast<BlockStatus*>(status);
    a.workspace         = static_cast<char*>(workspace);
    a.layout            = l;
    a.system_eps2       = system_eps2;
    a.eps2              = eps2;
    a.n                 = n;
    a.b                 = b;
    a.blocks            = block_ensemble_blocks(n);
    a.groups_per_system = block_launch_groups(n, 64 * stream_lane_bodies<T>());
    a.p                 = block_params_of(params);
    a.t_stop            = 0;
    return true;
}

template <typename T, int Order>
int init(T* pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
         unsigned n, unsigned b, T eps2, const T* system_eps2, const nb_hermite_block_params_t* params, nb_stream_t stream) {
    Args<T, Order> a{};
    if (!bind<T, Order>(a, pos, vel, acc, jerk, snap, crackle, ticks, levels, status, workspace, workspace_bytes, n, b, eps2, system_eps2, params)) return NB_ERR_INVALID_ARGUMENT;
    const auto s = static_cast<hipStream_t>(stream);
    if constexpr (Order == 6) {
        // The start wants a contiguous T[12 N B]: the front of the workspace (B * stride >= 12 N B sizeof T), free since nothing is kept there
        // between calls.
        if (const auto err = launch_ensemble6_start<T>(acc, jerk, snap, crackle, pos, vel, static_cast<T*>(workspace), n, b, eps2, system_eps2, s); err != hipSuccess) {
            return static_cast<int>(err);
        }
        return static_cast<int>(launch_block6_ensemble_init<T>(a, s));
    } else {
        EnsembleHermiteArgs<T> e{};
        e.pos = pos, e.vel_in = vel, e.acc = acc, e.jerk = jerk, e.n = n, e.src.eps2 = eps2, e.src.system_eps2 = system_eps2;
        if (const auto err = launch_ensemble_eval<T>(e, b, s); err != hipSuccess) return static_cast<int>(err);
        return static_cast<int>(launch_block_ensemble_init<T>(a, s));
    }
}

template <typename T, int Order>
int step(T* pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
         unsigned n, unsigned b, T eps2, const T* system_eps2, const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream) {
    Args<T, Order> a{};
    if (std::isnan(t_stop)) return NB_ERR_INVALID_ARGUMENT;
    if (!bind<T, Order>(a, pos, vel, acc, jerk, snap, crackle, ticks, levels, status, workspace, workspace_bytes, n, b, eps2, system_eps2, params)) return NB_ERR_INVALID_ARGUMENT;
    a.t_stop = t_stop;
    if constexpr (Order == 6) {
        return static_cast<int>(launch_block6_ensemble_step<T>(a, static_cast<hipStream_t>(stream)));
    } else {
        return static_cast<int>(launch_block_ensemble_step<T>(a, static_cast<hipStream_t>(stream)));
    }
}

template <typename T, int Order>
int sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const T* snap, const T* crackle, const uint64_t* ticks,
         const nb_hermite_block_status_t* status, unsigned n, unsigned b, const nb_hermite_block_params_t* params, nb_stream_t stream) {
    if (!size_ok<T, Order>(n, b) || !block_params_ok<T, Order>(params)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t count = static_cast<std::uintptr_t>(n) * b, bodies = count * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{pos_out, bodies, al}, {vel_out, bodies, al}, {pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al, kHigher<Order>},
                   {crackle, bodies, al, kHigher<Order>}, {ticks, count * 8, 8}, {status, static_cast<std::uintptr_t>(b) * 64, 8}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    const auto* const t  = reinterpret_cast<const unsigned long long*>(ticks);
    const auto* const st = reinterpret_cast<const BlockStatus*>(status);
    if constexpr (Order == 6) {
        return static_cast<int>(
            launch_block6_ensemble_sync<T>(pos_out, vel_out, pos, vel, acc, jerk, snap, crackle, t, st, n, b, block_params_of(params), static_cast<hipStream_t>(stream)));
    } else {
        return static_cast<int>(launch_block_ensemble_sync<T>(pos_out, vel_out, pos, vel, acc, jerk, t, st, n, b, block_params_of(params), static_cast<hipStream_t>(stream)));
    }
}

template <int Order> int summary(const nb_hermite_block_status_t* status, unsigned b, nb_hermite_block_ensemble_summary_t* out, nb_stream_t stream) {
    if (b < 1 || b > kBlockEnsembleMaxTotal) return NB_ERR_INVALID_ARGUMENT;
    if (!spans_ok({{status, static_cast<std::uintptr_t>(b) * 64, 8}, {out, 64, 8}})) return NB_ERR_INVALID_ARGUMENT;
    const auto* const st = reinterpret_cast<const BlockStatus*>(status);
    auto* const       o  = reinterpret_cast<BlockEnsembleSummary*>(out);
    if constexpr (Order == 6) {
        return static_cast<int>(launch_block6_ensemble_summary(st, b, o, static_cast<hipStream_t>(stream)));
    } else {
        return static_cast<int>(launch_block_ensemble_summary(st, b, o, static_cast<hipStream_t>(stream)));
    }
}

}  // namespace nb::block_ensemble
