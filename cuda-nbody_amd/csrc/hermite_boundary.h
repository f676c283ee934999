// hermite_boundary.h -- the extern "C" boundary of the Hermite libraries that step one system with one time step (hermite_capi.hip,
// hermite6_capi.hip), one text for both orders: the size check, the workspace, the plan query and every call's argument check and launch
// sequence, templated on <T, Order>.  Ahead of that, what the boundaries of all four shapes (this one, hermite_block_boundary.h,
// hermite_ensemble_boundary.h, hermite_block_ensemble_boundary.h) derive from the order.  Host only.
//
// Every argument is checked on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never waits
// for the device.  The 4th-order entry points pass nullptr for the arrays their scheme does not have (snap, crackle), which the one span
// list of a call takes as absent.
#pragma once

#include "../../include/nbody_hip.h"  // nb_stream_t, NB_ERR_*
#include "capi_check.h"
#include "hermite6_kernels.h"
#include "hermite_kernels.h"
#include "softening_floor.h"

#include <type_traits>

namespace nb {

// ---- what the order decides: 4 or 6, and nothing else compiles where one of these is used ---------------------------------------------------
// vec4 per predicted body in the workspace: {x, m}, {v, 0} and, with the snap, {a, 0}
template <int Order> requires(Order == 4 || Order == 6) inline constexpr unsigned kBodyVec4 = Order == 6 ? 3 : 2;
// the sums of the evaluation, and so its partial planes: ax ay az jx jy jz and, at order 6, sx sy sz
template <int Order> requires(Order == 4 || Order == 6) inline constexpr int kOrderSums = Order == 6 ? kHermite6Sums : kHermiteSums;
// U bodies j per scalar load group
template <typename T, int Order> constexpr int order_unroll() { return Order == 6 ? hermite6_unroll_for<T>() : unroll_for<T>(); }
// snap and crackle: arrays of the 6th-order scheme, absent (nullptr) at order 4
template <int Order> requires(Order == 4 || Order == 6) inline constexpr Span::Presence kHigher = Order == 6 ? Span::required : Span::optional;

template <typename T, int Order> StreamPlan order_plan(unsigned n) { return plan_stream<T>(n, kOrderSums<Order>, order_unroll<T, Order>()); }

namespace solo {

static_assert(kHermiteMaxBodies == kHermite6MaxBodies && kTimestepPartials == kHermite6TimestepPartials, "one size check and one scratch size for both orders");

inline bool size_ok(unsigned n) { return n >= 1 && n <= kHermiteMaxBodies; }

// the workspace: the predicted state
template <int Order> int workspace_bytes(unsigned n, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !size_ok(n) || !element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = static_cast<size_t>(n) * 4 * kBodyVec4<Order> * sizeof_T;
    return 0;
}

template <typename T, int Order, typename Plan> int plan_query(unsigned n, Plan* out) {
    if (out == nullptr || !size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    fill(out, order_plan<T, Order>(n));
    return 0;
}

// Order 4: acc and jerk of (pos, vel); there is no snap, acc_in or workspace.  Order 6: and the snap, which needs accelerations: the
// evaluation reads the workspace's copy of {pos, vel, acc_in}.
template <typename T, int Order>
int eval(T* acc, T* jerk, T* snap, const T* pos, const T* vel, const T* acc_in, void* workspace, size_t workspace_bytes, unsigned n, T eps2, nb_stream_t stream) {
    if (!size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    const auto           s      = static_cast<hipStream_t>(stream);
    if constexpr (Order == 6) {
        if (workspace_bytes < 3 * bodies) return NB_ERR_INVALID_ARGUMENT;
        // acc_out: acc_in itself (the evaluation reads the workspace's copy), or an array apart from everything
        if (!in_place_or_apart({acc, bodies, al}, acc_in,
                               {{jerk, bodies, al}, {snap, bodies, al}, {pos, bodies, al}, {vel, bodies, al}, {acc_in, bodies, al}, {workspace, 3 * bodies, al}})) {
            return NB_ERR_INVALID_ARGUMENT;
        }
        if (const auto err = launch_hermite6_pack<T>(static_cast<T*>(workspace), pos, vel, acc_in, nullptr, n, s); err != hipSuccess) return static_cast<int>(err);
        Hermite6Args<T> a{};
        a.state12 = static_cast<const T*>(workspace), a.acc = acc, a.jerk = jerk, a.snap = snap, a.n = n, a.eps2 = floored(eps2);
        return static_cast<int>(launch_hermite6_eval<T>(a, s));
    } else {
        if (!spans_ok({{acc, bodies, al}, {jerk, bodies, al}, {pos, bodies, al}, {vel, bodies, al}})) return NB_ERR_INVALID_ARGUMENT;
        HermiteArgs<T> a{};
        a.pos = pos, a.vel_in = vel, a.acc = acc, a.jerk = jerk, a.n = n, a.eps2 = floored(eps2);
        return static_cast<int>(launch_hermite_eval<T>(a, s));
    }
}

// the start of a 6th-order run (launch_hermite6_start); a 4th-order run starts with eval
template <typename T> int init(T* acc, T* jerk, T* snap, T* crackle, const T* pos, const T* vel, void* workspace, size_t workspace_bytes, unsigned n, T eps2, nb_stream_t stream) {
    if (!size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (workspace_bytes < 3 * bodies) return NB_ERR_INVALID_ARGUMENT;
    if (!spans_ok({{acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al}, {crackle, bodies, al}, {pos, bodies, al}, {vel, bodies, al}, {workspace, 3 * bodies, al}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    return static_cast<int>(launch_hermite6_start<T>(acc, jerk, snap, crackle, pos, vel, static_cast<T*>(workspace), n, floored(eps2), static_cast<hipStream_t>(stream)));
}

template <typename T, int Order>
int step(T* new_pos, const T* old_pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, void* workspace, size_t workspace_bytes, unsigned n, T dt, T eps2, nb_stream_t stream) {
    if (!size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T), state = kBodyVec4<Order> * bodies;
    if (workspace_bytes < state) return NB_ERR_INVALID_ARGUMENT;
    // new_positions: old_positions itself, or an array apart from everything
    if (!in_place_or_apart({new_pos, bodies, al}, old_pos,
                           {{old_pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al, kHigher<Order>},
                            {crackle, bodies, al, kHigher<Order>}, {workspace, state, al}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    std::conditional_t<Order == 6, Hermite6Args<T>, HermiteArgs<T>> a{};
    a.new_pos = new_pos, a.old_pos = old_pos, a.vel = vel, a.acc = acc, a.jerk = jerk, a.n = n, a.dt = dt, a.eps2 = floored(eps2);
    if constexpr (Order == 6) {
        a.state12 = static_cast<const T*>(workspace), a.snap = snap, a.crackle = crackle;
        return static_cast<int>(launch_hermite6_step<T>(a, static_cast<T*>(workspace), static_cast<hipStream_t>(stream)));
    } else {
        a.state8 = static_cast<const T*>(workspace);
        return static_cast<int>(launch_hermite_step<T>(a, static_cast<T*>(workspace), static_cast<hipStream_t>(stream)));
    }
}

template <typename T, int Order>
int timestep(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, T eta, T* dt_out, void* scratch, size_t scratch_bytes, nb_stream_t stream) {
    constexpr std::uintptr_t partials = kTimestepPartials * sizeof(double);  // NB_HERMITE_TIMESTEP_SCRATCH_BYTES
    if (!size_ok(n) || scratch_bytes < partials) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al, kHigher<Order>}, {crackle, bodies, al, kHigher<Order>}, {dt_out, sizeof(T), sizeof(T)},
                   {scratch, partials, 8}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    if constexpr (Order == 6) {
        return static_cast<int>(launch_hermite6_timestep<T>(acc, jerk, snap, crackle, n, eta, dt_out, static_cast<double*>(scratch), static_cast<hipStream_t>(stream)));
    } else {
        return static_cast<int>(launch_hermite_timestep<T>(acc, jerk, n, eta, dt_out, static_cast<double*>(scratch), static_cast<hipStream_t>(stream)));
    }
}

}  // namespace solo
}  // namespace nb
