// hermite_ensemble_boundary.h -- the extern "C" boundary of the Hermite libraries that step many independent systems, each with a time
// step of its own (hermite_ensemble_capi.hip, hermite6_ensemble_boundary.hip), one text for both orders, templated on <T, Order> as
// hermite_boundary.h: the size check, the workspace layout, the plan query and every call's argument check and launch sequence.  Host only.
//
// Every argument is checked on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never waits
// for the device.  softening^2 == 0 takes its floor per system, on the device (floored of softening_floor.h, in system_parameters).
#pragma once

#include "../../include/nbody_hip_hermite_ensemble.h"
#include "capi_check.h"
#include "hermite6_ensemble_kernels.h"
#include "hermite_boundary.h"  // what the order decides
#include "hermite_ensemble_kernels.h"
#include "softening_floor.h"

namespace nb::ensemble {

static_assert(NB_HERMITE_ENSEMBLE_MAX_BODIES == kEnsembleHermiteMaxBodies && NB_HERMITE_ENSEMBLE_MAX_TOTAL == kEnsembleHermiteMaxTotal, "the header's limits are the kernels'");
static_assert(NB_HERMITE_ENSEMBLE_DONE == kClockDone && NB_HERMITE_ENSEMBLE_STALLED == kClockStalled, "the header's flags are the kernels'");
static_assert(sizeof(nb_hermite_ensemble_clock_t) == sizeof(EnsembleClock) && sizeof(nb_hermite_ensemble_status_t) == sizeof(EnsembleStatus),
              "the header's records are the kernels'");
static_assert(kEnsembleTimestepBodies == 256 && kEnsembleClockSystems == 256, "the headers' workspace formula");

// the evaluation of B systems of N bodies is one launch: groups * B workgroups, 2^31 threads at the most
template <typename T, int Order> bool grid_ok(unsigned n, unsigned b) {
    const StreamPlan p = order_plan<T, Order>(n);
    return static_cast<unsigned long long>(p.groups) * b * p.block_threads <= (1ull << 31);
}

template <typename T, int Order> bool size_ok(unsigned n, unsigned b) {
    if (n < 1 || n > kEnsembleHermiteMaxBodies || b < 1 || static_cast<unsigned long long>(n) * b > kEnsembleHermiteMaxTotal) return false;
    return grid_ok<T, Order>(n, b);  // one launch per stage
}

// the workspace: the predicted state, the partial minima of every system, the partial status records
template <typename T, int Order> struct Layout {
    std::uintptr_t bodies, state, partial, total;
    Layout(unsigned n, unsigned b) {
        bodies  = static_cast<std::uintptr_t>(n) * b * 4 * sizeof(T);
        state   = kBodyVec4<Order> * bodies;
        partial = static_cast<std::uintptr_t>(b) * ensemble_partials(n) * sizeof(double);
        total   = state + partial + static_cast<std::uintptr_t>(ensemble_status_blocks(b)) * sizeof(EnsembleStatus);
    }
    double*         partials(void* ws) const { return reinterpret_cast<double*>(static_cast<char*>(ws) + state); }
    EnsembleStatus* blocks(void* ws) const { return reinterpret_cast<EnsembleStatus*>(static_cast<char*>(ws) + state + partial); }
};

template <typename T, int Order> int workspace_bytes_of(unsigned n, unsigned b, size_t* bytes) {
    if (!size_ok<T, Order>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = Layout<T, Order>(n, b).total;
    return 0;
}
template <int Order> int workspace_bytes(unsigned n, unsigned b, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    return sizeof_T == 4 ? workspace_bytes_of<float, Order>(n, b, bytes) : workspace_bytes_of<double, Order>(n, b, bytes);
}

template <typename T, int Order> int plan_query(unsigned n, unsigned b, nb_hermite_ensemble_plan_t* out) {
    if (out == nullptr || !size_ok<T, Order>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const StreamPlan p = order_plan<T, Order>(n);
    fill(out, p);
    out->groups_per_system = p.groups;
    out->reserved          = 0;
    out->grid_blocks       = static_cast<unsigned long long>(p.groups) * b;
    return 0;
}

// ---- the order's kernel interface ------------------------------------------------------------------------------------------------------
template <typename T, int Order> using Args = std::conditional_t<Order == 6, EnsembleHermite6Args<T>, EnsembleHermiteArgs<T>>;

// what a step works on (nb_*_step_*, nb_*_advance_*); the caller adds where dt and softening^2 come from (a.src)
template <typename T, int Order> Args<T, Order> step_args(T* new_pos, const T* old_pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, const void* workspace, unsigned n) {
    Args<T, Order> a{};
    a.new_pos = new_pos, a.old_pos = old_pos, a.vel = vel, a.acc = acc, a.jerk = jerk, a.n = n;
    if constexpr (Order == 6) {
        a.state12 = static_cast<const T*>(workspace), a.snap = snap, a.crackle = crackle;
    } else {
        a.state8 = static_cast<const T*>(workspace);
    }
    return a;
}
template <typename T, int Order> hipError_t launch_step(const Args<T, Order>& a, unsigned b, void* workspace, hipStream_t s) {
    if constexpr (Order == 6) {
        return launch_ensemble6_step<T>(a, b, static_cast<T*>(workspace), s);
    } else {
        return launch_ensemble_step<T>(a, b, static_cast<T*>(workspace), s);
    }
}
template <typename T, int Order>
hipError_t launch_clocks(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, unsigned b, T eta, T* dt_out, nb_hermite_ensemble_clock_t* clocks, bool begin,
                         const EnsembleSource<T>& src, double* partial, EnsembleStatus* block_status, nb_hermite_ensemble_status_t* status, hipStream_t s) {
    auto* const c  = reinterpret_cast<EnsembleClock*>(clocks);
    auto* const st = reinterpret_cast<EnsembleStatus*>(status);
    if constexpr (Order == 6) {
        return launch_ensemble6_clocks<T>(acc, jerk, snap, crackle, n, b, eta, dt_out, c, begin, src, partial, block_status, st, s);
    } else {
        return launch_ensemble_clocks<T>(acc, jerk, n, b, eta, dt_out, c, begin, src, partial, block_status, st, s);
    }
}

// ---- the calls -------------------------------------------------------------------------------------------------------------------------
// Order 4: acc and jerk of (pos, vel); there is no snap, acc_in or workspace.  Order 6: and the snap, which needs accelerations: the
// evaluation reads the workspace's copy of {pos, vel, acc_in}.
template <typename T, int Order>
int eval(T* acc, T* jerk, T* snap, const T* pos, const T* vel, const T* acc_in, void* workspace, size_t workspace_bytes, unsigned n, unsigned b, T eps2, const T* system_eps2,
         nb_stream_t stream) {
    if (!size_ok<T, Order>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T, Order> l(n, b);
    const std::uintptr_t   al = 4 * sizeof(T);
    const auto             s  = static_cast<hipStream_t>(stream);
    Args<T, Order>         a{};
    a.acc = acc, a.jerk = jerk, a.n = n, a.src.eps2 = eps2, a.src.system_eps2 = system_eps2;
    if constexpr (Order == 6) {
        if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
        // acc_out: acc_in itself (the evaluation reads the workspace's copy), or an array apart from everything
        if (!in_place_or_apart({acc, l.bodies, al}, acc_in,
                               {{jerk, l.bodies, al}, {snap, l.bodies, al}, {pos, l.bodies, al}, {vel, l.bodies, al}, {acc_in, l.bodies, al}, {workspace, l.total, al},
                                {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
            return NB_ERR_INVALID_ARGUMENT;
        }
        T* const w = static_cast<T*>(workspace);
        if (const auto err = launch_ensemble6_pack<T>(w, pos, vel, acc_in, nullptr, n, b, s); err != hipSuccess) return static_cast<int>(err);
        a.state12 = w, a.snap = snap;
        return static_cast<int>(launch_ensemble6_eval<T>(a, b, s));
    } else {
        if (!spans_ok({{acc, l.bodies, al}, {jerk, l.bodies, al}, {pos, l.bodies, al}, {vel, l.bodies, al}, {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
            return NB_ERR_INVALID_ARGUMENT;
        }
        a.pos = pos, a.vel_in = vel;
        return static_cast<int>(launch_ensemble_eval<T>(a, b, s));
    }
}

// the start of a 6th-order run (launch_ensemble6_start); a 4th-order run starts with eval
template <typename T>
int init(T* acc, T* jerk, T* snap, T* crackle, const T* pos, const T* vel, void* workspace, size_t workspace_bytes, unsigned n, unsigned b, T eps2, const T* system_eps2,
         nb_stream_t stream) {
    if (!size_ok<T, 6>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T, 6> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    if (!spans_ok({{acc, l.bodies, al}, {jerk, l.bodies, al}, {snap, l.bodies, al}, {crackle, l.bodies, al}, {pos, l.bodies, al}, {vel, l.bodies, al}, {workspace, l.total, al},
                   {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    return static_cast<int>(launch_ensemble6_start<T>(acc, jerk, snap, crackle, pos, vel, static_cast<T*>(workspace), n, b, eps2, system_eps2, static_cast<hipStream_t>(stream)));
}

template <typename T, int Order>
int step(T* new_pos, const T* old_pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, void* workspace, size_t workspace_bytes, unsigned n, unsigned b, T dt, T eps2,
         const T* params, nb_stream_t stream) {
    if (!size_ok<T, Order>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T, Order> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    // new_positions: old_positions itself, or an array apart from everything
    if (!in_place_or_apart({new_pos, l.bodies, al}, old_pos,
                           {{old_pos, l.bodies, al}, {vel, l.bodies, al}, {acc, l.bodies, al}, {jerk, l.bodies, al}, {snap, l.bodies, al, kHigher<Order>},
                            {crackle, l.bodies, al, kHigher<Order>}, {workspace, l.total, al}, {params, b * al, al, Span::optional}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    Args<T, Order> a = step_args<T, Order>(new_pos, old_pos, vel, acc, jerk, snap, crackle, workspace, n);
    a.src.dt = dt, a.src.eps2 = eps2, a.src.params = params;
    return static_cast<int>(launch_step<T, Order>(a, b, workspace, static_cast<hipStream_t>(stream)));
}

template <typename T, int Order>
int timestep(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, unsigned b, T eta, T* dt_out, void* workspace, size_t workspace_bytes, nb_stream_t stream) {
    if (!size_ok<T, Order>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T, Order> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    if (!spans_ok({{acc, l.bodies, al}, {jerk, l.bodies, al}, {snap, l.bodies, al, kHigher<Order>}, {crackle, l.bodies, al, kHigher<Order>}, {dt_out, b * sizeof(T), sizeof(T)},
                   {workspace, l.total, al}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    const EnsembleSource<T> none{};
    return static_cast<int>(
        launch_clocks<T, Order>(acc, jerk, snap, crackle, n, b, eta, dt_out, nullptr, false, none, l.partials(workspace), nullptr, nullptr, static_cast<hipStream_t>(stream)));
}

template <typename T, int Order>
int begin(T* acc, T* jerk, T* snap, T* crackle, const T* pos, const T* vel, nb_hermite_ensemble_clock_t* clocks, unsigned n, unsigned b, T eps2, const T* system_eps2, T eta,
          void* workspace, size_t workspace_bytes, nb_stream_t stream) {
    if (!size_ok<T, Order>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T, Order> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    if (!spans_ok({{acc, l.bodies, al}, {jerk, l.bodies, al}, {snap, l.bodies, al, kHigher<Order>}, {crackle, l.bodies, al, kHigher<Order>}, {pos, l.bodies, al},
                   {vel, l.bodies, al}, {clocks, b * sizeof(EnsembleClock), 8}, {workspace, l.total, al}, {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    const auto s = static_cast<hipStream_t>(stream);
    if constexpr (Order == 6) {
        if (const auto err = launch_ensemble6_start<T>(acc, jerk, snap, crackle, pos, vel, static_cast<T*>(workspace), n, b, eps2, system_eps2, s); err != hipSuccess) {
            return static_cast<int>(err);
        }
    } else {
        EnsembleHermiteArgs<T> a{};
        a.pos = pos, a.vel_in = vel, a.acc = acc, a.jerk = jerk, a.n = n, a.src.eps2 = eps2, a.src.system_eps2 = system_eps2;
        if (const auto err = launch_ensemble_eval<T>(a, b, s); err != hipSuccess) return static_cast<int>(err);
    }
    const EnsembleSource<T> none{};
    return static_cast<int>(launch_clocks<T, Order>(acc, jerk, snap, crackle, n, b, eta, nullptr, clocks, true, none, l.partials(workspace), nullptr, nullptr, s));
}

template <typename T, int Order>
int advance(T* new_pos, const T* old_pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, nb_hermite_ensemble_clock_t* clocks, nb_hermite_ensemble_status_t* status,
            void* workspace, size_t workspace_bytes, unsigned n, unsigned b, double t_stop, double dt_max, T eta, T eps2, const T* system_eps2, nb_stream_t stream) {
    if (!size_ok<T, Order>(n, b) || t_stop != t_stop || !(dt_max > 0)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T, Order> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    // new_positions: old_positions itself, or an array apart from everything
    if (!in_place_or_apart({new_pos, l.bodies, al}, old_pos,
                           {{old_pos, l.bodies, al}, {vel, l.bodies, al}, {acc, l.bodies, al}, {jerk, l.bodies, al}, {snap, l.bodies, al, kHigher<Order>},
                            {crackle, l.bodies, al, kHigher<Order>}, {workspace, l.total, al}, {clocks, b * sizeof(EnsembleClock), 8},
                            {status, sizeof(EnsembleStatus), 8, Span::optional}, {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    Args<T, Order> a = step_args<T, Order>(new_pos, old_pos, vel, acc, jerk, snap, crackle, workspace, n);
    a.src.clocks = reinterpret_cast<const EnsembleClock*>(clocks), a.src.t_stop = t_stop, a.src.dt_max = dt_max, a.src.eps2 = eps2, a.src.system_eps2 = system_eps2;
    const auto s = static_cast<hipStream_t>(stream);
    if (const auto err = launch_step<T, Order>(a, b, workspace, s); err != hipSuccess) return static_cast<int>(err);
    return static_cast<int>(launch_clocks<T, Order>(acc, jerk, snap, crackle, n, b, eta, nullptr, clocks, false, a.src, l.partials(workspace), l.blocks(workspace), status, s));
}

}  // namespace nb::ensemble
