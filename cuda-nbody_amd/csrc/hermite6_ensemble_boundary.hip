// hermite6_ensemble_boundary.hip -- the extern "C" boundary of libnbody_hip_hermite6_ensemble.so (include/nbody_hip_hermite6_ensemble.h).
// Every argument is checked on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never waits
// for the device.  softening^2 == 0 takes its floor per system, on the device (floored of softening_floor.h, in system_parameters).
#include "../../include/nbody_hip_hermite6_ensemble.h"
#include "capi_check.h"
#include "hermite6_ensemble_kernels.h"
#include "softening_floor.h"

namespace {

using nb::in_place_or_apart, nb::Span, nb::spans_ok;

static_assert(NB_HERMITE_ENSEMBLE_MAX_BODIES == nb::kEnsembleHermiteMaxBodies && NB_HERMITE_ENSEMBLE_MAX_TOTAL == nb::kEnsembleHermiteMaxTotal, "the header's limits are the kernels'");
static_assert(NB_HERMITE_ENSEMBLE_DONE == nb::kClockDone && NB_HERMITE_ENSEMBLE_STALLED == nb::kClockStalled, "the header's flags are the kernels'");
static_assert(sizeof(nb_hermite_ensemble_clock_t) == sizeof(nb::EnsembleClock) && sizeof(nb_hermite_ensemble_status_t) == sizeof(nb::EnsembleStatus),
              "the header's records are the kernels'");
static_assert(nb::kEnsembleTimestepBodies == 256 && nb::kEnsembleClockSystems == 256, "the header's workspace formula");

template <typename T> bool size_ok(unsigned n, unsigned b) {
    if (n < 1 || n > nb::kEnsembleHermiteMaxBodies || b < 1 || static_cast<unsigned long long>(n) * b > nb::kEnsembleHermiteMaxTotal) return false;
    const nb::EnsembleHermite6Plan p = nb::plan_hermite6_ensemble<T>(n, b);
    return p.grid_blocks * p.block_threads <= (1ull << 31);  // one launch per stage
}

// the workspace: the predicted state, the partial minima of every system, the partial status records
template <typename T> struct Layout {
    std::uintptr_t bodies, state, partial, total;
    Layout(unsigned n, unsigned b) {
        bodies  = static_cast<std::uintptr_t>(n) * b * 4 * sizeof(T);
        state   = 3 * bodies;
        partial = static_cast<std::uintptr_t>(b) * nb::ensemble_partials(n) * sizeof(double);
        total   = state + partial + static_cast<std::uintptr_t>(nb::ensemble_status_blocks(b)) * sizeof(nb::EnsembleStatus);
    }
    double*             partials(void* ws) const { return reinterpret_cast<double*>(static_cast<char*>(ws) + state); }
    nb::EnsembleStatus* blocks(void* ws) const { return reinterpret_cast<nb::EnsembleStatus*>(static_cast<char*>(ws) + state + partial); }
};

template <typename T> int plan_query(unsigned n, unsigned b, nb_hermite_ensemble_plan_t* out) {
    if (out == nullptr || !size_ok<T>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const nb::EnsembleHermite6Plan p = nb::plan_hermite6_ensemble<T>(n, b);
    out->bodies_per_lane   = p.bodies_per_lane;
    out->waves_per_group   = p.waves;
    out->unroll            = p.unroll;
    out->groups            = p.groups;
    out->block_threads     = p.block_threads;
    out->lds_bytes         = p.lds_bytes;
    out->groups_per_system = p.groups;
    out->reserved          = 0;
    out->grid_blocks       = p.grid_blocks;
    return 0;
}

template <typename T>
int eval(T* acc, T* jerk, T* snap, const T* pos, const T* vel, const T* acc_in, void* workspace, size_t workspace_bytes, unsigned n, unsigned b, T eps2, const T* system_eps2,
         nb_stream_t stream) {
    if (!size_ok<T>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    // acc_out: acc_in itself (the evaluation reads the workspace's copy), or an array apart from everything
    if (!in_place_or_apart({acc, l.bodies, al}, acc_in,
                           {{jerk, l.bodies, al}, {snap, l.bodies, al}, {pos, l.bodies, al}, {vel, l.bodies, al}, {acc_in, l.bodies, al}, {workspace, l.total, al},
                            {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    const auto s = static_cast<hipStream_t>(stream);
    T* const   w = static_cast<T*>(workspace);
    if (const auto err = nb::launch_ensemble6_pack<T>(w, pos, vel, acc_in, nullptr, n, b, s); err != hipSuccess) return static_cast<int>(err);
    nb::EnsembleHermite6Args<T> a{};
    a.state12 = w, a.acc = acc, a.jerk = jerk, a.snap = snap, a.n = n, a.src.eps2 = eps2, a.src.system_eps2 = system_eps2;
    return static_cast<int>(nb::launch_ensemble6_eval<T>(a, b, s));
}

// the four launches of nb_hermite6_init_*, for every system; the arrays are checked by the caller
template <typename T>
hipError_t init_launches(T* acc, T* jerk, T* snap, T* crackle, const T* pos, const T* vel, T* w, unsigned n, unsigned b, T eps2, const T* system_eps2, hipStream_t s) {
    nb::EnsembleHermite6Args<T> a{};
    a.state12 = w, a.acc = acc, a.jerk = jerk, a.snap = snap, a.n = n, a.src.eps2 = eps2, a.src.system_eps2 = system_eps2;
    // a and jerk do not depend on the accelerations: a first pass with b = 0, a second with that a for the snap
    if (const auto err = nb::launch_ensemble6_pack<T>(w, pos, vel, nullptr, nullptr, n, b, s); err != hipSuccess) return err;
    if (const auto err = nb::launch_ensemble6_eval<T>(a, b, s); err != hipSuccess) return err;
    if (const auto err = nb::launch_ensemble6_pack<T>(w, pos, vel, acc, crackle, n, b, s); err != hipSuccess) return err;
    return nb::launch_ensemble6_eval<T>(a, b, s);
}

template <typename T>
int init(T* acc, T* jerk, T* snap, T* crackle, const T* pos, const T* vel, void* workspace, size_t workspace_bytes, unsigned n, unsigned b, T eps2, const T* system_eps2,
         nb_stream_t stream) {
    if (!size_ok<T>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    if (!spans_ok({{acc, l.bodies, al}, {jerk, l.bodies, al}, {snap, l.bodies, al}, {crackle, l.bodies, al}, {pos, l.bodies, al}, {vel, l.bodies, al}, {workspace, l.total, al},
                   {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    return static_cast<int>(init_launches<T>(acc, jerk, snap, crackle, pos, vel, static_cast<T*>(workspace), n, b, eps2, system_eps2, static_cast<hipStream_t>(stream)));
}

template <typename T>
int step(T* new_pos, const T* old_pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, void* workspace, size_t workspace_bytes, unsigned n, unsigned b, T dt, T eps2,
         const T* params, nb_stream_t stream) {
    if (!size_ok<T>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    // new_positions: old_positions itself, or an array apart from everything
    if (!in_place_or_apart({new_pos, l.bodies, al}, old_pos,
                           {{old_pos, l.bodies, al}, {vel, l.bodies, al}, {acc, l.bodies, al}, {jerk, l.bodies, al}, {snap, l.bodies, al}, {crackle, l.bodies, al},
                            {workspace, l.total, al}, {params, b * al, al, Span::optional}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    nb::EnsembleHermite6Args<T> a{};
    a.state12 = static_cast<const T*>(workspace);
    a.new_pos = new_pos, a.old_pos = old_pos, a.vel = vel, a.acc = acc, a.jerk = jerk, a.snap = snap, a.crackle = crackle, a.n = n;
    a.src.dt = dt, a.src.eps2 = eps2, a.src.params = params;
    return static_cast<int>(nb::launch_ensemble6_step<T>(a, b, static_cast<T*>(workspace), static_cast<hipStream_t>(stream)));
}

template <typename T>
int timestep(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, unsigned b, T eta, T* dt_out, void* workspace, size_t workspace_bytes, nb_stream_t stream) {
    if (!size_ok<T>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    if (!spans_ok({{acc, l.bodies, al}, {jerk, l.bodies, al}, {snap, l.bodies, al}, {crackle, l.bodies, al}, {dt_out, b * sizeof(T), sizeof(T)}, {workspace, l.total, al}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    const nb::EnsembleSource<T> none{};
    return static_cast<int>(nb::launch_ensemble6_clocks<T>(acc, jerk, snap, crackle, n, b, eta, dt_out, nullptr, false, none, l.partials(workspace), nullptr, nullptr,
                                                           static_cast<hipStream_t>(stream)));
}

template <typename T>
int begin(T* acc, T* jerk, T* snap, T* crackle, const T* pos, const T* vel, nb_hermite_ensemble_clock_t* clocks, unsigned n, unsigned b, T eps2, const T* system_eps2, T eta,
          void* workspace, size_t workspace_bytes, nb_stream_t stream) {
    if (!size_ok<T>(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    if (!spans_ok({{acc, l.bodies, al}, {jerk, l.bodies, al}, {snap, l.bodies, al}, {crackle, l.bodies, al}, {pos, l.bodies, al}, {vel, l.bodies, al},
                   {clocks, b * sizeof(nb::EnsembleClock), 8}, {workspace, l.total, al}, {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    const auto s = static_cast<hipStream_t>(stream);
    if (const auto err = init_launches<T>(acc, jerk, snap, crackle, pos, vel, static_cast<T*>(workspace), n, b, eps2, system_eps2, s); err != hipSuccess) {
        return static_cast<int>(err);
    }
    const nb::EnsembleSource<T> none{};
    return static_cast<int>(nb::launch_ensemble6_clocks<T>(acc, jerk, snap, crackle, n, b, eta, nullptr, reinterpret_cast<nb::EnsembleClock*>(clocks), true, none,
                                                           l.partials(workspace), nullptr, nullptr, s));
}

template <typename T>
int advance(T* new_pos, const T* old_pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, nb_hermite_ensemble_clock_t* clocks, nb_hermite_ensemble_status_t* status,
            void* workspace, size_t workspace_bytes, unsigned n, unsigned b, double t_stop, double dt_max, T eta, T eps2, const T* system_eps2, nb_stream_t stream) {
    if (!size_ok<T>(n, b) || t_stop != t_stop || !(dt_max > 0)) return NB_ERR_INVALID_ARGUMENT;
    const Layout<T> l(n, b);
    if (workspace_bytes < l.total) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T);
    // new_positions: old_positions itself, or an array apart from everything
    if (!in_place_or_apart({new_pos, l.bodies, al}, old_pos,
                           {{old_pos, l.bodies, al}, {vel, l.bodies, al}, {acc, l.bodies, al}, {jerk, l.bodies, al}, {snap, l.bodies, al}, {crackle, l.bodies, al},
                            {workspace, l.total, al}, {clocks, b * sizeof(nb::EnsembleClock), 8}, {status, sizeof(nb::EnsembleStatus), 8, Span::optional},
                            {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    nb::EnsembleHermite6Args<T> a{};
    a.state12 = static_cast<const T*>(workspace);
    a.new_pos = new_pos, a.old_pos = old_pos, a.vel = vel, a.acc = acc, a.jerk = jerk, a.snap = snap, a.crackle = crackle, a.n = n;
    a.src.clocks = reinterpret_cast<const nb::EnsembleClock*>(clocks), a.src.t_stop = t_stop, a.src.dt_max = dt_max, a.src.eps2 = eps2, a.src.system_eps2 = system_eps2;
    const auto s = static_cast<hipStream_t>(stream);
    if (const auto err = nb::launch_ensemble6_step<T>(a, b, static_cast<T*>(workspace), s); err != hipSuccess) return static_cast<int>(err);
    return static_cast<int>(nb::launch_ensemble6_clocks<T>(acc, jerk, snap, crackle, n, b, eta, nullptr, reinterpret_cast<nb::EnsembleClock*>(clocks), false, a.src,
                                                           l.partials(workspace), l.blocks(workspace), reinterpret_cast<nb::EnsembleStatus*>(status), s));
}

}  // namespace

extern "C" {

int nb_hermite6_ensemble_workspace_bytes(unsigned num_bodies, unsigned num_systems, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !nb::element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    if (!(sizeof_T == 4 ? size_ok<float>(num_bodies, num_systems) : size_ok<double>(num_bodies, num_systems))) return NB_ERR_INVALID_ARGUMENT;
    *bytes = sizeof_T == 4 ? Layout<float>(num_bodies, num_systems).total : Layout<double>(num_bodies, num_systems).total;
    return 0;
}

int nb_hermite6_ensemble_plan_f32(unsigned num_bodies, unsigned num_systems, nb_hermite_ensemble_plan_t* plan) { return plan_query<float>(num_bodies, num_systems, plan); }
int nb_hermite6_ensemble_plan_f64(unsigned num_bodies, unsigned num_systems, nb_hermite_ensemble_plan_t* plan) { return plan_query<double>(num_bodies, num_systems, plan); }

#define NB_HERMITE6_ENSEMBLE_ENTRY_POINTS(T, SUFFIX)                                                                                                                        \
    int nb_hermite6_ensemble_eval_##SUFFIX(T* acc_out, T* jerk_out, T* snap_out, const T* positions, const T* velocities, const T* acc_in, void* workspace,                 \
                                           size_t workspace_bytes, unsigned num_bodies, unsigned num_systems, T softening_sq, const T* system_softening_sq,                 \
                                           nb_stream_t stream) {                                                                                                            \
        return eval<T>(acc_out, jerk_out, snap_out, positions, velocities, acc_in, workspace, workspace_bytes, num_bodies, num_systems, softening_sq, system_softening_sq,  \
                       stream);                                                                                                                                             \
    }                                                                                                                                                                       \
    int nb_hermite6_ensemble_init_##SUFFIX(T* accelerations, T* jerks, T* snaps, T* crackles, const T* positions, const T* velocities, void* workspace,                     \
                                           size_t workspace_bytes, unsigned num_bodies, unsigned num_systems, T softening_sq, const T* system_softening_sq,                 \
                                           nb_stream_t stream) {                                                                                                            \
        return init<T>(accelerations, jerks, snaps, crackles, positions, velocities, workspace, workspace_bytes, num_bodies, num_systems, softening_sq,                     \
                       system_softening_sq, stream);                                                                                                                        \
    }                                                                                                                                                                       \
    int nb_hermite6_ensemble_step_##SUFFIX(T* new_positions, const T* old_positions, T* velocities, T* accelerations, T* jerks, T* snaps, T* crackles, void* workspace,     \
                                           size_t workspace_bytes, unsigned num_bodies, unsigned num_systems, T delta_time, T softening_sq, const T* system_params,         \
                                           nb_stream_t stream) {                                                                                                            \
        return step<T>(new_positions, old_positions, velocities, accelerations, jerks, snaps, crackles, workspace, workspace_bytes, num_bodies, num_systems, delta_time,    \
                       softening_sq, system_params, stream);                                                                                                                \
    }                                                                                                                                                                       \
    int nb_hermite6_ensemble_timestep_##SUFFIX(const T* accelerations, const T* jerks, const T* snaps, const T* crackles, unsigned num_bodies, unsigned num_systems, T eta, \
                                               T* dt_out, void* workspace, size_t workspace_bytes, nb_stream_t stream) {                                                    \
        return timestep<T>(accelerations, jerks, snaps, crackles, num_bodies, num_systems, eta, dt_out, workspace, workspace_bytes, stream);                                \
    }                                                                                                                                                                       \
    int nb_hermite6_ensemble_begin_##SUFFIX(T* accelerations, T* jerks, T* snaps, T* crackles, const T* positions, const T* velocities,                                     \
                                            nb_hermite_ensemble_clock_t* clocks, unsigned num_bodies, unsigned num_systems, T softening_sq, const T* system_softening_sq,   \
                                            T eta, void* workspace, size_t workspace_bytes, nb_stream_t stream) {                                                           \
        return begin<T>(accelerations, jerks, snaps, crackles, positions, velocities, clocks, num_bodies, num_systems, softening_sq, system_softening_sq, eta, workspace,   \
                        workspace_bytes, stream);                                                                                                                           \
    }                                                                                                                                                                       \
    int nb_hermite6_ensemble_advance_##SUFFIX(T* new_positions, const T* old_positions, T* velocities, T* accelerations, T* jerks, T* snaps, T* crackles,                   \
                                              nb_hermite_ensemble_clock_t* clocks, nb_hermite_ensemble_status_t* status, void* workspace, size_t workspace_bytes,           \
                                              unsigned num_bodies, unsigned num_systems, double t_stop, double dt_max, T eta, T softening_sq,                               \
                                              const T* system_softening_sq, nb_stream_t stream) {                                                                           \
        return advance<T>(new_positions, old_positions, velocities, accelerations, jerks, snaps, crackles, clocks, status, workspace, workspace_bytes, num_bodies,          \
                          num_systems, t_stop, dt_max, eta, softening_sq, system_softening_sq, stream);                                                                     \
    }
NB_HERMITE6_ENSEMBLE_ENTRY_POINTS(float, f32)
NB_HERMITE6_ENSEMBLE_ENTRY_POINTS(double, f64)
#undef NB_HERMITE6_ENSEMBLE_ENTRY_POINTS

}  // extern "C"
