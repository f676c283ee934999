// hermite6_block_boundary.hip -- the extern "C" boundary of libnbody_hip_hermite6_block.so (include/nbody_hip_hermite6_block.h).  Every
// argument is checked on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never
// synchronises.  The initial evaluation is hermite6_eval.o's (linked in; that object exports nothing).
#include "../../include/nbody_hip_hermite6_block.h"
#include "capi_check.h"
#include "hermite6_block_kernels.h"
#include "hermite6_kernels.h"
#include "hermite6_block_boundary.h"  // block6_params_ok: the "Range of h"
#include "softening_floor.h"

namespace {

using nb::floored, nb::Span, nb::spans_ok;

static_assert(nb::kBlockMaxBodies <= nb::kHermite6MaxBodies, "the initial evaluation takes every N the block steps take");

nb::BlockLayout layout(unsigned n, size_t size_t_of) { return nb::block_layout(n, size_t_of, 3, nb::kBlock6Sums); }  // a predicted body is three vec4

template <typename T> int plan_query(unsigned n, unsigned n_active, nb_hermite_block_plan_t* out) {
    if (out == nullptr || !nb::block_size_ok(n) || n_active < 1 || n_active > n) return NB_ERR_INVALID_ARGUMENT;
    nb::block_plan_fill(out, n, n_active, sizeof(T), nb::kBlock6Sums, nb::hermite6_unroll_for<T>());
    out->launches       = 6;
    out->partial_offset = layout(n, sizeof(T)).partial;
    return 0;
}

// the arrays of a system and the workspace, checked; fills `a`
template <typename T>
bool bind(nb::Block6Args<T>& a, T* pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace,
          size_t workspace_bytes, unsigned n, const nb_hermite_block_params_t* params) {
    if (!nb::block_size_ok(n) || !nb::block6_params_ok<T>(params)) return false;
    const nb::BlockLayout l = layout(n, sizeof(T));
    if (workspace_bytes < l.bytes) return false;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al}, {crackle, bodies, al},
                   {ticks, static_cast<std::uintptr_t>(n) * 8, 8}, {levels, static_cast<std::uintptr_t>(n) * 4, 4}, {status, 64, 8}, {workspace, l.bytes, 32}})) {
        return false;
    }
    char* const ws = static_cast<char*>(workspace);
    a.pos = pos, a.vel = vel, a.acc = acc, a.jerk = jerk, a.snap = snap, a.crackle = crackle;
    a.ticks    = reinterpret_cast<unsigned long long*>(ticks);
    a.levels   = levels;
    a.status   = reinterpret_cast<nb::BlockStatus*>(status);
    a.state12  = reinterpret_cast<T*>(ws + l.state);
    a.partial  = reinterpret_cast<T*>(ws + l.partial);
    a.active   = reinterpret_cast<unsigned*>(ws + l.active);
    a.counts   = reinterpret_cast<unsigned*>(ws + l.counts);
    a.min_part = reinterpret_cast<unsigned long long*>(ws + l.min_part);
    a.lvl_part = reinterpret_cast<int*>(ws + l.lvl_part);
    a.ctrl     = reinterpret_cast<nb::BlockCtrl*>(ws + l.ctrl);
    a.n        = n;
    a.p        = nb::block_params_of(params);
    a.t_stop   = 0;
    return true;
}

template <typename T>
int init(T* pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
         unsigned n, T eps2, const nb_hermite_block_params_t* params, nb_stream_t stream) {
    nb::Block6Args<T> a{};
    if (!bind(a, pos, vel, acc, jerk, snap, crackle, ticks, levels, status, workspace, workspace_bytes, n, params)) return NB_ERR_INVALID_ARGUMENT;
    a.eps2       = floored(eps2);
    const auto s = static_cast<hipStream_t>(stream);
    // the four launches of nb_hermite6_init_*: a and jerk with b = 0, the snap with that a, crackle = 0
    nb::Hermite6Args<T> e{};
    e.state12 = a.state12, e.acc = acc, e.jerk = jerk, e.snap = snap, e.n = n, e.eps2 = a.eps2;
    if (const auto err = nb::launch_hermite6_pack<T>(a.state12, pos, vel, nullptr, nullptr, n, s); err != hipSuccess) return static_cast<int>(err);
    if (const auto err = nb::launch_hermite6_eval<T>(e, s); err != hipSuccess) return static_cast<int>(err);
    if (const auto err = nb::launch_hermite6_pack<T>(a.state12, pos, vel, acc, crackle, n, s); err != hipSuccess) return static_cast<int>(err);
    if (const auto err = nb::launch_hermite6_eval<T>(e, s); err != hipSuccess) return static_cast<int>(err);
    return static_cast<int>(nb::launch_block6_init<T>(a, s));
}

template <typename T>
int step(T* pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
         unsigned n, T eps2, const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream) {
    nb::Block6Args<T> a{};
    if (std::isnan(t_stop)) return NB_ERR_INVALID_ARGUMENT;
    if (!bind(a, pos, vel, acc, jerk, snap, crackle, ticks, levels, status, workspace, workspace_bytes, n, params)) return NB_ERR_INVALID_ARGUMENT;
    a.eps2   = floored(eps2);
    a.t_stop = t_stop;
    return static_cast<int>(nb::launch_block6_step<T>(a, static_cast<hipStream_t>(stream)));
}

template <typename T>
int sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const T* snap, const T* crackle, const uint64_t* ticks,
         const nb_hermite_block_status_t* status, unsigned n, const nb_hermite_block_params_t* params, nb_stream_t stream) {
    if (!nb::block_size_ok(n) || !nb::block6_params_ok<T>(params)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{pos_out, bodies, al}, {vel_out, bodies, al}, {pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al},
                   {crackle, bodies, al}, {ticks, static_cast<std::uintptr_t>(n) * 8, 8}, {status, 64, 8}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    return static_cast<int>(nb::launch_block6_sync<T>(pos_out, vel_out, pos, vel, acc, jerk, snap, crackle, reinterpret_cast<const unsigned long long*>(ticks),
                                                      reinterpret_cast<const nb::BlockStatus*>(status), n, nb::block_params_of(params), static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nb_hermite6_block_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !nb::block_size_ok(num_bodies) || !nb::element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = layout(num_bodies, sizeof_T).bytes;
    return 0;
}

int nb_hermite6_block_plan_f32(unsigned num_bodies, unsigned num_active, nb_hermite_block_plan_t* plan) { return plan_query<float>(num_bodies, num_active, plan); }
int nb_hermite6_block_plan_f64(unsigned num_bodies, unsigned num_active, nb_hermite_block_plan_t* plan) { return plan_query<double>(num_bodies, num_active, plan); }

int nb_hermite6_block_init_f32(float* positions, float* velocities, float* accelerations, float* jerks, float* snaps, float* crackles, uint64_t* ticks, int32_t* levels,
                               nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies, float softening_sq,
                               const nb_hermite_block_params_t* params, nb_stream_t stream) {
    return init<float>(positions, velocities, accelerations, jerks, snaps, crackles, ticks, levels, status, workspace, workspace_bytes, num_bodies, softening_sq, params, stream);
}
int nb_hermite6_block_init_f64(double* positions, double* velocities, double* accelerations, double* jerks, double* snaps, double* crackles, uint64_t* ticks, int32_t* levels,
                               nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies, double softening_sq,
                               const nb_hermite_block_params_t* params, nb_stream_t stream) {
    return init<double>(positions, velocities, accelerations, jerks, snaps, crackles, ticks, levels, status, workspace, workspace_bytes, num_bodies, softening_sq, params, stream);
}

int nb_hermite6_block_step_f32(float* positions, float* velocities, float* accelerations, float* jerks, float* snaps, float* crackles, uint64_t* ticks, int32_t* levels,
                               nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies, float softening_sq,
                               const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream) {
    return step<float>(positions, velocities, accelerations, jerks, snaps, crackles, ticks, levels, status, workspace, workspace_bytes, num_bodies, softening_sq, params, t_stop,
                       stream);
}
int nb_hermite6_block_step_f64(double* positions, double* velocities, double* accelerations, double* jerks, double* snaps, double* crackles, uint64_t* ticks, int32_t* levels,
                               nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies, double softening_sq,
                               const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream) {
    return step<double>(positions, velocities, accelerations, jerks, snaps, crackles, ticks, levels, status, workspace, workspace_bytes, num_bodies, softening_sq, params, t_stop,
                        stream);
}

int nb_hermite6_block_sync_f32(float* positions_out, float* velocities_out, const float* positions, const float* velocities, const float* accelerations, const float* jerks,
                               const float* snaps, const float* crackles, const uint64_t* ticks, const nb_hermite_block_status_t* status, unsigned num_bodies,
                               const nb_hermite_block_params_t* params, nb_stream_t stream) {
    return sync<float>(positions_out, velocities_out, positions, velocities, accelerations, jerks, snaps, crackles, ticks, status, num_bodies, params, stream);
}
int nb_hermite6_block_sync_f64(double* positions_out, double* velocities_out, const double* positions, const double* velocities, const double* accelerations, const double* jerks,
                               const double* snaps, const double* crackles, const uint64_t* ticks, const nb_hermite_block_status_t* status, unsigned num_bodies,
                               const nb_hermite_block_params_t* params, nb_stream_t stream) {
    return sync<double>(positions_out, velocities_out, positions, velocities, accelerations, jerks, snaps, crackles, ticks, status, num_bodies, params, stream);
}

}  // extern "C"
