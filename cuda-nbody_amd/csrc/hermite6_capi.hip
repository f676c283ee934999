// hermite6_capi.hip -- the extern "C" boundary of libnbody_hip_hermite6.so (include/nbody_hip_hermite6.h).  Every argument is checked
// on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never synchronises.
#include "../../include/nbody_hip_hermite6.h"
#include "capi_check.h"
#include "hermite6_kernels.h"
#include "softening_floor.h"

namespace {

using nb::floored, nb::in_place_or_apart, nb::Span, nb::spans_ok;

static_assert(NB_HERMITE6_MAX_BODIES == nb::kHermite6MaxBodies, "the header's limit is the kernels'");
static_assert(NB_HERMITE6_TIMESTEP_SCRATCH_BYTES == nb::kHermite6TimestepPartials * sizeof(double), "the header's scratch size is the kernels'");

bool size_ok(unsigned n) { return n >= 1 && n <= nb::kHermite6MaxBodies; }

template <typename T> int plan_query(unsigned n, nb_hermite6_plan_t* out) {
    if (out == nullptr || !size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    const nb::Hermite6Plan p = nb::plan_hermite6<T>(n);
    out->bodies_per_lane   = p.bodies_per_lane;
    out->waves_per_group   = p.waves;
    out->unroll            = p.unroll;
    out->groups            = p.groups;
    out->block_threads     = p.block_threads;
    out->lds_bytes         = p.lds_bytes;
    return 0;
}

template <typename T> int eval(T* acc, T* jerk, T* snap, const T* pos, const T* vel, const T* acc_in, void* workspace, size_t workspace_bytes, unsigned n, T eps2, nb_stream_t stream) {
    if (!size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (workspace_bytes < 3 * bodies) return NB_ERR_INVALID_ARGUMENT;
    // acc_out: acc_in itself (the evaluation reads the workspace's copy), or an array apart from everything
    if (!in_place_or_apart({acc, bodies, al}, acc_in,
                           {{jerk, bodies, al}, {snap, bodies, al}, {pos, bodies, al}, {vel, bodies, al}, {acc_in, bodies, al}, {workspace, 3 * bodies, al}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    const auto s = static_cast<hipStream_t>(stream);
    if (const auto err = nb::launch_hermite6_pack<T>(static_cast<T*>(workspace), pos, vel, acc_in, nullptr, n, s); err != hipSuccess) return static_cast<int>(err);
    nb::Hermite6Args<T> a{};
    a.state12 = static_cast<const T*>(workspace), a.acc = acc, a.jerk = jerk, a.snap = snap, a.n = n, a.eps2 = floored(eps2);
    return static_cast<int>(nb::launch_hermite6_eval<T>(a, s));
}

template <typename T> int init(T* acc, T* jerk, T* snap, T* crackle, const T* pos, const T* vel, void* workspace, size_t workspace_bytes, unsigned n, T eps2, nb_stream_t stream) {
    if (!size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (workspace_bytes < 3 * bodies) return NB_ERR_INVALID_ARGUMENT;
    if (!spans_ok({{acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al}, {crackle, bodies, al}, {pos, bodies, al}, {vel, bodies, al}, {workspace, 3 * bodies, al}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    const auto          s = static_cast<hipStream_t>(stream);
    T* const            w = static_cast<T*>(workspace);
    nb::Hermite6Args<T> a{};
    a.state12 = w, a.acc = acc, a.jerk = jerk, a.snap = snap, a.n = n, a.eps2 = floored(eps2);
    // a and jerk do not depend on the accelerations: a first pass with b = 0, a second with that a for the snap
    if (const auto err = nb::launch_hermite6_pack<T>(w, pos, vel, nullptr, nullptr, n, s); err != hipSuccess) return static_cast<int>(err);
    if (const auto err = nb::launch_hermite6_eval<T>(a, s); err != hipSuccess) return static_cast<int>(err);
    if (const auto err = nb::launch_hermite6_pack<T>(w, pos, vel, acc, crackle, n, s); err != hipSuccess) return static_cast<int>(err);
    return static_cast<int>(nb::launch_hermite6_eval<T>(a, s));
}

template <typename T>
int step(T* new_pos, const T* old_pos, T* vel, T* acc, T* jerk, T* snap, T* crackle, void* workspace, size_t workspace_bytes, unsigned n, T dt, T eps2, nb_stream_t stream) {
    if (!size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (workspace_bytes < 3 * bodies) return NB_ERR_INVALID_ARGUMENT;
    // new_positions: old_positions itself, or an array apart from everything
    if (!in_place_or_apart({new_pos, bodies, al}, old_pos,
                           {{old_pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al}, {crackle, bodies, al}, {workspace, 3 * bodies, al}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    nb::Hermite6Args<T> a{};
    a.state12 = static_cast<const T*>(workspace);
    a.new_pos = new_pos, a.old_pos = old_pos, a.vel = vel, a.acc = acc, a.jerk = jerk, a.snap = snap, a.crackle = crackle, a.n = n, a.dt = dt, a.eps2 = floored(eps2);
    return static_cast<int>(nb::launch_hermite6_step<T>(a, static_cast<T*>(workspace), static_cast<hipStream_t>(stream)));
}

template <typename T>
int timestep(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, T eta, T* dt_out, void* scratch, size_t scratch_bytes, nb_stream_t stream) {
    if (!size_ok(n) || scratch_bytes < NB_HERMITE6_TIMESTEP_SCRATCH_BYTES) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{acc, bodies, al}, {jerk, bodies, al}, {snap, bodies, al}, {crackle, bodies, al}, {dt_out, sizeof(T), sizeof(T)}, {scratch, NB_HERMITE6_TIMESTEP_SCRATCH_BYTES, 8}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    return static_cast<int>(nb::launch_hermite6_timestep<T>(acc, jerk, snap, crackle, n, eta, dt_out, static_cast<double*>(scratch), static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nb_hermite6_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !size_ok(num_bodies) || !nb::element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = static_cast<size_t>(num_bodies) * 12 * sizeof_T;
    return 0;
}

int nb_hermite6_plan_f32(unsigned num_bodies, nb_hermite6_plan_t* plan) { return plan_query<float>(num_bodies, plan); }
int nb_hermite6_plan_f64(unsigned num_bodies, nb_hermite6_plan_t* plan) { return plan_query<double>(num_bodies, plan); }

int nb_hermite6_eval_f32(float* acc_out, float* jerk_out, float* snap_out, const float* positions, const float* velocities, const float* acc_in, void* workspace,
                         size_t workspace_bytes, unsigned num_bodies, float softening_sq, nb_stream_t stream) {
    return eval<float>(acc_out, jerk_out, snap_out, positions, velocities, acc_in, workspace, workspace_bytes, num_bodies, softening_sq, stream);
}
int nb_hermite6_eval_f64(double* acc_out, double* jerk_out, double* snap_out, const double* positions, const double* velocities, const double* acc_in, void* workspace,
                         size_t workspace_bytes, unsigned num_bodies, double softening_sq, nb_stream_t stream) {
    return eval<double>(acc_out, jerk_out, snap_out, positions, velocities, acc_in, workspace, workspace_bytes, num_bodies, softening_sq, stream);
}

int nb_hermite6_init_f32(float* accelerations, float* jerks, float* snaps, float* crackles, const float* positions, const float* velocities, void* workspace,
                         size_t workspace_bytes, unsigned num_bodies, float softening_sq, nb_stream_t stream) {
    return init<float>(accelerations, jerks, snaps, crackles, positions, velocities, workspace, workspace_bytes, num_bodies, softening_sq, stream);
}
int nb_hermite6_init_f64(double* accelerations, double* jerks, double* snaps, double* crackles, const double* positions, const double* velocities, void* workspace,
                         size_t workspace_bytes, unsigned num_bodies, double softening_sq, nb_stream_t stream) {
    return init<double>(accelerations, jerks, snaps, crackles, positions, velocities, workspace, workspace_bytes, num_bodies, softening_sq, stream);
}

int nb_hermite6_step_f32(float* new_positions, const float* old_positions, float* velocities, float* accelerations, float* jerks, float* snaps, float* crackles,
                         void* workspace, size_t workspace_bytes, unsigned num_bodies, float delta_time, float softening_sq, nb_stream_t stream) {
    return step<float>(new_positions, old_positions, velocities, accelerations, jerks, snaps, crackles, workspace, workspace_bytes, num_bodies, delta_time, softening_sq, stream);
}
int nb_hermite6_step_f64(double* new_positions, const double* old_positions, double* velocities, double* accelerations, double* jerks, double* snaps, double* crackles,
                         void* workspace, size_t workspace_bytes, unsigned num_bodies, double delta_time, double softening_sq, nb_stream_t stream) {
    return step<double>(new_positions, old_positions, velocities, accelerations, jerks, snaps, crackles, workspace, workspace_bytes, num_bodies, delta_time, softening_sq, stream);
}

int nb_hermite6_timestep_f32(const float* accelerations, const float* jerks, const float* snaps, const float* crackles, unsigned num_bodies, float eta, float* dt_out,
                             void* scratch, size_t scratch_bytes, nb_stream_t stream) {
    return timestep<float>(accelerations, jerks, snaps, crackles, num_bodies, eta, dt_out, scratch, scratch_bytes, stream);
}
int nb_hermite6_timestep_f64(const double* accelerations, const double* jerks, const double* snaps, const double* crackles, unsigned num_bodies, double eta, double* dt_out,
                             void* scratch, size_t scratch_bytes, nb_stream_t stream) {
    return timestep<double>(accelerations, jerks, snaps, crackles, num_bodies, eta, dt_out, scratch, scratch_bytes, stream);
}

}  // extern "C"
