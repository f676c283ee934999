// hermite_capi.hip -- the extern "C" boundary of libnbody_hip_hermite.so (include/nbody_hip_hermite.h).  Every argument is checked
// on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never synchronises.
#include "../../include/nbody_hip_hermite.h"
#include "capi_check.h"
#include "hermite_kernels.h"
#include "softening_floor.h"

namespace {

using nb::floored, nb::in_place_or_apart, nb::Span, nb::spans_ok;

static_assert(NB_HERMITE_MAX_BODIES == nb::kHermiteMaxBodies, "the header's limit is the kernels'");
static_assert(NB_HERMITE_TIMESTEP_SCRATCH_BYTES == nb::kTimestepPartials * sizeof(double), "the header's scratch size is the kernels'");

bool size_ok(unsigned n) { return n >= 1 && n <= nb::kHermiteMaxBodies; }

template <typename T> int plan_query(unsigned n, nb_hermite_plan_t* out) {
    if (out == nullptr || !size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    const nb::HermitePlan p = nb::plan_hermite<T>(n);
    out->bodies_per_lane  = p.bodies_per_lane;
    out->waves_per_group  = p.waves;
    out->unroll           = p.unroll;
    out->groups           = p.groups;
    out->block_threads    = p.block_threads;
    out->lds_bytes        = p.lds_bytes;
    return 0;
}

template <typename T> int eval(T* acc, T* jerk, const T* pos, const T* vel, unsigned n, T eps2, nb_stream_t stream) {
    if (!size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{acc, bodies, al}, {jerk, bodies, al}, {pos, bodies, al}, {vel, bodies, al}})) return NB_ERR_INVALID_ARGUMENT;
    nb::HermiteArgs<T> a{};
    a.pos = pos, a.vel_in = vel, a.acc = acc, a.jerk = jerk, a.n = n, a.eps2 = floored(eps2);
    return static_cast<int>(nb::launch_hermite_eval<T>(a, static_cast<hipStream_t>(stream)));
}

template <typename T>
int step(T* new_pos, const T* old_pos, T* vel, T* acc, T* jerk, void* workspace, size_t workspace_bytes, unsigned n, T dt, T eps2, nb_stream_t stream) {
    if (!size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (workspace_bytes < 2 * bodies) return NB_ERR_INVALID_ARGUMENT;
    // new_positions: old_positions itself, or an array apart from everything
    if (!in_place_or_apart({new_pos, bodies, al}, old_pos, {{old_pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {workspace, 2 * bodies, al}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    nb::HermiteArgs<T> a{};
    a.state8 = static_cast<const T*>(workspace);
    a.new_pos = new_pos, a.old_pos = old_pos, a.vel = vel, a.acc = acc, a.jerk = jerk, a.n = n, a.dt = dt, a.eps2 = floored(eps2);
    return static_cast<int>(nb::launch_hermite_step<T>(a, static_cast<T*>(workspace), static_cast<hipStream_t>(stream)));
}

template <typename T> int timestep(const T* acc, const T* jerk, unsigned n, T eta, T* dt_out, void* scratch, size_t scratch_bytes, nb_stream_t stream) {
    if (!size_ok(n) || scratch_bytes < NB_HERMITE_TIMESTEP_SCRATCH_BYTES) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{acc, bodies, al}, {jerk, bodies, al}, {dt_out, sizeof(T), sizeof(T)}, {scratch, NB_HERMITE_TIMESTEP_SCRATCH_BYTES, 8}})) return NB_ERR_INVALID_ARGUMENT;
    return static_cast<int>(nb::launch_hermite_timestep<T>(acc, jerk, n, eta, dt_out, static_cast<double*>(scratch), static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nb_hermite_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !size_ok(num_bodies) || !nb::element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = static_cast<size_t>(num_bodies) * 8 * sizeof_T;
    return 0;
}

int nb_hermite_plan_f32(unsigned num_bodies, nb_hermite_plan_t* plan) { return plan_query<float>(num_bodies, plan); }
int nb_hermite_plan_f64(unsigned num_bodies, nb_hermite_plan_t* plan) { return plan_query<double>(num_bodies, plan); }

int nb_hermite_eval_f32(float* accelerations, float* jerks, const float* positions, const float* velocities, unsigned num_bodies, float softening_sq, nb_stream_t stream) {
    return eval<float>(accelerations, jerks, positions, velocities, num_bodies, softening_sq, stream);
}
int nb_hermite_eval_f64(double* accelerations, double* jerks, const double* positions, const double* velocities, unsigned num_bodies, double softening_sq, nb_stream_t stream) {
    return eval<double>(accelerations, jerks, positions, velocities, num_bodies, softening_sq, stream);
}

int nb_hermite_step_f32(float* new_positions, const float* old_positions, float* velocities, float* accelerations, float* jerks, void* workspace, size_t workspace_bytes,
                        unsigned num_bodies, float delta_time, float softening_sq, nb_stream_t stream) {
    return step<float>(new_positions, old_positions, velocities, accelerations, jerks, workspace, workspace_bytes, num_bodies, delta_time, softening_sq, stream);
}
int nb_hermite_step_f64(double* new_positions, const double* old_positions, double* velocities, double* accelerations, double* jerks, void* workspace, size_t workspace_bytes,
                        unsigned num_bodies, double delta_time, double softening_sq, nb_stream_t stream) {
    return step<double>(new_positions, old_positions, velocities, accelerations, jerks, workspace, workspace_bytes, num_bodies, delta_time, softening_sq, stream);
}

int nb_hermite_timestep_f32(const float* accelerations, const float* jerks, unsigned num_bodies, float eta, float* dt_out, void* scratch, size_t scratch_bytes, nb_stream_t stream) {
    return timestep<float>(accelerations, jerks, num_bodies, eta, dt_out, scratch, scratch_bytes, stream);
}
int nb_hermite_timestep_f64(const double* accelerations, const double* jerks, unsigned num_bodies, double eta, double* dt_out, void* scratch, size_t scratch_bytes, nb_stream_t stream) {
    return timestep<double>(accelerations, jerks, num_bodies, eta, dt_out, scratch, scratch_bytes, stream);
}

}  // extern "C"
