// ensemble_capi.hip -- the extern "C" boundary of libnbody_hip_ensemble.so (include/nbody_hip_ensemble.h).  Every argument is
// checked on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never synchronises.
#include "../../include/nbody_hip_ensemble.h"
#include "capi_check.h"
#include "ensemble_kernels.h"

namespace {

bool sizes_ok(unsigned n, unsigned b) {
    return n >= 1 && n <= nb::kEnsembleMaxBodies && b >= 1 && static_cast<unsigned long long>(n) * b <= nb::kEnsembleMaxTotal;
}

template <typename T> int plan_query(unsigned n, unsigned b, nb_ensemble_plan_t* out) {
    if (out == nullptr || !sizes_ok(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const nb::EnsemblePlan p = nb::plan_ensemble_fast<T>(n);
    out->bodies_per_lane   = p.bodies_per_lane;
    out->waves_per_group   = p.waves;
    out->groups_per_system = p.groups;
    out->block_threads     = p.block_threads;
    out->lds_bytes         = p.lds_bytes;
    out->grid_blocks       = static_cast<unsigned long long>(p.groups) * b;
    return 0;
}

template <typename T>
int integrate(T* new_pos, const T* old_pos, T* vel, unsigned n, unsigned b, T dt, T damping, T eps2, const T* params, int mode, nb_stream_t stream) {
    if (!sizes_ok(n, b)) return NB_ERR_INVALID_ARGUMENT;
    if (mode != NB_MODE_STRICT && mode != NB_MODE_FAST) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T), bodies = static_cast<std::uintptr_t>(n) * b * al;
    if (!nb::spans_ok({{new_pos, bodies, al}, {old_pos, bodies, al}, {vel, bodies, al}, {params, b * al, al, nb::Span::optional}})) return NB_ERR_INVALID_ARGUMENT;
    nb::EnsembleArgs<T> a{};
    a.new_pos = new_pos, a.old_pos = old_pos, a.vel = vel, a.params = params;
    a.n = n, a.dt = dt, a.damping = damping, a.eps2 = eps2;
    const auto s = static_cast<hipStream_t>(stream);
    if (mode == NB_MODE_STRICT) return static_cast<int>(nb::launch_ensemble_strict<T>(a, b, s));
    return static_cast<int>(nb::launch_ensemble_fast<T>(a, b, nb::plan_ensemble_fast<T>(n), s));
}

}  // namespace

extern "C" {

int nb_ensemble_plan_f32(unsigned num_bodies, unsigned num_systems, nb_ensemble_plan_t* plan) { return plan_query<float>(num_bodies, num_systems, plan); }
int nb_ensemble_plan_f64(unsigned num_bodies, unsigned num_systems, nb_ensemble_plan_t* plan) { return plan_query<double>(num_bodies, num_systems, plan); }

int nb_ensemble_integrate_f32(float* new_positions, const float* old_positions, float* velocities, unsigned num_bodies, unsigned num_systems, float delta_time, float damping,
                              float softening_sq, const float* system_params, int mode, nb_stream_t stream) {
    return integrate<float>(new_positions, old_positions, velocities, num_bodies, num_systems, delta_time, damping, softening_sq, system_params, mode, stream);
}
int nb_ensemble_integrate_f64(double* new_positions, const double* old_positions, double* velocities, unsigned num_bodies, unsigned num_systems, double delta_time,
                              double damping, double softening_sq, const double* system_params, int mode, nb_stream_t stream) {
    return integrate<double>(new_positions, old_positions, velocities, num_bodies, num_systems, delta_time, damping, softening_sq, system_params, mode, stream);
}

}  // extern "C"
