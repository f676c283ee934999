// ensemble_capi.hip -- the extern "C" boundary of libnbody_hip_ensemble.so (include/nbody_hip_ensemble.h).  Every argument is
// checked on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never synchronises.
#include "../../include/nbody_hip_ensemble.h"
#include "ensemble_kernels.h"

#include <cstdint>

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
    if (!new_pos || !old_pos || !vel || !sizes_ok(n, b)) return NB_ERR_INVALID_ARGUMENT;
    if (mode != NB_MODE_STRICT && mode != NB_MODE_FAST) return NB_ERR_INVALID_ARGUMENT;
    const auto addr    = [](const void* p) { return reinterpret_cast<std::uintptr_t>(p); };
    const auto aligned = [&](const void* p) { return addr(p) % (4 * sizeof(T)) == 0; };
    if (!aligned(new_pos) || !aligned(old_pos) || !aligned(vel) || (params && !aligned(params))) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t bodies = static_cast<std::uintptr_t>(n) * b * 4 * sizeof(T);
    const auto overlap = [&](const void* x, std::uintptr_t x_len, const void* y, std::uintptr_t y_len) { return addr(x) < addr(y) + y_len && addr(y) < addr(x) + x_len; };
    if (overlap(new_pos, bodies, old_pos, bodies) || overlap(new_pos, bodies, vel, bodies) || overlap(vel, bodies, old_pos, bodies)) return NB_ERR_INVALID_ARGUMENT;
    if (params) {
        const std::uintptr_t param_bytes = static_cast<std::uintptr_t>(b) * 4 * sizeof(T);
        for (const void* body_array : {static_cast<const void*>(new_pos), static_cast<const void*>(old_pos), static_cast<const void*>(vel)}) {
            if (overlap(params, param_bytes, body_array, bodies)) return NB_ERR_INVALID_ARGUMENT;
        }
    }
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
