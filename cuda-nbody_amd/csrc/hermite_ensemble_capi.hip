// hermite_ensemble_capi.hip -- the extern "C" boundary of libnbody_hip_hermite_ensemble.so (include/nbody_hip_hermite_ensemble.h): the
// entry points of hermite_ensemble_boundary.h's one text at order 4, where a body has no snap and no crackle and the evaluation needs no
// workspace.  (The static_asserts that hold the public header against the kernels are in that header: both orders share them.)
#include "../../include/nbody_hip_hermite_ensemble.h"
#include "hermite_ensemble_boundary.h"

extern "C" {

int nb_hermite_ensemble_workspace_bytes(unsigned num_bodies, unsigned num_systems, unsigned sizeof_T, size_t* bytes) {
    return nb::ensemble::workspace_bytes<4>(num_bodies, num_systems, sizeof_T, bytes);
}

#define NB_HERMITE_ENSEMBLE_ENTRY_POINTS(T, SUFFIX)                                                                                                                         \
    int nb_hermite_ensemble_plan_##SUFFIX(unsigned num_bodies, unsigned num_systems, nb_hermite_ensemble_plan_t* plan) {                                                    \
        return nb::ensemble::plan_query<T, 4>(num_bodies, num_systems, plan);                                                                                               \
    }                                                                                                                                                                       \
    int nb_hermite_ensemble_eval_##SUFFIX(T* accelerations, T* jerks, const T* positions, const T* velocities, unsigned num_bodies, unsigned num_systems, T softening_sq,   \
                                          const T* system_softening_sq, nb_stream_t stream) {                                                                               \
        return nb::ensemble::eval<T, 4>(accelerations, jerks, nullptr, positions, velocities, nullptr, nullptr, 0, num_bodies, num_systems, softening_sq,                   \
                                        system_softening_sq, stream);                                                                                                       \
    }                                                                                                                                                                       \
    int nb_hermite_ensemble_step_##SUFFIX(T* new_positions, const T* old_positions, T* velocities, T* accelerations, T* jerks, void* workspace, size_t workspace_bytes,     \
                                          unsigned num_bodies, unsigned num_systems, T delta_time, T softening_sq, const T* system_params, nb_stream_t stream) {            \
        return nb::ensemble::step<T, 4>(new_positions, old_positions, velocities, accelerations, jerks, nullptr, nullptr, workspace, workspace_bytes, num_bodies,           \
                                        num_systems, delta_time, softening_sq, system_params, stream);                                                                      \
    }                                                                                                                                                                       \
    int nb_hermite_ensemble_timestep_##SUFFIX(const T* accelerations, const T* jerks, unsigned num_bodies, unsigned num_systems, T eta, T* dt_out, void* workspace,         \
                                              size_t workspace_bytes, nb_stream_t stream) {                                                                                 \
        return nb::ensemble::timestep<T, 4>(accelerations, jerks, nullptr, nullptr, num_bodies, num_systems, eta, dt_out, workspace, workspace_bytes, stream);              \
    }                                                                                                                                                                       \
    int nb_hermite_ensemble_begin_##SUFFIX(T* accelerations, T* jerks, const T* positions, const T* velocities, nb_hermite_ensemble_clock_t* clocks, unsigned num_bodies,   \
                                           unsigned num_systems, T softening_sq, const T* system_softening_sq, T eta, void* workspace, size_t workspace_bytes,              \
                                           nb_stream_t stream) {                                                                                                            \
        return nb::ensemble::begin<T, 4>(accelerations, jerks, nullptr, nullptr, positions, velocities, clocks, num_bodies, num_systems, softening_sq, system_softening_sq, \
                                         eta, workspace, workspace_bytes, stream);                                                                                          \
    }                                                                                                                                                                       \
    int nb_hermite_ensemble_advance_##SUFFIX(T* new_positions, const T* old_positions, T* velocities, T* accelerations, T* jerks, nb_hermite_ensemble_clock_t* clocks,      \
                                             nb_hermite_ensemble_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems,      \
                                             double t_stop, double dt_max, T eta, T softening_sq, const T* system_softening_sq, nb_stream_t stream) {                       \
        return nb::ensemble::advance<T, 4>(new_positions, old_positions, velocities, accelerations, jerks, nullptr, nullptr, clocks, status, workspace, workspace_bytes,    \
                                           num_bodies, num_systems, t_stop, dt_max, eta, softening_sq, system_softening_sq, stream);                                        \
    }
NB_HERMITE_ENSEMBLE_ENTRY_POINTS(float, f32)
NB_HERMITE_ENSEMBLE_ENTRY_POINTS(double, f64)
#undef NB_HERMITE_ENSEMBLE_ENTRY_POINTS

}  // extern "C"
