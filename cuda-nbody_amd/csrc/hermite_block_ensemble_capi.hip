// hermite_block_ensemble_capi.hip -- the extern "C" boundary of libnbody_hip_hermite_block_ensemble.so
// (include/nbody_hip_hermite_block_ensemble.h): the entry points of hermite_block_ensemble_boundary.h's one text at order 4, where a body
// has no snap and no crackle.  (The static_asserts that hold the public header against the kernels are in that header: both orders share
// them.)
#include "../../include/nbody_hip_hermite_block_ensemble.h"
#include "hermite_block_ensemble_boundary.h"

extern "C" {

int nb_hermite_block_ensemble_workspace_bytes(unsigned num_bodies, unsigned num_systems, unsigned sizeof_T, size_t* bytes) {
    return nb::block_ensemble::workspace_bytes<4>(num_bodies, num_systems, sizeof_T, bytes);
}

int nb_hermite_block_ensemble_summary(const nb_hermite_block_status_t* status, unsigned num_systems, nb_hermite_block_ensemble_summary_t* summary, nb_stream_t stream) {
    return nb::block_ensemble::summary<4>(status, num_systems, summary, stream);
}

#define NB_HERMITE_BLOCK_ENSEMBLE_ENTRY_POINTS(T, SUFFIX)                                                                                                                   \
    int nb_hermite_block_ensemble_plan_##SUFFIX(unsigned num_bodies, unsigned num_systems, unsigned num_active, nb_hermite_block_ensemble_plan_t* plan) {                   \
        return nb::block_ensemble::plan_query<T, 4>(num_bodies, num_systems, num_active, plan);                                                                             \
    }                                                                                                                                                                       \
    int nb_hermite_block_ensemble_init_##SUFFIX(T* positions, T* velocities, T* accelerations, T* jerks, uint64_t* ticks, int32_t* levels,                                  \
                                                nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems,      \
                                                T softening_sq, const T* system_softening_sq, const nb_hermite_block_params_t* params, nb_stream_t stream) {                \
        return nb::block_ensemble::init<T, 4>(positions, velocities, accelerations, jerks, nullptr, nullptr, ticks, levels, status, workspace, workspace_bytes, num_bodies, \
                                              num_systems, softening_sq, system_softening_sq, params, stream);                                                              \
    }                                                                                                                                                                       \
    int nb_hermite_block_ensemble_step_##SUFFIX(T* positions, T* velocities, T* accelerations, T* jerks, uint64_t* ticks, int32_t* levels,                                  \
                                                nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems,      \
                                                T softening_sq, const T* system_softening_sq, const nb_hermite_block_params_t* params, double t_stop,                       \
                                                nb_stream_t stream) {                                                                                                       \
        return nb::block_ensemble::step<T, 4>(positions, velocities, accelerations, jerks, nullptr, nullptr, ticks, levels, status, workspace, workspace_bytes, num_bodies, \
                                              num_systems, softening_sq, system_softening_sq, params, t_stop, stream);                                                      \
    }                                                                                                                                                                       \
    int nb_hermite_block_ensemble_sync_##SUFFIX(T* positions_out, T* velocities_out, const T* positions, const T* velocities, const T* accelerations, const T* jerks,       \
                                                const uint64_t* ticks, const nb_hermite_block_status_t* status, unsigned num_bodies, unsigned num_systems,                  \
                                                const nb_hermite_block_params_t* params, nb_stream_t stream) {                                                              \
        return nb::block_ensemble::sync<T, 4>(positions_out, velocities_out, positions, velocities, accelerations, jerks, nullptr, nullptr, ticks, status, num_bodies,      \
                                              num_systems, params, stream);                                                                                                 \
    }
NB_HERMITE_BLOCK_ENSEMBLE_ENTRY_POINTS(float, f32)
NB_HERMITE_BLOCK_ENSEMBLE_ENTRY_POINTS(double, f64)
#undef NB_HERMITE_BLOCK_ENSEMBLE_ENTRY_POINTS

}  // extern "C"
