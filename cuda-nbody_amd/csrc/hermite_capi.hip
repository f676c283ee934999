// hermite_capi.hip -- the extern "C" boundary of libnbody_hip_hermite.so (include/nbody_hip_hermite.h): the entry points of
// hermite_boundary.h's one text at order 4, where a body has no snap and no crackle and the evaluation needs no workspace.
#include "../../include/nbody_hip_hermite.h"
#include "hermite_boundary.h"

static_assert(NB_HERMITE_MAX_BODIES == nb::kHermiteMaxBodies, "the header's limit is the kernels'");
static_assert(NB_HERMITE_TIMESTEP_SCRATCH_BYTES == nb::kTimestepPartials * sizeof(double), "the header's scratch size is the kernels'");

extern "C" {

int nb_hermite_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes) { return nb::solo::workspace_bytes<4>(num_bodies, sizeof_T, bytes); }

#define NB_HERMITE_ENTRY_POINTS(T, SUFFIX)                                                                                                                                  \
    int nb_hermite_plan_##SUFFIX(unsigned num_bodies, nb_hermite_plan_t* plan) { return nb::solo::plan_query<T, 4>(num_bodies, plan); }                                     \
    int nb_hermite_eval_##SUFFIX(T* accelerations, T* jerks, const T* positions, const T* velocities, unsigned num_bodies, T softening_sq, nb_stream_t stream) {            \
        return nb::solo::eval<T, 4>(accelerations, jerks, nullptr, positions, velocities, nullptr, nullptr, 0, num_bodies, softening_sq, stream);                           \
    }                                                                                                                                                                       \
    int nb_hermite_step_##SUFFIX(T* new_positions, const T* old_positions, T* velocities, T* accelerations, T* jerks, void* workspace, size_t workspace_bytes,              \
                                 unsigned num_bodies, T delta_time, T softening_sq, nb_stream_t stream) {                                                                   \
        return nb::solo::step<T, 4>(new_positions, old_positions, velocities, accelerations, jerks, nullptr, nullptr, workspace, workspace_bytes, num_bodies, delta_time,   \
                                    softening_sq, stream);                                                                                                                  \
    }                                                                                                                                                                       \
    int nb_hermite_timestep_##SUFFIX(const T* accelerations, const T* jerks, unsigned num_bodies, T eta, T* dt_out, void* scratch, size_t scratch_bytes,                    \
                                     nb_stream_t stream) {                                                                                                                  \
        return nb::solo::timestep<T, 4>(accelerations, jerks, nullptr, nullptr, num_bodies, eta, dt_out, scratch, scratch_bytes, stream);                                   \
    }
NB_HERMITE_ENTRY_POINTS(float, f32)
NB_HERMITE_ENTRY_POINTS(double, f64)
#undef NB_HERMITE_ENTRY_POINTS

}  // extern "C"
