// hermite6_capi.hip -- the extern "C" boundary of libnbody_hip_hermite6.so (include/nbody_hip_hermite6.h): the entry points of
// hermite_boundary.h's one text at order 6.
#include "../../include/nbody_hip_hermite6.h"
#include "hermite_boundary.h"

static_assert(NB_HERMITE6_MAX_BODIES == nb::kHermite6MaxBodies, "the header's limit is the kernels'");
static_assert(NB_HERMITE6_TIMESTEP_SCRATCH_BYTES == nb::kHermite6TimestepPartials * sizeof(double), "the header's scratch size is the kernels'");

extern "C" {

int nb_hermite6_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes) { return nb::solo::workspace_bytes<6>(num_bodies, sizeof_T, bytes); }

#define NB_HERMITE6_ENTRY_POINTS(T, SUFFIX)                                                                                                                                 \
    int nb_hermite6_plan_##SUFFIX(unsigned num_bodies, nb_hermite6_plan_t* plan) { return nb::solo::plan_query<T, 6>(num_bodies, plan); }                                   \
    int nb_hermite6_eval_##SUFFIX(T* acc_out, T* jerk_out, T* snap_out, const T* positions, const T* velocities, const T* acc_in, void* workspace, size_t workspace_bytes,  \
                                  unsigned num_bodies, T softening_sq, nb_stream_t stream) {                                                                                \
        return nb::solo::eval<T, 6>(acc_out, jerk_out, snap_out, positions, velocities, acc_in, workspace, workspace_bytes, num_bodies, softening_sq, stream);              \
    }                                                                                                                                                                       \
    int nb_hermite6_init_##SUFFIX(T* accelerations, T* jerks, T* snaps, T* crackles, const T* positions, const T* velocities, void* workspace, size_t workspace_bytes,      \
                                  unsigned num_bodies, T softening_sq, nb_stream_t stream) {                                                                                \
        return nb::solo::init<T>(accelerations, jerks, snaps, crackles, positions, velocities, workspace, workspace_bytes, num_bodies, softening_sq, stream);               \
    }                                                                                                                                                                       \
    int nb_hermite6_step_##SUFFIX(T* new_positions, const T* old_positions, T* velocities, T* accelerations, T* jerks, T* snaps, T* crackles, void* workspace,              \
                                  size_t workspace_bytes, unsigned num_bodies, T delta_time, T softening_sq, nb_stream_t stream) {                                          \
        return nb::solo::step<T, 6>(new_positions, old_positions, velocities, accelerations, jerks, snaps, crackles, workspace, workspace_bytes, num_bodies, delta_time,    \
                                    softening_sq, stream);                                                                                                                  \
    }                                                                                                                                                                       \
    int nb_hermite6_timestep_##SUFFIX(const T* accelerations, const T* jerks, const T* snaps, const T* crackles, unsigned num_bodies, T eta, T* dt_out, void* scratch,      \
                                      size_t scratch_bytes, nb_stream_t stream) {                                                                                           \
        return nb::solo::timestep<T, 6>(accelerations, jerks, snaps, crackles, num_bodies, eta, dt_out, scratch, scratch_bytes, stream);                                    \
    }
NB_HERMITE6_ENTRY_POINTS(float, f32)
NB_HERMITE6_ENTRY_POINTS(double, f64)
#undef NB_HERMITE6_ENTRY_POINTS

}  // extern "C"
