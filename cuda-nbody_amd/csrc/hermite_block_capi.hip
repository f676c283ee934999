// hermite_block_capi.hip -- the extern "C" boundary of libnbody_hip_hermite_block.so (include/nbody_hip_hermite_block.h): the entry
// points of hermite_block_boundary.h's one text at order 4, where a body has no snap and no crackle.  (The static_asserts that hold the
// public header against the kernels are in that header: all four block-step boundaries share them.)
#include "../../include/nbody_hip_hermite_block.h"
#include "hermite_block_boundary.h"

extern "C" {

int nb_hermite_block_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes) { return nb::block::workspace_bytes<4>(num_bodies, sizeof_T, bytes); }

#define NB_HERMITE_BLOCK_ENTRY_POINTS(T, SUFFIX)                                                                                                                            \
    int nb_hermite_block_plan_##SUFFIX(unsigned num_bodies, unsigned num_active, nb_hermite_block_plan_t* plan) {                                                           \
        return nb::block::plan_query<T, 4>(num_bodies, num_active, plan);                                                                                                   \
    }                                                                                                                                                                       \
    int nb_hermite_block_init_##SUFFIX(T* positions, T* velocities, T* accelerations, T* jerks, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status,        \
                                       void* workspace, size_t workspace_bytes, unsigned num_bodies, T softening_sq, const nb_hermite_block_params_t* params,               \
                                       nb_stream_t stream) {                                                                                                                \
        return nb::block::init<T, 4>(positions, velocities, accelerations, jerks, nullptr, nullptr, ticks, levels, status, workspace, workspace_bytes, num_bodies,          \
                                     softening_sq, params, stream);                                                                                                         \
    }                                                                                                                                                                       \
    int nb_hermite_block_step_##SUFFIX(T* positions, T* velocities, T* accelerations, T* jerks, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status,        \
                                       void* workspace, size_t workspace_bytes, unsigned num_bodies, T softening_sq, const nb_hermite_block_params_t* params,               \
                                       double t_stop, nb_stream_t stream) {                                                                                                 \
        return nb::block::step<T, 4>(positions, velocities, accelerations, jerks, nullptr, nullptr, ticks, levels, status, workspace, workspace_bytes, num_bodies,          \
                                     softening_sq, params, t_stop, stream);                                                                                                 \
    }                                                                                                                                                                       \
    int nb_hermite_block_sync_##SUFFIX(T* positions_out, T* velocities_out, const T* positions, const T* velocities, const T* accelerations, const T* jerks,                \
                                       const uint64_t* ticks, const nb_hermite_block_status_t* status, unsigned num_bodies, const nb_hermite_block_params_t* params,        \
                                       nb_stream_t stream) {                                                                                                                \
        return nb::block::sync<T, 4>(positions_out, velocities_out, positions, velocities, accelerations, jerks, nullptr, nullptr, ticks, status, num_bodies, params,       \
                                     stream);                                                                                                                               \
    }
NB_HERMITE_BLOCK_ENTRY_POINTS(float, f32)
NB_HERMITE_BLOCK_ENTRY_POINTS(double, f64)
#undef NB_HERMITE_BLOCK_ENTRY_POINTS

}  // extern "C"
