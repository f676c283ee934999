// hermite_block_ensemble_capi.hip -- the extern "C" boundary of libnbody_hip_hermite_block_ensemble.so
// (include/nbody_hip_hermite_block_ensemble.h).  Every argument is checked on the host before the first HIP call; a call then launches,
// allocates nothing, takes no lock and never synchronises.  The initial evaluation is hermite_ensemble.o's (linked in; that object
// exports nothing).
#include "../../include/nbody_hip_hermite_block_ensemble.h"
#include "capi_check.h"
#include "hermite_block_boundary.h"
#include "hermite_block_ensemble_kernels.h"
#include "hermite_ensemble_kernels.h"

namespace {

using nb::Span, nb::spans_ok;

static_assert(NB_HERMITE_BLOCK_ENSEMBLE_MAX_BODIES == nb::kBlockEnsembleMaxBodies && NB_HERMITE_BLOCK_ENSEMBLE_MAX_TOTAL == nb::kBlockEnsembleMaxTotal,
              "the header's limits are the kernels'");
static_assert(NB_HERMITE_BLOCK_ENSEMBLE_MAX_BODIES == nb::kEnsembleHermiteMaxBodies && NB_HERMITE_BLOCK_ENSEMBLE_MAX_TOTAL == nb::kEnsembleHermiteMaxTotal,
              "... and those of the ensemble evaluation init runs");
static_assert(nb::kBlockEnsembleMaxBodies <= 256 * nb::kBlockThreads, "a system's counts and partial minima: one per lane of a workgroup of 256");
static_assert(sizeof(nb_hermite_block_ensemble_summary_t) == 64 && sizeof(nb::BlockEnsembleSummary) == 64, "the summary record is 64 bytes");

nb::BlockEnsembleLayout layout(unsigned n, size_t size_t_of) { return nb::block_ensemble_layout(n, size_t_of, 2, nb::kBlockSums); }  // a predicted body is two vec4

// N, B and their products: every stage of every call is one launch
template <typename T> bool size_ok(unsigned n, unsigned b) {
    if (n < 1 || n > nb::kBlockEnsembleMaxBodies || b < 1 || static_cast<unsigned long long>(n) * b > nb::kBlockEnsembleMaxTotal) return false;
    constexpr unsigned       per_tile = sizeof(T) == 4 ? 128 : 64;
    const unsigned long long limit    = 1ull << 31;
    const unsigned long long eval     = static_cast<unsigned long long>(b) * nb::block_launch_groups(n, per_tile) * (64 * nb::block_waves(n));
    const unsigned long long schedule = static_cast<unsigned long long>(b) * nb::block_ensemble_blocks(n) * nb::kBlockThreads;
    const nb::EnsembleHermitePlan first = nb::plan_hermite_ensemble<T>(n, b);  // init's evaluation
    return eval <= limit && schedule <= limit && first.grid_blocks * first.block_threads <= limit;
}

template <typename T> int plan_query(unsigned n, unsigned b, unsigned n_active, nb_hermite_block_ensemble_plan_t* out) {
    if (out == nullptr || !size_ok<T>(n, b) || n_active < 1 || n_active > n) return NB_ERR_INVALID_ARGUMENT;
    const nb::BlockEnsembleLayout l = layout(n, sizeof(T));
    nb::block_plan_fill(out, n, n_active, sizeof(T), nb::kBlockSums, sizeof(T) == 4 ? 4 : 2);
    out->step_launches     = 5;
    out->partial_offset    = l.partial;
    out->groups_per_system = out->launch_groups;
    out->blocks_per_system = nb::block_ensemble_blocks(n);
    out->eval_grid         = static_cast<unsigned long long>(b) * out->groups_per_system;
    out->schedule_grid     = static_cast<unsigned long long>(b) * out->blocks_per_system;
    out->workspace_stride  = l.stride;
    return 0;
}

// the arrays of the B systems and the workspace, checked; fills `a`
template <typename T>
bool bind(nb::BlockEnsembleArgs<T>& a, T* pos, T* vel, T* acc, T* jerk, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes,
          unsigned n, unsigned b, T eps2, const T* system_eps2, const nb_hermite_block_params_t* params) {
    if (!size_ok<T>(n, b) || !nb::block_params_ok(params)) return false;
    const nb::BlockEnsembleLayout l     = layout(n, sizeof(T));
    const std::uintptr_t          total = static_cast<std::uintptr_t>(l.stride) * b;
    if (workspace_bytes < total) return false;
    const std::uintptr_t count = static_cast<std::uintptr_t>(n) * b, bodies = count * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {ticks, count * 8, 8}, {levels, count * 4, 4},
                   {status, static_cast<std::uintptr_t>(b) * 64, 8}, {workspace, total, 32}, {system_eps2, b * sizeof(T), sizeof(T), Span::optional}})) {
        return false;
    }
    a.pos = pos, a.vel = vel, a.acc = acc, a.jerk = jerk;
    a.ticks             = reinterpret_cast<unsigned long long*>(ticks);
    a.levels            = levels;
    a.status            = reinterpret_cast<nb::BlockStatus*>(status);
    a.workspace         = static_cast<char*>(workspace);
    a.layout            = l;
    a.system_eps2       = system_eps2;
    a.eps2              = eps2;
    a.n                 = n;
    a.b                 = b;
    a.blocks            = nb::block_ensemble_blocks(n);
    a.groups_per_system = nb::block_launch_groups(n, sizeof(T) == 4 ? 128 : 64);
    a.p                 = nb::block_params_of(params);
    a.t_stop            = 0;
    return true;
}

template <typename T>
int init(T* pos, T* vel, T* acc, T* jerk, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned n, unsigned b,
         T eps2, const T* system_eps2, const nb_hermite_block_params_t* params, nb_stream_t stream) {
    nb::BlockEnsembleArgs<T> a{};
    if (!bind(a, pos, vel, acc, jerk, ticks, levels, status, workspace, workspace_bytes, n, b, eps2, system_eps2, params)) return NB_ERR_INVALID_ARGUMENT;
    nb::EnsembleHermiteArgs<T> e{};
    e.pos = pos, e.vel_in = vel, e.acc = acc, e.jerk = jerk, e.n = n, e.src.eps2 = eps2, e.src.system_eps2 = system_eps2;
    if (const auto err = nb::launch_ensemble_eval<T>(e, b, static_cast<hipStream_t>(stream)); err != hipSuccess) return static_cast<int>(err);
    return static_cast<int>(nb::launch_block_ensemble_init<T>(a, static_cast<hipStream_t>(stream)));
}

template <typename T>
int step(T* pos, T* vel, T* acc, T* jerk, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned n, unsigned b,
         T eps2, const T* system_eps2, const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream) {
    nb::BlockEnsembleArgs<T> a{};
    if (std::isnan(t_stop)) return NB_ERR_INVALID_ARGUMENT;
    if (!bind(a, pos, vel, acc, jerk, ticks, levels, status, workspace, workspace_bytes, n, b, eps2, system_eps2, params)) return NB_ERR_INVALID_ARGUMENT;
    a.t_stop = t_stop;
    return static_cast<int>(nb::launch_block_ensemble_step<T>(a, static_cast<hipStream_t>(stream)));
}

template <typename T>
int sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const uint64_t* ticks, const nb_hermite_block_status_t* status, unsigned n, unsigned b,
         const nb_hermite_block_params_t* params, nb_stream_t stream) {
    if (!size_ok<T>(n, b) || !nb::block_params_ok(params)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t count = static_cast<std::uintptr_t>(n) * b, bodies = count * 4 * sizeof(T), al = 4 * sizeof(T);
    if (!spans_ok({{pos_out, bodies, al}, {vel_out, bodies, al}, {pos, bodies, al}, {vel, bodies, al}, {acc, bodies, al}, {jerk, bodies, al}, {ticks, count * 8, 8},
                   {status, static_cast<std::uintptr_t>(b) * 64, 8}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    return static_cast<int>(nb::launch_block_ensemble_sync<T>(pos_out, vel_out, pos, vel, acc, jerk, reinterpret_cast<const unsigned long long*>(ticks),
                                                              reinterpret_cast<const nb::BlockStatus*>(status), n, b, nb::block_params_of(params), static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nb_hermite_block_ensemble_workspace_bytes(unsigned num_bodies, unsigned num_systems, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !nb::element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    if (!(sizeof_T == 4 ? size_ok<float>(num_bodies, num_systems) : size_ok<double>(num_bodies, num_systems))) return NB_ERR_INVALID_ARGUMENT;
    *bytes = layout(num_bodies, sizeof_T).stride * num_systems;
    return 0;
}

int nb_hermite_block_ensemble_plan_f32(unsigned num_bodies, unsigned num_systems, unsigned num_active, nb_hermite_block_ensemble_plan_t* plan) {
    return plan_query<float>(num_bodies, num_systems, num_active, plan);
}
int nb_hermite_block_ensemble_plan_f64(unsigned num_bodies, unsigned num_systems, unsigned num_active, nb_hermite_block_ensemble_plan_t* plan) {
    return plan_query<double>(num_bodies, num_systems, num_active, plan);
}

int nb_hermite_block_ensemble_init_f32(float* positions, float* velocities, float* accelerations, float* jerks, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status,
                                       void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems, float softening_sq, const float* system_softening_sq,
                                       const nb_hermite_block_params_t* params, nb_stream_t stream) {
    return init<float>(positions, velocities, accelerations, jerks, ticks, levels, status, workspace, workspace_bytes, num_bodies, num_systems, softening_sq, system_softening_sq,
                       params, stream);
}
int nb_hermite_block_ensemble_init_f64(double* positions, double* velocities, double* accelerations, double* jerks, uint64_t* ticks, int32_t* levels,
                                       nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems, double softening_sq,
                                       const double* system_softening_sq, const nb_hermite_block_params_t* params, nb_stream_t stream) {
    return init<double>(positions, velocities, accelerations, jerks, ticks, levels, status, workspace, workspace_bytes, num_bodies, num_systems, softening_sq, system_softening_sq,
                        params, stream);
}

int nb_hermite_block_ensemble_step_f32(float* positions, float* velocities, float* accelerations, float* jerks, uint64_t* ticks, int32_t* levels, nb_hermite_block_status_t* status,
                                       void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems, float softening_sq, const float* system_softening_sq,
                                       const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream) {
    return step<float>(positions, velocities, accelerations, jerks, ticks, levels, status, workspace, workspace_bytes, num_bodies, num_systems, softening_sq, system_softening_sq,
                       params, t_stop, stream);
}
int nb_hermite_block_ensemble_step_f64(double* positions, double* velocities, double* accelerations, double* jerks, uint64_t* ticks, int32_t* levels,
                                       nb_hermite_block_status_t* status, void* workspace, size_t workspace_bytes, unsigned num_bodies, unsigned num_systems, double softening_sq,
                                       const double* system_softening_sq, const nb_hermite_block_params_t* params, double t_stop, nb_stream_t stream) {
    return step<double>(positions, velocities, accelerations, jerks, ticks, levels, status, workspace, workspace_bytes, num_bodies, num_systems, softening_sq, system_softening_sq,
                        params, t_stop, stream);
}

int nb_hermite_block_ensemble_sync_f32(float* positions_out, float* velocities_out, const float* positions, const float* velocities, const float* accelerations, const float* jerks,
                                       const uint64_t* ticks, const nb_hermite_block_status_t* status, unsigned num_bodies, unsigned num_systems,
                                       const nb_hermite_block_params_t* params, nb_stream_t stream) {
    return sync<float>(positions_out, velocities_out, positions, velocities, accelerations, jerks, ticks, status, num_bodies, num_systems, params, stream);
}
int nb_hermite_block_ensemble_sync_f64(double* positions_out, double* velocities_out, const double* positions, const double* velocities, const double* accelerations,
                                       const double* jerks, const uint64_t* ticks, const nb_hermite_block_status_t* status, unsigned num_bodies, unsigned num_systems,
                                       const nb_hermite_block_params_t* params, nb_stream_t stream) {
    return sync<double>(positions_out, velocities_out, positions, velocities, accelerations, jerks, ticks, status, num_bodies, num_systems, params, stream);
}

int nb_hermite_block_ensemble_summary(const nb_hermite_block_status_t* status, unsigned num_systems, nb_hermite_block_ensemble_summary_t* summary, nb_stream_t stream) {
    if (num_systems < 1 || num_systems > nb::kBlockEnsembleMaxTotal) return NB_ERR_INVALID_ARGUMENT;
    if (!spans_ok({{status, static_cast<std::uintptr_t>(num_systems) * 64, 8}, {summary, 64, 8}})) return NB_ERR_INVALID_ARGUMENT;
    return static_cast<int>(nb::launch_block_ensemble_summary(reinterpret_cast<const nb::BlockStatus*>(status), num_systems, reinterpret_cast<nb::BlockEnsembleSummary*>(summary),
                                                              static_cast<hipStream_t>(stream)));
}

}  // extern "C"
