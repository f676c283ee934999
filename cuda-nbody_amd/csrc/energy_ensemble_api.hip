// energy_ensemble_api.hip -- the extern "C" boundary of libnbody_hip_energy_ensemble.so (include/nbody_hip_energy_ensemble.h).  Every argument
// is checked on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never synchronises.
#include "../../include/nbody_hip_energy_ensemble.h"
#include "capi_check.h"
#include "energy_ensemble_kernels.h"

namespace {

using nb::Span, nb::spans_ok;

static_assert(sizeof(nb_energy_t) == 104, "the result is nb_energy_*'s");
static_assert(sizeof(nb_energy_ensemble_drift_t) == 64, "the drift record is 64 bytes");
static_assert(sizeof(nb_energy_ensemble_plan_t) == 32, "the plan");

constexpr std::uintptr_t kRecordBytes = 128;  // one fp64 record per workgroup

bool sizes_ok(unsigned n, unsigned b) {
    return n >= 1 && n <= nb::kEnsembleMaxBodies && b >= 1 && static_cast<unsigned long long>(n) * b <= nb::kEnsembleMaxTotal;
}

// for either precision: monotone in n and in b, at most 2 bytes per body and 1 KiB per system
size_t workspace_need(unsigned n, unsigned b) { return static_cast<size_t>(nb::energy_ensemble_records(n)) * b * kRecordBytes; }

template <typename T> int plan_query(unsigned n, unsigned b, nb_energy_ensemble_plan_t* out) {
    if (out == nullptr || !sizes_ok(n, b)) return NB_ERR_INVALID_ARGUMENT;
    const nb::EnergyEnsemblePlan p = nb::plan_energy_ensemble<T>(n);
    out->bodies_per_lane   = p.bodies_per_lane;
    out->waves_per_group   = p.waves;
    out->groups_per_system = p.groups;
    out->block_threads     = p.block_threads;
    out->lds_bytes         = p.lds_bytes;
    out->reserved          = 0;
    out->grid_blocks       = static_cast<unsigned long long>(p.groups) * b;
    return 0;
}

template <typename T>
int measure(const T* pos, const T* vel, unsigned n, unsigned b, T eps2, const T* system_eps2, unsigned stride, void* workspace, size_t workspace_bytes, nb_energy_t* results,
            nb_stream_t stream) {
    if (!sizes_ok(n, b) || stride < 1) return NB_ERR_INVALID_ARGUMENT;
    const size_t need = workspace_need(n, b);
    if (workspace_bytes < need) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t al = 4 * sizeof(T), bodies = static_cast<std::uintptr_t>(n) * b * al;
    if (static_cast<unsigned long long>(b - 1) * stride > (1ull << 58)) return NB_ERR_INVALID_ARGUMENT;  // (an array no address space holds)
    const std::uintptr_t softening = (static_cast<std::uintptr_t>(b - 1) * stride + 1) * sizeof(T);
    if (!spans_ok({{workspace, need, 8}, {results, static_cast<std::uintptr_t>(b) * sizeof(nb_energy_t), 8}, {system_eps2, softening, sizeof(T), Span::optional}},
                  {{pos, bodies, al}, {vel, bodies, al}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    nb::EnergyEnsembleArgs<T> a{};
    a.pos = pos, a.vel = vel, a.records = static_cast<double*>(workspace), a.results = results;
    a.system_eps2 = system_eps2, a.eps2_stride = stride, a.n = n, a.eps2 = eps2;
    return static_cast<int>(nb::launch_energy_ensemble<T>(a, b, nb::plan_energy_ensemble<T>(n), static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nb_energy_ensemble_plan_f32(unsigned num_bodies, unsigned num_systems, nb_energy_ensemble_plan_t* plan) { return plan_query<float>(num_bodies, num_systems, plan); }
int nb_energy_ensemble_plan_f64(unsigned num_bodies, unsigned num_systems, nb_energy_ensemble_plan_t* plan) { return plan_query<double>(num_bodies, num_systems, plan); }

int nb_energy_ensemble_workspace_bytes(unsigned num_bodies, unsigned num_systems, size_t* bytes) {
    if (bytes == nullptr || !sizes_ok(num_bodies, num_systems)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = workspace_need(num_bodies, num_systems);
    return 0;
}

int nb_energy_ensemble_f32(const float* positions, const float* velocities, unsigned num_bodies, unsigned num_systems, float softening_sq, const float* system_softening_sq,
                           unsigned softening_stride, void* workspace, size_t workspace_bytes, nb_energy_t* device_results, nb_stream_t stream) {
    return measure<float>(positions, velocities, num_bodies, num_systems, softening_sq, system_softening_sq, softening_stride, workspace, workspace_bytes, device_results, stream);
}
int nb_energy_ensemble_f64(const double* positions, const double* velocities, unsigned num_bodies, unsigned num_systems, double softening_sq, const double* system_softening_sq,
                           unsigned softening_stride, void* workspace, size_t workspace_bytes, nb_energy_t* device_results, nb_stream_t stream) {
    return measure<double>(positions, velocities, num_bodies, num_systems, softening_sq, system_softening_sq, softening_stride, workspace, workspace_bytes, device_results, stream);
}

int nb_energy_ensemble_drift(const nb_energy_t* start, const nb_energy_t* end, unsigned num_systems, nb_energy_ensemble_drift_t* device_summary, nb_stream_t stream) {
    if (num_systems < 1) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t results = static_cast<std::uintptr_t>(num_systems) * sizeof(nb_energy_t);
    if (!spans_ok({{device_summary, sizeof(nb_energy_ensemble_drift_t), 8}}, {{start, results, 8}, {end, results, 8}})) return NB_ERR_INVALID_ARGUMENT;
    return static_cast<int>(nb::launch_energy_ensemble_drift(start, end, num_systems, device_summary, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
