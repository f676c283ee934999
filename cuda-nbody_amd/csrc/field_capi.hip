// field_capi.hip -- the extern "C" boundary of libnbody_hip_field.so (include/nbody_hip_field.h).  Every argument is checked on the
// host before the first HIP call; a call then launches, allocates nothing, takes no lock and never synchronises.
#include "../../include/nbody_hip_field.h"
#include "capi_check.h"
#include "field_kernels.h"
#include "softening_floor.h"

namespace {

using nb::floored, nb::Span, nb::spans_ok;

static_assert(NB_FIELD_MAX_SOURCES == nb::kFieldMaxSources, "the header's limit is the kernels'");
static_assert(NB_FIELD_MAX_TARGETS == nb::kFieldMaxTargets, "the header's limit is the kernels'");
static_assert(NB_FIELD_NONE == nb::kFieldNone, "the header's `none` is the kernels'");

bool sizes_ok(unsigned n, unsigned m) { return n >= 1 && n <= nb::kFieldMaxSources && m >= 1 && m <= nb::kFieldMaxTargets; }

template <typename T> int plan_query(unsigned n, unsigned m, nb_field_plan_t* out) {
    if (out == nullptr || !sizes_ok(n, m)) return NB_ERR_INVALID_ARGUMENT;
    constexpr unsigned    per_tile = sizeof(T) == 4 ? 128 : 64;
    const nb::FieldGeom   g        = nb::field_geometry(n, m, per_tile);
    const nb::FieldLayout l        = nb::field_layout(n, m, sizeof(T));
    out->bodies_per_lane           = per_tile / 64;
    out->waves_per_group           = static_cast<int>(g.waves);
    out->unroll                    = sizeof(T) == 4 ? 4 : 2;
    out->tiles                     = g.tiles;
    out->ranges                    = g.ranges;
    out->groups                    = g.tiles * g.ranges;
    out->block_threads             = 64 * g.waves;
    out->lds_bytes                 = static_cast<unsigned>((g.waves > 1 ? g.waves - 1 : 1) * 7 * per_tile * sizeof(T));
    out->launches                  = g.ranges > 1 ? 2 : 1;
    out->reserved                  = 0;
    out->partial_offset            = l.partial;
    out->partial_bytes             = l.partial_bytes;
    return 0;
}

template <typename T>
int eval(const T* src, const T* src_vel, unsigned n, const T* tgt, const T* tgt_vel, const unsigned* self, unsigned m, T eps2, T* acc, T* jerk, T* pot, void* workspace,
         size_t workspace_bytes, nb_stream_t stream) {
    if (!sizes_ok(n, m) || src == nullptr || tgt == nullptr || !(eps2 >= T(0))) return NB_ERR_INVALID_ARGUMENT;  // (NaN compares false)
    if (acc == nullptr && jerk == nullptr && pot == nullptr) return NB_ERR_INVALID_ARGUMENT;
    if (jerk != nullptr && (src_vel == nullptr || tgt_vel == nullptr)) return NB_ERR_INVALID_ARGUMENT;
    const nb::FieldLayout l = nb::field_layout(n, m, sizeof(T));
    if (workspace_bytes < l.bytes || (l.bytes > 0 && workspace == nullptr)) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t N = n, M = m, V = 4 * sizeof(T);
    // what the call writes, apart from each other and from what it reads; the inputs may alias each other
    if (!spans_ok({{acc, M * V, V, Span::optional}, {jerk, M * V, V, Span::optional}, {pot, M * sizeof(T), sizeof(T), Span::optional}, {workspace, l.bytes, 32, Span::optional}},
                  {{src, N * V, V}, {src_vel, N * V, V, Span::optional}, {tgt, M * V, V}, {tgt_vel, M * V, V, Span::optional}, {self, M * 4, 4, Span::optional}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    nb::FieldArgs<T> a{};
    a.src = src, a.src_vel = src_vel, a.tgt = tgt, a.tgt_vel = tgt_vel, a.self = self;
    a.acc = acc, a.jerk = jerk, a.pot = pot;
    a.partial = l.bytes > 0 ? reinterpret_cast<T*>(static_cast<char*>(workspace) + l.partial) : nullptr;
    a.n = n, a.m = m, a.eps2 = floored(eps2);
    return static_cast<int>(nb::launch_field_eval<T>(a, static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nb_field_workspace_bytes(unsigned num_sources, unsigned num_targets, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !sizes_ok(num_sources, num_targets) || !nb::element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = nb::field_layout(num_sources, num_targets, sizeof_T).bytes;
    return 0;
}

int nb_field_plan_f32(unsigned num_sources, unsigned num_targets, nb_field_plan_t* plan) { return plan_query<float>(num_sources, num_targets, plan); }
int nb_field_plan_f64(unsigned num_sources, unsigned num_targets, nb_field_plan_t* plan) { return plan_query<double>(num_sources, num_targets, plan); }

int nb_field_eval_f32(const float* sources, const float* source_velocities, unsigned num_sources, const float* targets, const float* target_velocities,
                      const unsigned* self_index, unsigned num_targets, float softening_sq, float* accelerations, float* jerks, float* potentials, void* workspace,
                      size_t workspace_bytes, nb_stream_t stream) {
    return eval<float>(sources, source_velocities, num_sources, targets, target_velocities, self_index, num_targets, softening_sq, accelerations, jerks, potentials, workspace,
                       workspace_bytes, stream);
}
int nb_field_eval_f64(const double* sources, const double* source_velocities, unsigned num_sources, const double* targets, const double* target_velocities,
                      const unsigned* self_index, unsigned num_targets, double softening_sq, double* accelerations, double* jerks, double* potentials, void* workspace,
                      size_t workspace_bytes, nb_stream_t stream) {
    return eval<double>(sources, source_velocities, num_sources, targets, target_velocities, self_index, num_targets, softening_sq, accelerations, jerks, potentials, workspace,
                        workspace_bytes, stream);
}

}  // extern "C"
