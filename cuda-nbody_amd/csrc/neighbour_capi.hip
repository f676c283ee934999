// neighbour_capi.hip -- the extern "C" boundary of libnbody_hip_neighbour.so (include/nbody_hip_neighbour.h).  Every argument is checked
// on the host before the first HIP call; a call then launches, allocates nothing, takes no lock and never synchronises.
#include "../../include/nbody_hip_neighbour.h"
#include "capi_check.h"
#include "neighbour_kernels.h"

#include <cmath>

namespace {

using nb::Span, nb::spans_ok;

static_assert(NB_NEIGHBOUR_MAX_BODIES == nb::kNeighbourMaxBodies, "the header's limit is the kernels'");
static_assert(NB_NEIGHBOUR_NONE == nb::kNeighbourNone, "the header's `none` is the kernels'");
static_assert(NB_NEIGHBOUR_OVERFLOW == nb::kNeighbourOverflow, "the header's flag is the kernels'");
static_assert(sizeof(nb_neighbour_status_t) == 64 && sizeof(nb::NeighbourStatus) == 64, "the status record is 64 bytes");
static_assert(sizeof(nb::NeighbourCtrl) == 64, "the control record is 64 bytes");
static_assert(sizeof(nb::NeighbourTile) == 32, "a tile's record is 32 bytes");

bool size_ok(unsigned n) { return n >= 1 && n <= nb::kNeighbourMaxBodies; }

template <typename T> bool scalars_ok(T radius_sq, const T* radii, T eps2) {
    if (radii == nullptr && !(radius_sq >= T(0))) return false;  // (NaN compares false)
    return eps2 >= T(0);
}

template <typename T> void bind_workspace(nb::NeighbourArgs<T>& a, void* workspace, const nb::NeighbourLayout& l) {
    char* const ws = static_cast<char*>(workspace);
    a.planes       = reinterpret_cast<unsigned*>(ws + l.planes);
    a.block_sums   = reinterpret_cast<unsigned long long*>(ws + l.block_sums);
    a.tiles        = reinterpret_cast<nb::NeighbourTile*>(ws + l.tiles);
    a.ctrl         = reinterpret_cast<nb::NeighbourCtrl*>(ws + l.ctrl);
}

template <typename T> int plan_query(unsigned n, nb_neighbour_plan_t* out) {
    if (out == nullptr || !size_ok(n)) return NB_ERR_INVALID_ARGUMENT;
    constexpr unsigned per_tile = sizeof(T) == 4 ? 128 : 64;
    const unsigned     S        = nb::neighbour_waves(n);
    out->bodies_per_lane        = per_tile / 64;
    out->waves_per_group        = static_cast<int>(S);
    out->unroll                 = sizeof(T) == 4 ? 4 : 2;
    out->tiles                  = nb::neighbour_tiles(n, per_tile);
    out->block_threads          = 64 * S;
    out->lds_bytes              = S > 1 ? static_cast<unsigned>((S - 1) * 2 * per_tile * (sizeof(T) + 4)) : 0u;
    out->chunks                 = nb::neighbour_chunks(n);
    out->list_ranges            = nb::neighbour_ranges(n, per_tile);
    out->list_groups            = out->tiles * out->list_ranges;
    out->survey_launches        = 2;
    out->list_launches          = 5;
    out->reserved               = 0;
    out->planes_offset          = nb::neighbour_layout(n, sizeof(T)).planes;
    out->planes_bytes           = static_cast<unsigned long long>(out->list_ranges) * n * 4;
    return 0;
}

template <typename T>
int survey(const T* pos, unsigned n, T radius_sq, const T* radii, T eps2, unsigned* nearest, T* nearest_d2, unsigned* counts, T* potentials, nb_neighbour_status_t* status,
           void* workspace, size_t workspace_bytes, nb_stream_t stream) {
    if (!size_ok(n) || pos == nullptr || status == nullptr || workspace == nullptr || !scalars_ok(radius_sq, radii, eps2)) return NB_ERR_INVALID_ARGUMENT;
    if (nearest == nullptr && nearest_d2 == nullptr && counts == nullptr && potentials == nullptr) return NB_ERR_INVALID_ARGUMENT;
    const nb::NeighbourLayout l = nb::neighbour_layout(n, sizeof(T));
    if (workspace_bytes < l.bytes) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t N = n;
    if (!spans_ok({{pos, N * 4 * sizeof(T), 4 * sizeof(T)}, {radii, N * sizeof(T), sizeof(T), Span::optional}, {nearest, N * 4, 4, Span::optional},
                   {nearest_d2, N * sizeof(T), sizeof(T), Span::optional}, {counts, N * 4, 4, Span::optional}, {potentials, N * sizeof(T), sizeof(T), Span::optional},
                   {status, 64, 8}, {workspace, l.bytes, 32}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    nb::NeighbourArgs<T> a{};
    a.pos = pos, a.radii = radii, a.radius_sq = radii != nullptr ? T(0) : radius_sq, a.eps2 = eps2, a.n = n;
    a.nearest = nearest, a.nearest_d2 = nearest_d2, a.counts = counts, a.potentials = potentials;
    a.status = reinterpret_cast<nb::NeighbourStatus*>(status);
    bind_workspace(a, workspace, l);
    return static_cast<int>(nb::launch_neighbour_survey<T>(a, static_cast<hipStream_t>(stream)));
}

template <typename T>
int lists(const T* pos, unsigned n, T radius_sq, const T* radii, unsigned long long* offsets, unsigned* indices, unsigned long long capacity, nb_neighbour_status_t* status,
          void* workspace, size_t workspace_bytes, nb_stream_t stream) {
    if (!size_ok(n) || pos == nullptr || status == nullptr || workspace == nullptr || offsets == nullptr || !scalars_ok(radius_sq, radii, T(0))) return NB_ERR_INVALID_ARGUMENT;
    if (indices == nullptr && capacity > 0) return NB_ERR_INVALID_ARGUMENT;
    if (capacity > (~0ull >> 3)) return NB_ERR_INVALID_ARGUMENT;  // (its bytes are an address range)
    const nb::NeighbourLayout l = nb::neighbour_layout(n, sizeof(T));
    if (workspace_bytes < l.bytes) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t N = n;
    if (!spans_ok({{pos, N * 4 * sizeof(T), 4 * sizeof(T)}, {radii, N * sizeof(T), sizeof(T), Span::optional}, {offsets, (N + 1) * 8, 8},
                   {capacity > 0 ? indices : nullptr, static_cast<std::uintptr_t>(capacity) * 4, 4, Span::optional}, {status, 64, 8}, {workspace, l.bytes, 32}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    nb::NeighbourArgs<T> a{};
    a.pos = pos, a.radii = radii, a.radius_sq = radii != nullptr ? T(0) : radius_sq, a.eps2 = T(0), a.n = n;
    a.offsets = offsets, a.indices = indices, a.capacity = capacity;
    a.status = reinterpret_cast<nb::NeighbourStatus*>(status);
    bind_workspace(a, workspace, l);
    return static_cast<int>(nb::launch_neighbour_lists<T>(a, static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nb_neighbour_workspace_bytes(unsigned num_bodies, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !size_ok(num_bodies) || !nb::element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = nb::neighbour_layout(num_bodies, sizeof_T).bytes;
    return 0;
}

int nb_neighbour_plan_f32(unsigned num_bodies, nb_neighbour_plan_t* plan) { return plan_query<float>(num_bodies, plan); }
int nb_neighbour_plan_f64(unsigned num_bodies, nb_neighbour_plan_t* plan) { return plan_query<double>(num_bodies, plan); }

int nb_neighbour_survey_f32(const float* positions, unsigned num_bodies, float radius_sq, const float* radii_sq, float softening_sq, unsigned* nearest_index,
                            float* nearest_dist_sq, unsigned* counts, float* potentials, nb_neighbour_status_t* status, void* workspace, size_t workspace_bytes,
                            nb_stream_t stream) {
    return survey<float>(positions, num_bodies, radius_sq, radii_sq, softening_sq, nearest_index, nearest_dist_sq, counts, potentials, status, workspace, workspace_bytes, stream);
}
int nb_neighbour_survey_f64(const double* positions, unsigned num_bodies, double radius_sq, const double* radii_sq, double softening_sq, unsigned* nearest_index,
                            double* nearest_dist_sq, unsigned* counts, double* potentials, nb_neighbour_status_t* status, void* workspace, size_t workspace_bytes,
                            nb_stream_t stream) {
    return survey<double>(positions, num_bodies, radius_sq, radii_sq, softening_sq, nearest_index, nearest_dist_sq, counts, potentials, status, workspace, workspace_bytes, stream);
}

int nb_neighbour_lists_f32(const float* positions, unsigned num_bodies, float radius_sq, const float* radii_sq, unsigned long long* offsets, unsigned* indices,
                           unsigned long long capacity, nb_neighbour_status_t* status, void* workspace, size_t workspace_bytes, nb_stream_t stream) {
    return lists<float>(positions, num_bodies, radius_sq, radii_sq, offsets, indices, capacity, status, workspace, workspace_bytes, stream);
}
int nb_neighbour_lists_f64(const double* positions, unsigned num_bodies, double radius_sq, const double* radii_sq, unsigned long long* offsets, unsigned* indices,
                           unsigned long long capacity, nb_neighbour_status_t* status, void* workspace, size_t workspace_bytes, nb_stream_t stream) {
    return lists<double>(positions, num_bodies, radius_sq, radii_sq, offsets, indices, capacity, status, workspace, workspace_bytes, stream);
}

}  // extern "C"
