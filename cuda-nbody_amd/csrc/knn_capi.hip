// knn_capi.hip -- the extern "C" boundary of libnbody_hip_knn.so (include/nbody_hip_knn.h).  Every argument is checked on the host before
// the first HIP call; a call then launches, allocates nothing, takes no lock and never synchronises.
#include "../../include/nbody_hip_knn.h"
#include "capi_check.h"
#include "knn_kernels.h"

namespace {

using nb::Span, nb::spans_ok;

static_assert(NB_NEIGHBOUR_MAX_BODIES == nb::kKnnMaxBodies, "the limit of the neighbour header is the kernels'");
static_assert(NB_NEIGHBOUR_NONE == nb::kKnnNone, "the header's `none` is the kernels'");
static_assert(NB_KNN_MAX_K == nb::kKnnMaxK, "the header's largest K is the kernels'");
static_assert(NB_KNN_DEGENERATE == nb::kKnnDegenerate && NB_KNN_NO_DENSITY == nb::kKnnNoDensity, "the header's flags are the kernels'");
static_assert(sizeof(nb_knn_structure_t) == 128 && sizeof(nb::KnnStructure) == 128, "the structure record is 128 bytes");
static_assert(sizeof(nb::KnnTile) == 72 && sizeof(nb::KnnRing) == 24, "the workspace records");
static_assert(sizeof(nb_knn_plan_t) == 64, "the plan");

bool size_ok(unsigned n, unsigned k) { return n >= 1 && n <= nb::kKnnMaxBodies && k >= 1 && k <= nb::kKnnMaxK; }

template <typename T> int plan_query(unsigned n, unsigned k, nb_knn_plan_t* out) {
    if (out == nullptr || !size_ok(n, k)) return NB_ERR_INVALID_ARGUMENT;
    constexpr unsigned per_tile = sizeof(T) == 4 ? 128 : 64;
    const unsigned     S        = nb::knn_waves(n);
    out->bodies_per_lane        = per_tile / 64;
    out->waves_per_group        = static_cast<int>(S);
    out->unroll                 = sizeof(T) == 4 ? 4 : 2;
    out->capacity               = static_cast<int>(nb::knn_capacity(k));
    out->ranges                 = 1;
    out->tiles                  = nb::knn_tiles(n, per_tile);
    out->block_threads          = 64 * S;
    out->lds_bytes              = nb::knn_lds_bytes(n, k, sizeof(T));
    out->chunks                 = nb::knn_chunks(n);
    out->blocks                 = nb::knn_blocks(n);
    out->search_launches        = 1;
    out->structure_launches     = k >= 2 ? 3 : 0;
    out->density_offset         = nb::knn_layout(n, sizeof(T)).rho;
    out->density_bytes          = static_cast<unsigned long long>(n) * 8;
    return 0;
}

template <typename T>
int survey(const T* pos, unsigned n, unsigned k, unsigned* index, T* dist_sq, T* densities, nb_knn_structure_t* structure, void* workspace, size_t workspace_bytes,
           nb_stream_t stream) {
    if (!size_ok(n, k) || pos == nullptr || workspace == nullptr) return NB_ERR_INVALID_ARGUMENT;
    if (index == nullptr && dist_sq == nullptr && densities == nullptr && structure == nullptr) return NB_ERR_INVALID_ARGUMENT;
    if (k < 2 && (densities != nullptr || structure != nullptr)) return NB_ERR_INVALID_ARGUMENT;
    const nb::KnnLayout l = nb::knn_layout(n, sizeof(T));
    if (workspace_bytes < l.bytes) return NB_ERR_INVALID_ARGUMENT;
    const std::uintptr_t N = n, K = k;
    if (!spans_ok({{pos, N * 4 * sizeof(T), 4 * sizeof(T)}, {index, N * K * 4, 4, Span::optional}, {dist_sq, N * K * sizeof(T), sizeof(T), Span::optional},
                   {densities, N * sizeof(T), sizeof(T), Span::optional}, {structure, 128, 8, Span::optional}, {workspace, l.bytes, 32}})) {
        return NB_ERR_INVALID_ARGUMENT;
    }
    nb::KnnArgs<T> a{};
    a.pos = pos, a.n = n, a.k = k, a.index = index, a.dist_sq = dist_sq, a.densities = densities;
    a.structure   = reinterpret_cast<nb::KnnStructure*>(structure);
    char* const ws = static_cast<char*>(workspace);
    a.rho   = reinterpret_cast<double*>(ws + l.rho);
    a.tiles = reinterpret_cast<nb::KnnTile*>(ws + l.tiles);
    a.rings = reinterpret_cast<nb::KnnRing*>(ws + l.rings);
    a.head  = reinterpret_cast<nb::KnnStructure*>(ws + l.head);
    return static_cast<int>(nb::launch_knn_survey<T>(a, static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nb_knn_workspace_bytes(unsigned num_bodies, unsigned k, unsigned sizeof_T, size_t* bytes) {
    if (bytes == nullptr || !size_ok(num_bodies, k) || !nb::element_size_ok(sizeof_T)) return NB_ERR_INVALID_ARGUMENT;
    *bytes = nb::knn_layout(num_bodies, sizeof_T).bytes;
    return 0;
}

int nb_knn_plan_f32(unsigned num_bodies, unsigned k, nb_knn_plan_t* plan) { return plan_query<float>(num_bodies, k, plan); }
int nb_knn_plan_f64(unsigned num_bodies, unsigned k, nb_knn_plan_t* plan) { return plan_query<double>(num_bodies, k, plan); }

int nb_knn_survey_f32(const float* positions, unsigned num_bodies, unsigned k, unsigned* knn_index, float* knn_dist_sq, float* densities, nb_knn_structure_t* structure,
                      void* workspace, size_t workspace_bytes, nb_stream_t stream) {
    return survey<float>(positions, num_bodies, k, knn_index, knn_dist_sq, densities, structure, workspace, workspace_bytes, stream);
}
int nb_knn_survey_f64(const double* positions, unsigned num_bodies, unsigned k, unsigned* knn_index, double* knn_dist_sq, double* densities, nb_knn_structure_t* structure,
                      void* workspace, size_t workspace_bytes, nb_stream_t stream) {
    return survey<double>(positions, num_bodies, k, knn_index, knn_dist_sq, densities, structure, workspace, workspace_bytes, stream);
}

}  // extern "C"
