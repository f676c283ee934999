// knn_kernels.h -- internal launch interface of libnbody_hip_knn.so (include/nbody_hip_knn.h) between its C-ABI unit (knn_capi.hip) and
// its kernel unit (knn.hip, contraction on), and the geometry both sides (and the kernels themselves) derive from (N, K, precision).
#pragma once

#include <hip/hip_runtime.h>

namespace nb {

inline constexpr unsigned kKnnMaxBodies  = 1u << 24;
inline constexpr unsigned kKnnMaxK       = 16;
inline constexpr unsigned kKnnNone       = 0xFFFFFFFFu;
inline constexpr unsigned kKnnDegenerate = 1u;
inline constexpr unsigned kKnnNoDensity  = 2u;
inline constexpr unsigned kKnnChunk      = 128;   // bodies j per wave and chunk
inline constexpr unsigned kKnnThreads    = 256;   // block size of the pass for the radii: one body per lane
inline constexpr unsigned kKnnFold       = 512;   // lanes of the two one-workgroup folds

struct KnnStructure {  // nb_knn_structure_t, 128 bytes
    double   sum_density, centre[3], density_radius, core_radius, max_density, min_kth_d2, max_kth_d2;
    unsigned max_density_body, defined, degenerate, flags;
    unsigned reserved[10];
};
struct KnnTile {  // what a search workgroup leaves of its tile for the record (workspace), 72 bytes
    double   sum_rho, sum_x, sum_y, sum_z;  // sum rho, sum rho x ... over the tile
    double   max_rho, min_d2, max_d2;
    unsigned max_body, defined, degenerate, reserved;
};
struct KnnRing {  // what a block of 256 bodies leaves for the two radii (workspace), 24 bytes
    double first, second, weight;  // sum rho |x - x_d|, sum rho^2 |x - x_d|^2, sum rho^2
};

// ---- geometry: a function of (N, K, precision) alone ---------------------------------------------------------------------------------
__host__ __device__ inline unsigned knn_waves(unsigned n) {  // S: 1 below 256 bodies, 2 from 256, 4 from 512
    unsigned s = 1;
    while (s < 4 && 2 * s * kKnnChunk <= n) s *= 2;
    return s;
}
__host__ __device__ inline unsigned knn_capacity(unsigned k) { return k <= 4 ? 4u : k <= 8 ? 8u : 16u; }
__host__ __device__ inline unsigned knn_chunks(unsigned n) { return (n + kKnnChunk - 1) / kKnnChunk; }
__host__ __device__ inline unsigned knn_tiles(unsigned n, unsigned per_tile) { return (n + per_tile - 1) / per_tile; }
__host__ __device__ inline unsigned knn_blocks(unsigned n) { return (n + kKnnThreads - 1) / kKnnThreads; }
// LDS of a search workgroup: S / 2 lists of `capacity` (d2, j) entries per body of the tile
__host__ __device__ inline unsigned knn_lds_bytes(unsigned n, unsigned k, unsigned size_t_of) {
    const unsigned per_tile = size_t_of == 4 ? 128 : 64, s = knn_waves(n);
    return (s / 2) * knn_capacity(k) * per_tile * (size_t_of + 4);
}

// ---- workspace layout (byte offsets, each section on a 256-byte boundary) ------------------------------------------------------------
struct KnnLayout {
    size_t rho, tiles, rings, head, bytes;
};
inline KnnLayout knn_layout(unsigned n, size_t size_t_of) {
    const unsigned per_tile = size_t_of == 4 ? 128 : 64;
    const auto     up       = [](size_t b) { return (b + 255) & ~static_cast<size_t>(255); };
    KnnLayout      l;
    size_t         at = 0;
    l.rho = at, at += up(static_cast<size_t>(n) * 8);
    l.tiles = at, at += up(static_cast<size_t>(knn_tiles(n, per_tile)) * sizeof(KnnTile));
    l.rings = at, at += up(static_cast<size_t>(knn_blocks(n)) * sizeof(KnnRing));
    l.head = at, at += up(sizeof(KnnStructure));
    l.bytes = at;
    return l;
}

template <typename T> struct KnnArgs {
    const T*      pos;  // T[4N]
    unsigned      n, k;
    unsigned*     index;      // outputs, each may be null
    T*            dist_sq;
    T*            densities;
    KnnStructure* structure;
    double*       rho;  // workspace sections
    KnnTile*      tiles;
    KnnRing*      rings;
    KnnStructure* head;
};

template <typename T> hipError_t launch_knn_survey(const KnnArgs<T>& a, hipStream_t stream);

}  // namespace nb
