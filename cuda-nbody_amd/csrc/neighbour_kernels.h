// neighbour_kernels.h -- internal launch interface of libnbody_hip_neighbour.so (include/nbody_hip_neighbour.h) between its C-ABI unit
// (neighbour_capi.hip) and its kernel unit (neighbour.hip, contraction on), and the geometry both sides (and the kernels themselves)
// derive from (N, precision).
#pragma once

#include <hip/hip_runtime.h>

namespace nb {

inline constexpr unsigned kNeighbourMaxBodies = 1u << 24;
inline constexpr unsigned kNeighbourNone      = 0xFFFFFFFFu;
inline constexpr unsigned kNeighbourOverflow  = 1u;
inline constexpr unsigned kNeighbourChunk     = 128;   // bodies j per wave and chunk
inline constexpr unsigned kNeighbourTarget    = 2048;  // one-wave workgroups the lists' passes aim at: 8 per CU of 256
inline constexpr unsigned kNeighbourThreads   = 256;   // block size of the scan kernels: one body per lane

struct NeighbourStatus {  // nb_neighbour_status_t, 64 bytes
    unsigned long long total;
    double             closest_d2;
    unsigned           closest_i, closest_j, max_count, max_count_body, flags;
    unsigned           reserved[7];
};
struct NeighbourCtrl {  // what a lists call passes from launch to launch (workspace)
    unsigned long long total;
    unsigned           go;
    unsigned           reserved[13];
};
struct NeighbourTile {  // what a survey workgroup leaves of its tile for the status record (workspace), 32 bytes
    double             d2;  // the tile's smallest nearest_dist_sq (T widened) ...
    unsigned           i, j;  // ... its body (the lowest on equal bits) and that body's nearest
    unsigned long long count_sum;
    unsigned           max_count, max_body;
};

// ---- geometry: a function of (N, precision) alone -----------------------------------------------------------------------------------
__host__ __device__ inline unsigned neighbour_waves(unsigned n) {  // S, as plan_stream
    unsigned s = 1;
    while (s < 8 && 2 * s * kNeighbourChunk <= n) s *= 2;
    return s;
}
__host__ __device__ inline unsigned neighbour_chunks(unsigned n) { return (n + kNeighbourChunk - 1) / kNeighbourChunk; }
__host__ __device__ inline unsigned neighbour_tiles(unsigned n, unsigned per_tile) { return (n + per_tile - 1) / per_tile; }
__host__ __device__ inline unsigned neighbour_ranges(unsigned n, unsigned per_tile) {  // J
    const unsigned tiles = neighbour_tiles(n, per_tile), chunks = neighbour_chunks(n);
    const unsigned need  = (kNeighbourTarget + tiles - 1) / tiles;
    unsigned       j     = 1;
    while (j < need && 2 * j <= chunks) j *= 2;
    return j;
}

// ---- workspace layout (byte offsets, each section on a 256-byte boundary) ------------------------------------------------------------
struct NeighbourLayout {
    size_t planes, block_sums, tiles, ctrl, bytes;
};
inline NeighbourLayout neighbour_layout(unsigned n, size_t size_t_of) {
    const unsigned  per_tile = size_t_of == 4 ? 128 : 64;
    const auto      up       = [](size_t b) { return (b + 255) & ~static_cast<size_t>(255); };
    NeighbourLayout l;
    size_t          at = 0;
    l.planes = at, at += up(static_cast<size_t>(neighbour_ranges(n, per_tile)) * n * 4);
    l.block_sums = at, at += up(static_cast<size_t>((n + kNeighbourThreads - 1) / kNeighbourThreads) * 8);
    l.tiles = at, at += up(static_cast<size_t>(neighbour_tiles(n, per_tile)) * sizeof(NeighbourTile));
    l.ctrl = at, at += up(sizeof(NeighbourCtrl));
    l.bytes = at;
    return l;
}

template <typename T> struct NeighbourArgs {
    const T*            pos;    // T[4N]
    const T*            radii;  // T[N] or null
    T                   radius_sq, eps2;
    unsigned            n;
    unsigned*           nearest;  // outputs, each may be null
    T*                  nearest_d2;
    unsigned*           counts;
    T*                  potentials;
    unsigned long long* offsets;  // lists
    unsigned*           indices;
    unsigned long long  capacity;
    NeighbourStatus*    status;
    unsigned*           planes;  // workspace sections
    unsigned long long* block_sums;
    NeighbourTile*      tiles;
    NeighbourCtrl*      ctrl;
};

template <typename T> hipError_t launch_neighbour_survey(const NeighbourArgs<T>& a, hipStream_t stream);
template <typename T> hipError_t launch_neighbour_lists(const NeighbourArgs<T>& a, hipStream_t stream);

}  // namespace nb
