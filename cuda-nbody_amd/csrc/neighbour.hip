// neighbour.hip -- the kernels of libnbody_hip_neighbour.so (include/nbody_hip_neighbour.h): nearest neighbours, counts within a radius,
// potentials and neighbour lists over all pairs.  gfx950 only; FMA contraction on (d2 is written with explicit fused operations, so
// the flag changes no bit of it).
//
// A survey is two launches, a lists call five; no atomics, every word written by one lane:
//   neighbour_survey<T, S, POT>  the hot path: a workgroup owns one tile of 64 W bodies i (a lane holds W: fp32 one packed pair, fp64 one);
//                                bodies j arrive wave-uniform through scalar loads, U at a time into two register sets, one group ahead;
//                                the S waves split the chunks of 128 bodies j (chunk c -> wave c mod S), fold through LDS in wave order
//                                and wave 0 stores the outputs that were asked for and one record of the tile
//   neighbour_status             ONE workgroup folds the tiles' records into the status record
//   neighbour_count<T>           one wave per (tile, range of chunks): counts into the planes [J][N]
//   list_block                   per 256 bodies: the sum and the largest of the counts
//   list_scan                    ONE workgroup: exclusive prefix of those sums in index order, the total, the decision about the
//                                capacity, the status record
//   list_offsets                 offsets[i]
//   neighbour_fill<T>            one wave per (tile, range): (range, body) writes at offsets[i] + the counts of the ranges before it,
//                                ascending; returns at once when the scan refused
//
// The streaming loop holds no LDS access, barrier or scratch.  Per body j and packed pair of bodies i it is 3 v_pk_add_f32 +
// v_pk_mul_f32 + 2 v_pk_fma_f32 for d2 (NB_NEIGHBOUR_DIST_SQ, the one expression of the header), and per body i a v_min_f32 and a
// v_cmp_lt_f32 + add-with-carry for the count.  The nearest INDEX is not carried per body j: per group of U bodies j one
// v_cmp_lt_f32 + 2 v_cndmask_b32 keep the minimum and the first body of the first group that lowered it (strictly, groups ascending),
// and the index is found after the loop as the first of those U bodies whose d2 equals the minimum.  (One v_mov_b32 per group brings
// that first index into a vector register: a VOP3 select reads one scalar operand, and its mask is one.)  With potentials: one v_pk_add_f32
// (s2 = d2 + softening_sq), 2 v_rsq_f32 and one v_pk_fma_f32 (the mass is the multiplier: no unit / mixed forms are needed).
// The chunk that holds the workgroup's own bodies runs a second compiled form of the loop that turns d2(i, i) into +inf by INDEX.
#include "neighbour_kernels.h"

#include "../../include/nbody_hip_neighbour.h"

namespace nb {
namespace {

#include "nbody_lane.h"

constexpr int kFlushEvery = 8;  // chunks a register sum of potentials may collect
template <typename T> constexpr int unroll_for() { return sizeof(T) == 8 ? 2 : 4; }  // U: a body j is 4 (fp32) / 8 (fp64) scalar registers

__device__ __forceinline__ float  min_of(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double min_of(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ float  fma_of(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_of(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename T> __device__ __forceinline__ T infinity() { return static_cast<T>(__builtin_huge_valf()); }

// d2(i, j) of one pair outside the streaming loops: the same operations, so the same bits
template <typename T> __device__ __forceinline__ T dist_sq(T xi, T yi, T zi, T xj, T yj, T zj) {
    const T dx = xj - xi, dy = yj - yi, dz = zj - zi;
    return NB_NEIGHBOUR_DIST_SQ(fma_of, dx, dy, dz);
}

// 1 / sqrt(s2).  fp32: v_rsq_f32 (1 ulp).  fp64: the v_rsq_f64 seed y0 (relative error <= 2^-23) and, with r = 1 - s2 y0^2,
// y0 (1 - r)^(-1/2) = y0 (1 + r/2 + 3/8 r^2 + O(r^3)), truncation 5/16 r^3 < 2^-67; s2 = 0 and +inf (r is NaN) keep the seed's inf and 0.
__device__ __forceinline__ v2f inv_sqrt(v2f s2) { return v2f{__builtin_amdgcn_rsqf(s2.x), __builtin_amdgcn_rsqf(s2.y)}; }
__device__ __forceinline__ double inv_sqrt(double s2) {
    const double y0 = __builtin_amdgcn_rsq(s2);
    const double r  = __builtin_fma(-s2, y0 * y0, 1.0);
    const double y  = __builtin_fma(y0 * r, __builtin_fma(r, 0.375, 0.5), y0);
    return r == r ? y : y0;
}

// The streaming loop the three all-pairs kernels share.  Chunks c_first, c_first + c_step, ... < c_end of 128 bodies j; f is called
// as f.template operator()<MASKED, UB>(b, j0) with UB bodies j (UB = U, or 1 in the ragged end of the last chunk) starting at body j0
// in scalar registers, MASKED for the chunk `own_chunk`; after_chunk() after each chunk.
template <typename T, typename F, typename G>
__device__ __forceinline__ void stream_chunks(const T* pos, unsigned n, unsigned c_first, unsigned c_end, unsigned c_step, unsigned own_chunk, F&& f, G&& after_chunk) {
    using raw4      = typename Lane<T>::raw4;
    constexpr int U = unroll_for<T>();
    constexpr unsigned CH = kNeighbourChunk;
    static_assert(CH % U == 0, "the streaming loop is unrolled by U");
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx16
    const stream_ptr jp = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(pos));

    auto group   = [&](size_t j0, raw4(&b)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) b[u] = jp[j0 + u];
    };
    auto arrived = [](const raw4(&b)[U]) { asm volatile("" : : "s"(b[0]) : "memory"); };  // what follows is issued after the set's wait
    // b0 holds (or is loading) group 0 of the chunk at body `chunk`; on return it is loading the first group at body `next`
    auto stream = [&]<bool MASKED>(unsigned chunk, unsigned groups, size_t next, raw4(&b0)[U], raw4(&b1)[U]) {
        unsigned g = 0;
#pragma unroll 1
        for (; g + 2 <= groups; g += 2) {
            arrived(b0);
            group(static_cast<size_t>(chunk) + (g + 1) * U, b1);
            __builtin_amdgcn_sched_barrier(0);  // (the load stays ahead of the compute it overlaps)
            f.template operator()<MASKED, U>(b0, chunk + g * U);
            arrived(b1);
            group(g + 2 < groups ? static_cast<size_t>(chunk) + (g + 2) * U : next, b0);
            __builtin_amdgcn_sched_barrier(0);
            f.template operator()<MASKED, U>(b1, chunk + (g + 1) * U);
        }
        if (g < groups) f.template operator()<MASKED, U>(b0, chunk + g * U);  // (odd count: the ragged last chunk, nothing follows it)
    };

    raw4     b0[U], b1[U];
    unsigned c = c_first;
    if (c < c_end && n - c * CH >= static_cast<unsigned>(U)) group(static_cast<size_t>(c) * CH, b0);
    for (; c < c_end; c += c_step) {
        const unsigned first_j = c * CH;
        const unsigned count   = min(CH, n - first_j);
        const unsigned groups  = count / U;
        const size_t   next    = ((c + c_step) < c_end && n - (first_j + c_step * CH) >= static_cast<unsigned>(U)) ? static_cast<size_t>(first_j) + c_step * CH : first_j;
        const bool     own     = c == own_chunk;
        if (groups > 0) {
            if (own) {
                stream.template operator()<true>(first_j, groups, next, b0, b1);
            } else {
                stream.template operator()<false>(first_j, groups, next, b0, b1);
            }
        }
#pragma unroll 1
        for (unsigned jj = groups * U; jj < count; ++jj) {  // ragged end of the last chunk
            raw4 one[1];
            one[0] = jp[static_cast<size_t>(first_j) + jj];
            if (own) {
                f.template operator()<true, 1>(one, first_j + jj);
            } else {
                f.template operator()<false, 1>(one, first_j + jj);
            }
        }
        after_chunk();
    }
}

// the lane's W bodies i of the tile at tile_base: index (clamped into the state for the loads) and coordinates
template <typename T> struct BodiesI {
    using LT = Lane<T>;
    typename LT::vec px, py, pz;
    unsigned         index[LT::W];
    bool             valid[LT::W];
    __device__ __forceinline__ void load(const T* pos, unsigned n, unsigned tile_base, unsigned lane) {
#pragma unroll
        for (int k = 0; k < LT::W; ++k) {
            const unsigned i = tile_base + k * 64 + lane;
            valid[k]         = i < n;
            index[k]         = i;
            const typename LT::vec4 p = reinterpret_cast<const typename LT::vec4*>(pos)[valid[k] ? i : n - 1];
            LT::set(px, k, p.x), LT::set(py, k, p.y), LT::set(pz, k, p.z);
        }
    }
};

// d2 of UB bodies j against the lane's vector of bodies i; MASKED: d2(i, i) = +inf by index
template <typename T, bool MASKED, int UB>
__device__ __forceinline__ void distances(const typename Lane<T>::raw4* b, unsigned j0, const BodiesI<T>& me, typename Lane<T>::vec (&d2)[UB]) {
    using LT = Lane<T>;
#pragma unroll
    for (int u = 0; u < UB; ++u) {
        const typename LT::vec dx = LT::splat(b[u].x) - me.px, dy = LT::splat(b[u].y) - me.py, dz = LT::splat(b[u].z) - me.pz;
        d2[u]                     = NB_NEIGHBOUR_DIST_SQ(LT::fma, dx, dy, dz);
    }
    if constexpr (MASKED) {
#pragma unroll
        for (int u = 0; u < UB; ++u) {
#pragma unroll
            for (int k = 0; k < LT::W; ++k) LT::set(d2[u], k, j0 + u == me.index[k] ? infinity<T>() : LT::get(d2[u], k));
        }
    }
}

template <typename T> __device__ __forceinline__ typename Lane<T>::vec radii_of(const T* radii, T radius_sq, const BodiesI<T>& me) {
    typename Lane<T>::vec r2;
#pragma unroll
    for (int k = 0; k < Lane<T>::W; ++k) {
        // (a lane past the end of the state counts and lists nobody)
        Lane<T>::set(r2, k, !me.valid[k] ? __builtin_nanf("") : (radii != nullptr ? radii[me.index[k]] : radius_sq));
    }
    return r2;
}

struct Closest {
    double   d2;
    unsigned i, j;
};
__device__ __forceinline__ bool closer(const Closest& a, const Closest& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.i < b.i); }
struct Fullest {
    unsigned count, body;
};
__device__ __forceinline__ bool fuller(const Fullest& a, const Fullest& b) { return a.count > b.count || (a.count == b.count && a.body < b.body); }

template <typename T, int S, bool POT>
__global__ __launch_bounds__(64 * S) void neighbour_survey(const T* pos, const T* radii, T radius_sq, T eps2_in, unsigned n, unsigned* nearest, T* nearest_d2, unsigned* counts,
                                                          T* potentials, NeighbourTile* tiles) {
    using LT        = Lane<T>;
    using vec       = typename LT::vec;
    using raw4      = typename LT::raw4;
    constexpr int W = LT::W;
    constexpr int U = unroll_for<T>();

    const int      tid       = threadIdx.x;
    const int      wave      = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lane      = tid & 63;
    const unsigned tile_base = blockIdx.x * (64 * W);
    BodiesI<T>     me;
    me.load(pos, n, tile_base, lane);
    const vec r2   = radii_of<T>(radii, radius_sq, me);
    vec       eps2 = LT::splat(eps2_in);
    LT::keep_in_vgpr(eps2);

    T        best[W];
    unsigned first_of[W], count[W];
    vec      first = LT::splat(0), second = LT::splat(0);
#pragma unroll
    for (int k = 0; k < W; ++k) best[k] = infinity<T>(), first_of[k] = kNeighbourNone, count[k] = 0;

    auto body = [&]<bool MASKED, int UB>(const raw4* b, unsigned j0) {
        vec d2[UB];
        distances<T, MASKED, UB>(b, j0, me, d2);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            T least = LT::get(d2[0], k);
#pragma unroll
            for (int u = 1; u < UB; ++u) least = min_of(least, LT::get(d2[u], k));
            const bool lower = least < best[k];  // strictly: the first group that reaches the minimum keeps it
            first_of[k]      = lower ? j0 : first_of[k];
            best[k]          = lower ? least : best[k];
#pragma unroll
            for (int u = 0; u < UB; ++u) count[k] += LT::get(d2[u], k) < LT::get(r2, k) ? 1u : 0u;
        }
        if constexpr (POT) {
#pragma unroll
            for (int u = 0; u < UB; ++u) first = LT::fma(inv_sqrt(d2[u] + eps2), LT::splat(b[u].w), first);
        }
    };
    unsigned held        = 0;
    auto     after_chunk = [&]() {
        if constexpr (POT) {
            if (++held == kFlushEvery) second = second + first, first = LT::splat(0), held = 0;
        }
    };
    const unsigned own_chunk = tile_base / kNeighbourChunk;
    stream_chunks<T>(pos, n, static_cast<unsigned>(wave), neighbour_chunks(n), S, own_chunk, body, after_chunk);
    second = second + first;

    // the index: the first of the U bodies from first_of whose d2 is the minimum (the same operations, so the same bits)
    unsigned index[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        index[k] = kNeighbourNone;
        if (best[k] < infinity<T>()) {
            const T xi = LT::get(me.px, k), yi = LT::get(me.py, k), zi = LT::get(me.pz, k);
#pragma unroll 1
            for (unsigned j = first_of[k]; j < first_of[k] + U && j < n; ++j) {
                if (j == me.index[k]) continue;
                const typename LT::vec4 p = reinterpret_cast<const typename LT::vec4*>(pos)[j];
                if (dist_sq<T>(xi, yi, zi, p.x, p.y, p.z) == best[k]) {
                    index[k] = j;
                    break;
                }
            }
        }
    }

    // fold the S waves (waves 1..S-1 -> wave 0) through LDS in wave order: (d2, index) lexicographically, counts and potentials add
    __shared__ T        red_t[(S > 1 ? S - 1 : 1) * 2 * W * 64];
    __shared__ unsigned red_u[(S > 1 ? S - 1 : 1) * 2 * W * 64];
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int at = ((wave - 1) * W + k) * 2 * 64 + lane;
            red_t[at] = best[k], red_t[at + 64] = LT::get(second, k);
            red_u[at] = index[k], red_u[at + 64] = count[k];
        }
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll 1
    for (int g = 1; g < S; ++g) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int      at = ((g - 1) * W + k) * 2 * 64 + lane;
            const T        d2 = red_t[at];
            const unsigned j  = red_u[at];
            if (d2 < best[k] || (d2 == best[k] && j < index[k])) best[k] = d2, index[k] = j;
            count[k] += red_u[at + 64];
            LT::set(second, k, LT::get(second, k) + red_t[at + 64]);
        }
    }
    Closest  near{static_cast<double>(infinity<float>()), kNeighbourNone, kNeighbourNone};
    Fullest  most{0u, kNeighbourNone};
    unsigned long long total = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        if (!me.valid[k]) continue;
        const unsigned i = me.index[k];
        if (nearest != nullptr) nearest[i] = index[k];
        if (nearest_d2 != nullptr) nearest_d2[i] = best[k];
        if (counts != nullptr) counts[i] = count[k];
        if constexpr (POT) potentials[i] = -LT::get(second, k);
        const Closest mine{static_cast<double>(best[k]), index[k] == kNeighbourNone ? kNeighbourNone : i, index[k]};
        if (closer(mine, near)) near = mine;
        const Fullest full{count[k], i};
        if (fuller(full, most)) most = full;
        total += count[k];
    }
    // the tile's record: a butterfly over the wave (minima, maxima and integer sums: the order changes nothing)
#pragma unroll
    for (int step = 1; step < 64; step *= 2) {
        const Closest other{__shfl_xor(near.d2, step), __shfl_xor(near.i, step), __shfl_xor(near.j, step)};
        if (closer(other, near)) near = other;
        const Fullest full{__shfl_xor(most.count, step), __shfl_xor(most.body, step)};
        if (fuller(full, most)) most = full;
        total += __shfl_xor(total, step);
    }
    if (lane == 0) tiles[blockIdx.x] = NeighbourTile{near.d2, near.i, near.j, total, most.count, most.body};
}

// the workgroup-wide fold of the records' three quantities (1 024 lanes)
__device__ __forceinline__ void fold_1024(Closest& near, Fullest& most, unsigned long long& total) {
    __shared__ Closest            lds_near[1024];
    __shared__ Fullest            lds_most[1024];
    __shared__ unsigned long long lds_total[1024];
    const unsigned                tid = threadIdx.x;
    lds_near[tid] = near, lds_most[tid] = most, lds_total[tid] = total;
    __syncthreads();
#pragma unroll 1
    for (unsigned half = 512; half > 0; half >>= 1) {
        if (tid < half) {
            if (closer(lds_near[tid + half], lds_near[tid])) lds_near[tid] = lds_near[tid + half];
            if (fuller(lds_most[tid + half], lds_most[tid])) lds_most[tid] = lds_most[tid + half];
            lds_total[tid] += lds_total[tid + half];
        }
        __syncthreads();
    }
    near = lds_near[0], most = lds_most[0], total = lds_total[0];
}

__global__ __launch_bounds__(1024) void neighbour_status(const NeighbourTile* tiles, unsigned count, NeighbourStatus* status) {
    Closest            near{static_cast<double>(infinity<float>()), kNeighbourNone, kNeighbourNone};
    Fullest            most{0u, kNeighbourNone};
    unsigned long long total = 0;
    for (unsigned t = threadIdx.x; t < count; t += 1024u) {
        const NeighbourTile r = tiles[t];
        const Closest       c{r.d2, r.i, r.j};
        if (closer(c, near)) near = c;
        const Fullest f{r.max_count, r.max_body};
        if (fuller(f, most)) most = f;
        total += r.count_sum;
    }
    fold_1024(near, most, total);
    if (threadIdx.x == 0) {
        NeighbourStatus s{};
        s.total = total, s.closest_d2 = near.d2, s.closest_i = near.i, s.closest_j = near.j;
        s.max_count = most.count, s.max_count_body = most.body, s.flags = 0;
        *status = s;
    }
}

// ---- lists -----------------------------------------------------------------------------------------------------------------------------

// (tile, range) of a one-wave workgroup of the count and the fill pass, and the range's chunks [c_lo, c_hi): never empty (J <= chunks)
struct ListWork {
    unsigned tile_base, range, c_lo, c_hi;
};
template <typename T> __device__ __forceinline__ ListWork list_work(unsigned n) {
    constexpr unsigned per_tile = 64 * Lane<T>::W;
    const unsigned     ranges = neighbour_ranges(n, per_tile), chunks = neighbour_chunks(n);
    ListWork           w;
    w.tile_base = (blockIdx.x / ranges) * per_tile;
    w.range     = blockIdx.x % ranges;
    w.c_lo      = static_cast<unsigned>(static_cast<unsigned long long>(w.range) * chunks / ranges);
    w.c_hi      = static_cast<unsigned>(static_cast<unsigned long long>(w.range + 1) * chunks / ranges);
    return w;
}

template <typename T> __global__ __launch_bounds__(64) void neighbour_count(const T* pos, const T* radii, T radius_sq, unsigned n, unsigned* planes) {
    using LT        = Lane<T>;
    using vec       = typename LT::vec;
    using raw4      = typename LT::raw4;
    constexpr int W = LT::W;
    const ListWork w = list_work<T>(n);
    BodiesI<T>     me;
    me.load(pos, n, w.tile_base, threadIdx.x);
    const vec r2 = radii_of<T>(radii, radius_sq, me);
    unsigned  count[W];
#pragma unroll
    for (int k = 0; k < W; ++k) count[k] = 0;
    auto body = [&]<bool MASKED, int UB>(const raw4* b, unsigned j0) {
        vec d2[UB];
        distances<T, MASKED, UB>(b, j0, me, d2);
#pragma unroll
        for (int k = 0; k < W; ++k) {
#pragma unroll
            for (int u = 0; u < UB; ++u) count[k] += LT::get(d2[u], k) < LT::get(r2, k) ? 1u : 0u;
        }
    };
    stream_chunks<T>(pos, n, w.c_lo, w.c_hi, 1u, w.tile_base / kNeighbourChunk, body, []() {});
#pragma unroll
    for (int k = 0; k < W; ++k) {
        if (me.valid[k]) planes[static_cast<size_t>(w.range) * n + me.index[k]] = count[k];
    }
}

__device__ __forceinline__ unsigned planes_sum(const unsigned* planes, unsigned ranges, unsigned n, unsigned i) {
    unsigned sum = 0;
    for (unsigned r = 0; r < ranges; ++r) sum += planes[static_cast<size_t>(r) * n + i];
    return sum;
}

__global__ __launch_bounds__(256) void list_block(const unsigned* planes, unsigned ranges, unsigned n, NeighbourTile* blocks) {
    __shared__ unsigned lds_sum[256], lds_count[256], lds_body[256];
    const unsigned      tid = threadIdx.x, i = blockIdx.x * 256u + tid;
    const unsigned      mine = i < n ? planes_sum(planes, ranges, n, i) : 0u;
    lds_sum[tid] = mine, lds_count[tid] = mine, lds_body[tid] = i < n ? i : kNeighbourNone;
    __syncthreads();
#pragma unroll 1
    for (unsigned half = 128; half > 0; half >>= 1) {
        if (tid < half) {
            lds_sum[tid] += lds_sum[tid + half];  // (256 counts of at most 2^24: no overflow)
            const Fullest other{lds_count[tid + half], lds_body[tid + half]};
            if (fuller(other, Fullest{lds_count[tid], lds_body[tid]})) lds_count[tid] = other.count, lds_body[tid] = other.body;
        }
        __syncthreads();
    }
    if (tid == 0) blocks[blockIdx.x] = NeighbourTile{0.0, 0u, 0u, lds_sum[0], lds_count[0], lds_body[0]};
}

// block_sums[b] = the entries of the blocks before b; the total, offsets[N], the decision and the status record.  One workgroup of 1 024.
__global__ __launch_bounds__(1024) void list_scan(const NeighbourTile* blocks, unsigned count, unsigned n, unsigned long long capacity, unsigned long long* block_sums,
                                                  unsigned long long* offsets, NeighbourCtrl* ctrl, NeighbourStatus* status) {
    __shared__ unsigned long long sums[1024];
    const unsigned                tid = threadIdx.x, per = (count + 1023u) / 1024u;
    const unsigned                lo = tid * per < count ? tid * per : count, hi = lo + per < count ? lo + per : count;
    Closest                       near{static_cast<double>(infinity<float>()), kNeighbourNone, kNeighbourNone};
    Fullest                       most{0u, kNeighbourNone};
    unsigned long long            mine = 0;
    for (unsigned b = lo; b < hi; ++b) {
        const NeighbourTile r = blocks[b];
        const Fullest       f{r.max_count, r.max_body};
        if (fuller(f, most)) most = f;
        mine += r.count_sum;
    }
    sums[tid] = mine;
    __syncthreads();
#pragma unroll 1
    for (unsigned step = 1; step < 1024u; step *= 2) {  // inclusive scan; integer sums, so the order changes nothing
        const unsigned long long add = tid >= step ? sums[tid - step] : 0ull;
        __syncthreads();
        sums[tid] += add;
        __syncthreads();
    }
    unsigned long long before = sums[tid] - mine;
    for (unsigned b = lo; b < hi; ++b) {
        block_sums[b] = before;
        before += blocks[b].count_sum;
    }
    unsigned long long total = mine;
    fold_1024(near, most, total);
    if (tid == 0) {
        const bool fits = total <= capacity;
        ctrl->total = total, ctrl->go = fits ? 1u : 0u;
        offsets[n]  = total;
        NeighbourStatus s{};
        s.total = total, s.closest_d2 = near.d2, s.closest_i = kNeighbourNone, s.closest_j = kNeighbourNone;
        s.max_count = most.count, s.max_count_body = most.body, s.flags = fits ? 0u : kNeighbourOverflow;
        *status = s;
    }
}

__global__ __launch_bounds__(256) void list_offsets(const unsigned* planes, unsigned ranges, unsigned n, const unsigned long long* block_sums, unsigned long long* offsets) {
    __shared__ unsigned scan[256];
    const unsigned      tid = threadIdx.x, i = blockIdx.x * 256u + tid;
    const unsigned      mine = i < n ? planes_sum(planes, ranges, n, i) : 0u;
    scan[tid]                = mine;
    __syncthreads();
#pragma unroll 1
    for (unsigned step = 1; step < 256u; step *= 2) {
        const unsigned add = tid >= step ? scan[tid - step] : 0u;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    if (i < n) offsets[i] = block_sums[blockIdx.x] + (scan[tid] - mine);
}

template <typename T>
__global__ __launch_bounds__(64) void neighbour_fill(const T* pos, const T* radii, T radius_sq, unsigned n, const unsigned* planes, const unsigned long long* offsets,
                                                    const NeighbourCtrl* ctrl, unsigned* indices) {
    using LT        = Lane<T>;
    using vec       = typename LT::vec;
    using raw4      = typename LT::raw4;
    constexpr int W = LT::W;
    if (ctrl->go == 0) return;
    const ListWork w = list_work<T>(n);
    BodiesI<T>     me;
    me.load(pos, n, w.tile_base, threadIdx.x);
    const vec          r2 = radii_of<T>(radii, radius_sq, me);
    unsigned long long at[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        at[k] = 0;
        if (me.valid[k]) at[k] = offsets[me.index[k]] + planes_sum(planes, w.range, n, me.index[k]);
    }
    auto body = [&]<bool MASKED, int UB>(const raw4* b, unsigned j0) {
        vec d2[UB];
        distances<T, MASKED, UB>(b, j0, me, d2);
#pragma unroll
        for (int u = 0; u < UB; ++u) {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                if (LT::get(d2[u], k) < LT::get(r2, k)) indices[at[k]++] = j0 + u;  // (r2 is NaN past the end of the state)
            }
        }
    };
    stream_chunks<T>(pos, n, w.c_lo, w.c_hi, 1u, w.tile_base / kNeighbourChunk, body, []() {});
}

template <typename T, int S, bool POT> hipError_t launch_survey_s(const NeighbourArgs<T>& a, unsigned groups, hipStream_t stream) {
    hipLaunchKernelGGL((neighbour_survey<T, S, POT>), dim3(groups), dim3(64 * S), 0, stream, a.pos, a.radii, a.radius_sq, a.eps2, a.n, a.nearest, a.nearest_d2, a.counts,
                       a.potentials, a.tiles);
    return hipGetLastError();
}
template <typename T, bool POT> hipError_t launch_survey_pot(const NeighbourArgs<T>& a, unsigned groups, hipStream_t stream) {
    switch (neighbour_waves(a.n)) {
        case 1: return launch_survey_s<T, 1, POT>(a, groups, stream);
        case 2: return launch_survey_s<T, 2, POT>(a, groups, stream);
        case 4: return launch_survey_s<T, 4, POT>(a, groups, stream);
        case 8: return launch_survey_s<T, 8, POT>(a, groups, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

template <typename T> hipError_t launch_neighbour_survey(const NeighbourArgs<T>& a, hipStream_t stream) {
    const unsigned groups = neighbour_tiles(a.n, 64 * Lane<T>::W);
    (void)hipGetLastError();
    const hipError_t err = a.potentials != nullptr ? launch_survey_pot<T, true>(a, groups, stream) : launch_survey_pot<T, false>(a, groups, stream);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(neighbour_status, dim3(1), dim3(1024), 0, stream, static_cast<const NeighbourTile*>(a.tiles), groups, a.status);
    return hipGetLastError();
}

template <typename T> hipError_t launch_neighbour_lists(const NeighbourArgs<T>& a, hipStream_t stream) {
    constexpr unsigned per_tile = 64 * Lane<T>::W;
    const unsigned     ranges = neighbour_ranges(a.n, per_tile), groups = neighbour_tiles(a.n, per_tile) * ranges;
    const unsigned     blocks = (a.n + kNeighbourThreads - 1) / kNeighbourThreads;
    (void)hipGetLastError();
    hipLaunchKernelGGL((neighbour_count<T>), dim3(groups), dim3(64), 0, stream, a.pos, a.radii, a.radius_sq, a.n, a.planes);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL(list_block, dim3(blocks), dim3(256), 0, stream, static_cast<const unsigned*>(a.planes), ranges, a.n, a.tiles);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL(list_scan, dim3(1), dim3(1024), 0, stream, static_cast<const NeighbourTile*>(a.tiles), blocks, a.n, a.capacity, a.block_sums, a.offsets, a.ctrl, a.status);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL(list_offsets, dim3(blocks), dim3(256), 0, stream, static_cast<const unsigned*>(a.planes), ranges, a.n, static_cast<const unsigned long long*>(a.block_sums),
                       a.offsets);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL((neighbour_fill<T>), dim3(groups), dim3(64), 0, stream, a.pos, a.radii, a.radius_sq, a.n, static_cast<const unsigned*>(a.planes),
                       static_cast<const unsigned long long*>(a.offsets), static_cast<const NeighbourCtrl*>(a.ctrl), a.indices);
    return hipGetLastError();
}

template hipError_t launch_neighbour_survey<float>(const NeighbourArgs<float>&, hipStream_t);
template hipError_t launch_neighbour_survey<double>(const NeighbourArgs<double>&, hipStream_t);
template hipError_t launch_neighbour_lists<float>(const NeighbourArgs<float>&, hipStream_t);
template hipError_t launch_neighbour_lists<double>(const NeighbourArgs<double>&, hipStream_t);

}  // namespace nb
