// knn.hip -- the kernels of libnbody_hip_knn.so (include/nbody_hip_knn.h): the K nearest neighbours of every body, the local densities and
// the structure record.  gfx950 only; FMA contraction on (d2 is written with explicit fused operations, so the flag changes no bit of it,
// and the density is products, one square root and one quotient in double: nothing to contract).
//
// A call is one launch, or four with the record; no atomics, every word written by one lane:
//   knn_search<T, CAP, S>  the hot path, on the wave-stream plan of neighbour_survey: a workgroup owns one tile of 64 W bodies i (a lane holds
//                          W: fp32 one packed pair, fp64 one); bodies j arrive wave-uniform through scalar loads, U at a time into two register
//                          sets, one group ahead; the S waves split the chunks of 128 bodies j (chunk c -> wave c mod S).  Per body i a lane
//                          keeps a SORTED list of CAP >= K entries (d2, j) in registers.  The waves' lists merge pairwise through LDS by
//                          (d2, j); wave 0 stores the outputs that were asked for, the double rho[N] and one record of the tile.
//   knn_centre             ONE workgroup folds the tiles' records: sum rho, the density centre, the extremes, the counts, the flags
//   knn_rings<T>           per 256 bodies: sum rho |x - x_d|, sum rho^2 |x - x_d|^2, sum rho^2
//   knn_record             ONE workgroup folds those into the two radii and stores the structure record
//
// The streaming loop.  Per group of U bodies j: d2 as the survey computes it (NB_NEIGHBOUR_DIST_SQ, the one expression of the header), per
// body i the group's least d2 (v_min) and a compare with the body's K-th entry, and ONE ballot: only when some lane's least d2 is below its
// K-th entry does the wave enter the insertion path.  There, per candidate (body j, body i of the lane) one more ballot, and for the
// candidates some lane wants, the insertion: a fully unrolled chain over the CAP slots under lane predicates (per slot one compare and the
// selects of d2 and j; no register array is indexed at run time), and the K-th entry read back through a select chain over the slots (K
// is a run-time value, CAP a compiled one).  The no-insertion path holds no LDS access, barrier, scratch or vector memory access.
// Within a wave j ascends, so a strict `<` on d2 keeps the tie rule (the lowest j first on equal bits); across waves the merge compares
// (d2, j).  The chunk that holds the workgroup's own bodies runs a second compiled form that turns d2(i, i) into +inf by INDEX.
#include "knn_kernels.h"

#include "../../include/nbody_hip_knn.h"

namespace nb {
namespace {

#include "nbody_lane.h"

template <typename T> constexpr int unroll_for() { return sizeof(T) == 8 ? 2 : 4; }  // U: a body j is 4 (fp32) / 8 (fp64) scalar registers

__device__ __forceinline__ float  min_of(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double min_of(double a, double b) { return __builtin_fmin(a, b); }
template <typename T> __device__ __forceinline__ T infinity() { return static_cast<T>(__builtin_huge_valf()); }

// The streaming loop (the plan of neighbour.hip's).  Chunks c_first, c_first + c_step, ... < c_end of 128 bodies j; f is called as
// f.template operator()<MASKED, UB>(b, j0) with UB bodies j (UB = U, or 1 in the ragged end of the last chunk) starting at body j0 in
// scalar registers, MASKED for the chunk `own_chunk`.
template <typename T, typename F>
__device__ __forceinline__ void stream_chunks(const T* pos, unsigned n, unsigned c_first, unsigned c_end, unsigned c_step, unsigned own_chunk, F&& f) {
    using raw4      = typename Lane<T>::raw4;
    constexpr int U = unroll_for<T>();
    constexpr unsigned CH = kKnnChunk;
    static_assert(CH % U == 0, "the streaming loop is unrolled by U");
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx16
    const stream_ptr jp = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(pos));

    auto group   = [&](size_t j0, raw4(&b)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) b[u] = jp[j0 + u];
    };
    auto arrived = [](const raw4(&b)[U]) { asm volatile("" : : "s"(b[0]) : "memory"); };  // what follows is issued after the set's wait
    // b0 holds (or is loading) group 0 of the chunk at body `chunk`; on return it is loading the first group at body `next`
    auto stream = [&]<bool MASKED>(unsigned chunk, unsigned groups, size_t next, raw4(&b0)[U], raw4(&b1)[U]) __attribute__((always_inline)) {
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

// ---- a body's sorted list of CAP entries (d2, j) in registers -------------------------------------------------------------------------
// The slots are the elements of two vectors, read and written by constant element only.  (As arrays they went to private memory and LDS: the
// compiler turns a select between two loads of an array into one load through a selected address, and that address is a run-time index.)
template <typename V, int CAP> using Slots = V __attribute__((ext_vector_type(CAP)));

// `before(s)` says whether the new entry sorts before the entry in slot s; the list is sorted, so it is false ... false true ... true down
// the slots.  Slot s then takes the entry above it when the new entry sorts before that one too, the new entry when it does not, and keeps
// its own otherwise.  An entry of d2 = +inf (or NaN) sorts before nothing: inserting it changes no slot.
template <typename T, int CAP, typename Before>
__device__ __forceinline__ void insert_sorted(Slots<T, CAP>& ld, Slots<unsigned, CAP>& lj, T d, unsigned j, Before&& before) {
    const Slots<T, CAP>        od = ld;
    const Slots<unsigned, CAP> oj = lj;
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        const int  up    = s > 0 ? s - 1 : 0;
        const bool here  = before(od[s], oj[s]);
        const bool above = s > 0 && before(od[up], oj[up]);
        ld[s]            = here ? (above ? od[up] : d) : od[s];
        lj[s]            = here ? (above ? oj[up] : j) : oj[s];
    }
}
// within a wave (j ascends): strictly by d2
template <typename T, int CAP> __device__ __forceinline__ void insert_ascending(Slots<T, CAP>& ld, Slots<unsigned, CAP>& lj, T d, unsigned j) {
    insert_sorted<T, CAP>(ld, lj, d, j, [&](T sd, unsigned) { return d < sd; });
}
// across waves: by (d2, j)
template <typename T, int CAP> __device__ __forceinline__ void insert_by_pair(Slots<T, CAP>& ld, Slots<unsigned, CAP>& lj, T d, unsigned j) {
    insert_sorted<T, CAP>(ld, lj, d, j, [&](T sd, unsigned sj) { return d < sd || (d == sd && j < sj); });
}
// slot `rank` (a run-time value below CAP) through a select chain
template <typename V, int CAP> __device__ __forceinline__ V slot_of(Slots<V, CAP> l, unsigned rank) {
    V v = l[0];
#pragma unroll
    for (int s = 1; s < CAP; ++s) v = rank == static_cast<unsigned>(s) ? l[s] : v;
    return v;
}

struct Densest {
    double   rho;
    unsigned body;
};
__device__ __forceinline__ bool denser(const Densest& a, const Densest& b) { return a.rho > b.rho || (a.rho == b.rho && a.body < b.body); }

template <typename T, int CAP, int S>
__global__ __launch_bounds__(64 * S) void knn_search(const T* pos, unsigned n, unsigned k_count, unsigned* out_index, T* out_d2, T* densities, double* rho_out, KnnTile* tiles) {
    using LT        = Lane<T>;
    using vec       = typename LT::vec;
    using raw4      = typename LT::raw4;
    constexpr int W = LT::W;

    const int      tid       = threadIdx.x;
    const int      wave      = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lane      = tid & 63;
    const unsigned tile_base = blockIdx.x * (64 * W);
    const unsigned last      = k_count - 1;  // the rank of the K-th entry
    BodiesI<T>     me;
    me.load(pos, n, tile_base, lane);

    Slots<T, CAP>        ld[W];
    Slots<unsigned, CAP> lj[W];
    T                    kth[W];
#pragma unroll
    for (int k = 0; k < W; ++k) kth[k] = infinity<T>(), ld[k] = infinity<T>(), lj[k] = kKnnNone;

    // (always inline: a call would put the lists, which it reaches by reference, into memory)
    auto body = [&]<bool MASKED, int UB>(const raw4* b, unsigned j0) __attribute__((always_inline)) {
        vec d2[UB];
        distances<T, MASKED, UB>(b, j0, me, d2);
        bool any = false;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            T least = LT::get(d2[0], k);
#pragma unroll
            for (int u = 1; u < UB; ++u) least = min_of(least, LT::get(d2[u], k));
            any = any || least < kth[k];
        }
        if (__builtin_amdgcn_ballot_w64(any) == 0) return;  // wave-uniform: no lane has a candidate in this group
#pragma unroll
        for (int u = 0; u < UB; ++u) {  // (j ascending)
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const T    d    = LT::get(d2[u], k);
                const bool mine = d < kth[k];
                if (__builtin_amdgcn_ballot_w64(mine) == 0) continue;
                insert_ascending<T, CAP>(ld[k], lj[k], mine ? d : infinity<T>(), j0 + u);
                kth[k] = slot_of<T, CAP>(ld[k], last);
            }
        }
    };
    stream_chunks<T>(pos, n, static_cast<unsigned>(wave), knn_chunks(n), S, tile_base / kKnnChunk, body);

    // merge the S waves' lists pairwise through LDS: at distance `step` wave w + step hands its first K entries to wave w, which inserts
    // them by (d2, j).  The K smallest pairs of a union are the same set in any order of merging.
    if constexpr (S > 1) {
        constexpr int       PER = W * CAP * 64;
        __shared__ T        red_d[(S / 2) * PER];
        __shared__ unsigned red_j[(S / 2) * PER];
#pragma unroll
        for (int step = 1; step < S; step *= 2) {
            const int  slot     = wave / (2 * step);
            const bool sender   = (wave & (2 * step - 1)) == step;
            const bool receiver = (wave & (2 * step - 1)) == 0;
            if (sender) {
#pragma unroll
                for (int k = 0; k < W; ++k) {
#pragma unroll
                    for (int s = 0; s < CAP; ++s) {
                        const int at = slot * PER + (k * CAP + s) * 64 + lane;
                        red_d[at] = ld[k][s], red_j[at] = lj[k][s];
                    }
                }
            }
            __syncthreads();
            if (receiver) {
#pragma unroll 1
                for (unsigned e = 0; e < k_count; ++e) {
#pragma unroll
                    for (int k = 0; k < W; ++k) {
                        const int at = slot * PER + (k * CAP + static_cast<int>(e)) * 64 + lane;
                        insert_by_pair<T, CAP>(ld[k], lj[k], red_d[at], red_j[at]);
                    }
                }
            }
            __syncthreads();  // (the next stage writes the same slots)
        }
    }
    if (wave != 0) return;

    // wave 0: the outputs, rho in double, the tile's record
    const bool with_density = k_count >= 2;
    double     sum_rho = 0.0, sum_x = 0.0, sum_y = 0.0, sum_z = 0.0, min_d2 = infinity<double>(), max_d2 = -infinity<double>();
    Densest    most{-infinity<double>(), kKnnNone};
    unsigned   defined = 0, degenerate = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        if (!me.valid[k]) continue;
        const unsigned i   = me.index[k];
        const size_t   row = static_cast<size_t>(i) * k_count;
#pragma unroll
        for (int s = 0; s < CAP; ++s) {
            if (static_cast<unsigned>(s) < k_count) {
                if (out_index != nullptr) out_index[row + s] = lj[k][s];
                if (out_d2 != nullptr) out_d2[row + s] = ld[k][s];
            }
        }
        if (!with_density) continue;
        const double dk   = static_cast<double>(slot_of<T, CAP>(ld[k], last));
        const double cube = dk * __builtin_sqrt(dk), volume = NB_KNN_SPHERE * cube;
        const bool   good = cube >= 0x1p-1022 && volume < infinity<double>();  // a positive NORMAL cube, a finite volume (fp64: d_K^2 from ~2^-681.3 to ~2^681.2)
        double       mass = 0.0;  // the K - 1 inner neighbours, in rank order
#pragma unroll
        for (int s = 0; s + 1 < CAP; ++s) {
            const unsigned j = lj[k][s];
            if (good && static_cast<unsigned>(s) < last && j < n) mass += static_cast<double>(pos[4 * static_cast<size_t>(j) + 3]);
        }
        const double rho = good ? mass / volume : 0.0;
        rho_out[i]       = rho;
        if (densities != nullptr) densities[i] = static_cast<T>(rho);
        defined += good ? 1u : 0u, degenerate += good ? 0u : 1u;
        if (dk < infinity<double>()) min_d2 = __builtin_fmin(min_d2, dk), max_d2 = __builtin_fmax(max_d2, dk);
        if (denser(Densest{rho, i}, most)) most = Densest{rho, i};
        if (rho != 0.0) {  // (a density defined as 0 adds nothing, wherever the body is)
            sum_rho += rho;
            sum_x += rho * static_cast<double>(LT::get(me.px, k)), sum_y += rho * static_cast<double>(LT::get(me.py, k)), sum_z += rho * static_cast<double>(LT::get(me.pz, k));
        }
    }
    if (!with_density) return;
    // a butterfly over the wave: every lane adds the same two values at every step, so every lane ends with the same bits
#pragma unroll
    for (int step = 1; step < 64; step *= 2) {
        sum_rho += __shfl_xor(sum_rho, step), sum_x += __shfl_xor(sum_x, step), sum_y += __shfl_xor(sum_y, step), sum_z += __shfl_xor(sum_z, step);
        min_d2 = __builtin_fmin(min_d2, __shfl_xor(min_d2, step)), max_d2 = __builtin_fmax(max_d2, __shfl_xor(max_d2, step));
        const Densest other{__shfl_xor(most.rho, step), __shfl_xor(most.body, step)};
        if (denser(other, most)) most = other;
        defined += __shfl_xor(defined, step), degenerate += __shfl_xor(degenerate, step);
    }
    if (lane == 0) tiles[blockIdx.x] = KnnTile{sum_rho, sum_x, sum_y, sum_z, most.rho, min_d2, max_d2, most.body, defined, degenerate, 0u};
}

// ---- the record -----------------------------------------------------------------------------------------------------------------------

// the sum of every lane's `count` doubles over a workgroup of LANES (a power of two), in a fixed order: lane 0 holds it
template <int LANES, int COUNT> __device__ __forceinline__ void fold_sums(double (&v)[COUNT], double* lds) {
    const unsigned tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < COUNT; ++c) lds[c * LANES + tid] = v[c];
    __syncthreads();
#pragma unroll 1
    for (unsigned half = LANES / 2; half > 0; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int c = 0; c < COUNT; ++c) lds[c * LANES + tid] += lds[c * LANES + tid + half];
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < COUNT; ++c) v[c] = lds[c * LANES];
}

__global__ __launch_bounds__(kKnnFold) void knn_centre(const KnnTile* tiles, unsigned count, KnnStructure* head) {
    __shared__ double   lds_sum[4 * kKnnFold];
    __shared__ double   lds_rho[kKnnFold], lds_min[kKnnFold], lds_max[kKnnFold];
    __shared__ unsigned lds_body[kKnnFold], lds_defined[kKnnFold], lds_degenerate[kKnnFold];
    const unsigned      tid = threadIdx.x;
    double              sums[4] = {0.0, 0.0, 0.0, 0.0}, min_d2 = infinity<double>(), max_d2 = -infinity<double>();
    Densest             most{-infinity<double>(), kKnnNone};
    unsigned            defined = 0, degenerate = 0;
    for (unsigned t = tid; t < count; t += kKnnFold) {
        const KnnTile r = tiles[t];
        sums[0] += r.sum_rho, sums[1] += r.sum_x, sums[2] += r.sum_y, sums[3] += r.sum_z;
        min_d2 = __builtin_fmin(min_d2, r.min_d2), max_d2 = __builtin_fmax(max_d2, r.max_d2);
        if (denser(Densest{r.max_rho, r.max_body}, most)) most = Densest{r.max_rho, r.max_body};
        defined += r.defined, degenerate += r.degenerate;
    }
    lds_rho[tid] = most.rho, lds_body[tid] = most.body, lds_min[tid] = min_d2, lds_max[tid] = max_d2, lds_defined[tid] = defined, lds_degenerate[tid] = degenerate;
    fold_sums<kKnnFold, 4>(sums, lds_sum);  // (its first barrier publishes the six arrays above too)
#pragma unroll 1
    for (unsigned half = kKnnFold / 2; half > 0; half >>= 1) {
        if (tid < half) {
            if (denser(Densest{lds_rho[tid + half], lds_body[tid + half]}, Densest{lds_rho[tid], lds_body[tid]})) lds_rho[tid] = lds_rho[tid + half], lds_body[tid] = lds_body[tid + half];
            lds_min[tid] = __builtin_fmin(lds_min[tid], lds_min[tid + half]), lds_max[tid] = __builtin_fmax(lds_max[tid], lds_max[tid + half]);
            lds_defined[tid] += lds_defined[tid + half], lds_degenerate[tid] += lds_degenerate[tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {
        KnnStructure s{};
        const bool   dense = sums[0] > 0.0;
        const double nan   = __builtin_nan("");
        s.sum_density      = sums[0];
        s.centre[0] = dense ? sums[1] / sums[0] : nan, s.centre[1] = dense ? sums[2] / sums[0] : nan, s.centre[2] = dense ? sums[3] / sums[0] : nan;
        s.density_radius = nan, s.core_radius = nan;
        s.max_density = lds_rho[0], s.max_density_body = lds_body[0], s.min_kth_d2 = lds_min[0], s.max_kth_d2 = lds_max[0];
        s.defined = lds_defined[0], s.degenerate = lds_degenerate[0];
        s.flags = (s.degenerate > 0 ? kKnnDegenerate : 0u) | (dense ? 0u : kKnnNoDensity);
        *head = s;
    }
}

template <typename T> __global__ __launch_bounds__(kKnnThreads) void knn_rings(const T* pos, const double* rho, unsigned n, const KnnStructure* head, KnnRing* rings) {
    __shared__ double lds[3 * kKnnThreads];
    const unsigned    i = blockIdx.x * kKnnThreads + threadIdx.x;
    double            v[3] = {0.0, 0.0, 0.0};
    if (i < n) {
        const double r = rho[i];
        if (r != 0.0) {
            const typename Lane<T>::vec4 p  = reinterpret_cast<const typename Lane<T>::vec4*>(pos)[i];
            const double                 ox = static_cast<double>(p.x) - head->centre[0], oy = static_cast<double>(p.y) - head->centre[1], oz = static_cast<double>(p.z) - head->centre[2];
            const double                 r2 = ox * ox + oy * oy + oz * oz;  // (from the centre, in double: not a d2(i, j))
            v[0] = r * __builtin_sqrt(r2), v[1] = (r * r) * r2, v[2] = r * r;
        }
    }
    fold_sums<kKnnThreads, 3>(v, lds);
    if (threadIdx.x == 0) rings[blockIdx.x] = KnnRing{v[0], v[1], v[2]};
}

__global__ __launch_bounds__(kKnnFold) void knn_record(const KnnRing* rings, unsigned count, const KnnStructure* head, KnnStructure* structure) {
    __shared__ double lds[3 * kKnnFold];
    double            v[3] = {0.0, 0.0, 0.0};
    for (unsigned b = threadIdx.x; b < count; b += kKnnFold) {
        const KnnRing r = rings[b];
        v[0] += r.first, v[1] += r.second, v[2] += r.weight;
    }
    fold_sums<kKnnFold, 3>(v, lds);
    if (threadIdx.x == 0) {
        KnnStructure s{};  // (field by field: a copy of the whole record goes through private memory)
        const bool   dense = (head->flags & kKnnNoDensity) == 0;
        s.sum_density = head->sum_density, s.centre[0] = head->centre[0], s.centre[1] = head->centre[1], s.centre[2] = head->centre[2];
        s.density_radius = dense ? v[0] / head->sum_density : head->density_radius, s.core_radius = dense ? __builtin_sqrt(v[1] / v[2]) : head->core_radius;
        s.max_density = head->max_density, s.min_kth_d2 = head->min_kth_d2, s.max_kth_d2 = head->max_kth_d2;
        s.max_density_body = head->max_density_body, s.defined = head->defined, s.degenerate = head->degenerate, s.flags = head->flags;
        *structure = s;
    }
}

template <typename T, int CAP, int S> hipError_t launch_search_s(const KnnArgs<T>& a, unsigned groups, hipStream_t stream) {
    hipLaunchKernelGGL((knn_search<T, CAP, S>), dim3(groups), dim3(64 * S), 0, stream, a.pos, a.n, a.k, a.index, a.dist_sq, a.densities, a.rho, a.tiles);
    return hipGetLastError();
}
template <typename T, int CAP> hipError_t launch_search_cap(const KnnArgs<T>& a, unsigned groups, hipStream_t stream) {
    switch (knn_waves(a.n)) {
        case 1: return launch_search_s<T, CAP, 1>(a, groups, stream);
        case 2: return launch_search_s<T, CAP, 2>(a, groups, stream);
        case 4: return launch_search_s<T, CAP, 4>(a, groups, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

template <typename T> hipError_t launch_knn_survey(const KnnArgs<T>& a, hipStream_t stream) {
    const unsigned groups = knn_tiles(a.n, 64 * Lane<T>::W), blocks = knn_blocks(a.n);
    (void)hipGetLastError();
    hipError_t err = hipErrorInvalidValue;
    switch (knn_capacity(a.k)) {
        case 4: err = launch_search_cap<T, 4>(a, groups, stream); break;
        case 8: err = launch_search_cap<T, 8>(a, groups, stream); break;
        case 16: err = launch_search_cap<T, 16>(a, groups, stream); break;
        default: break;
    }
    if (err != hipSuccess || a.structure == nullptr) return err;
    hipLaunchKernelGGL(knn_centre, dim3(1), dim3(kKnnFold), 0, stream, static_cast<const KnnTile*>(a.tiles), groups, a.head);
    if (err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL((knn_rings<T>), dim3(blocks), dim3(kKnnThreads), 0, stream, a.pos, static_cast<const double*>(a.rho), a.n, static_cast<const KnnStructure*>(a.head), a.rings);
    if (err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL(knn_record, dim3(1), dim3(kKnnFold), 0, stream, static_cast<const KnnRing*>(a.rings), blocks, static_cast<const KnnStructure*>(a.head), a.structure);
    return hipGetLastError();
}

template hipError_t launch_knn_survey<float>(const KnnArgs<float>&, hipStream_t);
template hipError_t launch_knn_survey<double>(const KnnArgs<double>&, hipStream_t);

}  // namespace nb
