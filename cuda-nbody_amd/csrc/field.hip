// field.hip -- the kernels of libnbody_hip_field.so (include/nbody_hip_field.h): acceleration, jerk and potential of N sources at M
// points of the caller's own.  gfx950 only; FMA contraction on.
//
// field_eval<T, S, JERK> is on the wave-stream plan (wave_stream.h: a lane holds one vector of targets -- fp32: a packed pair ->
// v_pk_*_f32; fp64: one --, the sources are wave-uniform, come in through scalar loads U at a time, one group ahead, two register sets,
// and enter the packed subtractions as scalar operands) with hermite_block_eval's division of work: a workgroup owns one tile of 64 W
// targets and one of J contiguous ranges of the chunks of 128 sources; its S waves split the range's chunks (chunk c of the range ->
// wave c mod S) and fold through LDS in wave order.  No LDS access and no barrier inside the streaming loops, no atomics anywhere, no
// scratch, <= 128 VGPRs.  The streaming of a chunk's groups (wave_groups.inc), SIMD-mate priority (wave_mates.inc) and the fold
// (wave_fold.inc) are the text hermite_stream.inc includes; the interaction and the chunk loop (mask form, no unit form) are this
// kernel's own.  field_finish adds the J ranges' planes with hermite_block_finish's text (range_sum.inc).
//
// Per interaction, r = x_j - p, w = v_j - u, s2 = r.r + eps2, k = m_j s^-3:
//     a += k r,   jerk += k (w - 3 (r.w) s^-2 r),   phi_sum += m_j s^-1        (phi = -phi_sum, at the store)
// The raw mass multiplies in the loop: there is no "unit" form here, because a result must not depend on what the OTHER sources of a
// chunk weigh (exclusion is "mass 0", bit for bit).  fp32, per packed pair: 13 v_pk_* + 2 v_rsq_f32 without the jerk, 27 + 2 with it.
//
// Exclusion.  A lane holds self_index of its targets.  Per chunk the wave decides, uniformly, whether any of them lies inside the
// chunk; only then it runs the MASK form of the loop, in which the mass is a vector, selected per target (0 where j == self_index).
// Every other chunk runs the plain form, whose mass is the scalar operand.  m * s^-3 and fma(s^-1, m, sum) round the same from a
// scalar or a vector register, so both forms give the same bits for a pair that is not excluded.
//
// Sums.  A register sum collects at most 8 chunks (1 024 sources), then is added to the lane's second-level sum; the S waves' sums and
// the J ranges' sums are added in wave and in range order.  The order depends on (N, M, precision) alone.
#include "field_kernels.h"

namespace nb {
namespace {

#include "nbody_lane.h"

#include "hermite_stream.h"

// s^-1, s^-2 and s^-3 from s2: hermite_stream.h's Powers and the first power beside them.  fp32: v_rsq_f32 (1 ulp) and two products; s^-1
// is the v_rsq result itself.  fp64: s^-2 and s^-3 as Powers<double> (the v_rsq_f64 seed and the series of Lane<double>::coupling), and
// s^-1 = s2 s^-3: one product and one more rounding, where a series of its own would hold another constant in registers (with it the
// S > 1 jerk kernels went 12 bytes into scratch).
template <typename T> struct FieldPowers;
template <> struct FieldPowers<float> {
    using vec = Lane<float>::vec;
    static __device__ __forceinline__ void of(vec s2, const Lane<float>::Consts&, vec& inv, vec& inv2, vec& inv3) {
        inv  = vec{__builtin_amdgcn_rsqf(s2.x), __builtin_amdgcn_rsqf(s2.y)};
        inv2 = inv * inv;
        inv3 = inv * inv2;
    }
};
template <> struct FieldPowers<double> {
    static __device__ __forceinline__ void of(double s2, const Lane<double>::Consts& k, double& inv, double& inv2, double& inv3) {
        Powers<double>::of(s2, k, inv2, inv3);
        inv = s2 * inv3;
    }
};

// the mass of source j as target(s) of this lane see it: 0 for the one whose self_index is j
template <typename T> struct Masked;
template <> struct Masked<float> {
    static __device__ __forceinline__ v2f mass(float m, unsigned j, const unsigned (&self)[2]) { return v2f{self[0] == j ? 0.0f : m, self[1] == j ? 0.0f : m}; }
};
template <> struct Masked<double> {
    static __device__ __forceinline__ double mass(double m, unsigned j, const unsigned (&self)[1]) { return self[0] == j ? 0.0 : m; }
};

// sums of a lane: 0 1 2 = a, 3 = sum of m / s, 4 5 6 = jerk
template <bool JERK> constexpr int sums_of() { return JERK ? 7 : 4; }

template <typename T, int S, bool JERK>
__global__ __launch_bounds__(64 * S) __attribute__((amdgpu_waves_per_eu(4, 4))) void field_eval(FieldArgs<T> a, unsigned ranges) {
    using LT          = Lane<T>;
    using vec4        = typename LT::vec4;
    using vec         = typename LT::vec;
    using raw4        = typename LT::raw4;
    constexpr int W   = LT::W;  // targets per lane
    constexpr int U   = unroll_for<T>();
    constexpr int CH  = kChunk;
    constexpr int NS  = sums_of<JERK>();
    static_assert(CH % U == 0, "the streaming loop is unrolled by U");
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx4/x8/x16

    const stream_ptr jp   = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(a.src));
    const stream_ptr jv   = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(a.src_vel));
    const unsigned   n    = a.n;
    const unsigned   m    = a.m;
    const int        tid  = threadIdx.x;
    const int        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int        lane = tid & 63;
    const unsigned   tile  = blockIdx.x / ranges;
    const unsigned   range = blockIdx.x % ranges;

    // targets of this lane: tile_base + k*64 + lane (coalesced across the lanes of a wave); a lane past M holds the last target
    const unsigned tile_base = tile * (64 * W);
    vec            px, py, pz, vx, vy, vz;
    unsigned       self[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned local = tile_base + k * 64 + lane;
        const size_t   i     = local < m ? local : m - 1;
        const vec4     p     = reinterpret_cast<const vec4*>(a.tgt)[i];
        LT::set(px, k, p.x), LT::set(py, k, p.y), LT::set(pz, k, p.z);
        if constexpr (JERK) {
            const vec4 v = reinterpret_cast<const vec4*>(a.tgt_vel)[i];
            LT::set(vx, k, v.x), LT::set(vy, k, v.y), LT::set(vz, k, v.z);
        }
        self[k] = a.self != nullptr ? a.self[i] : kFieldNone;
    }
    vec eps2 = LT::splat(a.eps2);
    LT::keep_in_vgpr(eps2);
    const vec                 minus3 = LT::splat(T(-3));
    const typename LT::Consts consts = LT::make_consts();

    vec first[NS], second[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) first[q] = second[q] = LT::splat(0);

    // the range's chunks: [c_lo, c_hi), never empty (J <= n_chunks / S)
    const unsigned n_chunks = stream_chunks(n);
    const unsigned c_lo     = static_cast<unsigned>(static_cast<unsigned long long>(range) * n_chunks / ranges);
    const unsigned c_hi     = static_cast<unsigned>(static_cast<unsigned long long>(range + 1) * n_chunks / ranges);

    // does a self_index of this wave lie in sources [first_j, first_j + count)?  (NB_FIELD_NONE never does: first_j <= 2^26)
    auto chunk_has_self = [&](unsigned first_j, unsigned count) -> bool {
        bool hit = false;
#pragma unroll
        for (int k = 0; k < W; ++k) hit = hit || (self[k] - first_j) < count;
        return __builtin_amdgcn_ballot_w64(hit) != 0;
    };
    auto group = [&](size_t j0, BodyJ<T> (&b)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            b[u].p = jp[j0 + u];
            if constexpr (JERK) b[u].v = jv[j0 + u];
        }
    };

    // UB sources (the first is source j0) against the lane's vector of targets, written stage by stage: UB independent chains in flight
    auto compute = [&]<bool MASK, int UB>(const BodyJ<T>* b, unsigned j0, vec (&sum)[NS]) {
        vec dx[UB], dy[UB], dz[UB], ex[UB], ey[UB], ez[UB], s2[UB], rv[UB], k3[UB], k1[UB], mass[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            dx[u] = LT::splat(b[u].p.x) - px, dy[u] = LT::splat(b[u].p.y) - py, dz[u] = LT::splat(b[u].p.z) - pz;
            if constexpr (JERK) ex[u] = LT::splat(b[u].v.x) - vx, ey[u] = LT::splat(b[u].v.y) - vy, ez[u] = LT::splat(b[u].v.z) - vz;
            if constexpr (MASK) mass[u] = Masked<T>::mass(b[u].p.w, j0 + u, self);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            s2[u] = LT::fma(dx[u], dx[u], eps2);
            if constexpr (JERK) rv[u] = dx[u] * ex[u];
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            s2[u] = LT::fma(dy[u], dy[u], s2[u]);
            if constexpr (JERK) rv[u] = LT::fma(dy[u], ey[u], rv[u]);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            s2[u] = LT::fma(dz[u], dz[u], s2[u]);
            if constexpr (JERK) rv[u] = LT::fma(dz[u], ez[u], rv[u]);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            vec inv2;
            FieldPowers<T>::of(s2[u], consts, k1[u], inv2, k3[u]);
            if constexpr (JERK) rv[u] = (rv[u] * inv2) * minus3;  // -3 (r.w) / s^2
            if constexpr (MASK) {
                k3[u] = k3[u] * mass[u];
            } else {
                k3[u] = k3[u] * LT::splat(b[u].p.w);
            }
        }
        if constexpr (JERK) {
#pragma unroll
            for (int u = 0; u < UB; ++u) ex[u] = LT::fma(rv[u], dx[u], ex[u]), ey[u] = LT::fma(rv[u], dy[u], ey[u]), ez[u] = LT::fma(rv[u], dz[u], ez[u]);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            sum[0] = LT::fma(dx[u], k3[u], sum[0]), sum[1] = LT::fma(dy[u], k3[u], sum[1]), sum[2] = LT::fma(dz[u], k3[u], sum[2]);
            if constexpr (MASK) {
                sum[3] = LT::fma(k1[u], mass[u], sum[3]);
            } else {
                sum[3] = LT::fma(k1[u], LT::splat(b[u].p.w), sum[3]);
            }
            if constexpr (JERK) sum[4] = LT::fma(ex[u], k3[u], sum[4]), sum[5] = LT::fma(ey[u], k3[u], sum[5]), sum[6] = LT::fma(ez[u], k3[u], sum[6]);
        }
    };
#include "wave_groups.inc"
    auto flush = [&]() {
#pragma unroll
        for (int q = 0; q < NS; ++q) second[q] = second[q] + first[q], first[q] = LT::splat(0);
    };

#define WAVE_MATES_SETUP
#include "wave_mates.inc"

    unsigned c    = c_lo + wave;  // wave w streams chunks c_lo + w, c_lo + w + S, ...
    unsigned held = 0;            // chunks in `first`
    BodyJ<T> b0[U], b1[U];
    if (c < c_hi && n - c * CH >= static_cast<unsigned>(U)) group(static_cast<size_t>(c) * CH, b0);
    for (; c < c_hi; c += S) {
#define WAVE_MATES_CHUNK
#include "wave_mates.inc"
        const unsigned first_j = c * CH;
        const unsigned count   = min(static_cast<unsigned>(CH), n - first_j);
        const unsigned groups  = count / U;
        // the wave's next chunk, when it has a whole group (else anything readable: the set is not used again)
        const size_t next   = ((c + S) < c_hi && n - (first_j + S * CH) >= static_cast<unsigned>(U)) ? static_cast<size_t>(first_j) + S * CH : first_j;
        const bool   masked = chunk_has_self(first_j, count);
        if (held == kFlushEvery) flush(), held = 0;
        if (groups > 0) {
            if (masked) {
                stream.template operator()<true>(first_j, groups, next, b0, b1);
            } else {
                stream.template operator()<false>(first_j, groups, next, b0, b1);
            }
        }
#pragma unroll 1
        for (unsigned jj = groups * U; jj < count; ++jj) {  // ragged end of the last chunk
            BodyJ<T> one[1];
            one[0].p = jp[static_cast<size_t>(first_j) + jj];
            if constexpr (JERK) one[0].v = jv[static_cast<size_t>(first_j) + jj];
            compute.template operator()<true, 1>(one, first_j + jj, first);
        }
        ++held;
#define WAVE_MATES_DONE
#include "wave_mates.inc"
    }
#define WAVE_MATES_LEAVE
#include "wave_mates.inc"
    flush();

#include "wave_fold.inc"

    if (ranges > 1) {
        // planes [J][NS][slots]: word (range, q, slot), coalesced across the wave; the slots past M of the last tile hold a copy of the last target's sums
        const size_t slots = static_cast<size_t>(gridDim.x / ranges) * (64 * W);
#pragma unroll
        for (int q = 0; q < NS; ++q) {
#pragma unroll
            for (int k = 0; k < W; ++k) a.partial[(static_cast<size_t>(range) * NS + q) * slots + tile_base + k * 64 + lane] = LT::get(second[q], k);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned local = tile_base + k * 64 + lane;
        if (local >= m) continue;
        const size_t i = local;
        if (a.acc != nullptr) {
            vec4 a1;
            a1.x = LT::get(second[0], k), a1.y = LT::get(second[1], k), a1.z = LT::get(second[2], k), a1.w = 0;
            reinterpret_cast<vec4*>(a.acc)[i] = a1;
        }
        if constexpr (JERK) {
            vec4 j1;
            j1.x = LT::get(second[4], k), j1.y = LT::get(second[5], k), j1.z = LT::get(second[6], k), j1.w = 0;
            reinterpret_cast<vec4*>(a.jerk)[i] = j1;
        }
        if (a.pot != nullptr) a.pot[i] = -LT::get(second[3], k);
    }
}

// one lane per target: the J ranges' partial sums in range order (range_sum.inc)
template <typename T, bool JERK> __global__ __launch_bounds__(256) void field_finish(FieldArgs<T> a, unsigned ranges, unsigned tiles) {
    using vec4         = typename Lane<T>::vec4;
    constexpr int NS   = sums_of<JERK>();
    const unsigned slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= a.m) return;
    const size_t slots = static_cast<size_t>(tiles) * (64 * Lane<T>::W);
    const T* const partial = a.partial;
#include "range_sum.inc"
    if (a.acc != nullptr) {
        vec4 a1;
        a1.x = sum[0], a1.y = sum[1], a1.z = sum[2], a1.w = 0;
        reinterpret_cast<vec4*>(a.acc)[slot] = a1;
    }
    if constexpr (JERK) {
        vec4 j1;
        j1.x = sum[4], j1.y = sum[5], j1.z = sum[6], j1.w = 0;
        reinterpret_cast<vec4*>(a.jerk)[slot] = j1;
    }
    if (a.pot != nullptr) a.pot[slot] = -sum[3];
}

template <typename T, bool JERK> hipError_t launch_planned(const FieldArgs<T>& a, hipStream_t stream) {
    const FieldGeom g = field_geometry(a.n, a.m, 64 * Lane<T>::W);
    return with_stream_waves(g.waves, [&](auto waves) {
        constexpr int S = decltype(waves)::value;
        (void)hipGetLastError();  // a launch reports ITS OWN error
        hipLaunchKernelGGL((field_eval<T, S, JERK>), dim3(g.tiles * g.ranges), dim3(64 * S), 0, stream, a, g.ranges);
        if (const auto err = hipGetLastError(); err != hipSuccess || g.ranges == 1) return err;
        hipLaunchKernelGGL((field_finish<T, JERK>), dim3((a.m + kFieldThreads - 1) / kFieldThreads), dim3(kFieldThreads), 0, stream, a, g.ranges, g.tiles);
        return hipGetLastError();
    });
}

}  // namespace

template <typename T> hipError_t launch_field_eval(const FieldArgs<T>& a, hipStream_t stream) {
    return a.jerk != nullptr ? launch_planned<T, true>(a, stream) : launch_planned<T, false>(a, stream);
}

template hipError_t launch_field_eval<float>(const FieldArgs<float>&, hipStream_t);
template hipError_t launch_field_eval<double>(const FieldArgs<double>&, hipStream_t);

}  // namespace nb
