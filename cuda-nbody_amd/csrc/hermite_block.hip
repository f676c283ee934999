// hermite_block.hip -- the kernels of libnbody_hip_hermite_block.so (include/nbody_hip_hermite_block.h): 4th-order Hermite steps with
// block time steps.  gfx950 only; FMA contraction on.
//
// One block step is six launches, no atomics, every word written by one lane:
//   block_min_partial    per workgroup, the minimum of tick + ticks(level) (and the deepest level held)
//   block_predict_count  every workgroup folds those partials (<= 1 024) to `now`; workgroup 0 records it, decides about t_stop and
//                        writes the flag; every body is predicted to `now` into the workspace; active bodies are counted per workgroup
//   block_scan           ONE workgroup: exclusive prefix of the counts in index order, n_act, the status counters
//   block_scatter        the active list, ascending body index
//   hermite_block_eval   the hot path, see below
//   hermite_block_finish one lane per active slot: J partials in index order, corrector, dt_A, new level, the body's stored state
// A step that would pass t_stop leaves go = 0 in the control record and the four launches after it return at once.
//
// hermite_block_eval<T, S> has hermite_eval's streaming loops (one text, hermite_stream.inc with wave_groups.inc, wave_mates.inc and
// wave_fold.inc inside it: bodies j by scalar loads U at a time into two register sets, unit / mixed forms, two-level sums, SIMD-mate
// priority, the fold; 25 / 26 v_pk_* + 2 v_rsq_f32 per packed pair, no LDS, barrier or scratch inside the loops) around another
// distribution of work: a workgroup owns one tile of 64 W ACTIVE bodies, gathered through the active list from the predicted state, and
// one of J contiguous ranges of the chunks of bodies j.  Its S waves split the range's chunks (chunk c of the range -> wave c mod S), fold
// through LDS in wave order, and wave 0 stores six partial sums per body, in units of the reference mass, to the planes
// [J][6][tiles 64 W].  (tile, range) come from n_act, which the workgroup reads from the control record: the launch grid is sized for the
// worst n_act of this N and the workgroups beyond tiles J leave.  The kernel below is the active list, the tile / range derivation
// (stream_geometry, wave_stream.h), the include, and the plane store.  hermite_block_finish adds the planes (range_sum.inc) and corrects
// (hermite_correct.inc); the predictor of block_predict_count and block_sync is hermite_body.h's.
#include "hermite_block_kernels.h"

namespace nb {
namespace {

#include "nbody_lane.h"

#include "hermite_stream.h"

#include "hermite_body.h"

#include "hermite_block_kernels_shared.h"

template <typename T, int S>
__global__ __launch_bounds__(64 * S) __attribute__((amdgpu_waves_per_eu(4, 4))) void hermite_block_eval(const T* state8, const unsigned* active, const BlockCtrl* ctrl, T* partial,
                                                                                                       unsigned n, T eps2_in) {
    using LT         = Lane<T>;
    using vec4       = typename LT::vec4;
    using vec        = typename LT::vec;
    using raw4       = typename LT::raw4;
    using bits       = typename LT::bits;
    constexpr int W      = LT::W;  // bodies i per lane
    constexpr int U      = unroll_for<T>();
    constexpr int STRIDE = 2;  // vec4 per body of state8
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx8 / x16

    if (ctrl->go == 0) return;
    const unsigned  n_act = ctrl->n_act;
    const BlockGeom geom  = stream_geometry(n, n_act, 64 * W, kBlockTarget);
    if (blockIdx.x >= geom.tiles * geom.ranges) return;
    const unsigned ranges = geom.ranges;
    const unsigned tile   = blockIdx.x / ranges;
    const unsigned range  = blockIdx.x % ranges;
    const unsigned slots  = geom.tiles * (64 * W);

    const T* const   pos_base = state8;
    const stream_ptr jp   = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(state8));
    const int        tid  = threadIdx.x;
    const int        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int        lane = tid & 63;

    // bodies i of this lane: slots tile_base + k*64 + lane of the active list
    const unsigned tile_base = tile * (64 * W);
    vec            px, py, pz, vx, vy, vz;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned slot = tile_base + k * 64 + lane;
        const size_t   i    = active[slot < n_act ? slot : n_act - 1];
        const vec4     p    = reinterpret_cast<const vec4*>(state8)[2 * i];
        const vec4     v    = reinterpret_cast<const vec4*>(state8)[2 * i + 1];
        LT::set(px, k, p.x), LT::set(py, k, p.y), LT::set(pz, k, p.z);
        LT::set(vx, k, v.x), LT::set(vy, k, v.y), LT::set(vz, k, v.z);
    }
    vec eps2 = LT::splat(eps2_in);
    LT::keep_in_vgpr(eps2);

    auto body_j = [&](size_t j, BodyJ<T>& b) { b.p = jp[2 * j], b.v = jp[2 * j + 1]; };  // adjacent: one s_load_dwordx8 / x16
#define HERMITE_STREAM_UNIT_SUMS  // the partial planes are in units of the reference mass; the finish kernel multiplies
#include "hermite_stream.inc"

    // planes [J][6][slots]: word (range, q, slot), coalesced across the wave; the slots past n_act of the last tile hold a copy of the last body's sums
#pragma unroll
    for (int q = 0; q < 6; ++q) {
#pragma unroll
        for (int k = 0; k < W; ++k) partial[(static_cast<size_t>(range) * 6 + q) * slots + tile_base + k * 64 + lane] = LT::get(second[q], k);
    }
}

// ---- the schedule ---------------------------------------------------------------------------------------------------------------------

#include "hermite_block_schedule.inc"  // block_min_partial, block_scan, block_scatter: one text with hermite6_block.hip

template <typename T> __global__ __launch_bounds__(256) void block_predict_count(BlockArgs<T> a, unsigned partials) {
    using vec4 = typename Lane<T>::vec4;
    __shared__ unsigned long long lds_next[256];
    __shared__ int                lds_level[256];
    __shared__ unsigned           wave_count[4];
    MinLevel                      m{~0ull, 0};
    for (unsigned i = threadIdx.x; i < partials; i += 256u) {
        const unsigned long long next = a.min_part[i];
        const int                k    = a.lvl_part[i];
        if (next < m.next) m.next = next;
        if (k > m.level) m.level = k;
    }
    m                            = block_fold(m, lds_next, lds_level);
    const unsigned long long now = m.next;
    const double             q   = tick_length(a.p);
    const bool               go  = static_cast<double>(now) * q <= a.t_stop;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctrl->now = now, a.ctrl->go = go ? 1u : 0u;
        if (!go) a.ctrl->n_act = 0;
        const unsigned flags    = a.status->flags;
        a.status->flags         = go ? (flags & ~kBlockStopped) : (flags | kBlockStopped);
        const int deepest       = a.status->deepest_level;
        a.status->deepest_level = m.level > deepest ? m.level : deepest;
    }
    if (!go) return;
    const unsigned i      = blockIdx.x * 256u + threadIdx.x;
    bool           active = false;
    if (i < a.n) {
        const unsigned long long tick = a.ticks[i];
        active                        = tick + ticks_of(a.levels[i], a.p.max_level) == now;
        const T                  dt   = static_cast<T>(static_cast<double>(now - tick) * q);
        const vec4 x = reinterpret_cast<const vec4*>(a.pos)[i], v = reinterpret_cast<const vec4*>(a.vel)[i];
        const vec4 acc = reinterpret_cast<const vec4*>(a.acc)[i], jerk = reinterpret_cast<const vec4*>(a.jerk)[i];
        vec4       xp, vp;
        predict_body<T>(x, v, acc, jerk, dt, xp, vp);
        reinterpret_cast<vec4*>(a.state8)[2 * static_cast<size_t>(i)]     = xp;
        reinterpret_cast<vec4*>(a.state8)[2 * static_cast<size_t>(i) + 1] = vp;
    }
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(active);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = static_cast<unsigned>(__builtin_popcountll(mask));
    __syncthreads();
    if (threadIdx.x == 0) a.counts[blockIdx.x] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

template <typename T> __global__ __launch_bounds__(256) void hermite_block_finish(BlockArgs<T> a) {
    using vec4 = typename Lane<T>::vec4;
    constexpr unsigned per_tile = 64 * Lane<T>::W;
    if (a.ctrl->go == 0) return;
    const unsigned n_act = a.ctrl->n_act;
    const unsigned slot  = blockIdx.x * 256u + threadIdx.x;
    if (slot >= n_act) return;
    const BlockGeom          geom  = stream_geometry(a.n, n_act, per_tile, kBlockTarget);
    const size_t             slots = static_cast<size_t>(geom.tiles) * per_tile;
    const unsigned long long now   = a.ctrl->now;
    const size_t             i     = a.active[slot];
    // sum[6]: the J ranges' partial sums of this slot, in range order
    constexpr int            NS      = 6;
    const T* const           partial = a.partial;
    const unsigned           ranges  = geom.ranges;
#include "range_sum.inc"
    const T m_first = a.state8[3];
    const T m_ref   = usable_unit(m_first) ? m_first : T(1);
    vec4    a1, j1;
    a1.x = sum[0] * m_ref, a1.y = sum[1] * m_ref, a1.z = sum[2] * m_ref, a1.w = 0;
    j1.x = sum[3] * m_ref, j1.y = sum[4] * m_ref, j1.z = sum[5] * m_ref, j1.w = 0;

    int                      k     = a.levels[i];
    k                              = k < 0 ? 0 : (k > a.p.max_level ? a.p.max_level : k);
    const double             q     = tick_length(a.p);
    const unsigned long long own   = 1ull << (a.p.max_level - k);
    const double             dt_i  = static_cast<double>(own) * q;
    const T                  dt    = static_cast<T>(dt_i);
    // the corrector of nb_hermite_step_*, with the body's own dt
    const vec4 x  = reinterpret_cast<const vec4*>(a.pos)[i];
    vec4       v  = reinterpret_cast<const vec4*>(a.vel)[i];
    const vec4 a0 = reinterpret_cast<const vec4*>(a.acc)[i];
    const vec4 j0 = reinterpret_cast<const vec4*>(a.jerk)[i];
#include "hermite_correct.inc"
    reinterpret_cast<vec4*>(a.pos)[i]  = x1;
    reinterpret_cast<vec4*>(a.vel)[i]  = v;
    reinterpret_cast<vec4*>(a.acc)[i]  = a1;
    reinterpret_cast<vec4*>(a.jerk)[i] = j1;

    const double dt_a = aarseth_dt(a0, j0, a1, j1, dt_i, a.p.eta, a.p.dt_max);
    if (dt_a < dt_i) {
        while (k < a.p.max_level && static_cast<double>(1ull << (a.p.max_level - k)) * q > dt_a) ++k;
    } else if (dt_a >= 2.0 * dt_i && k > 0 && now % (2 * own) == 0) {
        --k;
    }
    a.levels[i] = k;
    a.ticks[i]  = now;
}

// init: levels from the accelerations and jerks nb_hermite_eval left, ticks 0, the status record cleared
template <typename T> __global__ __launch_bounds__(256) void block_init_levels(BlockArgs<T> a) {
    using vec4       = typename Lane<T>::vec4;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) {
        BlockStatus s{};
        *a.status = s;
        BlockCtrl c{};
        *a.ctrl = c;
    }
    if (i >= a.n) return;
    const vec4   acc = reinterpret_cast<const vec4*>(a.acc)[i], jerk = reinterpret_cast<const vec4*>(a.jerk)[i];
    const double want0 = a.p.eta_start * norm3(acc.x, acc.y, acc.z) / norm3(jerk.x, jerk.y, jerk.z);
    const double want  = (want0 == want0 && want0 - want0 == 0 && want0 > 0) ? want0 : a.p.dt_max;
    const double q     = tick_length(a.p);
    int          k     = 0;
    while (k < a.p.max_level && static_cast<double>(1ull << (a.p.max_level - k)) * q > want) ++k;
    a.levels[i] = k;
    a.ticks[i]  = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void block_sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const unsigned long long* ticks,
                                                  const BlockStatus* status, unsigned n, BlockParams p) {
    using vec4       = typename Lane<T>::vec4;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned long long now = status->now_ticks, tick = ticks[i];
    const T                  dt  = static_cast<T>(static_cast<double>(now > tick ? now - tick : 0ull) * tick_length(p));
    const vec4 x = reinterpret_cast<const vec4*>(pos)[i], v = reinterpret_cast<const vec4*>(vel)[i];
    vec4       xp, vp;
    predict_body<T>(x, v, reinterpret_cast<const vec4*>(acc)[i], reinterpret_cast<const vec4*>(jerk)[i], dt, xp, vp);
    vp.w                                 = v.w;
    reinterpret_cast<vec4*>(pos_out)[i] = xp;
    reinterpret_cast<vec4*>(vel_out)[i] = vp;
}

template <typename T, int S> hipError_t launch_eval_s(const BlockArgs<T>& a, unsigned groups, hipStream_t stream) {
    hipLaunchKernelGGL((hermite_block_eval<T, S>), dim3(groups), dim3(64 * S), 0, stream, static_cast<const T*>(a.state8), static_cast<const unsigned*>(a.active),
                       static_cast<const BlockCtrl*>(a.ctrl), a.partial, a.n, a.eps2);
    return hipGetLastError();
}

}  // namespace

template <typename T> hipError_t launch_block_init(const BlockArgs<T>& a, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((block_init_levels<T>), dim3((a.n + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <typename T> hipError_t launch_block_step(const BlockArgs<T>& a, hipStream_t stream) {
    constexpr unsigned per_tile = 64 * Lane<T>::W;
    const unsigned     blocks   = (a.n + 255u) / 256u;
    const unsigned     partials = blocks < kBlockMinPartials ? blocks : kBlockMinPartials;
    (void)hipGetLastError();
    hipLaunchKernelGGL(block_min_partial, dim3(partials), dim3(256), 0, stream, static_cast<const unsigned long long*>(a.ticks), static_cast<const int*>(a.levels), a.n,
                       a.p.max_level, a.min_part, a.lvl_part);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL((block_predict_count<T>), dim3(blocks), dim3(256), 0, stream, a, partials);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL(block_scan, dim3(1), dim3(1024), 0, stream, a.counts, blocks, a.ctrl, a.status);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL(block_scatter, dim3(blocks), dim3(256), 0, stream, static_cast<const unsigned long long*>(a.ticks), static_cast<const int*>(a.levels),
                       static_cast<const unsigned*>(a.counts), static_cast<const BlockCtrl*>(a.ctrl), a.active, a.n, a.p.max_level);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    const unsigned groups = block_launch_groups(a.n, per_tile);
    hipError_t     err    = hipErrorInvalidValue;
    switch (block_waves(a.n)) {
        case 1: err = launch_eval_s<T, 1>(a, groups, stream); break;
        case 2: err = launch_eval_s<T, 2>(a, groups, stream); break;
        case 4: err = launch_eval_s<T, 4>(a, groups, stream); break;
        case 8: err = launch_eval_s<T, 8>(a, groups, stream); break;
        default: break;
    }
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((hermite_block_finish<T>), dim3(blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_block_sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const unsigned long long* ticks, const BlockStatus* status, unsigned n,
                             const BlockParams& p, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((block_sync<T>), dim3((n + 255u) / 256u), dim3(256), 0, stream, pos_out, vel_out, pos, vel, acc, jerk, ticks, status, n, p);
    return hipGetLastError();
}

template hipError_t launch_block_init<float>(const BlockArgs<float>&, hipStream_t);
template hipError_t launch_block_init<double>(const BlockArgs<double>&, hipStream_t);
template hipError_t launch_block_step<float>(const BlockArgs<float>&, hipStream_t);
template hipError_t launch_block_step<double>(const BlockArgs<double>&, hipStream_t);
template hipError_t launch_block_sync<float>(float*, float*, const float*, const float*, const float*, const float*, const unsigned long long*, const BlockStatus*, unsigned,
                                             const BlockParams&, hipStream_t);
template hipError_t launch_block_sync<double>(double*, double*, const double*, const double*, const double*, const double*, const unsigned long long*, const BlockStatus*, unsigned,
                                              const BlockParams&, hipStream_t);

}  // namespace nb
