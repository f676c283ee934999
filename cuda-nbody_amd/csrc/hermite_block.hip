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
// (hermite_correct.inc); the predictor of block_predict_count and block_sync is hermite_body.h's.  What these kernels share with
// hermite6_block.hip and hermite_block_ensemble.hip around that arithmetic is hermite_block_parts.inc and hermite_block_kernels_shared.h.
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
    using bits       = typename LT::bits;
    constexpr int W      = LT::W;  // bodies i per lane
    constexpr int U      = unroll_for<T>();
    constexpr int STRIDE = 2;  // vec4 per body of state8
    const unsigned local = blockIdx.x;
    const T* const state = state8;
#define BLOCK_PART_EVAL_HEAD
#include "hermite_block_parts.inc"
#define BLOCK_PART_EVAL_BODIES
#include "hermite_block_parts.inc"
    vec eps2 = LT::splat(eps2_in);
    LT::keep_in_vgpr(eps2);

    auto body_j = [&](size_t j, BodyJ<T>& b) { b.p = jp[2 * j], b.v = jp[2 * j + 1]; };  // adjacent: one s_load_dwordx8 / x16
#define HERMITE_STREAM_UNIT_SUMS  // the partial planes are in units of the reference mass; the finish kernel multiplies
#include "hermite_stream.inc"
#define BLOCK_PART_EVAL_STORE
#include "hermite_block_parts.inc"
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
    m = block_fold(m, lds_next, lds_level);
    const unsigned block = blockIdx.x;
#define BLOCK_CTRL a.ctrl
#define BLOCK_STATUS a.status
#define BLOCK_PART_DECIDE
#include "hermite_block_parts.inc"
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
    block_count(active, wave_count, a.counts, blockIdx.x);
}

template <typename T> __global__ __launch_bounds__(256) void hermite_block_finish(BlockArgs<T> a) {
    using vec4 = typename Lane<T>::vec4;
    const BlockCtrl* const ctrl  = a.ctrl;
    const unsigned         block = blockIdx.x;
#define BLOCK_PART_FINISH_HEAD
#include "hermite_block_parts.inc"
    constexpr int  NS      = 6;
    const size_t   i       = a.active[slot];
    const T* const state   = a.state8;
    const T* const partial = a.partial;
#define BLOCK_PART_FINISH_SUMS
#include "hermite_block_parts.inc"
    const T    dt = static_cast<T>(dt_i);
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
#define BLOCK_PART_FINISH_LEVEL
#include "hermite_block_parts.inc"
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
    a.levels[i] = first_level(acc, jerk, a.p);
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
