// hermite6_block.hip -- the kernels of libnbody_hip_hermite6_block.so (include/nbody_hip_hermite6_block.h): 6th-order Hermite steps
// (Nitadori & Makino 2008) with block time steps.  gfx950 only; FMA contraction on.
//
// One block step is the six launches of hermite_block.hip, no atomics, every word written by one lane:
//   block_min_partial      per workgroup, the minimum of tick + ticks(level) (and the deepest level held)    (hermite_block_schedule.inc)
//   block6_predict_count   block_predict_count with the 6th-order predictor: `now`, t_stop and the flag; every body predicted to `now`
//                          into the workspace, three vec4 each {x_p, m, v_p, 0, a_p, 0}; active bodies counted per workgroup
//   block_scan             ONE workgroup: exclusive prefix of the counts in index order, n_act, the status counters            (.inc)
//   block_scatter          the active list, ascending body index                                                               (.inc)
//   hermite6_block_eval    the hot path, see below
//   hermite6_block_finish  one lane per active slot: J partials in index order, corrector, crackle, dt_A, new level, the stored state
// A step that would pass t_stop leaves go = 0 in the control record and the four launches after it return at once.
//
// hermite6_block_eval<T, S> is hermite_block_eval's distribution of work -- a workgroup owns one tile of 64 W ACTIVE bodies, gathered
// through the active list from the predicted state, and one of J contiguous ranges of the chunks of bodies j; (tile, range) from n_act,
// read on the device; wave 0 stores the partial sums, in units of the reference mass, to planes [J][9][slots] -- around hermite6_eval's
// streaming loops: hermite_stream.inc with nine sums and hermite6_interaction.inc, a body j three adjacent vec4 by scalar loads, 47 / 48
// v_pk_* + 2 v_rsq_f32 per packed pair, no LDS, barrier or scratch inside the loops.  Compiled, as hermite6_eval, for 4 (fp32) / 3 (fp64)
// waves per SIMD.  hermite6_block_finish adds the planes (range_sum.inc) and applies hermite6_eval's corrector with the body's own step
// (hermite6_correct.inc).  Around that arithmetic the kernels are hermite_block.hip's text: hermite_block_parts.inc.
#include "hermite6_block_kernels.h"
#include "hermite6_kernels.h"

namespace nb {
namespace {

#include "nbody_lane.h"

#include "hermite_powers.h"

template <typename T> struct BodyJ {
    typename Lane<T>::raw4 p, v, a;  // {x, y, z, m}, {vx, vy, vz, -}, {ax, ay, az, -} in scalar registers
};

#include "hermite_block_kernels_shared.h"

#include "hermite_block_schedule.inc"

#include "hermite6_block_body.h"  // predict6_body, aarseth6_dt

// the waves per SIMD hermite6_eval is compiled for (hermite6_eval.hip says why); U is hermite6_unroll_for (hermite6_kernels.h)
template <typename T> inline constexpr int kWavesPerSimd = sizeof(T) == 8 ? 3 : 4;

template <typename T, int S>
__global__ __launch_bounds__(64 * S) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd<T>, kWavesPerSimd<T>))) void hermite6_block_eval(const T* state12, const unsigned* active,
                                                                                                                                    const BlockCtrl* ctrl, T* partial, unsigned n,
                                                                                                                                    T eps2_in) {
    using LT             = Lane<T>;
    using vec4           = typename LT::vec4;
    using vec            = typename LT::vec;
    using bits           = typename LT::bits;
    constexpr int W      = LT::W;  // bodies i per lane
    constexpr int U      = hermite6_unroll_for<T>();
    constexpr int STRIDE = 3;  // vec4 per body of state12
    const unsigned local = blockIdx.x;
    const T* const state = state12;
#define BLOCK_PART_EVAL_HEAD
#include "hermite_block_parts.inc"
#define BLOCK_PART_EVAL_BODIES
#include "hermite_block_parts.inc"
    vec eps2 = LT::splat(eps2_in);
    LT::keep_in_vgpr(eps2);

    auto body_j = [&](size_t j, BodyJ<T>& b) { b.p = jp[3 * j], b.v = jp[3 * j + 1], b.a = jp[3 * j + 2]; };  // adjacent
#define HERMITE_STREAM_SUMS 9
#define HERMITE_STREAM_INTERACTION "hermite6_interaction.inc"
#define HERMITE_STREAM_UNIT_SUMS  // the partial planes are in units of the reference mass; the finish kernel multiplies
#include "hermite_stream.inc"
#define BLOCK_PART_EVAL_STORE
#include "hermite_block_parts.inc"
}

// ---- the predictor ------------------------------------------------------------------------------------------------------------------------

template <typename T> __global__ __launch_bounds__(256) void block6_predict_count(Block6Args<T> a, unsigned partials) {
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
        const Predicted6<T>      o    = predict6_body<T>(reinterpret_cast<const vec4*>(a.pos)[i], reinterpret_cast<const vec4*>(a.vel)[i], reinterpret_cast<const vec4*>(a.acc)[i],
                                                         reinterpret_cast<const vec4*>(a.jerk)[i], reinterpret_cast<const vec4*>(a.snap)[i],
                                                         reinterpret_cast<const vec4*>(a.crackle)[i], dt);
        vec4* const              out  = reinterpret_cast<vec4*>(a.state12) + 3 * static_cast<size_t>(i);
        out[0] = o.x, out[1] = o.v, out[2] = o.a;
    }
    block_count(active, wave_count, a.counts, blockIdx.x);
}

// ---- the finish -----------------------------------------------------------------------------------------------------------------------

template <typename T> __global__ __launch_bounds__(256) void hermite6_block_finish(Block6Args<T> a) {
    using vec4 = typename Lane<T>::vec4;
    const BlockCtrl* const ctrl  = a.ctrl;
    const unsigned         block = blockIdx.x;
#define BLOCK_PART_FINISH_HEAD
#include "hermite_block_parts.inc"
    constexpr int  NS      = 9;
    const size_t   i       = a.active[slot];
    const T* const state   = a.state12;
    const T* const partial = a.partial;
#define BLOCK_PART_FINISH_SUMS
#include "hermite_block_parts.inc"
    // the corrector and the crackle of nb_hermite6_step_* (hermite6_eval's epilogue), with the body's own step, in place
    const struct {
        const T *old_pos, *vel, *acc, *jerk, *snap;
    } stored{a.pos, a.vel, a.acc, a.jerk, a.snap};
#define HERMITE6_STEP_DT static_cast<T>(dt_i)
#define HERMITE6_STORED(array) stored.array
#include "hermite6_correct.inc"
    reinterpret_cast<vec4*>(a.pos)[i]     = x1;
    reinterpret_cast<vec4*>(a.vel)[i]     = v;
    reinterpret_cast<vec4*>(a.acc)[i]     = a1;
    reinterpret_cast<vec4*>(a.jerk)[i]    = j1;
    reinterpret_cast<vec4*>(a.snap)[i]    = s1;
    reinterpret_cast<vec4*>(a.crackle)[i] = c1;

    const double dt_a = aarseth6_dt(a1, j1, s1, c1, a.p.eta, a.p.dt_max);
#define BLOCK_PART_FINISH_LEVEL
#include "hermite_block_parts.inc"
}

// init: levels from the accelerations and jerks nb_hermite6_init's launches left, ticks 0, the status record cleared
template <typename T> __global__ __launch_bounds__(256) void block6_init_levels(Block6Args<T> a) {
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
__global__ __launch_bounds__(256) void block6_sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const T* snap, const T* crackle,
                                                   const unsigned long long* ticks, const BlockStatus* status, unsigned n, BlockParams p) {
    using vec4       = typename Lane<T>::vec4;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned long long now = status->now_ticks, tick = ticks[i];
    const T                  dt  = static_cast<T>(static_cast<double>(now > tick ? now - tick : 0ull) * tick_length(p));
    const vec4               v   = reinterpret_cast<const vec4*>(vel)[i];
    Predicted6<T>            o   = predict6_body<T>(reinterpret_cast<const vec4*>(pos)[i], v, reinterpret_cast<const vec4*>(acc)[i], reinterpret_cast<const vec4*>(jerk)[i],
                                                    reinterpret_cast<const vec4*>(snap)[i], reinterpret_cast<const vec4*>(crackle)[i], dt);
    o.v.w                               = v.w;
    reinterpret_cast<vec4*>(pos_out)[i] = o.x;
    reinterpret_cast<vec4*>(vel_out)[i] = o.v;
}

template <typename T, int S> hipError_t launch_eval_s(const Block6Args<T>& a, unsigned groups, hipStream_t stream) {
    hipLaunchKernelGGL((hermite6_block_eval<T, S>), dim3(groups), dim3(64 * S), 0, stream, static_cast<const T*>(a.state12), static_cast<const unsigned*>(a.active),
                       static_cast<const BlockCtrl*>(a.ctrl), a.partial, a.n, a.eps2);
    return hipGetLastError();
}

}  // namespace

template <typename T> hipError_t launch_block6_init(const Block6Args<T>& a, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((block6_init_levels<T>), dim3((a.n + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <typename T> hipError_t launch_block6_step(const Block6Args<T>& a, hipStream_t stream) {
    constexpr unsigned per_tile = 64 * Lane<T>::W;
    const unsigned     blocks   = (a.n + 255u) / 256u;
    const unsigned     partials = blocks < kBlockMinPartials ? blocks : kBlockMinPartials;
    (void)hipGetLastError();
    hipLaunchKernelGGL(block_min_partial, dim3(partials), dim3(256), 0, stream, static_cast<const unsigned long long*>(a.ticks), static_cast<const int*>(a.levels), a.n,
                       a.p.max_level, a.min_part, a.lvl_part);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL((block6_predict_count<T>), dim3(blocks), dim3(256), 0, stream, a, partials);
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
    hipLaunchKernelGGL((hermite6_block_finish<T>), dim3(blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_block6_sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const T* snap, const T* crackle, const unsigned long long* ticks,
                              const BlockStatus* status, unsigned n, const BlockParams& p, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((block6_sync<T>), dim3((n + 255u) / 256u), dim3(256), 0, stream, pos_out, vel_out, pos, vel, acc, jerk, snap, crackle, ticks, status, n, p);
    return hipGetLastError();
}

template hipError_t launch_block6_init<float>(const Block6Args<float>&, hipStream_t);
template hipError_t launch_block6_init<double>(const Block6Args<double>&, hipStream_t);
template hipError_t launch_block6_step<float>(const Block6Args<float>&, hipStream_t);
template hipError_t launch_block6_step<double>(const Block6Args<double>&, hipStream_t);
template hipError_t launch_block6_sync<float>(float*, float*, const float*, const float*, const float*, const float*, const float*, const float*, const unsigned long long*,
                                              const BlockStatus*, unsigned, const BlockParams&, hipStream_t);
template hipError_t launch_block6_sync<double>(double*, double*, const double*, const double*, const double*, const double*, const double*, const double*,
                                               const unsigned long long*, const BlockStatus*, unsigned, const BlockParams&, hipStream_t);

}  // namespace nb
