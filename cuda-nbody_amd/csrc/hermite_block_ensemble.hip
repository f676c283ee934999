// hermite_block_ensemble.hip -- the kernels of libnbody_hip_hermite_block_ensemble.so (include/nbody_hip_hermite_block_ensemble.h): block
// time steps (hermite_block.hip) of B independent systems of N bodies, one launch per stage whatever B is.  gfx950 only; FMA contraction on.
//
// One call is five launches, no atomics, every word written by one lane.  Workgroup g of a stage belongs to system g / (workgroups per
// system) and never touches another system; each system has its own control record, `now`, active set and n_act in its own slice of the
// workspace (hermite_block_ensemble_kernels.h):
//   block_ensemble_min_partial    per workgroup of 256 bodies, the minimum of tick + ticks(level) (and the deepest level held)
//                                 (this, the scatter, init's levels and the summary: hermite_block_ensemble_schedule.inc, one text with
//                                 hermite6_block_ensemble.hip)
//   block_ensemble_predict_count  every workgroup folds its system's partials (<= 256) to the system's `now`; the system's first workgroup
//                                 records it, decides about t_stop and writes the flag; every body is predicted to `now` into the system's
//                                 slice of the workspace; active bodies are counted per workgroup
//   block_ensemble_scatter        every workgroup adds the (<= 256) counts before its own, in index order, and writes its part of the
//                                 active list, ascending body index; the system's first workgroup records n_act and the status counters
//   hermite_block_ensemble_eval   the hot path, see below
//   hermite_block_ensemble_finish one lane per active slot: J partials in range order, corrector, dt_A, new level, the body's stored state
// The workgroups of a system whose step would pass t_stop leave after reading go = 0 from its control record; the other systems step.
// (The solo library scans up to 65 536 counts in a launch of its own; with N <= 65 536 a system has at most 256 count blocks, which every
// workgroup of the scatter adds itself.  Minima and integer sums are exact in any order: the schedule and the counters are the solo ones.)
//
// hermite_block_ensemble_eval<T, S> is hermite_block_eval (hermite_block.hip) per system: between a lane's bodies i and its six sums lies
// the same TEXT (hermite_stream.inc with wave_groups.inc, wave_mates.inc and wave_fold.inc inside it), and (tile, range) come from
// stream_geometry(N, n_act of THIS system, 64 W, kBlockTarget) and the workgroup's index within its system, on a per-system grid of
// block_launch_groups(N, 64 W).  So tiles, J and with them the order of every sum are the solo step's, and the bits are.  A target that
// shrank with B would save workgroups and partial planes but make a system's bits depend on B: not taken.  Only the bases of the system's
// arrays, its control record and its softening^2 are fetched per system, wave-uniform, before the loops; the reference mass is the mass of
// the system's first body (hermite_stream.inc reads it through the system's scalar-load pointer).
#include "hermite_block_ensemble_kernels.h"
#include "softening_floor.h"

namespace nb {
namespace {

#include "nbody_lane.h"

#include "hermite_stream.h"

#include "hermite_body.h"

#include "hermite_block_kernels_shared.h"

#include "hermite_block_ensemble_schedule.inc"

// What the evaluation needs of a call: the workspace and where a system's sections lie in its slice of it.
template <typename T> struct BlockEnsembleEvalArgs {
    char*    workspace;
    size_t   stride, state8, partial, active, ctrl;
    const T* system_eps2;
    T        eps2;
    unsigned n, groups_per_system;
};

template <typename T, int S>
__global__ __launch_bounds__(64 * S) __attribute__((amdgpu_waves_per_eu(4, 4))) void hermite_block_ensemble_eval(BlockEnsembleEvalArgs<T> a) {
    using LT         = Lane<T>;
    using vec4       = typename LT::vec4;
    using vec        = typename LT::vec;
    using bits       = typename LT::bits;
    constexpr int W      = LT::W;  // bodies i per lane
    constexpr int U      = unroll_for<T>();
    constexpr int STRIDE = 2;  // vec4 per body of state8

    // the workgroup's system, and its index among that system's workgroups (wave-uniform: the whole workgroup leaves together)
    const unsigned system = blockIdx.x / a.groups_per_system;
    const unsigned local  = blockIdx.x - system * a.groups_per_system;
    char* const    slice  = a.workspace + static_cast<size_t>(system) * a.stride;
    const BlockCtrl* const ctrl = reinterpret_cast<const BlockCtrl*>(slice + a.ctrl);
    const unsigned         n    = a.n;
#define BLOCK_PART_EVAL_HEAD
#include "hermite_block_parts.inc"
    const T* const        state   = reinterpret_cast<const T*>(slice + a.state8);
    const unsigned* const active  = reinterpret_cast<const unsigned*>(slice + a.active);
    T* const              partial = reinterpret_cast<T*>(slice + a.partial);
    const T               eps2_system = floored(a.system_eps2 != nullptr ? uniform_load(a.system_eps2, system) : a.eps2);
#define BLOCK_PART_EVAL_BODIES
#include "hermite_block_parts.inc"
    vec eps2 = LT::splat(eps2_system);
    LT::keep_in_vgpr(eps2);

    auto body_j = [&](size_t j, BodyJ<T>& b) { b.p = jp[2 * j], b.v = jp[2 * j + 1]; };  // adjacent: one s_load_dwordx8 / x16
#define HERMITE_STREAM_UNIT_SUMS  // the partial planes are in units of the reference mass; the finish kernel multiplies
#include "hermite_stream.inc"
#define BLOCK_PART_EVAL_STORE
#include "hermite_block_parts.inc"
}

// ---- the schedule, per system -----------------------------------------------------------------------------------------------------------

// Every workgroup folds its system's partial minima (one per lane) to the system's `now` and decides about t_stop; the system's first
// workgroup records both in the control record and the flag and deepest_level in the status record; every body of the system is predicted
// to `now` into the workspace; active bodies are counted per workgroup.
template <typename T> __global__ __launch_bounds__(256) void block_ensemble_predict_count(BlockEnsembleArgs<T> a) {
    using vec4 = typename Lane<T>::vec4;
    __shared__ unsigned long long lds_next[256];
    __shared__ int                lds_level[256];
    __shared__ unsigned           wave_count[4];
    const unsigned                system = blockIdx.x / a.blocks;
    const unsigned                block  = blockIdx.x - system * a.blocks;
    char* const                   slice  = slice_of(a, system);
    MinLevel                      m{~0ull, 0};
    if (threadIdx.x < a.blocks) {
        m.next  = reinterpret_cast<const unsigned long long*>(slice + a.layout.min_part)[threadIdx.x];
        m.level = reinterpret_cast<const int*>(slice + a.layout.lvl_part)[threadIdx.x];
    }
    m = block_fold(m, lds_next, lds_level);
#define BLOCK_CTRL ctrl_of(a, system)
#define BLOCK_STATUS (a.status + system)
#define BLOCK_PART_DECIDE
#include "hermite_block_parts.inc"
    const unsigned local  = block * 256u + threadIdx.x;
    bool           active = false;
    if (local < a.n) {
        const size_t             i    = static_cast<size_t>(system) * a.n + local;
        const unsigned long long tick = a.ticks[i];
        active                        = tick + ticks_of(a.levels[i], a.p.max_level) == now;
        const T                  dt   = static_cast<T>(static_cast<double>(now - tick) * q);
        const vec4 x = reinterpret_cast<const vec4*>(a.pos)[i], v = reinterpret_cast<const vec4*>(a.vel)[i];
        const vec4 acc = reinterpret_cast<const vec4*>(a.acc)[i], jerk = reinterpret_cast<const vec4*>(a.jerk)[i];
        vec4       xp, vp;
        predict_body<T>(x, v, acc, jerk, dt, xp, vp);
        vec4* const state8 = reinterpret_cast<vec4*>(slice + a.layout.state);
        state8[2 * static_cast<size_t>(local)]     = xp;
        state8[2 * static_cast<size_t>(local) + 1] = vp;
    }
    block_count(active, wave_count, reinterpret_cast<unsigned*>(slice + a.layout.counts), block);
}

template <typename T> __global__ __launch_bounds__(256) void hermite_block_ensemble_finish(BlockEnsembleArgs<T> a) {
    using vec4 = typename Lane<T>::vec4;
    const unsigned         system = blockIdx.x / a.blocks;
    const unsigned         block  = blockIdx.x - system * a.blocks;
    const BlockCtrl* const ctrl   = ctrl_of(a, system);
#define BLOCK_PART_FINISH_HEAD
#include "hermite_block_parts.inc"
    constexpr int     NS      = 6;
    const char* const slice   = slice_of(a, system);
    const T* const    state   = reinterpret_cast<const T*>(slice + a.layout.state);
    const size_t      i       = static_cast<size_t>(system) * a.n + reinterpret_cast<const unsigned*>(slice + a.layout.active)[slot];
    const T* const    partial = reinterpret_cast<const T*>(slice + a.layout.partial);
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

// every body predicted to ITS system's status time
template <typename T>
__global__ __launch_bounds__(256) void block_ensemble_sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const unsigned long long* ticks,
                                                           const BlockStatus* status, unsigned n, unsigned blocks, BlockParams p) {
    using vec4            = typename Lane<T>::vec4;
    const unsigned system = blockIdx.x / blocks;
    const unsigned local  = (blockIdx.x - system * blocks) * 256u + threadIdx.x;
    if (local >= n) return;
    const size_t             i   = static_cast<size_t>(system) * n + local;
    const unsigned long long now = status[system].now_ticks, tick = ticks[i];
    const T                  dt  = static_cast<T>(static_cast<double>(now > tick ? now - tick : 0ull) * tick_length(p));
    const vec4 x = reinterpret_cast<const vec4*>(pos)[i], v = reinterpret_cast<const vec4*>(vel)[i];
    vec4       xp, vp;
    predict_body<T>(x, v, reinterpret_cast<const vec4*>(acc)[i], reinterpret_cast<const vec4*>(jerk)[i], dt, xp, vp);
    vp.w                                 = v.w;
    reinterpret_cast<vec4*>(pos_out)[i] = xp;
    reinterpret_cast<vec4*>(vel_out)[i] = vp;
}

template <typename T, int S> hipError_t launch_eval_s(const BlockEnsembleArgs<T>& a, hipStream_t stream) {
    BlockEnsembleEvalArgs<T> e{};
    e.workspace = a.workspace, e.stride = a.layout.stride, e.state8 = a.layout.state, e.partial = a.layout.partial, e.active = a.layout.active, e.ctrl = a.layout.ctrl;
    e.system_eps2 = a.system_eps2, e.eps2 = a.eps2, e.n = a.n, e.groups_per_system = a.groups_per_system;
    hipLaunchKernelGGL((hermite_block_ensemble_eval<T, S>), dim3(a.groups_per_system * a.b), dim3(64 * S), 0, stream, e);
    return hipGetLastError();
}

}  // namespace

template <typename T> hipError_t launch_block_ensemble_init(const BlockEnsembleArgs<T>& a, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((block_ensemble_init_levels<T>), dim3(a.blocks * a.b), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <typename T> hipError_t launch_block_ensemble_step(const BlockEnsembleArgs<T>& a, hipStream_t stream) {
    const unsigned grid = a.blocks * a.b;
    (void)hipGetLastError();
    hipLaunchKernelGGL((block_ensemble_min_partial<T>), dim3(grid), dim3(256), 0, stream, a);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL((block_ensemble_predict_count<T>), dim3(grid), dim3(256), 0, stream, a);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL((block_ensemble_scatter<T>), dim3(grid), dim3(256), 0, stream, a);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipError_t err = hipErrorInvalidValue;
    switch (block_waves(a.n)) {
        case 1: err = launch_eval_s<T, 1>(a, stream); break;
        case 2: err = launch_eval_s<T, 2>(a, stream); break;
        case 4: err = launch_eval_s<T, 4>(a, stream); break;
        case 8: err = launch_eval_s<T, 8>(a, stream); break;
        default: break;
    }
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((hermite_block_ensemble_finish<T>), dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_block_ensemble_sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const unsigned long long* ticks, const BlockStatus* status,
                                      unsigned n, unsigned b, const BlockParams& p, hipStream_t stream) {
    const unsigned blocks = block_ensemble_blocks(n);
    (void)hipGetLastError();
    hipLaunchKernelGGL((block_ensemble_sync<T>), dim3(blocks * b), dim3(256), 0, stream, pos_out, vel_out, pos, vel, acc, jerk, ticks, status, n, blocks, p);
    return hipGetLastError();
}

hipError_t launch_block_ensemble_summary(const BlockStatus* status, unsigned b, BlockEnsembleSummary* out, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(block_ensemble_summary, dim3(1), dim3(256), 0, stream, status, b, out);
    return hipGetLastError();
}

template hipError_t launch_block_ensemble_init<float>(const BlockEnsembleArgs<float>&, hipStream_t);
template hipError_t launch_block_ensemble_init<double>(const BlockEnsembleArgs<double>&, hipStream_t);
template hipError_t launch_block_ensemble_step<float>(const BlockEnsembleArgs<float>&, hipStream_t);
template hipError_t launch_block_ensemble_step<double>(const BlockEnsembleArgs<double>&, hipStream_t);
template hipError_t launch_block_ensemble_sync<float>(float*, float*, const float*, const float*, const float*, const float*, const unsigned long long*, const BlockStatus*,
                                                      unsigned, unsigned, const BlockParams&, hipStream_t);
template hipError_t launch_block_ensemble_sync<double>(double*, double*, const double*, const double*, const double*, const double*, const unsigned long long*, const BlockStatus*,
                                                       unsigned, unsigned, const BlockParams&, hipStream_t);

}  // namespace nb
