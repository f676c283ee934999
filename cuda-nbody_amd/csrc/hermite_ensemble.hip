// hermite_ensemble.hip -- the kernels of libnbody_hip_hermite_ensemble.so (include/nbody_hip_hermite_ensemble.h): 4th-order Hermite steps
// of B independent systems of N bodies in one launch per stage, each system with a time step of its own.  gfx950 only; FMA contraction on.
//
// hermite_ensemble_eval<T, S, STEP> is hermite_eval (hermite_eval.hip) per system: workgroup g works on tile g mod G of system g / G, G the
// workgroups plan_stream (wave_stream.h) gives one system of N bodies, S = stream_waves(N).  What lies between a lane's bodies i and its sums is the
// same TEXT (hermite_stream.inc with wave_groups.inc, wave_mates.inc and wave_fold.inc inside it; hermite_body.h; hermite_correct.inc), so
// a system's sums are formed in the order the solo kernel forms them and its bits are the solo call's.  Only the bases of the arrays, dt
// and softening^2 are the system's own, all wave-uniform: a workgroup never touches two systems.
//
// The adaptive form keeps a 32-byte clock per system on the device.  Every stage of nb_hermite_ensemble_advance_* derives the system's dt
// from that record (clock_decision), which only the clock stage -- after every stage that reads it -- writes; the workgroups of a system
// that is done or stalled leave after that one scalar load.  No atomics anywhere: the status record is integer sums and exact minima.
#include "hermite_ensemble_kernels.h"
#include "softening_floor.h"

namespace nb {
namespace {

#include "nbody_lane.h"

#include "hermite_stream.h"

#include "hermite_body.h"

#include "hermite_ratio.h"

// clock_decision, uniform_load, system_parameters, block_min, the tally and the status kernel: one text with hermite6_ensemble.hip
#include "hermite_ensemble_clock.inc"

template <typename T, int S, bool STEP>
__global__ __launch_bounds__(64 * S) __attribute__((amdgpu_waves_per_eu(4, 4))) void hermite_ensemble_eval(EnsembleHermiteArgs<T> a) {
    using LT            = Lane<T>;
    using vec4          = typename LT::vec4;
    using vec           = typename LT::vec;
    using raw4          = typename LT::raw4;
    using bits          = typename LT::bits;
    constexpr int W     = LT::W;  // bodies i per lane
    constexpr int U     = unroll_for<T>();
    constexpr int STRIDE = STEP ? 2 : 1;  // vec4 per body where the bodies are read
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx4/x8/x16

    // the workgroup's system and its tile of that system's bodies i
    const unsigned system = blockIdx.x / a.groups_per_system;
    const unsigned tile   = blockIdx.x - system * a.groups_per_system;
    T              dt, eps2_system;
    if (!system_parameters<T, STEP>(a.src, system, dt, eps2_system)) return;  // (wave-uniform: the whole workgroup leaves)

    const unsigned   n        = a.n;
    const size_t     origin   = 4 * static_cast<size_t>(system) * n;  // the system's first element in an array of T[4 N B]
    const T* const   pos_base = STEP ? a.state8 + 2 * origin : a.pos + origin;
    const T* const   vel_base = STEP ? a.state8 + 2 * origin + 4 : a.vel_in + origin;
    const stream_ptr jp       = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(pos_base));
    const stream_ptr jv       = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(vel_base));
    const int        tid      = threadIdx.x;
    const int        wave     = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int        lane     = tid & 63;

    // bodies i of this lane: block_base + k*64 + lane (coalesced across the lanes of a wave), within the system
    const unsigned block_base = tile * (64 * W);
    vec            px, py, pz, vx, vy, vz;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned local = block_base + k * 64 + lane;
        const size_t   i     = local < n ? local : n - 1;
        const vec4     p     = reinterpret_cast<const vec4*>(pos_base)[i * STRIDE];
        const vec4     v     = reinterpret_cast<const vec4*>(vel_base)[i * STRIDE];
        LT::set(px, k, p.x), LT::set(py, k, p.y), LT::set(pz, k, p.z);
        LT::set(vx, k, v.x), LT::set(vy, k, v.y), LT::set(vz, k, v.z);
    }
    vec eps2 = LT::splat(eps2_system);
    LT::keep_in_vgpr(eps2);

    constexpr unsigned range = 0, ranges = 1;  // every workgroup streams every chunk of its system
    auto body_j = [&](size_t j, BodyJ<T>& b) {
        if constexpr (STEP) {
            b.p = jp[2 * j], b.v = jp[2 * j + 1];  // adjacent: one s_load_dwordx8 / x16
        } else {
            b.p = jp[j], b.v = jv[j];
        }
    };
#include "hermite_stream.inc"

    T* const acc  = a.acc + origin;
    T* const jerk = a.jerk + origin;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned local = block_base + k * 64 + lane;
        if (local >= n) continue;
        const size_t i = local;
        vec4         a1, j1;
        a1.x = LT::get(second[0], k) * out_scale, a1.y = LT::get(second[1], k) * out_scale, a1.z = LT::get(second[2], k) * out_scale, a1.w = 0;
        j1.x = LT::get(second[3], k) * out_scale, j1.y = LT::get(second[4], k) * out_scale, j1.z = LT::get(second[5], k) * out_scale, j1.w = 0;
        if constexpr (STEP) {
            const vec4 x  = reinterpret_cast<const vec4*>(a.old_pos + origin)[i];
            vec4       v  = reinterpret_cast<const vec4*>(a.vel + origin)[i];
            const vec4 a0 = reinterpret_cast<const vec4*>(acc)[i];
            const vec4 j0 = reinterpret_cast<const vec4*>(jerk)[i];
#include "hermite_correct.inc"
            reinterpret_cast<vec4*>(a.new_pos + origin)[i] = x1;
            reinterpret_cast<vec4*>(a.vel + origin)[i]     = v;
        }
        reinterpret_cast<vec4*>(acc)[i]  = a1;
        reinterpret_cast<vec4*>(jerk)[i] = j1;
    }
}

// The predictor (hermite_body.h) -> state8 {x_p, m, v_p, 0}, on the grid of the evaluation: one wave per tile of 64 W bodies.  HBM-bound.
template <typename T>
__global__ __launch_bounds__(64) void hermite_ensemble_predict(const T* pos, const T* vel, const T* acc, const T* jerk, T* state8, unsigned n, unsigned groups_per_system,
                                                               EnsembleSource<T> src) {
    using vec4          = typename Lane<T>::vec4;
    constexpr int W     = Lane<T>::W;
    const unsigned system = blockIdx.x / groups_per_system;
    const unsigned tile   = blockIdx.x - system * groups_per_system;
    T              dt, eps2;
    if (!system_parameters<T, true>(src, system, dt, eps2)) return;
    const size_t first = static_cast<size_t>(system) * n;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned local = tile * (64 * W) + k * 64 + threadIdx.x;
        if (local >= n) continue;
        const size_t i = first + local;
        const vec4   x = reinterpret_cast<const vec4*>(pos)[i], v = reinterpret_cast<const vec4*>(vel)[i];
        const vec4   a = reinterpret_cast<const vec4*>(acc)[i], j = reinterpret_cast<const vec4*>(jerk)[i];
        vec4         xp, vp;
        predict_body<T>(x, v, a, j, dt, xp, vp);
        reinterpret_cast<vec4*>(state8)[2 * i]     = xp;
        reinterpret_cast<vec4*>(state8)[2 * i + 1] = vp;
    }
}

// min |a| / |jerk| over kEnsembleTimestepBodies bodies of one system -> partial[system * partials + p].  (The minimum is exact in any
// order, so the partials of the solo call and these give one value.)  With clocks: the systems that take no step in this call are left out.
template <typename T>
__global__ __launch_bounds__(256) void hermite_ensemble_timestep_partial(const T* acc, const T* jerk, unsigned n, unsigned partials, EnsembleSource<T> src, bool stepping,
                                                                         double* partial) {
    using vec4 = typename Lane<T>::vec4;
    __shared__ double lds[256];
    const unsigned    system = blockIdx.x / partials;
    const unsigned    p      = blockIdx.x - system * partials;
    if (stepping) {
        T dt, eps2;
        if (!system_parameters<T, true>(src, system, dt, eps2)) return;
    }
    const unsigned local = p * kEnsembleTimestepBodies + threadIdx.x;
    double         m     = __builtin_inf();
    if (local < n) {
        const size_t i = static_cast<size_t>(system) * n + local;
        m              = norm_ratio<T>(reinterpret_cast<const vec4*>(acc)[i], reinterpret_cast<const vec4*>(jerk)[i]);
    }
    m = block_min(m, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// One thread per system: the minimum of the system's partials, dt = eta (T)min -- the expression of hermite_timestep_final -- and
//   dt_out != nullptr   dt_out[s] = dt                                     (nb_hermite_ensemble_timestep_*)
//   begin               the clock of a run that starts                      (nb_hermite_ensemble_begin_*)
//   else                the clock after this call's step, by the rule of the header (nb_hermite_ensemble_advance_*), and the block's tally
template <typename T>
__global__ __launch_bounds__(256) void hermite_ensemble_clock(const double* partial, unsigned partials, unsigned b, T eta, T* dt_out, EnsembleClock* clocks, bool begin,
                                                              EnsembleSource<T> src, EnsembleStatus* block_status) {
    __shared__ unsigned long long sums[5][256];
    __shared__ double             mins[2][256];
    const unsigned                s = blockIdx.x * kEnsembleClockSystems + threadIdx.x;
    Tally                         t{0, 0, 0, 0, 0, __builtin_inf(), __builtin_inf()};
    if (s < b) {
        auto next_dt = [&]() {
            double m = __builtin_inf();
            for (unsigned p = 0; p < partials; ++p) m = fmin(m, partial[static_cast<size_t>(s) * partials + p]);
            return eta * static_cast<T>(m);
        };
#include "hermite_ensemble_clock_update.inc"
    }
    if (block_status == nullptr) return;  // (uniform: a kernel argument)
    t = block_tally(t, sums, mins);
    if (threadIdx.x == 0) store_tally(t, block_status + blockIdx.x);
}

static_assert(stream_lane_bodies<float>() == Lane<float>::W && stream_lane_bodies<double>() == Lane<double>::W, "plan_stream's bodies i per lane are the kernel's");

template <typename T, bool STEP> hipError_t launch_planned(EnsembleHermiteArgs<T> a, unsigned b, hipStream_t stream) {
    const StreamPlan p  = plan_stream<T>(a.n, kHermiteSums, unroll_for<T>());
    a.groups_per_system = p.groups;
    return with_stream_waves(p.waves, [&](auto waves) {
        constexpr int S = decltype(waves)::value;
        (void)hipGetLastError();  // a launch reports ITS OWN error
        hipLaunchKernelGGL((hermite_ensemble_eval<T, S, STEP>), dim3(p.groups * b), dim3(64 * S), 0, stream, a);
        return hipGetLastError();
    });
}

}  // namespace

template <typename T> hipError_t launch_ensemble_eval(const EnsembleHermiteArgs<T>& a, unsigned b, hipStream_t stream) { return launch_planned<T, false>(a, b, stream); }

template <typename T> hipError_t launch_ensemble_step(const EnsembleHermiteArgs<T>& a, unsigned b, T* state8, hipStream_t stream) {
    const StreamPlan p = plan_stream<T>(a.n, kHermiteSums, unroll_for<T>());
    (void)hipGetLastError();
    hipLaunchKernelGGL((hermite_ensemble_predict<T>), dim3(p.groups * b), dim3(64), 0, stream, a.old_pos, static_cast<const T*>(a.vel),
                       static_cast<const T*>(a.acc), static_cast<const T*>(a.jerk), state8, a.n, p.groups, a.src);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    return launch_planned<T, true>(a, b, stream);
}

template <typename T>
hipError_t launch_ensemble_clocks(const T* acc, const T* jerk, unsigned n, unsigned b, T eta, T* dt_out, EnsembleClock* clocks, bool begin, const EnsembleSource<T>& src,
                                  double* partial, EnsembleStatus* block_status, EnsembleStatus* status, hipStream_t stream) {
    const unsigned partials = ensemble_partials(n), blocks = ensemble_status_blocks(b);
    const bool     stepping = dt_out == nullptr && !begin;
    (void)hipGetLastError();
    hipLaunchKernelGGL((hermite_ensemble_timestep_partial<T>), dim3(partials * b), dim3(256), 0, stream, acc, jerk, n, partials, src, stepping, partial);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL((hermite_ensemble_clock<T>), dim3(blocks), dim3(256), 0, stream, static_cast<const double*>(partial), partials, b, eta, dt_out, clocks, begin, src,
                       status != nullptr ? block_status : nullptr);
    if (const auto err = hipGetLastError(); err != hipSuccess || status == nullptr) return err;
    hipLaunchKernelGGL(hermite_ensemble_status, dim3(1), dim3(256), 0, stream, static_cast<const EnsembleStatus*>(block_status), blocks, status);
    return hipGetLastError();
}

template hipError_t launch_ensemble_eval<float>(const EnsembleHermiteArgs<float>&, unsigned, hipStream_t);
template hipError_t launch_ensemble_eval<double>(const EnsembleHermiteArgs<double>&, unsigned, hipStream_t);
template hipError_t launch_ensemble_step<float>(const EnsembleHermiteArgs<float>&, unsigned, float*, hipStream_t);
template hipError_t launch_ensemble_step<double>(const EnsembleHermiteArgs<double>&, unsigned, double*, hipStream_t);
template hipError_t launch_ensemble_clocks<float>(const float*, const float*, unsigned, unsigned, float, float*, EnsembleClock*, bool, const EnsembleSource<float>&, double*,
                                                  EnsembleStatus*, EnsembleStatus*, hipStream_t);
template hipError_t launch_ensemble_clocks<double>(const double*, const double*, unsigned, unsigned, double, double*, EnsembleClock*, bool, const EnsembleSource<double>&,
                                                   double*, EnsembleStatus*, EnsembleStatus*, hipStream_t);

}  // namespace nb
