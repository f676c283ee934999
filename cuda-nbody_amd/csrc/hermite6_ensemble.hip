// hermite6_ensemble.hip -- the kernels of libnbody_hip_hermite6_ensemble.so (include/nbody_hip_hermite6_ensemble.h): 6th-order Hermite steps
// of B independent systems of N bodies in one launch per stage, each system with a time step of its own.  gfx950 only; FMA contraction on.
//
// hermite6_ensemble_eval<T, S, STEP> is hermite6_eval (hermite6_eval.hip) per system: workgroup g works on tile g mod G of system g / G, G the
// workgroups plan_stream (wave_stream.h) gives one system of N bodies, S = stream_waves(N).  What lies between a lane's bodies i and its nine sums is the
// same TEXT (hermite_stream.inc with HERMITE_STREAM_SUMS 9 and hermite6_interaction.inc, a body j of three adjacent vec4), and so are the
// predictor (hermite6_predict.inc), the corrector with the new crackle (hermite6_correct.inc), the pack (hermite6_pack.inc) and the ratio
// behind the time step (hermite6_ratio.h): a system's sums are formed in the order the solo kernel forms them and its bits are the solo
// call's.  Only the bases of the arrays, dt and softening^2 are the system's own, all wave-uniform: a workgroup never touches two systems.
//
// The adaptive form is that of hermite_ensemble.hip, one text with it (hermite_ensemble_clock.inc): a 32-byte clock per system on the device,
// from which every stage of nb_hermite6_ensemble_advance_* derives the system's dt and which only the clock stage -- after every stage that
// reads it -- writes; the workgroups of a system that is done or stalled leave after that one scalar load.  The clock kernel here forms the
// next dt as hermite6_timestep_final does.  Nothing here adds to memory from two threads: the status record is integer sums and exact minima.
#include "hermite6_ensemble_kernels.h"
#include "softening_floor.h"

namespace nb {
namespace {

#include "nbody_lane.h"

#include "hermite_powers.h"

#include "hermite6_ratio.h"

#include "hermite_ensemble_clock.inc"

template <typename T> struct BodyJ {
    typename Lane<T>::raw4 p, v, a;  // {x, y, z, m}, {vx, vy, vz, -}, {ax, ay, az, -} in scalar registers
};

// Waves per SIMD, as hermite6_eval: fp32 fits 4 (<= 128 VGPRs), fp64 is compiled for 3.
template <typename T> inline constexpr int kWavesPerSimd = sizeof(T) == 8 ? 3 : 4;

template <typename T, int S, bool STEP>
__global__ __launch_bounds__(64 * S) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd<T>, kWavesPerSimd<T>))) void hermite6_ensemble_eval(EnsembleHermite6Args<T> a) {
    using LT             = Lane<T>;
    using vec4           = typename LT::vec4;
    using vec            = typename LT::vec;
    using raw4           = typename LT::raw4;
    using bits           = typename LT::bits;
    constexpr int W      = LT::W;  // bodies i per lane
    constexpr int U      = hermite6_unroll_for<T>();
    constexpr int STRIDE = 3;  // vec4 per body where the bodies are read
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx4/x8/x16

    // the workgroup's system and its tile of that system's bodies i
    const unsigned system = blockIdx.x / a.groups_per_system;
    const unsigned tile   = blockIdx.x - system * a.groups_per_system;
    T              dt, eps2_system;
    if (!system_parameters<T, STEP>(a.src, system, dt, eps2_system)) return;  // (wave-uniform: the whole workgroup leaves)

    const unsigned   n        = a.n;
    const T* const   pos_base = a.state12 + 12 * static_cast<size_t>(system) * n;  // the system's first body in T[12 N B]
    const stream_ptr jp       = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(pos_base));
    const int        tid      = threadIdx.x;
    const int        wave     = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int        lane     = tid & 63;

    // bodies i of this lane: block_base + k*64 + lane, within the system
    const unsigned block_base = tile * (64 * W);
    vec            px, py, pz, vx, vy, vz, ax, ay, az;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned local = block_base + k * 64 + lane;
        const size_t   i     = local < n ? local : n - 1;
        const vec4     p     = reinterpret_cast<const vec4*>(pos_base)[i * STRIDE];
        const vec4     v     = reinterpret_cast<const vec4*>(pos_base)[i * STRIDE + 1];
        const vec4     b     = reinterpret_cast<const vec4*>(pos_base)[i * STRIDE + 2];
        LT::set(px, k, p.x), LT::set(py, k, p.y), LT::set(pz, k, p.z);
        LT::set(vx, k, v.x), LT::set(vy, k, v.y), LT::set(vz, k, v.z);
        LT::set(ax, k, b.x), LT::set(ay, k, b.y), LT::set(az, k, b.z);
    }
    vec eps2 = LT::splat(eps2_system);
    LT::keep_in_vgpr(eps2);

    constexpr unsigned range = 0, ranges = 1;  // every workgroup streams every chunk of its system
    auto body_j = [&](size_t j, BodyJ<T>& b) { b.p = jp[3 * j], b.v = jp[3 * j + 1], b.a = jp[3 * j + 2]; };  // adjacent
#define HERMITE_STREAM_SUMS 9
#define HERMITE_STREAM_INTERACTION "hermite6_interaction.inc"
#include "hermite_stream.inc"

    // the epilogue's pointers are fetched from the kernel arguments here, behind the loops, where they cost no scalar registers, as in
    // hermite6_eval.  What else the epilogue needs of the system -- its index, its tile, its dt -- is formed again from them for the same
    // reason: held across the mixed loops of the fp32 STEP kernels, those scalars pushed vector registers to scratch.
#if defined(__HIP_DEVICE_COMPILE__)
    const EnsembleHermite6Args<T>* late = static_cast<const EnsembleHermite6Args<T>*>(__builtin_amdgcn_kernarg_segment_ptr());  // the one argument, at offset 0
    asm volatile("" : "+s"(late));
#else
    const EnsembleHermite6Args<T>* late = &a;  // (the host pass only parses the kernel)
#endif
    const EnsembleHermite6Args<T> e = *late;
    const unsigned                system_late = blockIdx.x / e.groups_per_system;
    const unsigned                base_late   = (blockIdx.x - system_late * e.groups_per_system) * (64 * W);
    const size_t                  origin      = 4 * static_cast<size_t>(system_late) * e.n;  // the system's first element in an array of T[4 N B]
    T                             dt_late = 0, eps2_late;
    if constexpr (STEP) system_parameters<T, STEP>(e.src, system_late, dt_late, eps2_late);  // (the same loads: the same dt)
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned local = base_late + k * 64 + lane;
        if (local >= e.n) continue;
        const size_t i = local;
        vec4         a1, j1, s1;
        a1.x = LT::get(second[0], k) * out_scale, a1.y = LT::get(second[1], k) * out_scale, a1.z = LT::get(second[2], k) * out_scale, a1.w = 0;
        j1.x = LT::get(second[3], k) * out_scale, j1.y = LT::get(second[4], k) * out_scale, j1.z = LT::get(second[5], k) * out_scale, j1.w = 0;
        s1.x = LT::get(second[6], k) * out_scale, s1.y = LT::get(second[7], k) * out_scale, s1.z = LT::get(second[8], k) * out_scale, s1.w = 0;
        if constexpr (STEP) {
#define HERMITE6_STEP_DT dt_late
#define HERMITE6_STORED(array) (e.array + origin)
#include "hermite6_correct.inc"
            reinterpret_cast<vec4*>(e.new_pos + origin)[i] = x1;
            reinterpret_cast<vec4*>(e.vel + origin)[i]     = v;
            reinterpret_cast<vec4*>(e.crackle + origin)[i] = c1;
        }
        reinterpret_cast<vec4*>(e.acc + origin)[i]  = a1;
        reinterpret_cast<vec4*>(e.jerk + origin)[i] = j1;
        reinterpret_cast<vec4*>(e.snap + origin)[i] = s1;
    }
}

// state12 <- {pos, vel, acc_in or 0} of one system's bodies; `zero`, when given, <- 0.  256 bodies of ONE system per workgroup.  HBM-bound.
template <typename T>
__global__ __launch_bounds__(256) void hermite6_ensemble_pack(T* state12, const T* pos, const T* vel, const T* acc_in, T* zero, unsigned n, unsigned partials) {
    using vec4            = typename Lane<T>::vec4;
    const unsigned system = blockIdx.x / partials;
    const unsigned local  = (blockIdx.x - system * partials) * 256u + threadIdx.x;
    if (local >= n) return;
    const size_t i = static_cast<size_t>(system) * n + local;
#include "hermite6_pack.inc"
}

// The predictor (hermite6_predict.inc) -> state12 {x_p, m, v_p, 0, a_p, 0} with the system's own dt.  256 bodies of ONE system per workgroup;
// the workgroups of a system that takes no step leave.  HBM-bound.
template <typename T>
__global__ __launch_bounds__(256) void hermite6_ensemble_predict(const T* pos, const T* vel, const T* acc, const T* jerk, const T* snap, const T* crackle, T* state12,
                                                                 unsigned n, unsigned partials, EnsembleSource<T> src) {
    using vec4            = typename Lane<T>::vec4;
    const unsigned system = blockIdx.x / partials;
    const unsigned local  = (blockIdx.x - system * partials) * 256u + threadIdx.x;
    T              dt, eps2;
    if (!system_parameters<T, true>(src, system, dt, eps2)) return;
    if (local >= n) return;
    const size_t i = static_cast<size_t>(system) * n + local;
    const vec4   x = reinterpret_cast<const vec4*>(pos)[i], v = reinterpret_cast<const vec4*>(vel)[i], a = reinterpret_cast<const vec4*>(acc)[i];
    const vec4   j = reinterpret_cast<const vec4*>(jerk)[i], s = reinterpret_cast<const vec4*>(snap)[i], c = reinterpret_cast<const vec4*>(crackle)[i];
#include "hermite6_predict.inc"
    reinterpret_cast<vec4*>(state12)[3 * i]     = xp;
    reinterpret_cast<vec4*>(state12)[3 * i + 1] = vp;
    reinterpret_cast<vec4*>(state12)[3 * i + 2] = ap;
}

// min of the Aarseth ratio over kEnsembleTimestepBodies bodies of one system -> partial[system * partials + p].  (The minimum is exact in
// any order, so the partials of the solo call and these give one value.)  With clocks: the systems that take no step in this call are left out.
template <typename T>
__global__ __launch_bounds__(256) void hermite6_ensemble_timestep_partial(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, unsigned partials,
                                                                          EnsembleSource<T> src, bool stepping, double* partial) {
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
        m = aarseth_ratio<T>(reinterpret_cast<const vec4*>(acc)[i], reinterpret_cast<const vec4*>(jerk)[i], reinterpret_cast<const vec4*>(snap)[i],
                             reinterpret_cast<const vec4*>(crackle)[i]);
    }
    m = block_min(m, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// One thread per system: the minimum of the system's partials, dt = (T)(eta sqrt(min)) -- the expression of hermite6_timestep_final -- and
// what hermite_ensemble_clock_update.inc does with it: dt_out[s], the clock of a run that starts, or the clock after this call's step
// by the rule of the header, with the block's tally.
template <typename T>
__global__ __launch_bounds__(256) void hermite6_ensemble_clock(const double* partial, unsigned partials, unsigned b, T eta, T* dt_out, EnsembleClock* clocks, bool begin,
                                                               EnsembleSource<T> src, EnsembleStatus* block_status) {
    __shared__ unsigned long long sums[5][256];
    __shared__ double             mins[2][256];
    const unsigned                s = blockIdx.x * kEnsembleClockSystems + threadIdx.x;
    Tally                         t{0, 0, 0, 0, 0, __builtin_inf(), __builtin_inf()};
    if (s < b) {
        auto next_dt = [&]() {
            double m = __builtin_inf();
            for (unsigned p = 0; p < partials; ++p) m = fmin(m, partial[static_cast<size_t>(s) * partials + p]);
            return static_cast<T>(static_cast<double>(eta) * __builtin_sqrt(m));
        };
#include "hermite_ensemble_clock_update.inc"
    }
    if (block_status == nullptr) return;  // (uniform: a kernel argument)
    t = block_tally(t, sums, mins);
    if (threadIdx.x == 0) store_tally(t, block_status + blockIdx.x);
}

static_assert(stream_lane_bodies<float>() == Lane<float>::W && stream_lane_bodies<double>() == Lane<double>::W, "plan_stream's bodies i per lane are the kernel's");

template <typename T, bool STEP> hipError_t launch_planned(EnsembleHermite6Args<T> a, unsigned b, hipStream_t stream) {
    const StreamPlan p  = plan_stream<T>(a.n, kHermite6Sums, hermite6_unroll_for<T>());
    a.groups_per_system = p.groups;
    return with_stream_waves(p.waves, [&](auto waves) {
        constexpr int S = decltype(waves)::value;
        (void)hipGetLastError();  // a launch reports ITS OWN error
        hipLaunchKernelGGL((hermite6_ensemble_eval<T, S, STEP>), dim3(p.groups * b), dim3(64 * S), 0, stream, a);
        return hipGetLastError();
    });
}

}  // namespace

template <typename T> hipError_t launch_ensemble6_pack(T* state12, const T* pos, const T* vel, const T* acc_in, T* zero, unsigned n, unsigned b, hipStream_t stream) {
    const unsigned partials = ensemble_partials(n);
    (void)hipGetLastError();
    hipLaunchKernelGGL((hermite6_ensemble_pack<T>), dim3(partials * b), dim3(256), 0, stream, state12, pos, vel, acc_in, zero, n, partials);
    return hipGetLastError();
}

template <typename T> hipError_t launch_ensemble6_eval(const EnsembleHermite6Args<T>& a, unsigned b, hipStream_t stream) { return launch_planned<T, false>(a, b, stream); }

template <typename T> hipError_t launch_ensemble6_step(const EnsembleHermite6Args<T>& a, unsigned b, T* state12, hipStream_t stream) {
    const unsigned partials = ensemble_partials(a.n);
    (void)hipGetLastError();
    hipLaunchKernelGGL((hermite6_ensemble_predict<T>), dim3(partials * b), dim3(256), 0, stream, a.old_pos, static_cast<const T*>(a.vel), static_cast<const T*>(a.acc),
                       static_cast<const T*>(a.jerk), static_cast<const T*>(a.snap), static_cast<const T*>(a.crackle), state12, a.n, partials, a.src);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    return launch_planned<T, true>(a, b, stream);
}

template <typename T>
hipError_t launch_ensemble6_clocks(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, unsigned b, T eta, T* dt_out, EnsembleClock* clocks, bool begin,
                                   const EnsembleSource<T>& src, double* partial, EnsembleStatus* block_status, EnsembleStatus* status, hipStream_t stream) {
    const unsigned partials = ensemble_partials(n), blocks = ensemble_status_blocks(b);
    const bool     stepping = dt_out == nullptr && !begin;
    (void)hipGetLastError();
    hipLaunchKernelGGL((hermite6_ensemble_timestep_partial<T>), dim3(partials * b), dim3(256), 0, stream, acc, jerk, snap, crackle, n, partials, src, stepping, partial);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL((hermite6_ensemble_clock<T>), dim3(blocks), dim3(256), 0, stream, static_cast<const double*>(partial), partials, b, eta, dt_out, clocks, begin, src,
                       status != nullptr ? block_status : nullptr);
    if (const auto err = hipGetLastError(); err != hipSuccess || status == nullptr) return err;
    hipLaunchKernelGGL(hermite_ensemble_status, dim3(1), dim3(256), 0, stream, static_cast<const EnsembleStatus*>(block_status), blocks, status);
    return hipGetLastError();
}

template hipError_t launch_ensemble6_pack<float>(float*, const float*, const float*, const float*, float*, unsigned, unsigned, hipStream_t);
template hipError_t launch_ensemble6_pack<double>(double*, const double*, const double*, const double*, double*, unsigned, unsigned, hipStream_t);
template hipError_t launch_ensemble6_eval<float>(const EnsembleHermite6Args<float>&, unsigned, hipStream_t);
template hipError_t launch_ensemble6_eval<double>(const EnsembleHermite6Args<double>&, unsigned, hipStream_t);
template hipError_t launch_ensemble6_step<float>(const EnsembleHermite6Args<float>&, unsigned, float*, hipStream_t);
template hipError_t launch_ensemble6_step<double>(const EnsembleHermite6Args<double>&, unsigned, double*, hipStream_t);
template hipError_t launch_ensemble6_clocks<float>(const float*, const float*, const float*, const float*, unsigned, unsigned, float, float*, EnsembleClock*, bool,
                                                   const EnsembleSource<float>&, double*, EnsembleStatus*, EnsembleStatus*, hipStream_t);
template hipError_t launch_ensemble6_clocks<double>(const double*, const double*, const double*, const double*, unsigned, unsigned, double, double*, EnsembleClock*, bool,
                                                    const EnsembleSource<double>&, double*, EnsembleStatus*, EnsembleStatus*, hipStream_t);

}  // namespace nb
