// hermite6_eval.hip -- the kernels of libnbody_hip_hermite6.so (include/nbody_hip_hermite6.h): accelerations, jerks AND snaps of a
// system, the 6th-order Hermite predictor and corrector around them (Nitadori & Makino 2008), and the shared time step.  gfx950 only;
// FMA contraction on.
//
// hermite6_eval<T, S, STEP> is hermite_eval (hermite_eval.hip) with a third derivative: one-sided, on the wave-stream plan, a lane holds
// one vector of bodies i -- position, velocity, acceleration: 9 vectors, and 9 sums at two levels --, the bodies j are wave-uniform,
// three adjacent vec4 of the workspace each, come in through scalar loads U at a time and enter the subtractions as scalar operands.
// The interaction is hermite6_interaction.inc; everything between the bodies i and the sums -- the chunk loop with its unit / mixed
// forms and kFlushEvery, SIMD-mate priority, the ragged last chunk, the fold -- is hermite_stream.inc, the text of hermite_eval, which
// takes the number of sums and the interaction from its includer.  The kernel below is its arguments, its bodies i, how one body j is
// addressed, and its epilogue: the corrector and the new crackle.
#include "hermite6_kernels.h"

namespace nb {
namespace {

#include "nbody_lane.h"

#include "hermite_powers.h"

#include "hermite6_ratio.h"

template <typename T> struct BodyJ {
    typename Lane<T>::raw4 p, v, a;  // {x, y, z, m}, {vx, vy, vz, -}, {ax, ay, az, -} in scalar registers
};

// Waves per SIMD the kernel is compiled for.  fp32 fits 4 (<= 128 VGPRs) like hermite_eval; fp64 -- 9 + 18 doubles of state and sums before
// a single temporary -- spilt six registers to scratch at 4 and is compiled for 3.
template <typename T> inline constexpr int kWavesPerSimd = sizeof(T) == 8 ? 3 : 4;

template <typename T, int S, bool STEP>
__global__ __launch_bounds__(64 * S) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd<T>, kWavesPerSimd<T>))) void hermite6_eval(Hermite6Args<T> a) {
    using LT             = Lane<T>;
    using vec4           = typename LT::vec4;
    using vec            = typename LT::vec;
    using raw4           = typename LT::raw4;
    using bits           = typename LT::bits;
    constexpr int W      = LT::W;  // bodies i per lane
    constexpr int U      = hermite6_unroll_for<T>();
    constexpr int STRIDE = 3;  // vec4 per body where the bodies are read
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx4/x8/x16

    const T* const   pos_base = a.state12;
    const stream_ptr jp       = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(pos_base));
    const unsigned   n        = a.n;
    const int        tid      = threadIdx.x;
    const int        wave     = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int        lane     = tid & 63;

    // bodies i of this lane: block_base + k*64 + lane
    const unsigned block_base = blockIdx.x * (64 * W);
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
    vec eps2 = LT::splat(a.eps2);
    LT::keep_in_vgpr(eps2);

    constexpr unsigned range = 0, ranges = 1;  // every workgroup streams every chunk
    auto body_j = [&](size_t j, BodyJ<T>& b) { b.p = jp[3 * j], b.v = jp[3 * j + 1], b.a = jp[3 * j + 2]; };  // adjacent
#define HERMITE_STREAM_SUMS 9
#define HERMITE_STREAM_INTERACTION "hermite6_interaction.inc"
#include "hermite_stream.inc"

    // the epilogue's pointers are fetched from the kernel arguments here, behind the loops, where they cost no scalar registers
    // (the mixed loops of the STEP kernels reloaded 16 spilt scalar registers per trip while all nine pointers were live across them)
#if defined(__HIP_DEVICE_COMPILE__)
    const Hermite6Args<T>* late = static_cast<const Hermite6Args<T>*>(__builtin_amdgcn_kernarg_segment_ptr());  // the one argument, at offset 0
    asm volatile("" : "+s"(late));
#else
    const Hermite6Args<T>* late = &a;  // (the host pass only parses the kernel)
#endif
    const Hermite6Args<T> e = *late;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned local = block_base + k * 64 + lane;
        if (local >= n) continue;
        const size_t i = local;
        vec4         a1, j1, s1;
        a1.x = LT::get(second[0], k) * out_scale, a1.y = LT::get(second[1], k) * out_scale, a1.z = LT::get(second[2], k) * out_scale, a1.w = 0;
        j1.x = LT::get(second[3], k) * out_scale, j1.y = LT::get(second[4], k) * out_scale, j1.z = LT::get(second[5], k) * out_scale, j1.w = 0;
        s1.x = LT::get(second[6], k) * out_scale, s1.y = LT::get(second[7], k) * out_scale, s1.z = LT::get(second[8], k) * out_scale, s1.w = 0;
        if constexpr (STEP) {
#define HERMITE6_STEP_DT e.dt
#define HERMITE6_STORED(array) e.array
#include "hermite6_correct.inc"
            reinterpret_cast<vec4*>(e.new_pos)[i] = x1;
            reinterpret_cast<vec4*>(e.vel)[i]     = v;
            reinterpret_cast<vec4*>(e.crackle)[i] = c1;
        }
        reinterpret_cast<vec4*>(e.acc)[i]  = a1;
        reinterpret_cast<vec4*>(e.jerk)[i] = j1;
        reinterpret_cast<vec4*>(e.snap)[i] = s1;
    }
}

// workspace <- {pos, vel, acc_in or 0}; `zero`, when given, <- 0.  HBM-bound.
template <typename T> __global__ __launch_bounds__(256) void hermite6_pack(T* state12, const T* pos, const T* vel, const T* acc_in, T* zero, unsigned n) {
    using vec4       = typename Lane<T>::vec4;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
#include "hermite6_pack.inc"
}

// The predictor -> state12 {x_p, m, v_p, 0, a_p, 0}, Horner in dt.  HBM-bound.
template <typename T>
__global__ __launch_bounds__(256) void hermite6_predict(const T* pos, const T* vel, const T* acc, const T* jerk, const T* snap, const T* crackle, T* state12, unsigned n, T dt) {
    using vec4       = typename Lane<T>::vec4;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const vec4 x = reinterpret_cast<const vec4*>(pos)[i], v = reinterpret_cast<const vec4*>(vel)[i], a = reinterpret_cast<const vec4*>(acc)[i];
    const vec4 j = reinterpret_cast<const vec4*>(jerk)[i], s = reinterpret_cast<const vec4*>(snap)[i], c = reinterpret_cast<const vec4*>(crackle)[i];
#include "hermite6_predict.inc"
    reinterpret_cast<vec4*>(state12)[3 * static_cast<size_t>(i)]     = xp;
    reinterpret_cast<vec4*>(state12)[3 * static_cast<size_t>(i) + 1] = vp;
    reinterpret_cast<vec4*>(state12)[3 * static_cast<size_t>(i) + 2] = ap;
}

#include "block_min.inc"

template <typename T>
__global__ __launch_bounds__(256) void hermite6_timestep_partial(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, double* partial) {
    using vec4 = typename Lane<T>::vec4;
    __shared__ double lds[256];
    double            m = __builtin_inf();
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256u) {
        m = fmin(m, aarseth_ratio<T>(reinterpret_cast<const vec4*>(acc)[i], reinterpret_cast<const vec4*>(jerk)[i], reinterpret_cast<const vec4*>(snap)[i],
                                     reinterpret_cast<const vec4*>(crackle)[i]));
    }
    m = block_min(m, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

template <typename T> __global__ __launch_bounds__(256) void hermite6_timestep_final(const double* partial, unsigned count, T eta, T* dt_out) {
    __shared__ double lds[256];
    double            m = __builtin_inf();
    for (unsigned i = threadIdx.x; i < count; i += 256u) m = fmin(m, partial[i]);
    m = block_min(m, lds);
    if (threadIdx.x == 0) dt_out[0] = static_cast<T>(static_cast<double>(eta) * __builtin_sqrt(m));
}

static_assert(stream_lane_bodies<float>() == Lane<float>::W && stream_lane_bodies<double>() == Lane<double>::W, "plan_stream's bodies i per lane are the kernel's");

template <typename T, bool STEP> hipError_t launch_planned(const Hermite6Args<T>& a, hipStream_t stream) {
    const StreamPlan p = plan_stream<T>(a.n, kHermite6Sums, hermite6_unroll_for<T>());
    return with_stream_waves(p.waves, [&](auto waves) {
        constexpr int S = decltype(waves)::value;
        (void)hipGetLastError();  // a launch reports ITS OWN error
        hipLaunchKernelGGL((hermite6_eval<T, S, STEP>), dim3(p.groups), dim3(64 * S), 0, stream, a);
        return hipGetLastError();
    });
}

}  // namespace

template <typename T> hipError_t launch_hermite6_pack(T* workspace, const T* pos, const T* vel, const T* acc_in, T* zero, unsigned n, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((hermite6_pack<T>), dim3((n + 255u) / 256u), dim3(256), 0, stream, workspace, pos, vel, acc_in, zero, n);
    return hipGetLastError();
}

template <typename T> hipError_t launch_hermite6_eval(const Hermite6Args<T>& a, hipStream_t stream) { return launch_planned<T, false>(a, stream); }

template <typename T> hipError_t launch_hermite6_step(const Hermite6Args<T>& a, T* workspace, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((hermite6_predict<T>), dim3((a.n + 255u) / 256u), dim3(256), 0, stream, a.old_pos, static_cast<const T*>(a.vel), static_cast<const T*>(a.acc),
                       static_cast<const T*>(a.jerk), static_cast<const T*>(a.snap), static_cast<const T*>(a.crackle), workspace, a.n, a.dt);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    return launch_planned<T, true>(a, stream);
}

template <typename T>
hipError_t launch_hermite6_timestep(const T* acc, const T* jerk, const T* snap, const T* crackle, unsigned n, T eta, T* dt_out, double* scratch, hipStream_t stream) {
    const unsigned blocks = (n + 255u) / 256u < kHermite6TimestepPartials ? (n + 255u) / 256u : kHermite6TimestepPartials;
    (void)hipGetLastError();
    hipLaunchKernelGGL((hermite6_timestep_partial<T>), dim3(blocks), dim3(256), 0, stream, acc, jerk, snap, crackle, n, scratch);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL((hermite6_timestep_final<T>), dim3(1), dim3(256), 0, stream, static_cast<const double*>(scratch), blocks, eta, dt_out);
    return hipGetLastError();
}

template hipError_t launch_hermite6_pack<float>(float*, const float*, const float*, const float*, float*, unsigned, hipStream_t);
template hipError_t launch_hermite6_pack<double>(double*, const double*, const double*, const double*, double*, unsigned, hipStream_t);
template hipError_t launch_hermite6_eval<float>(const Hermite6Args<float>&, hipStream_t);
template hipError_t launch_hermite6_eval<double>(const Hermite6Args<double>&, hipStream_t);
template hipError_t launch_hermite6_step<float>(const Hermite6Args<float>&, float*, hipStream_t);
template hipError_t launch_hermite6_step<double>(const Hermite6Args<double>&, double*, hipStream_t);
template hipError_t launch_hermite6_timestep<float>(const float*, const float*, const float*, const float*, unsigned, float, float*, double*, hipStream_t);
template hipError_t launch_hermite6_timestep<double>(const double*, const double*, const double*, const double*, unsigned, double, double*, double*, hipStream_t);

}  // namespace nb
