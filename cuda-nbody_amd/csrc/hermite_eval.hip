// hermite_eval.hip -- the kernels of libnbody_hip_hermite.so (include/nbody_hip_hermite.h): accelerations AND jerks of a system,
// the 4th-order Hermite predictor and corrector around them, and the shared time step.  gfx950 only; FMA contraction on.
//
// hermite_eval<T, S, STEP> is one-sided, on the plan of the wave-stream kernel (nbody_fast_stream.inc): a lane holds one vector of
// bodies i (fp32: a packed pair -> v_pk_*_f32; fp64: one body) -- position, velocity, acceleration sum and jerk sum, 12 vectors --,
// the bodies j are wave-uniform, come in through scalar loads U at a time (one group ahead of the one being computed, two register
// sets) and enter the packed subtractions as scalar operands; the S waves of a workgroup share the bodies i, split the bodies j by
// chunks of 128 (chunk c -> wave c mod S) and fold their sums through LDS in a fixed order.  No LDS access and no barrier inside
// the streaming loops, no atomics anywhere, no scratch, <= 128 VGPRs.
//
// Per interaction, r = x_j - x_i, w = v_j - v_i, s2 = r.r + eps2:
//     k = m_j s^-3,   a += k r,   jerk += k (w - 3 (r.w) s^-2 r)
// fp32: 25 packed ops + 2 v_rsq_f32 per packed pair in the loop without the mass multiply, 26 with it.
//
// Sums.  A register sum collects at most 8 chunks (1 024 bodies j) of ONE form -- "unit": every mass of the chunk is the reference
// mass (the first body's, when usable_unit allows), no multiply in the loop; "mixed": the raw mass multiplies in the loop -- and is
// then added to the lane's second-level sum, scaled once (1, or 1 / m_ref).  Two levels of <= 1 024 and <= N / (1 024 S) + form
// changes terms keep an fp32 sum at a few 1e-6 of its term magnitudes for any N.  The order depends on (N, precision) and the
// masses alone, so results are bit-identical from call to call, stream to stream and device to device.
//
// Where the text lives.  The kernel below is its arguments, its bodies i, how one body j is addressed, and its epilogue; everything
// between the bodies i and the sums -- the interaction, the chunk loop, SIMD-mate priority, the fold -- is hermite_stream.inc (with
// wave_groups.inc, wave_mates.inc and wave_fold.inc inside it), which hermite_block_eval includes too.  The predictor is
// hermite_body.h, the corrector hermite_correct.inc, S and the chunk count wave_stream.h.
#include "hermite_kernels.h"

namespace nb {
namespace {

#include "nbody_lane.h"

#include "hermite_stream.h"

#include "hermite_body.h"

template <typename T, int S, bool STEP>
__global__ __launch_bounds__(64 * S) __attribute__((amdgpu_waves_per_eu(4, 4))) void hermite_eval(HermiteArgs<T> a) {
    using LT            = Lane<T>;
    using vec4          = typename LT::vec4;
    using vec           = typename LT::vec;
    using raw4          = typename LT::raw4;
    using bits          = typename LT::bits;
    constexpr int W     = LT::W;  // bodies i per lane
    constexpr int U     = unroll_for<T>();
    constexpr int STRIDE = STEP ? 2 : 1;  // vec4 per body where the bodies are read
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx4/x8/x16

    const T* const   pos_base = STEP ? a.state8 : a.pos;
    const T* const   vel_base = STEP ? a.state8 + 4 : a.vel_in;
    const stream_ptr jp       = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(pos_base));
    const stream_ptr jv       = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(vel_base));
    const unsigned   n        = a.n;
    const int        tid      = threadIdx.x;
    const int        wave     = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int        lane     = tid & 63;

    // bodies i of this lane: block_base + k*64 + lane (coalesced across the lanes of a wave)
    const unsigned block_base = blockIdx.x * (64 * W);
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
    vec eps2 = LT::splat(a.eps2);
    LT::keep_in_vgpr(eps2);

    constexpr unsigned range = 0, ranges = 1;  // every workgroup streams every chunk
    auto body_j = [&](size_t j, BodyJ<T>& b) {
        if constexpr (STEP) {
            b.p = jp[2 * j], b.v = jp[2 * j + 1];  // adjacent: one s_load_dwordx8 / x16
        } else {
            b.p = jp[j], b.v = jv[j];
        }
    };
#include "hermite_stream.inc"

#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned local = block_base + k * 64 + lane;
        if (local >= n) continue;
        const size_t i = local;
        vec4         a1, j1;
        a1.x = LT::get(second[0], k) * out_scale, a1.y = LT::get(second[1], k) * out_scale, a1.z = LT::get(second[2], k) * out_scale, a1.w = 0;
        j1.x = LT::get(second[3], k) * out_scale, j1.y = LT::get(second[4], k) * out_scale, j1.z = LT::get(second[5], k) * out_scale, j1.w = 0;
        if constexpr (STEP) {
            const T    dt = a.dt;
            const vec4 x  = reinterpret_cast<const vec4*>(a.old_pos)[i];
            vec4       v  = reinterpret_cast<const vec4*>(a.vel)[i];
            const vec4 a0 = reinterpret_cast<const vec4*>(a.acc)[i];
            const vec4 j0 = reinterpret_cast<const vec4*>(a.jerk)[i];
#include "hermite_correct.inc"
            reinterpret_cast<vec4*>(a.new_pos)[i] = x1;
            reinterpret_cast<vec4*>(a.vel)[i]     = v;
        }
        reinterpret_cast<vec4*>(a.acc)[i]  = a1;
        reinterpret_cast<vec4*>(a.jerk)[i] = j1;
    }
}

// The predictor (hermite_body.h) -> state8 {x_p, m, v_p, 0}.  HBM-bound.
template <typename T> __global__ __launch_bounds__(256) void hermite_predict(const T* pos, const T* vel, const T* acc, const T* jerk, T* state8, unsigned n, T dt) {
    using vec4       = typename Lane<T>::vec4;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const vec4 x = reinterpret_cast<const vec4*>(pos)[i], v = reinterpret_cast<const vec4*>(vel)[i];
    const vec4 a = reinterpret_cast<const vec4*>(acc)[i], j = reinterpret_cast<const vec4*>(jerk)[i];
    vec4       xp, vp;
    predict_body<T>(x, v, a, j, dt, xp, vp);
    reinterpret_cast<vec4*>(state8)[2 * static_cast<size_t>(i)]     = xp;
    reinterpret_cast<vec4*>(state8)[2 * static_cast<size_t>(i) + 1] = vp;
}

#include "hermite_ratio.h"

#include "block_min.inc"

template <typename T> __global__ __launch_bounds__(256) void hermite_timestep_partial(const T* acc, const T* jerk, unsigned n, double* partial) {
    using vec4 = typename Lane<T>::vec4;
    __shared__ double lds[256];
    double            m = __builtin_inf();
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256u) {
        m = fmin(m, norm_ratio<T>(reinterpret_cast<const vec4*>(acc)[i], reinterpret_cast<const vec4*>(jerk)[i]));
    }
    m = block_min(m, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

template <typename T> __global__ __launch_bounds__(256) void hermite_timestep_final(const double* partial, unsigned count, T eta, T* dt_out) {
    __shared__ double lds[256];
    double            m = __builtin_inf();
    for (unsigned i = threadIdx.x; i < count; i += 256u) m = fmin(m, partial[i]);
    m = block_min(m, lds);
    if (threadIdx.x == 0) dt_out[0] = eta * static_cast<T>(m);  // m: the smallest |a| / |jerk| (hermite_ratio.h)
}

static_assert(stream_lane_bodies<float>() == Lane<float>::W && stream_lane_bodies<double>() == Lane<double>::W, "plan_stream's bodies i per lane are the kernel's");

template <typename T, bool STEP> hipError_t launch_planned(const HermiteArgs<T>& a, hipStream_t stream) {
    const StreamPlan p = plan_stream<T>(a.n, kHermiteSums, unroll_for<T>());
    return with_stream_waves(p.waves, [&](auto waves) {
        constexpr int S = decltype(waves)::value;
        (void)hipGetLastError();  // a launch reports ITS OWN error
        hipLaunchKernelGGL((hermite_eval<T, S, STEP>), dim3(p.groups), dim3(64 * S), 0, stream, a);
        return hipGetLastError();
    });
}

}  // namespace

template <typename T> hipError_t launch_hermite_eval(const HermiteArgs<T>& a, hipStream_t stream) { return launch_planned<T, false>(a, stream); }

template <typename T> hipError_t launch_hermite_step(const HermiteArgs<T>& a, T* workspace, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((hermite_predict<T>), dim3((a.n + 255u) / 256u), dim3(256), 0, stream, a.old_pos, static_cast<const T*>(a.vel), static_cast<const T*>(a.acc),
                       static_cast<const T*>(a.jerk), workspace, a.n, a.dt);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    return launch_planned<T, true>(a, stream);
}

template <typename T> hipError_t launch_hermite_timestep(const T* acc, const T* jerk, unsigned n, T eta, T* dt_out, double* scratch, hipStream_t stream) {
    const unsigned blocks = (n + 255u) / 256u < kTimestepPartials ? (n + 255u) / 256u : kTimestepPartials;
    (void)hipGetLastError();
    hipLaunchKernelGGL((hermite_timestep_partial<T>), dim3(blocks), dim3(256), 0, stream, acc, jerk, n, scratch);
    if (const auto err = hipGetLastError(); err != hipSuccess) return err;
    hipLaunchKernelGGL((hermite_timestep_final<T>), dim3(1), dim3(256), 0, stream, static_cast<const double*>(scratch), blocks, eta, dt_out);
    return hipGetLastError();
}

template hipError_t launch_hermite_eval<float>(const HermiteArgs<float>&, hipStream_t);
template hipError_t launch_hermite_eval<double>(const HermiteArgs<double>&, hipStream_t);
template hipError_t launch_hermite_step<float>(const HermiteArgs<float>&, float*, hipStream_t);
template hipError_t launch_hermite_step<double>(const HermiteArgs<double>&, double*, hipStream_t);
template hipError_t launch_hermite_timestep<float>(const float*, const float*, unsigned, float, float*, double*, hipStream_t);
template hipError_t launch_hermite_timestep<double>(const double*, const double*, unsigned, double, double*, double*, hipStream_t);

}  // namespace nb
