// nbody_strict.hip -- the bit-reproducing kernels (NB_MODE_STRICT).  gfx950 only.
//
// MUST be compiled with -ffp-contract=off (csrc/Makefile does): every arithmetic op below has to stay
// the separate IEEE-754 mul/add/sub/div/sqrt the reference's CPU path executes
// (/root/reference/src/nbody/bodysystemcpu.cpp:140-303).  hipcc's defaults supply the rest:
// correctly rounded fp32 divide/sqrt (-fhip-fp32-correctly-rounded-divide-sqrt is on by default),
// fp32 denormals kept, IEEE mode on.
//
// Mapping: one lane = one body i (bodysystemcuda.cu:151 uses the same mapping); every wave streams ALL bodies j of the
// range in ascending order through its own double-buffered 128-body LDS ring (no workgroup barrier in the loop: a wave
// reads only what it wrote itself), so each body i sees j = j_begin .. j_begin+j_count-1 in exactly the CPU path's order
// (bodysystemcpu.cpp:156 / :251).  Results do not depend on the launch geometry, so launch_strict picks it; the
// reference's --blockSize is validated and otherwise a hint.
//
// Two arithmetic forms of the same IEEE operations:
//   * generic : `/` and sqrtf as hipcc expands them (v_div_scale/v_rcp/fma chain/v_div_fmas/v_div_fixup; v_sqrt + the
//     +-1 ulp residual checks + denormal-range scaling): correct for every input, ~37 VALU per interaction.
//   * fast (fp32): two CONSECUTIVE bodies j travel as a PACKED pair against the lane's body i (v_pk_add/mul/fma_f32 are
//     the same IEEE operations, two lanes' worth per instruction; only the three running sums take the two results
//     one after the other, in j order), and divide / sqrt run WITHOUT the scaling and fix-up steps: those only act
//     on operands outside a window that is checked up front -- all coordinates |c| <= 2^18, softening^2 in
//     [2^-39, 2^38], masses +0 or 2^-40 <= |m| <= 2^40 -- per wave (bodies i) and per 128-body chunk (bodies j), and any
//     chunk outside it takes the generic form.  Inside the window r2 is in [2^-39, 2^40], r2^2 in [2^-78, 2^80], and
//       sqrt : r = rsq(x); s = x*r; h = r/2; d = fma(-s,s,x); s = fma(d,h,s)
//              == sqrtf(x) for EVERY float in [2^-100, 2^127)   (exhaustive: tools/strict_unit_mass_check.hip; so is LLVM's
//              longer form with the extra e = fma(-h,s,1/2); h = fma(h,e,h); s = fma(s,e,s) step, which rounds 1-3 used)
//       div  : r = rcp(d); e = fma(-d,r,1); r = fma(e,r,r); q = n*r; e = fma(-d,q,n); q = fma(e,r,q)
//              == n/d for EVERY pair of significands (2^46 quotients, tools/strict_divide_exhaustive.hip,
//              profiles/round2_strict_divide_exhaustive.txt; every step scales exactly with the operands' exponents inside the
//              window, v_rcp_f32 included, so that covers all operands).  hipcc's own sequence corrects the quotient a second
//              time (e = fma(-d,q,n); q = fma(e,r,q) again): also exact, never needed.
//     23 packed ops + 6 adds + 4 transcendentals per two interactions.
//       unit : a chunk whose masses are all exactly 1.0f (every start-up configuration of the reference) needs 1/d, not m/d:
//              r = rcp(d); e = fma(-d,r,1); r = fma(e,r,r) == 1.0f/d for EVERY float d in [2^-100, 2^101) (exhaustive, same
//              tool, profiles/round2_strict_unit_mass_check.txt): 20 packed ops + 6 adds + 4 transcendentals.
//   * fast (fp64): one interaction at a time (no packed fp64), the same scaling-free divide and sqrt with its own window.
#include "nbody_kernels.h"

namespace nb {
namespace {

#include "nbody_strict_body.h"

template <typename T> __global__ __launch_bounds__(512, 4) void integrate_bodies_strict(Shard<T> s) {
    const unsigned block = blockIdx.x;
#include "nbody_strict_step.inc"
}

}  // namespace

// Geometry: results do not depend on it, so the library picks it (the caller's --blockSize is validated by the C-ABI and
// otherwise a hint).  512-thread workgroups (two waves per SIMD each, kept level by the priority scheme; two of them
// share a CU) while that still gives every CU at least one; smaller workgroups for smaller shards so that the bodies
// spread over all CUs.
template <typename T> hipError_t launch_strict(const Shard<T>& s, int block_size, int cu_count, hipStream_t stream, bool prepare_only) {
    (void)block_size;
    unsigned p = 512;
    while (p > 64 && (s.i_count + p - 1) / p < static_cast<unsigned>(cu_count)) p /= 2;
    const unsigned blocks = (s.i_count + p - 1) / p;
    const size_t   smem   = static_cast<size_t>(p / 64) * 2 * kChunk * 4 * sizeof(T) + 256;  // the waves' rings + progress words
    if (smem > 64u * 1024u) {  // fp64 at p = 512: 65 792 B
        if (const auto err = allow_large_lds<&integrate_bodies_strict<T>>(); err != hipSuccess) return err;
    }
    if (prepare_only) return hipSuccess;  // graph capture arms the attribute before hipStreamBeginCapture
    (void)hipGetLastError();  // a launch reports ITS OWN error: the call returns, and clears, the thread's last error whatever left it (a refused allocation, say)
    hipLaunchKernelGGL(integrate_bodies_strict<T>, dim3(blocks), dim3(p), smem, stream, s);
    return hipGetLastError();
}

template hipError_t launch_strict<float>(const Shard<float>&, int, int, hipStream_t, bool);
template hipError_t launch_strict<double>(const Shard<double>&, int, int, hipStream_t, bool);

}  // namespace nb
