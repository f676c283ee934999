// nbody_strict_body.h -- the bit-reproducing STRICT step, shared by nbody_strict.hip (integrate_bodies_strict) and ensemble_strict.hip
// (one such step per system of an ensemble): the interaction forms and operand windows below, and nbody_strict_step.inc, the kernel
// body itself.  See nbody_strict.hip's header for the arithmetic.  Every unit that includes it MUST be compiled with nbody_strict.o's
// flags (-ffp-contract=off -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp: csrc/Makefile).  Included inside the unit's
// own anonymous namespace.
#pragma once

typedef float v2f __attribute__((ext_vector_type(2)));

template <typename T> struct V4;
template <> struct V4<float> { using type = float4; };
template <> struct V4<double> { using type = double4; };

// sqrtf/sqrt lower to llvm.sqrt and `/` to fdiv, both expanded correctly rounded under hipcc's defaults.
// (NOT __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS that is the 1-ulp native v_sqrt_f32.)
__device__ __forceinline__ float  sqrt_T(float x) { return sqrtf(x); }
__device__ __forceinline__ double sqrt_T(double x) { return sqrt(x); }

// r2 as the CPU path forms it:
//   fp32  bodysystemcpu.cpp:186-188   ((eps2 + dx2) + dy2) + dz2
//   fp64  bodysystemcpu.cpp:262-266   (dx2 + dy2) + (dz2 + eps2)
__device__ __forceinline__ float  r2_T(float dx2, float dy2, float dz2, float eps2) { return ((eps2 + dx2) + dy2) + dz2; }
__device__ __forceinline__ double r2_T(double dx2, double dy2, double dz2, double eps2) { return (dx2 + dy2) + (dz2 + eps2); }

// one interaction, generic form (any operand values)
template <typename T> __device__ __forceinline__ void interact_generic(const typename V4<T>::type bj, T pix, T piy, T piz, T& ax, T& ay, T& az, T eps2) {
    const T dx  = bj.x - pix;
    const T dy  = bj.y - piy;
    const T dz  = bj.z - piz;
    const T dx2 = dx * dx;
    const T dy2 = dy * dy;
    const T dz2 = dz * dz;
    const T r2  = r2_T(dx2, dy2, dz2, eps2);
    const T r   = sqrt_T(r2);
    const T mr4 = bj.w / (r2 * r2);
    const T mr3 = mr4 * r;
    ax          = ax + mr3 * dx;  // contraction is off: mul, then add (bodysystemcpu.cpp:200-210 / :278-280)
    ay          = ay + mr3 * dy;
    az          = az + mr3 * dz;
}

__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }

// 2*U interactions: the lane's body i against U pairs {j, j+1} of consecutive bodies, fast form; valid inside the operand
// window only.  Written stage by stage over the U independent pairs so that their dependent chains interleave (the
// divide and sqrt chains are ~20 dependent operations long); the running sums take the 2*U results in j order.
// UNIT: every mass of the pairs is exactly 1.0f (bm is not read).
template <int U, bool UNIT>
__device__ __forceinline__ void interact_jpairs_fast(const v2f (&bx)[U], const v2f (&by)[U], const v2f (&bz)[U], const v2f (&bm)[U], float pix, float piy, float piz, float& ax, float& ay, float& az, v2f eps2) {
    const v2f half = {0.5f, 0.5f}, one = {1.0f, 1.0f};
    v2f dx[U], dy[U], dz[U], x[U], r[U], mr3[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        dx[u] = bx[u] - v2f{pix, pix};
        dy[u] = by[u] - v2f{piy, piy};
        dz[u] = bz[u] - v2f{piz, piz};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = ((eps2 + dx[u] * dx[u]) + dy[u] * dy[u]) + dz[u] * dz[u];  // r2
    {   // r = sqrt(r2), correctly rounded
        v2f s[U], h[U], dd[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const v2f rs = v2f{__builtin_amdgcn_rsqf(x[u].x), __builtin_amdgcn_rsqf(x[u].y)};
            s[u]         = x[u] * rs;
            h[u]         = rs * half;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) dd[u] = pk_fma(-s[u], s[u], x[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = pk_fma(dd[u], h[u], s[u]);
    }
    {   // mr4 = m / (r2*r2), correctly rounded; mr3 = mr4 * r
        v2f d[U], rc[U], q[U], e[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            d[u]  = x[u] * x[u];
            rc[u] = v2f{__builtin_amdgcn_rcpf(d[u].x), __builtin_amdgcn_rcpf(d[u].y)};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) e[u] = pk_fma(-d[u], rc[u], one);
#pragma unroll
        for (int u = 0; u < U; ++u) rc[u] = pk_fma(e[u], rc[u], rc[u]);
        if constexpr (UNIT) {  // 1/d: the Newton step above already gave the correctly rounded reciprocal
#pragma unroll
            for (int u = 0; u < U; ++u) mr3[u] = rc[u] * r[u];
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) q[u] = bm[u] * rc[u];
#pragma unroll
            for (int u = 0; u < U; ++u) e[u] = pk_fma(-d[u], q[u], bm[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) mr3[u] = pk_fma(e[u], rc[u], q[u]) * r[u];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const v2f tx = mr3[u] * dx[u], ty = mr3[u] * dy[u], tz = mr3[u] * dz[u];
        ax = (ax + tx.x) + tx.y;
        ay = (ay + ty.x) + ty.y;
        az = (az + tz.x) + tz.y;
    }
}

// fp64 has no packed form, but the same scaling-free divide and sqrt apply: hipcc's own sequences (v_rcp_f64 + two Newton
// steps + quotient + one residual correction; v_rsq_f64 + Goldschmidt step + two residual corrections) without
// v_div_scale / v_div_fmas' scaling / v_div_fixup / the 2^256 pre-scaling and the class check of sqrt, all of which are the
// identity inside the window: |coordinate| <= 2^100, softening^2 in [2^-100, 2^100], mass +0 or 2^-100 <= |m| <= 2^100
// (r2 in [2^-100, 2^203], r2^2 in [2^-200, 2^406], quotient in [2^-506, 2^300]).  Checked on 1.7e10 random + structured
// operands and by asking v_div_scale_f64 itself over the window's exponent range (tools/strict_fastpath_check.hip).
__device__ __forceinline__ double fast_sqrt_f64(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double       g = x * y;
    double       h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g              = __builtin_fma(g, r, g);
    h              = __builtin_fma(h, r, h);
    double d       = __builtin_fma(-g, g, x);
    g              = __builtin_fma(d, h, g);
    d              = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
__device__ __forceinline__ double fast_div_f64(double n, double d) {
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
    r        = __builtin_fma(r, e, r);
    e        = __builtin_fma(-d, r, 1.0);
    r        = __builtin_fma(r, e, r);
    const double q = n * r;
    e              = __builtin_fma(-d, q, n);
    return __builtin_fma(e, r, q);
}
// UNIT: the body's mass is exactly 1.0 -- the same sequence with n = 1, where q = n*r is r itself (bj.w is not read)
template <bool UNIT> __device__ __forceinline__ void interact_fast_f64(const double4 bj, double pix, double piy, double piz, double& ax, double& ay, double& az, double eps2) {
    const double dx  = bj.x - pix;
    const double dy  = bj.y - piy;
    const double dz  = bj.z - piz;
    const double r2  = r2_T(dx * dx, dy * dy, dz * dz, eps2);
    const double r   = fast_sqrt_f64(r2);
    const double mr4 = fast_div_f64(UNIT ? 1.0 : bj.w, r2 * r2);
    const double mr3 = mr4 * r;
    ax               = ax + mr3 * dx;
    ay               = ay + mr3 * dy;
    az               = az + mr3 * dz;
}
__device__ __forceinline__ bool coord_in_window(double c) { return __builtin_fabs(c) <= 0x1p100; }  // false for NaN / inf
__device__ __forceinline__ bool mass_in_window(double m) {
    const double a = __builtin_fabs(m);
    return __double_as_longlong(m) == 0ll || (a >= 0x1p-100 && a <= 0x1p100);
}
__device__ __forceinline__ bool softening_in_window(float e2) { return e2 >= 0x1p-39f && e2 <= 0x1p38f; }
__device__ __forceinline__ bool softening_in_window(double e2) { return e2 >= 0x1p-100 && e2 <= 0x1p100; }

// operand window of the fast form (see the header)
__device__ __forceinline__ bool coord_in_window(float c) { return __builtin_fabsf(c) <= 0x1p18f; }  // false for NaN / inf
__device__ __forceinline__ bool mass_in_window(float m) {
    const float a = __builtin_fabsf(m);
    return __float_as_uint(m) == 0u || (a >= 0x1p-40f && a <= 0x1p40f);  // -0 excluded: the sequence returns +0 for it
}

// A wave's LDS traffic is ordered, so data a wave writes for ITSELF needs no s_barrier.
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

constexpr int kChunk = 128;  // bodies j per wave and ring slot, two per lane (64: +2.3 % time, 256: -0.7 % but fp64 rings would halve the occupancy)
constexpr int kPerLane = kChunk / 64;
