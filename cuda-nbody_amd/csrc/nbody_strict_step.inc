// nbody_strict_step.inc -- the body of the STRICT kernel (nbody_strict_body.h), included INSIDE a kernel's braces: by
// integrate_bodies_strict (nbody_strict.hip) and by the ensemble's STRICT kernel (ensemble_strict.hip).  The kernel provides
//   `s`     : Shard<T>, the shard to step (the ensemble's: its system's arrays and parameters)
//   `block` : unsigned, the workgroup's index within that shard's grid (bodies i [block * blockDim.x, (block + 1) * blockDim.x))
// A text include rather than a __device__ function: inlined from a function the body compiles to other (equivalent) ISA, and the
// product's kernel keeps the ISA it had.  No include guard on purpose.
// The ring holds the chunk as x[64] y[64] z[64] m[64] (so that {j, j+1} of one component is one aligned 8-byte broadcast read).
    using vec4 = typename V4<T>::type;
    extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];

    const vec4* __restrict__ old_pos = reinterpret_cast<const vec4*>(s.old_pos);
    const unsigned p    = blockDim.x;
    const unsigned tid  = threadIdx.x;
    const unsigned lane = tid & 63u;
    T* ring = reinterpret_cast<T*>(smem_raw) + (tid >> 6) * (2 * 4 * kChunk);  // this wave's [2][4][kChunk]

    const unsigned local  = block * p + tid;
    const bool     active = local < s.i_count;
    const unsigned i      = s.i_begin + (active ? local : s.i_count - 1);
    const vec4     pi     = old_pos[i];
    T              ax = 0, ay = 0, az = 0;
    if (s.acc_in) {
        const vec4 a = reinterpret_cast<const vec4*>(s.acc)[i];
        ax = a.x, ay = a.y, az = a.z;
    }
    const T eps2 = s.eps2;

    // fast form: decided per wave for the bodies i ...
    bool wave_in_window;
    {
        const bool mine = coord_in_window(pi.x) && coord_in_window(pi.y) && coord_in_window(pi.z);
        wave_in_window  = __builtin_amdgcn_ballot_w64(!mine) == 0 && softening_in_window(eps2);
    }

    // The SIMD arbiter is strictly oldest-first, and one wave alone reaches only 3/4 of a SIMD's issue rate: without help
    // the older of the two waves a 512-thread workgroup puts on each SIMD finishes well before the younger, which runs
    // the rest alone.  As in the FAST kernel (nbody_fast.hip), each wave publishes its chunk count and the one that is not
    // ahead of its SIMD mates (HW_ID.SIMD_ID) runs at priority 3, the other at 0.
    unsigned* const    balance    = reinterpret_cast<unsigned*>(smem_raw + static_cast<size_t>(p / 64) * 2 * 4 * kChunk * sizeof(T));
    unsigned* const    simd_count = balance;                                            // [4]
    volatile unsigned* progress   = reinterpret_cast<volatile unsigned*>(balance + 4);  // [4][8]
    if (tid < 36) balance[tid] = tid < 4 ? 0u : 0xffffffffu;
    __syncthreads();
    const unsigned simd = static_cast<unsigned>(__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4));  // HW_REG_HW_ID[5:4]
    unsigned       slot = 0;
    if (lane == 0) slot = atomicAdd(&simd_count[simd], 1u);
    slot                = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(slot))) & 7u;
    volatile unsigned* const mine = progress + simd * 8;
    if (lane == 0) mine[slot] = 0;

    const unsigned n_chunks = (s.j_count + kChunk - 1) / kChunk;
    struct Loaded {
        vec4 v[kPerLane];
    };
    auto load_chunk = [&](unsigned c) -> Loaded {
        Loaded out;
#pragma unroll
        for (int r = 0; r < kPerLane; ++r) {
            const unsigned j = c * kChunk + r * 64 + lane;
            vec4           v;
            v.x = v.y = v.z = v.w = 0;
            if (j < s.j_count) v = old_pos[s.j_begin + j];
            out.v[r] = v;
        }
        return out;
    };
    // ... and per chunk for the bodies j (slots past the end of the range hold zeros and are never visited)
    // (returns 0: outside the window, 1: inside, 2: inside and every mass of the chunk is exactly 1)
    auto store_chunk = [&](int buf, unsigned c, const Loaded& loaded) -> int {
        bool ok = true, unit = true;
#pragma unroll
        for (int r = 0; r < kPerLane; ++r) {
            const vec4 v   = loaded.v[r];
            T*         dst = ring + buf * (4 * kChunk) + r * 64 + lane;
            dst[0 * kChunk] = v.x, dst[1 * kChunk] = v.y, dst[2 * kChunk] = v.z, dst[3 * kChunk] = v.w;
            ok   = ok && coord_in_window(v.x) && coord_in_window(v.y) && coord_in_window(v.z) && mass_in_window(v.w);
            unit = unit && (v.w == T(1) || c * kChunk + r * 64 + lane >= s.j_count);
        }
        if (__builtin_amdgcn_ballot_w64(!ok) != 0) return 0;
        return __builtin_amdgcn_ballot_w64(!unit) == 0 ? 2 : 1;
    };

    int    chunk_form = 0;
    Loaded next;
    if (n_chunks > 0) {
        next       = load_chunk(0);
        chunk_form = store_chunk(0, 0, next);
    }
    wave_lds_sync();

    int cur = 0;
    for (unsigned c = 0; c < n_chunks; ++c) {
        const bool have_next = (c + 1) < n_chunks;
        if (have_next) next = load_chunk(c + 1);  // in flight across the compute below
        {
            unsigned least = c;
#pragma unroll
            for (int q = 0; q < 8; ++q) least = min(least, mine[q]);  // unsynchronised reads: a stale value only delays a priority change
            if (static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(least))) >= c) {
                __builtin_amdgcn_s_setprio(3);
            } else {
                __builtin_amdgcn_s_setprio(0);
            }
        }
        const unsigned cnt = min(static_cast<unsigned>(kChunk), s.j_count - c * kChunk);
        const T* __restrict__ cx = ring + cur * (4 * kChunk);
        const T* __restrict__ cy = cx + kChunk;
        const T* __restrict__ cz = cy + kChunk;
        const T* __restrict__ cm = cz + kChunk;

        unsigned k = 0;
        if constexpr (sizeof(T) == 4) {
            if (wave_in_window && chunk_form != 0) {
                const v2f e2 = {eps2, eps2};
                constexpr int U = 4;  // pairs in flight
                if (chunk_form == 2) {  // unit masses: the reciprocal form, the masses are not even read
#pragma unroll 1
                    for (; k + 2 * U <= cnt; k += 2 * U) {
                        v2f bx[U], by[U], bz[U], bm[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            bx[u] = *reinterpret_cast<const v2f*>(cx + k + 2 * u), by[u] = *reinterpret_cast<const v2f*>(cy + k + 2 * u);
                            bz[u] = *reinterpret_cast<const v2f*>(cz + k + 2 * u), bm[u] = v2f{1.0f, 1.0f};
                        }
                        interact_jpairs_fast<U, true>(bx, by, bz, bm, pi.x, pi.y, pi.z, ax, ay, az, e2);
                    }
                } else {
#pragma unroll 1
                    for (; k + 2 * U <= cnt; k += 2 * U) {
                        v2f bx[U], by[U], bz[U], bm[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            bx[u] = *reinterpret_cast<const v2f*>(cx + k + 2 * u), by[u] = *reinterpret_cast<const v2f*>(cy + k + 2 * u);
                            bz[u] = *reinterpret_cast<const v2f*>(cz + k + 2 * u), bm[u] = *reinterpret_cast<const v2f*>(cm + k + 2 * u);
                        }
                        interact_jpairs_fast<U, false>(bx, by, bz, bm, pi.x, pi.y, pi.z, ax, ay, az, e2);
                    }
                }
#pragma unroll 1
                for (; k + 2 <= cnt; k += 2) {  // ragged chunk: pair by pair
                    const v2f bx[1] = {*reinterpret_cast<const v2f*>(cx + k)}, by[1] = {*reinterpret_cast<const v2f*>(cy + k)};
                    const v2f bz[1] = {*reinterpret_cast<const v2f*>(cz + k)}, bm[1] = {*reinterpret_cast<const v2f*>(cm + k)};
                    interact_jpairs_fast<1, false>(bx, by, bz, bm, pi.x, pi.y, pi.z, ax, ay, az, e2);
                }
            }
        }
        if constexpr (sizeof(T) == 8) {
            if (wave_in_window && chunk_form == 2) {
#pragma unroll 4
                for (; k < cnt; ++k) {
                    vec4 bj;
                    bj.x = cx[k], bj.y = cy[k], bj.z = cz[k], bj.w = 1;
                    interact_fast_f64<true>(bj, pi.x, pi.y, pi.z, ax, ay, az, eps2);
                }
            } else if (wave_in_window && chunk_form != 0) {
#pragma unroll 4
                for (; k < cnt; ++k) {
                    vec4 bj;
                    bj.x = cx[k], bj.y = cy[k], bj.z = cz[k], bj.w = cm[k];
                    interact_fast_f64<false>(bj, pi.x, pi.y, pi.z, ax, ay, az, eps2);
                }
            }
        }
        // generic form: the whole chunk, or the odd body at the end of a ragged one
#pragma unroll 4
        for (; k < cnt; ++k) {
            vec4 bj;
            bj.x = cx[k], bj.y = cy[k], bj.z = cz[k], bj.w = cm[k];
            interact_generic<T>(bj, pi.x, pi.y, pi.z, ax, ay, az, eps2);
        }

        if (have_next) chunk_form = store_chunk(cur ^ 1, c + 1, next);
        if (lane == 0) mine[slot] = c + 1;
        wave_lds_sync();
        cur ^= 1;
    }
    if (lane == 0) mine[slot] = 0xffffffffu;  // finished: never the one the others defer to
    __builtin_amdgcn_s_setprio(0);

    if (!active) return;
    if (s.finalize) {
        // bodysystemcpu.cpp:228-234 (fp32) / :283-298 (fp64): dv = acc*dt; v = (v + dv)*damping; p += v*dt
        vec4 v  = reinterpret_cast<const vec4*>(s.vel)[i];
        vec4 pn = pi;
        const T dvx = ax * s.dt, dvy = ay * s.dt, dvz = az * s.dt;
        v.x = (v.x + dvx) * s.damping;
        v.y = (v.y + dvy) * s.damping;
        v.z = (v.z + dvz) * s.damping;
        pn.x = pn.x + v.x * s.dt;
        pn.y = pn.y + v.y * s.dt;
        pn.z = pn.z + v.z * s.dt;
        reinterpret_cast<vec4*>(s.new_pos)[i] = pn;
        reinterpret_cast<vec4*>(s.vel)[i]     = v;
    } else {
        vec4 a;
        a.x = ax, a.y = ay, a.z = az, a.w = 0;
        reinterpret_cast<vec4*>(s.acc)[i] = a;
    }
