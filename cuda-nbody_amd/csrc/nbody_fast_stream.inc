// nbody_fast_stream.inc -- the body of the wave-stream FAST kernel (nbody_fast_stream.h), included INSIDE a kernel's braces: by
// integrate_bodies_fast (nbody_fast.hip) and by the ensemble's FAST kernel (ensemble_fast.hip).  The kernel is a template of
// <typename T, int R, int S, int LPT> (T: float|double, R: vectors per lane (I = R*W bodies i), S: waves splitting j, LPT: vec4
// loads per lane per chunk), runs 64*S threads and provides
//   `s`     : Shard<T>, the shard to step (the ensemble's: its system's arrays and parameters)
//   `block` : unsigned, the workgroup's index within that shard's grid (bodies i [block * 64*I, (block + 1) * 64*I))
// A text include rather than a __device__ function: inlined from a function the body compiles to other (equivalent) ISA, and the
// product's kernel keeps the ISA it had.  No include guard on purpose.
    using LT            = Lane<T>;
    using vec4          = typename LT::vec4;
    using vec           = typename LT::vec;
    constexpr int W     = LT::W;
    constexpr int I     = R * W;     // bodies i per lane
    constexpr int CH    = 64 * LPT;  // bodies j per wave per chunk
    constexpr int BODIES_PER_BLOCK = 64 * I;
    // j bodies in flight per lane: 8 independent interaction chains (R vectors x U bodies j) hide the VALU latency.
    // Every geometry is capped at 128 VGPRs (4 waves/SIMD: 16 waves per CU in 1, 2 or 4 workgroups), so with R >= 2 the
    // loop unrolls less instead of spilling (an R = 4 body at U = 8 spilled 1.2 KB/lane to scratch: 1.2 GB of HBM writes per launch).
    constexpr int U = sizeof(T) == 8 && R == 1 ? 4 : (R >= 2 ? 8 / R : 8);  // (fp64 bodies take 8 scalar registers each)
    static_assert(CH % U == 0, "inner loop is unrolled by U");

    extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];

    using raw4 = typename LT::raw4;
    typedef const raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx4/x8/x16
    const vec4* __restrict__ old_pos = reinterpret_cast<const vec4*>(s.old_pos);
    const stream_ptr         bodies  = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(s.old_pos));
    const int tid  = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;

    // bodies i of this lane: block_base + k*64 + lane, k = r*W + w  (coalesced across the lanes of a wave)
    const unsigned block_base = block * BODIES_PER_BLOCK;
    vec      px[R], py[R], pz[R], ax[R], ay[R], az[R];
    unsigned idx[I];
    bool     active[I];
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const unsigned local = block_base + k * 64 + lane;
        active[k]            = local < s.i_count;
        idx[k]               = s.i_begin + (active[k] ? local : s.i_count - 1);
        const vec4 p         = old_pos[idx[k]];
        LT::set(px[k / W], k % W, p.x);
        LT::set(py[k / W], k % W, p.y);
        LT::set(pz[k / W], k % W, p.z);
    }
    const T m_ref    = reference_mass(s, bodies);
    const T inv_mref = T(1) / m_ref;
#pragma unroll
    for (int r = 0; r < R; ++r) ax[r] = ay[r] = az[r] = LT::splat(0);
    if (s.acc_in && wave == 0) {
#pragma unroll
        for (int k = 0; k < I; ++k) {
            const vec4 a = reinterpret_cast<const vec4*>(s.acc)[idx[k]];
            LT::set(ax[k / W], k % W, a.x * inv_mref);
            LT::set(ay[k / W], k % W, a.y * inv_mref);
            LT::set(az[k / W], k % W, a.z * inv_mref);
        }
    }
    vec eps2 = LT::splat(s.eps2);
    LT::keep_in_vgpr(eps2);
    vec inv_mref_v = LT::splat(inv_mref);
    LT::keep_in_vgpr(inv_mref_v);
    const typename LT::Consts consts = LT::make_consts();
    const typename LT::bits   unit_bits = __builtin_bit_cast(typename LT::bits, m_ref);

    const unsigned j_end    = s.j_begin + s.j_count;
    const unsigned n_chunks = (s.j_count + CH - 1) / CH;

#ifdef NB_STAMPS  // diagnostic build only (tools/stamp_probe.py): when does each wave start / finish streaming?
    const unsigned long long stamp_t0 = __builtin_amdgcn_s_memrealtime();  // (100 MHz, one clock for the whole chip)
#endif

    // The SIMD arbiter is strictly oldest-first: left alone, the four waves that share a SIMD finish equal shares of work
    // at 30 % / 53 % / 76 % / 100 % of the workgroup's time (profiles/round2_wave_finish_times.txt), and for the last
    // quarter each SIMD is down to ONE wave, which only reaches 76 % of the issue rate four waves sustain (80.6 against 61.5
    // cycles per interaction pair).  s_setprio outranks age, so progress is equalised instead: each wave publishes how many
    // chunks it has done; a wave that is level with the slowest wave of ITS SIMD (HW_ID.SIMD_ID) runs at priority 3, one that is ahead
    // at 0.  With two waves per SIMD and workgroup (S = 8, the production geometry: two 512-thread workgroups per CU) they
    // finish within 0.5 % of each other; with four (S = 16) the two youngest still trail (a starved wave cannot re-evaluate
    // itself; graded levels made it worse, and letting a yielding wave look again every 8 bodies cost 1 % at S = 8 and 27 % on
    // one-workgroup-per-CU shards), which is why S = 8 is the default.  The chunk -> wave assignment stays static, so the summation order (and every result bit) is the same
    // from run to run.  (Putting the leaders to sleep instead equalises too, but costs 15 %: a SIMD needs 3-4 runnable waves.)
    constexpr size_t kFoldBytes = static_cast<size_t>(S - 1) * 3 * I * 64 * sizeof(T);
    unsigned* const   balance    = reinterpret_cast<unsigned*>(smem_raw + kFoldBytes);
    unsigned* const   simd_count = balance;                                     // [4] waves of this workgroup per SIMD
    volatile unsigned* progress  = reinterpret_cast<volatile unsigned*>(balance + 4);  // [4][8] chunks done, by SIMD and slot
    if (tid < 36) balance[tid] = tid < 4 ? 0u : 0xffffffffu;
    __syncthreads();
    const unsigned simd = static_cast<unsigned>(__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4));  // HW_REG_HW_ID[5:4] = SIMD_ID
    unsigned       slot = 0;
    if (lane == 0) slot = atomicAdd(&simd_count[simd], 1u);
    slot                = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(slot))) & 7u;
    volatile unsigned* const mine = progress + simd * 8;
    unsigned done = 0;
    if (lane == 0) mine[slot] = 0;

    // fp32: a register sum only ever collects kFlush chunks (1 024 bodies j); it is then added to the lane's own second-level
    // sum in LDS.  One running fp32 sum over N/S terms loses ~sqrt(N/S) ulp (1.6e-5 relative at 1 Mi bodies against an fp64
    // direct sum); two levels of <= 1 024 and <= N/(1024 S) terms keep it at a few 1e-6 for any N.  (fp64 has the bits to spare.)
    constexpr bool     kTwoLevel = sizeof(T) == 4;
    constexpr unsigned kFlush    = 1024 / CH;
    T* const second = reinterpret_cast<T*>(balance + 64) + static_cast<size_t>(wave) * (3 * I * 64) + lane;  // [S][3][I][64]
    if constexpr (kTwoLevel) {
#pragma unroll
        for (int q = 0; q < 3 * I; ++q) second[q * 64] = 0;
    }
    auto flush = [&]() {
#pragma unroll
        for (int k = 0; k < I; ++k) {
            second[(0 * I + k) * 64] += LT::get(ax[k / W], k % W);
            second[(1 * I + k) * 64] += LT::get(ay[k / W], k % W);
            second[(2 * I + k) * 64] += LT::get(az[k / W], k % W);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) ax[r] = ay[r] = az[r] = LT::splat(0);
    };

    // Every lane of a wave meets the same body j, so the bodies j are not staged anywhere: the wave reads them U at a time with
    // scalar loads (through the constant address space: `old_pos` is read-only for the whole launch) straight into scalar
    // registers, one group ahead of the one it is computing, and they enter the packed subtractions as scalar operands.
    // Against a per-wave LDS ring read back with ds_read_b128 (rounds 1-2) the loop loses its LDS instructions and 4
    // vector-register reads per body j.
    // Whether a chunk takes the loop without the mass multiply (every mass == m_ref) is found one chunk ahead: each lane
    // looks at the masses of two bodies of the wave's next chunk with an ordinary vector load.
    // The masses of chunk c, one or more per lane; wave-uniform answer.  kUnit: every mass is m_ref.  kUniform: the bodies of
    // the chunk all have the SAME mass (a species of a galaxy file) -- the chunk then runs the loop without the mass
    // multiply into sums of its own, which join the running sums scaled by that mass.  kMixed: the mass-multiplying loop.
    // (A ragged chunk -- the last of the range -- is only judged by the bodies it has; its odd bodies go one by one anyway.)
    enum : int { kMixed = 0, kUnit = 1, kUniform = 2 };
    auto chunk_form = [&](unsigned c, T& common_mass) -> int {
        const unsigned first_j = s.j_begin + c * CH;
        using bits = typename LT::bits;
        const bits first_bits = __builtin_bit_cast(bits, s.old_pos[4 * static_cast<size_t>(first_j) + 3]);  // (uniform address)
        bool same = true;
#pragma unroll
        for (int r = 0; r < LPT; ++r) {
            const unsigned j = first_j + r * 64 + lane;
            same             = same && (j >= j_end || __builtin_bit_cast(bits, s.old_pos[4 * static_cast<size_t>(j < j_end ? j : first_j) + 3]) == first_bits);
        }
        common_mass = __builtin_bit_cast(T, first_bits);
        if (__builtin_amdgcn_ballot_w64(!same) != 0 || !(common_mass == common_mass)) return kMixed;  // (NaN masses take the plain loop)
        return first_bits == unit_bits ? kUnit : kUniform;
    };
    auto group = [&](stream_ptr from, raw4 (&b)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) b[u] = from[u];
    };

    // U bodies j against the R vectors of bodies i, written stage by stage (all differences, all squared distances, all
    // reciprocal square roots, ...): U*R independent chains in flight whatever the instruction scheduler makes of it
    auto compute = [&]<bool UNIT>(const raw4 (&b)[U], vec (&ax)[R], vec (&ay)[R], vec (&az)[R]) {
        constexpr int UB = (4 / R > 0 ? 4 / R : 1) < U ? (4 / R > 0 ? 4 / R : 1) : U;  // bodies j per stage block: >= 4 chains
#pragma unroll
        for (int h = 0; h < U; h += UB) {
            vec dx[UB][R], dy[UB][R], dz[UB][R], w[UB][R];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const vec bx = LT::splat(b[h + u].x), by = LT::splat(b[h + u].y), bz = LT::splat(b[h + u].z);
#pragma unroll
                for (int r = 0; r < R; ++r) dx[u][r] = bx - px[r], dy[u][r] = by - py[r], dz[u][r] = bz - pz[r];
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
#pragma unroll
                for (int r = 0; r < R; ++r) w[u][r] = LT::fma(dx[u][r], dx[u][r], eps2);
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
#pragma unroll
                for (int r = 0; r < R; ++r) w[u][r] = LT::fma(dy[u][r], dy[u][r], w[u][r]);
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
#pragma unroll
                for (int r = 0; r < R; ++r) w[u][r] = LT::fma(dz[u][r], dz[u][r], w[u][r]);
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                vec mrel = inv_mref_v;
                if constexpr (!UNIT) mrel = LT::splat(b[h + u].w);  // (the raw mass, a scalar operand; the chunk's sums are scaled once)
#pragma unroll
                for (int r = 0; r < R; ++r) w[u][r] = LT::template coupling_rel<UNIT>(mrel, w[u][r], consts);
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    ax[r] = LT::fma(dx[u][r], w[u][r], ax[r]);
                    ay[r] = LT::fma(dy[u][r], w[u][r], ay[r]);
                    az[r] = LT::fma(dz[u][r], w[u][r], az[r]);
                }
            }
        }
    };
    auto arrived = [](const raw4 (&b)[U]) { asm volatile("" : : "s"(b[0]) : "memory"); };  // first use of the set: what follows is issued after its wait
    // b0 holds (or is loading) group 0 of the chunk; on return it is loading the first group at `next` (the wave's next chunk)
    auto stream = [&]<bool UNIT>(stream_ptr chunk, unsigned groups, stream_ptr next, raw4 (&b0)[U], raw4 (&b1)[U], vec (&sx)[R], vec (&sy)[R], vec (&sz)[R]) {
        unsigned g = 0;
#pragma unroll 1
        for (; g + 2 <= groups; g += 2) {
            arrived(b0);
            group(chunk + (g + 1) * U, b1);
            __builtin_amdgcn_sched_barrier(0);  // (the load stays ahead of the compute it overlaps)
            compute.template operator()<UNIT>(b0, sx, sy, sz);
            arrived(b1);
            group(g + 2 < groups ? chunk + (g + 2) * U : next, b0);
            __builtin_amdgcn_sched_barrier(0);
            compute.template operator()<UNIT>(b1, sx, sy, sz);
        }
        if (g < groups) {  // (odd count: the ragged last chunk of the range, nothing follows it)
            compute.template operator()<UNIT>(b0, sx, sy, sz);
        }
    };

    unsigned c    = wave;  // wave w streams chunks w, w+S, w+2S, ...
    T        common_mass = 0, next_mass = 0;
    int      form = c < n_chunks ? chunk_form(c, common_mass) : kMixed;
    raw4     b0[U], b1[U];  // two register sets: while one group is computed the next one is in flight.  (Scalar loads return in
                            // any order, so a wait is for everything outstanding: a set is loaded only once the other has been waited for.)
    if (c < n_chunks && j_end - (s.j_begin + c * CH) >= static_cast<unsigned>(U)) group(bodies + (s.j_begin + c * CH), b0);
    for (; c < n_chunks; c += S) {
        const int next_form = (c + S) < n_chunks ? chunk_form(c + S, next_mass) : kMixed;  // (its loads are in flight across the compute below)
#ifndef NB_NO_BALANCE  // (diagnostic builds switch it off: tools/stamp_probe.py)
        // a wave that is not ahead of any wave of its SIMD (same workgroup) runs at priority 3, the others at 0
        {
            unsigned least = done;
#pragma unroll
            for (int q = 0; q < 8; ++q) least = min(least, mine[q]);  // unsynchronised reads: a stale value only delays a priority change
            if (static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(least))) >= done) {
                __builtin_amdgcn_s_setprio(3);
            } else {
                __builtin_amdgcn_s_setprio(0);
            }
        }
#endif
        const unsigned   first  = s.j_begin + c * CH;
        const unsigned   count  = min(static_cast<unsigned>(CH), j_end - first);
        const unsigned   groups = count / U;
        const stream_ptr chunk  = bodies + first;
        // the wave's next chunk, when it has a whole group (else anything readable: the set is not used again)
        const stream_ptr next = ((c + S) < n_chunks && j_end - (first + S * CH) >= static_cast<unsigned>(U)) ? chunk + S * CH : chunk;
        if (groups > 0) {
            if (form == kUnit) {
                stream.template operator()<true>(chunk, groups, next, b0, b1, ax, ay, az);
            } else if (form == kUniform) {
                vec cx[R], cy[R], cz[R];
#pragma unroll
                for (int r = 0; r < R; ++r) cx[r] = cy[r] = cz[r] = LT::splat(0);
                stream.template operator()<true>(chunk, groups, next, b0, b1, cx, cy, cz);
                const vec scale = LT::splat(common_mass) * inv_mref_v;
#pragma unroll
                for (int r = 0; r < R; ++r) ax[r] = LT::fma(cx[r], scale, ax[r]), ay[r] = LT::fma(cy[r], scale, ay[r]), az[r] = LT::fma(cz[r], scale, az[r]);
            } else {  // mixed masses: the raw mass multiplies inside the loop, 1/m_ref once per chunk
                vec cx[R], cy[R], cz[R];
#pragma unroll
                for (int r = 0; r < R; ++r) cx[r] = cy[r] = cz[r] = LT::splat(0);
                stream.template operator()<false>(chunk, groups, next, b0, b1, cx, cy, cz);
#pragma unroll
                for (int r = 0; r < R; ++r) ax[r] = LT::fma(cx[r], inv_mref_v, ax[r]), ay[r] = LT::fma(cy[r], inv_mref_v, ay[r]), az[r] = LT::fma(cz[r], inv_mref_v, az[r]);
            }
        }
#pragma unroll 1
        for (unsigned jj = groups * U; jj < count; ++jj) {  // ragged end of the range
            const raw4 b = chunk[jj];
            interact_uniform<T, R, false>(b, LT::splat(b.w) * inv_mref_v, px, py, pz, ax, ay, az, eps2, consts);
        }
        form = next_form, common_mass = next_mass;
        ++done;
        if constexpr (kTwoLevel) {
            if (done % kFlush == 0) flush();
        }
        if (lane == 0) mine[slot] = done;
    }
    if (lane == 0) mine[slot] = 0xffffffffu;  // finished: never the one the others defer to
    __builtin_amdgcn_s_setprio(0);
    if constexpr (kTwoLevel) {
#pragma unroll
        for (int k = 0; k < I; ++k) {
            LT::set(ax[k / W], k % W, second[(0 * I + k) * 64] + LT::get(ax[k / W], k % W));
            LT::set(ay[k / W], k % W, second[(1 * I + k) * 64] + LT::get(ay[k / W], k % W));
            LT::set(az[k / W], k % W, second[(2 * I + k) * 64] + LT::get(az[k / W], k % W));
        }
    }
#ifdef NB_STAMPS
    if (lane == 0 && s.acc != nullptr && s.finalize && !s.acc_in) {
        unsigned long long* stamps = reinterpret_cast<unsigned long long*>(s.acc) + (static_cast<size_t>(block) * S + wave) * 2;
        stamps[0] = stamp_t0, stamps[1] = __builtin_amdgcn_s_memrealtime();
    }
#endif

    // fold the S partial sums (waves 1..S-1 -> wave 0) through LDS, fixed order
    T* red = reinterpret_cast<T*>(smem_raw);  // [(S-1)][3][I][64]
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < I; ++k) {
            red[(((wave - 1) * 3 + 0) * I + k) * 64 + lane] = LT::get(ax[k / W], k % W);
            red[(((wave - 1) * 3 + 1) * I + k) * 64 + lane] = LT::get(ay[k / W], k % W);
            red[(((wave - 1) * 3 + 2) * I + k) * 64 + lane] = LT::get(az[k / W], k % W);
        }
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll 1  // (fully unrolled, the S = 16 fold hoists 45*I LDS loads and spills)
    for (int g = 1; g < S; ++g) {
#pragma unroll
        for (int k = 0; k < I; ++k) {
            LT::set(ax[k / W], k % W, LT::get(ax[k / W], k % W) + red[(((g - 1) * 3 + 0) * I + k) * 64 + lane]);
            LT::set(ay[k / W], k % W, LT::get(ay[k / W], k % W) + red[(((g - 1) * 3 + 1) * I + k) * 64 + lane]);
            LT::set(az[k / W], k % W, LT::get(az[k / W], k % W) + red[(((g - 1) * 3 + 2) * I + k) * 64 + lane]);
        }
    }

#pragma unroll
    for (int k = 0; k < I; ++k) {
        // (index and activity are worked out again from a lane number the compiler cannot tie to the one above: held across
        // the streaming loop they cost I registers that the loop's stage blocks need)
        unsigned lane_again = lane;
        asm volatile("" : "+v"(lane_again));
        const unsigned local = block_base + k * 64 + lane_again;
        if (local >= s.i_count) continue;
        const unsigned i  = s.i_begin + local;
        const T        fx = LT::get(ax[k / W], k % W) * m_ref, fy = LT::get(ay[k / W], k % W) * m_ref, fz = LT::get(az[k / W], k % W) * m_ref;
        if (s.finalize) {
            // integrateBodies, bodysystemcuda.cu:166-183
            vec4 v  = reinterpret_cast<const vec4*>(s.vel)[i];
            vec4 pn = old_pos[i];
            v.x     = __builtin_fma(fx, s.dt, v.x) * s.damping;
            v.y     = __builtin_fma(fy, s.dt, v.y) * s.damping;
            v.z     = __builtin_fma(fz, s.dt, v.z) * s.damping;
            pn.x    = __builtin_fma(v.x, s.dt, pn.x);
            pn.y    = __builtin_fma(v.y, s.dt, pn.y);
            pn.z    = __builtin_fma(v.z, s.dt, pn.z);
            reinterpret_cast<vec4*>(s.new_pos)[i] = pn;
            reinterpret_cast<vec4*>(s.vel)[i]     = v;
        } else {
            vec4 a;
            a.x = fx, a.y = fy, a.z = fz, a.w = 0;
            reinterpret_cast<vec4*>(s.acc)[i] = a;
        }
    }
