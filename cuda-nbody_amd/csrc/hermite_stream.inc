// hermite_stream.inc -- everything the Hermite evaluation kernels share between loading their bodies i and storing their sums, as TEXT
// included inside the kernel body (hermite_eval in hermite_eval.hip, hermite_block_eval in hermite_block.hip, their ensemble forms, and
// hermite6_eval in hermite6_eval.hip; no include guard): the interaction, the streaming loops (wave_groups.inc), the chunk loop of a wave
// with its unit / mixed forms and two-level sums, SIMD-mate priority (wave_mates.inc) and the fold of the S waves (wave_fold.inc).
//
// The kernel defines before it: T, LT, vec, bits, W, U, S; n, tid, wave, lane; the lane's bodies i px, py, pz, vx, vy, vz; eps2; and
//   range, ranges       the workgroup streams range `range` of the J = `ranges` contiguous ranges of the chunks of bodies j
//   jp                  the scalar-load pointer whose element 0 is body 0's {x, y, z, m}
//   pos_base, STRIDE    body j's {x, y, z, m} is the vec4 at pos_base + 4 STRIDE j (an ordinary pointer: the masses, one chunk ahead)
//   body_j(j, b)        the scalar loads of body j into b
// It gets: m_ref, out_scale and, in wave 0 alone (the other waves return inside), second[6]: ax ay az jx jy jz of the lane's bodies i
// over the workgroup's chunks, in units of out_scale -- the kernel multiplies by it when it stores.  out_scale is m_ref, as the sums
// are kept in units of m_ref (a unit-form register sum is added as it is, a mixed one divided by m_ref once) -- unless a wave met a
// register sum that units of a m_ref below 1 could not hold: behind a first body of 2^-20, jerk sums of heavy close pairs pass FLT_MAX
// while the jerk itself is representable (tests/test_hermite_domain.py).  That wave multiplies its second-level sum by m_ref and goes
// on in plain units; before the fold the other waves of the workgroup follow, and out_scale is 1.  Ordinary inputs never get there
// and keep their bits.  A kernel whose sums are a stored format in units of m_ref -- the partial planes of hermite_block_eval and its
// ensemble form, which their finish kernels multiply by m_ref -- defines HERMITE_STREAM_UNIT_SUMS in front of the include (undefined
// here) and has no such escape: its sums hold min(1, |m_ref|) of what they could.
//
// A kernel with another interaction defines HERMITE_STREAM_SUMS (the number of sums, NS) and HERMITE_STREAM_INTERACTION (the file that
// holds its `compute`, in the shape of the one below) in front of the include, which undefines both; it gets second[NS].  Without them
// the text is the acceleration + jerk kernels', token for token.
#ifndef HERMITE_STREAM_SUMS
#define HERMITE_STREAM_SUMS 6
#endif
    constexpr int NS  = HERMITE_STREAM_SUMS;
    constexpr int CH  = kChunk;
    constexpr int LPT = CH / 64;
    static_assert(CH % U == 0, "the streaming loop is unrolled by U");

    const T    m_first   = jp[0].w;  // (a scalar load)
    const T    m_ref     = usable_unit(m_first) ? m_first : T(1);
    const T    inv_mref  = T(1) / m_ref;
    const bits unit_bits = __builtin_bit_cast(bits, m_ref);
    const vec  minus3    = LT::splat(T(-3));
    const typename LT::Consts consts = LT::make_consts();

    // sums: ax ay az jx jy jz.  `first`: the register sum of the current form; `second`: the lane's second-level sum
    vec first[NS], second[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) first[q] = second[q] = LT::splat(0);

    // the range's chunks: [c_lo, c_hi), never empty (J <= n_chunks / S)
    const unsigned n_chunks = stream_chunks(n);
    const unsigned c_lo     = static_cast<unsigned>(static_cast<unsigned long long>(range) * n_chunks / ranges);
    const unsigned c_hi     = static_cast<unsigned>(static_cast<unsigned long long>(range + 1) * n_chunks / ranges);

    // Is every mass of chunk c the reference mass?  Each lane looks at LPT masses with an ordinary vector load, one chunk ahead.
    // (A chunk that is not a whole number of groups -- the last -- takes the mixed loop, and its odd bodies go one by one.)
    auto chunk_is_unit = [&](unsigned c) -> bool {
        const unsigned first_j = c * CH;
        bool           same    = n - first_j >= static_cast<unsigned>(CH) || (n - first_j) % U == 0;
#pragma unroll
        for (int r = 0; r < LPT; ++r) {
            const unsigned j = first_j + r * 64 + lane;
            same             = same && (j >= n || __builtin_bit_cast(bits, pos_base[(4 * STRIDE) * static_cast<size_t>(j < n ? j : first_j) + 3]) == unit_bits);
        }
        return __builtin_amdgcn_ballot_w64(!same) == 0;
    };
    auto group = [&](size_t j0, BodyJ<T> (&b)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) body_j(j0 + u, b[u]);
    };

#ifdef HERMITE_STREAM_INTERACTION
#include HERMITE_STREAM_INTERACTION
#else
    // UB bodies j against the lane's vector of bodies i, written stage by stage: UB independent chains in flight.  (wave_groups.inc passes
    // the index of the first; nothing here depends on it.)
    auto compute = [&]<bool UNIT, int UB>(const BodyJ<T>* b, unsigned, vec (&sum)[NS]) {
        vec dx[UB], dy[UB], dz[UB], ex[UB], ey[UB], ez[UB], s2[UB], rv[UB], k3[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            dx[u] = LT::splat(b[u].p.x) - px, dy[u] = LT::splat(b[u].p.y) - py, dz[u] = LT::splat(b[u].p.z) - pz;
            ex[u] = LT::splat(b[u].v.x) - vx, ey[u] = LT::splat(b[u].v.y) - vy, ez[u] = LT::splat(b[u].v.z) - vz;
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) s2[u] = LT::fma(dx[u], dx[u], eps2), rv[u] = dx[u] * ex[u];
#pragma unroll
        for (int u = 0; u < UB; ++u) s2[u] = LT::fma(dy[u], dy[u], s2[u]), rv[u] = LT::fma(dy[u], ey[u], rv[u]);
#pragma unroll
        for (int u = 0; u < UB; ++u) s2[u] = LT::fma(dz[u], dz[u], s2[u]), rv[u] = LT::fma(dz[u], ez[u], rv[u]);
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            vec inv2;
            Powers<T>::of(s2[u], consts, inv2, k3[u]);
            rv[u] = (rv[u] * inv2) * minus3;  // -3 (r.w) / s^2
            if constexpr (!UNIT) k3[u] = k3[u] * LT::splat(b[u].p.w);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) ex[u] = LT::fma(rv[u], dx[u], ex[u]), ey[u] = LT::fma(rv[u], dy[u], ey[u]), ez[u] = LT::fma(rv[u], dz[u], ez[u]);
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            sum[0] = LT::fma(dx[u], k3[u], sum[0]), sum[1] = LT::fma(dy[u], k3[u], sum[1]), sum[2] = LT::fma(dz[u], k3[u], sum[2]);
            sum[3] = LT::fma(ex[u], k3[u], sum[3]), sum[4] = LT::fma(ey[u], k3[u], sum[4]), sum[5] = LT::fma(ez[u], k3[u], sum[5]);
        }
    };
#endif
#include "wave_groups.inc"
    bool is_unit = true;   // the form `first` holds
    bool plain   = false;  // (wave-uniform) `second` has left the units of m_ref for plain units
    auto flush   = [&]() {
#ifndef HERMITE_STREAM_UNIT_SUMS
        if (!plain && (m_ref < T(1) && m_ref > T(-1))) {  // counted in a unit below 1 the sums grow: is there room?
            constexpr T huge = sizeof(T) == 4 ? T(0x1p124) : T(0x1p1020);
            const T     room = is_unit ? huge : huge * (m_ref < 0 ? -m_ref : m_ref);
            bool        big  = false;
#pragma unroll
            for (int q = 0; q < NS; ++q) {
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    const T f = LT::get(first[q], k), s = LT::get(second[q], k);
                    big       = big || (f < 0 ? -f : f) > room || (s < 0 ? -s : s) > huge;
                }
            }
            if (__builtin_amdgcn_ballot_w64(big) != 0) {
                const vec back = LT::splat(m_ref);
#pragma unroll
                for (int q = 0; q < NS; ++q) second[q] = second[q] * back;
                plain = true;
            }
        }
#endif
        const vec scale = LT::splat(plain ? (is_unit ? m_ref : T(1)) : (is_unit ? T(1) : inv_mref));
#pragma unroll
        for (int q = 0; q < NS; ++q) second[q] = LT::fma(first[q], scale, second[q]), first[q] = LT::splat(0);
    };

#define WAVE_MATES_SETUP
#include "wave_mates.inc"

    unsigned c       = c_lo + wave;  // wave w streams chunks c_lo + w, c_lo + w + S, ...
    bool     unit    = c < c_hi ? chunk_is_unit(c) : false;
    unsigned held    = 0;     // chunks in `first`
    BodyJ<T> b0[U], b1[U];
    if (c < c_hi && n - c * CH >= static_cast<unsigned>(U)) group(static_cast<size_t>(c) * CH, b0);
    for (; c < c_hi; c += S) {
        const bool next_unit = (c + S) < c_hi ? chunk_is_unit(c + S) : false;  // (its loads are in flight across the compute below)
#define WAVE_MATES_CHUNK
#include "wave_mates.inc"
        const unsigned first_j = c * CH;
        const unsigned count   = min(static_cast<unsigned>(CH), n - first_j);
        const unsigned groups  = count / U;
        // the wave's next chunk, when it has a whole group (else anything readable: the set is not used again)
        const size_t next = ((c + S) < c_hi && n - (first_j + S * CH) >= static_cast<unsigned>(U)) ? static_cast<size_t>(first_j) + S * CH : first_j;
        if (unit != is_unit || held == kFlushEvery) {
            flush();
            is_unit = unit, held = 0;
        }
        if (groups > 0) {
            if (unit) {
                stream.template operator()<true>(first_j, groups, next, b0, b1);
            } else {
                stream.template operator()<false>(first_j, groups, next, b0, b1);
            }
        }
#pragma unroll 1
        for (unsigned jj = groups * U; jj < count; ++jj) {  // ragged end of the last chunk (mixed)
            BodyJ<T> one[1];
            body_j(static_cast<size_t>(first_j) + jj, one[0]);
            compute.template operator()<false, 1>(one, first_j + jj, first);
        }
        ++held;
        unit = next_unit;
#define WAVE_MATES_DONE
#include "wave_mates.inc"
    }
#define WAVE_MATES_LEAVE
#include "wave_mates.inc"
    flush();

    // the unit the workgroup's sums are handed over in: m_ref, or 1 when a wave went over to plain units (then all of them do)
#ifndef HERMITE_STREAM_UNIT_SUMS
    T out_scale = m_ref;
    if (S > 1 && m_ref < T(1) && m_ref > T(-1)) {  // (workgroup-uniform: the condition under which flush may go over)
        __shared__ int went_plain;
        if (tid == 0) went_plain = 0;
        __syncthreads();
        if (plain && lane == 0) went_plain = 1;
        __syncthreads();
        if (went_plain != 0 && !plain) {
            const vec back = LT::splat(m_ref);
#pragma unroll
            for (int q = 0; q < NS; ++q) second[q] = second[q] * back;
        }
        plain = went_plain != 0;
    }
    if (plain) out_scale = T(1);
#endif

#include "wave_fold.inc"
#undef HERMITE_STREAM_SUMS
#undef HERMITE_STREAM_UNIT_SUMS
#undef HERMITE_STREAM_INTERACTION
