// hermite_block_parts.inc -- what the kernels of a block step share around their own arithmetic, as TEXT included inside the kernel body, in
// seven parts: one text for hermite_block.hip, hermite6_block.hip, hermite_block_ensemble.hip and hermite6_block_ensemble.hip.  The includer defines ONE of the names
// below in front of each include (the fragment undefines it).  Where its records and its bodies lie it says with local names, defined
// where its own listing wants them: between two parts where they hang on a system's slice, which the ensemble forms behind the early returns.
//   BLOCK_PART_DECIDE        *_predict_count, behind the fold.  Requires a (p, t_stop), m (the folded MinLevel), block (the workgroup's
//                            index within its system: the first records) and the macros BLOCK_CTRL and BLOCK_STATUS, the records' addresses,
//                            formed by the recording lane alone.  Defines now, q, go; the workgroup leaves where go is false.
//   BLOCK_PART_EVAL_HEAD     *_block*_eval, first thing.  Requires W, ctrl, n, local (the workgroup's index within its system).  Defines
//                            n_act, ranges, tile, range, slots; the workgroups beyond tiles x ranges leave.
//   BLOCK_PART_EVAL_BODIES   Requires LT, vec, vec4, STRIDE (vec4 per predicted body: 2, or 3 with the acceleration), state, active.
//                            Defines pos_base, jp, tid, wave, lane, tile_base and the lane's bodies i px .. vz (ax, ay, az), gathered
//                            through the active list.
//   BLOCK_PART_EVAL_STORE    *_block*_eval, last thing.  Requires partial and what hermite_stream.inc left (NS, second).
//   BLOCK_PART_FINISH_HEAD   *_finish, first thing.  Requires T, a (n), ctrl, block.  Defines n_act, slot, slots, ranges, now; the lanes
//                            beyond n_act leave.
//   BLOCK_PART_FINISH_SUMS   Requires vec4, NS (6, or 9 with the snap), a (p, levels), i, state, partial.  Defines a1, j1 (s1) in plain
//                            units, and the body's level k, q, own (its step in ticks) and dt_i.
//   BLOCK_PART_FINISH_LEVEL  *_finish, last thing.  Requires dt_a on top of those.  Stores the body's new level and its tick.
#if defined(BLOCK_PART_DECIDE)
#undef BLOCK_PART_DECIDE
    const unsigned long long now = m.next;
    const double             q   = tick_length(a.p);
    const bool               go  = static_cast<double>(now) * q <= a.t_stop;
    if (block == 0 && threadIdx.x == 0) {
        BlockCtrl* const   ctrl   = BLOCK_CTRL;
        BlockStatus* const status = BLOCK_STATUS;
        ctrl->now = now, ctrl->go = go ? 1u : 0u;
        if (!go) ctrl->n_act = 0;
        const unsigned flags  = status->flags;
        status->flags         = go ? (flags & ~kBlockStopped) : (flags | kBlockStopped);
        const int deepest     = status->deepest_level;
        status->deepest_level = m.level > deepest ? m.level : deepest;
    }
    if (!go) return;
#undef BLOCK_CTRL
#undef BLOCK_STATUS
#elif defined(BLOCK_PART_EVAL_HEAD)
#undef BLOCK_PART_EVAL_HEAD
    if (ctrl->go == 0) return;
    const unsigned  n_act = ctrl->n_act;
    const BlockGeom geom  = stream_geometry(n, n_act, 64 * W, kBlockTarget);
    if (local >= geom.tiles * geom.ranges) return;
    const unsigned ranges = geom.ranges;
    const unsigned tile   = local / ranges;
    const unsigned range  = local % ranges;
    const unsigned slots  = geom.tiles * (64 * W);
#elif defined(BLOCK_PART_EVAL_BODIES)
#undef BLOCK_PART_EVAL_BODIES
    typedef const typename LT::raw4 __attribute__((address_space(4)))* stream_ptr;  // read-only for the whole launch -> s_load_dwordx4 / x8 / x16
    const T* const   pos_base = state;
    const stream_ptr jp   = reinterpret_cast<stream_ptr>(reinterpret_cast<unsigned long long>(state));
    const int        tid  = threadIdx.x;
    const int        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int        lane = tid & 63;

    // bodies i of this lane: slots tile_base + k*64 + lane of the active list (past n_act: the last active body again)
    const unsigned             tile_base = tile * (64 * W);
    vec                        px, py, pz, vx, vy, vz;
    [[maybe_unused]] vec       ax, ay, az;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned slot = tile_base + k * 64 + lane;
        const size_t   i    = active[slot < n_act ? slot : n_act - 1];
        const vec4     p    = reinterpret_cast<const vec4*>(state)[STRIDE * i];
        const vec4     v    = reinterpret_cast<const vec4*>(state)[STRIDE * i + 1];
        LT::set(px, k, p.x), LT::set(py, k, p.y), LT::set(pz, k, p.z);
        LT::set(vx, k, v.x), LT::set(vy, k, v.y), LT::set(vz, k, v.z);
        if constexpr (STRIDE == 3) {
            const vec4 b = reinterpret_cast<const vec4*>(state)[STRIDE * i + 2];
            LT::set(ax, k, b.x), LT::set(ay, k, b.y), LT::set(az, k, b.z);
        }
    }
#elif defined(BLOCK_PART_EVAL_STORE)
#undef BLOCK_PART_EVAL_STORE
    // planes [J][NS][slots]: word (range, q, slot), coalesced across the wave; the slots past n_act of the last tile hold a copy of the last body's sums
#pragma unroll
    for (int q = 0; q < NS; ++q) {
#pragma unroll
        for (int k = 0; k < W; ++k) partial[(static_cast<size_t>(range) * NS + q) * slots + tile_base + k * 64 + lane] = LT::get(second[q], k);
    }
#elif defined(BLOCK_PART_FINISH_HEAD)
#undef BLOCK_PART_FINISH_HEAD
    constexpr unsigned per_tile = 64 * Lane<T>::W;
    if (ctrl->go == 0) return;
    const unsigned n_act = ctrl->n_act;
    const unsigned slot  = block * 256u + threadIdx.x;
    if (slot >= n_act) return;
    const BlockGeom          geom   = stream_geometry(a.n, n_act, per_tile, kBlockTarget);
    const size_t             slots  = static_cast<size_t>(geom.tiles) * per_tile;
    const unsigned long long now    = ctrl->now;
    const unsigned           ranges = geom.ranges;
#elif defined(BLOCK_PART_FINISH_SUMS)
#undef BLOCK_PART_FINISH_SUMS
#include "range_sum.inc"  // sum[NS]: the J ranges' partial sums of this slot, in range order, in units of the reference mass
    const T m_first = state[3];
    const T m_ref   = usable_unit(m_first) ? m_first : T(1);
    vec4    a1, j1;
    a1.x = sum[0] * m_ref, a1.y = sum[1] * m_ref, a1.z = sum[2] * m_ref, a1.w = 0;
    j1.x = sum[3] * m_ref, j1.y = sum[4] * m_ref, j1.z = sum[5] * m_ref, j1.w = 0;
    [[maybe_unused]] vec4 s1;
    if constexpr (NS == 9) s1.x = sum[6] * m_ref, s1.y = sum[7] * m_ref, s1.z = sum[8] * m_ref, s1.w = 0;

    int                      k    = a.levels[i];
    k                             = k < 0 ? 0 : (k > a.p.max_level ? a.p.max_level : k);
    const double             q    = tick_length(a.p);
    const unsigned long long own  = 1ull << (a.p.max_level - k);
    const double             dt_i = static_cast<double>(own) * q;
#elif defined(BLOCK_PART_FINISH_LEVEL)
#undef BLOCK_PART_FINISH_LEVEL
    // deeper at once; one level up only where the step is long enough twice over and `now` is a multiple of the longer step
    if (dt_a < dt_i) {
        k = deepened(k, dt_a, a.p, q);
    } else if (dt_a >= 2.0 * dt_i && k > 0 && now % (2 * own) == 0) {
        --k;
    }
    a.levels[i] = k;
    a.ticks[i]  = now;
#else
#error "hermite_block_parts.inc: define one of the BLOCK_PART_* names in front of the include"
#endif
