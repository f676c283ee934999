// hermite_block_ensemble_schedule.inc -- the per-system schedule kernels of a block step of B systems that do not depend on the order of the
// scheme, one text for hermite_block_ensemble.hip (nb_hermite_block_ensemble_*) and hermite6_block_ensemble.hip
// (nb_hermite6_block_ensemble_*): a system's slice and control record, the partial minima of tick + ticks(level), the scan and scatter of the
// active list, init's levels and the summary of the status records.  They read BlockEnsembleArgs<T> (hermite_block_ensemble_kernels.h) alone;
// the 6th-order unit hands them the base of its own arguments.  Included inside each translation unit's own anonymous namespace, after
// nbody_lane.h (Lane) and hermite_block_kernels_shared.h (ticks_of, block_fold, first_level).

// (read-only for the whole launch -> a scalar load where the index is wave-uniform)
template <typename V> __device__ __forceinline__ V uniform_load(const V* p, size_t index) {
    typedef const V __attribute__((address_space(4)))* uniform_ptr;
    return reinterpret_cast<uniform_ptr>(reinterpret_cast<unsigned long long>(p))[index];
}

template <typename T> __device__ __forceinline__ char* slice_of(const BlockEnsembleArgs<T>& a, unsigned system) { return a.workspace + static_cast<size_t>(system) * a.layout.stride; }
template <typename T> __device__ __forceinline__ BlockCtrl* ctrl_of(const BlockEnsembleArgs<T>& a, unsigned system) {
    return reinterpret_cast<BlockCtrl*>(slice_of(a, system) + a.layout.ctrl);
}

// Per workgroup of 256 bodies, the minimum of tick + ticks(level) and the deepest level held -> the system's partial minima (<= 256).
template <typename T> __global__ __launch_bounds__(256) void block_ensemble_min_partial(BlockEnsembleArgs<T> a) {
    __shared__ unsigned long long lds_next[256];
    __shared__ int                lds_level[256];
    const unsigned                system = blockIdx.x / a.blocks;
    const unsigned                block  = blockIdx.x - system * a.blocks;
    const unsigned                local  = block * 256u + threadIdx.x;
    MinLevel                      m{~0ull, 0};
    if (local < a.n) {
        const size_t i = static_cast<size_t>(system) * a.n + local;
        m.level        = a.levels[i];
        m.next         = a.ticks[i] + ticks_of(m.level, a.p.max_level);
        m.level        = m.level > 0 ? m.level : 0;
    }
    m = block_fold(m, lds_next, lds_level);
    if (threadIdx.x != 0) return;
    char* const slice = slice_of(a, system);
    reinterpret_cast<unsigned long long*>(slice + a.layout.min_part)[block] = m.next;
    reinterpret_cast<int*>(slice + a.layout.lvl_part)[block]                = m.level;
}

// The scan and the scatter in one launch: a system has at most 256 counts, so every workgroup adds those before its own itself (integer
// sums: the order changes nothing) and writes its active bodies behind them, ascending.  The counts are only read.  The system's first
// workgroup adds all of them: n_act and the status counters, as block_scan records them.
template <typename T> __global__ __launch_bounds__(256) void block_ensemble_scatter(BlockEnsembleArgs<T> a) {
    __shared__ unsigned wave_count[4];
    __shared__ unsigned before_part[4], all_part[4];
    const unsigned      system = blockIdx.x / a.blocks;
    const unsigned      block  = blockIdx.x - system * a.blocks;
    BlockCtrl* const    c      = ctrl_of(a, system);
    if (c->go == 0) return;
    const unsigned long long now    = c->now;
    const unsigned* const    counts = reinterpret_cast<const unsigned*>(slice_of(a, system) + a.layout.counts);
    const unsigned           wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // lane t holds count t of the system
    const unsigned mine   = threadIdx.x < a.blocks ? counts[threadIdx.x] : 0u;
    unsigned       before = threadIdx.x < block ? mine : 0u, all = mine;
#pragma unroll
    for (int shift = 32; shift > 0; shift >>= 1) before += __shfl_xor(before, shift, 64), all += __shfl_xor(all, shift, 64);
    const unsigned           local  = block * 256u + threadIdx.x;
    const size_t             i      = static_cast<size_t>(system) * a.n + local;
    const bool               active = local < a.n && a.ticks[i] + ticks_of(a.levels[i], a.p.max_level) == now;
    const unsigned long long mask   = __builtin_amdgcn_ballot_w64(active);
    if (lane == 0) wave_count[wave] = static_cast<unsigned>(__builtin_popcountll(mask)), before_part[wave] = before, all_part[wave] = all;
    __syncthreads();
    if (block == 0 && threadIdx.x == 0) {
        const unsigned     n_act = all_part[0] + all_part[1] + all_part[2] + all_part[3];
        BlockStatus* const s     = a.status + system;
        c->n_act                 = n_act;
        s->now_ticks             = now;
        s->block_steps += 1;
        s->body_steps += n_act;
        s->last_active = n_act;
    }
    if (!active) return;
    unsigned at = before_part[0] + before_part[1] + before_part[2] + before_part[3] + static_cast<unsigned>(__builtin_popcountll(mask & ((1ull << lane) - 1ull)));
    for (unsigned w = 0; w < wave; ++w) at += wave_count[w];
    reinterpret_cast<unsigned*>(slice_of(a, system) + a.layout.active)[at] = local;
}

// init: per system, levels from the accelerations and jerks the ensemble evaluation left, ticks 0, the status and control records cleared
template <typename T> __global__ __launch_bounds__(256) void block_ensemble_init_levels(BlockEnsembleArgs<T> a) {
    using vec4            = typename Lane<T>::vec4;
    const unsigned system = blockIdx.x / a.blocks;
    const unsigned local  = (blockIdx.x - system * a.blocks) * 256u + threadIdx.x;
    if (local == 0) {
        BlockStatus s{};
        a.status[system] = s;
        BlockCtrl c{};
        *ctrl_of(a, system) = c;
    }
    if (local >= a.n) return;
    const size_t i     = static_cast<size_t>(system) * a.n + local;
    const vec4   acc = reinterpret_cast<const vec4*>(a.acc)[i], jerk = reinterpret_cast<const vec4*>(a.jerk)[i];
    a.levels[i] = first_level(acc, jerk, a.p);
    a.ticks[i]  = 0;
}

// The B status records folded into one: integer sums and exact minima / maxima, so the order changes nothing.  One workgroup.
__global__ __launch_bounds__(256) void block_ensemble_summary(const BlockStatus* status, unsigned b, BlockEnsembleSummary* out) {
    __shared__ unsigned long long lds[5][256];
    __shared__ int                lds_level[256];
    const int                     tid = threadIdx.x;
    unsigned long long            lo = ~0ull, hi = 0, blocks = 0, bodies = 0, stopped = 0;
    int                           deepest = 0;
    for (unsigned s = tid; s < b; s += 256u) {
        const BlockStatus r = status[s];
        lo = r.now_ticks < lo ? r.now_ticks : lo, hi = r.now_ticks > hi ? r.now_ticks : hi;
        blocks += r.block_steps, bodies += r.body_steps, stopped += (r.flags & kBlockStopped) ? 1 : 0;
        deepest = r.deepest_level > deepest ? r.deepest_level : deepest;
    }
    lds[0][tid] = lo, lds[1][tid] = hi, lds[2][tid] = blocks, lds[3][tid] = bodies, lds[4][tid] = stopped, lds_level[tid] = deepest;
    __syncthreads();
#pragma unroll 1
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half) {
            if (lds[0][tid + half] < lds[0][tid]) lds[0][tid] = lds[0][tid + half];
            if (lds[1][tid + half] > lds[1][tid]) lds[1][tid] = lds[1][tid + half];
            lds[2][tid] += lds[2][tid + half], lds[3][tid] += lds[3][tid + half], lds[4][tid] += lds[4][tid + half];
            if (lds_level[tid + half] > lds_level[tid]) lds_level[tid] = lds_level[tid + half];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    BlockEnsembleSummary r{};
    r.min_now_ticks = lds[0][0], r.max_now_ticks = lds[1][0], r.block_steps = lds[2][0], r.body_steps = lds[3][0];
    r.systems = b, r.stopped = static_cast<unsigned>(lds[4][0]), r.deepest_level = lds_level[0];
    *out = r;
}
