// hermite_block_schedule.inc -- the schedule kernels of a block step that do not depend on the order of the scheme, one text for
// hermite_block.hip (nb_hermite_block_*) and hermite6_block.hip (nb_hermite6_block_*): the partial minima of tick + ticks(level), the
// fixed-order scan of the per-workgroup active counts, and the scatter of the active list.  Included inside each translation unit's own
// anonymous namespace, after hermite_block_kernels.h (BlockCtrl, BlockStatus) and hermite_block_kernels_shared.h (ticks_of, block_fold).

__global__ __launch_bounds__(256) void block_min_partial(const unsigned long long* ticks, const int* levels, unsigned n, int max_level, unsigned long long* min_part, int* lvl_part) {
    __shared__ unsigned long long lds_next[256];
    __shared__ int                lds_level[256];
    MinLevel                      m{~0ull, 0};
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256u) {
        const int                k    = levels[i];
        const unsigned long long next = ticks[i] + ticks_of(k, max_level);
        if (next < m.next) m.next = next;
        if (k > m.level) m.level = k;
    }
    m = block_fold(m, lds_next, lds_level);
    if (threadIdx.x == 0) min_part[blockIdx.x] = m.next, lvl_part[blockIdx.x] = m.level;
}

// counts[b] -> the number of active bodies in the workgroups before b (in place); n_act; the status counters.  One workgroup of 1 024.
__global__ __launch_bounds__(1024) void block_scan(unsigned* counts, unsigned blocks, BlockCtrl* ctrl, BlockStatus* status) {
    __shared__ unsigned sums[1024];
    if (ctrl->go == 0) return;
    const unsigned tid = threadIdx.x, per = (blocks + 1023u) / 1024u;
    const unsigned lo = tid * per < blocks ? tid * per : blocks, hi = lo + per < blocks ? lo + per : blocks;
    unsigned       mine = 0;
    for (unsigned b = lo; b < hi; ++b) mine += counts[b];
    sums[tid] = mine;
    __syncthreads();
#pragma unroll 1
    for (unsigned step = 1; step < 1024u; step *= 2) {  // inclusive scan; integer sums, so the order changes nothing
        const unsigned add = tid >= step ? sums[tid - step] : 0u;
        __syncthreads();
        sums[tid] += add;
        __syncthreads();
    }
    unsigned before = sums[tid] - mine;
    for (unsigned b = lo; b < hi; ++b) {
        const unsigned count = counts[b];
        counts[b]            = before;
        before += count;
    }
    if (tid == 1023u) {
        const unsigned n_act = sums[1023];
        ctrl->n_act          = n_act;
        status->now_ticks    = ctrl->now;
        status->block_steps += 1;
        status->body_steps += n_act;
        status->last_active = n_act;
    }
}

__global__ __launch_bounds__(256) void block_scatter(const unsigned long long* ticks, const int* levels, const unsigned* offsets, const BlockCtrl* ctrl, unsigned* active_list,
                                                     unsigned n, int max_level) {
    __shared__ unsigned wave_count[4];
    if (ctrl->go == 0) return;
    const unsigned long long now    = ctrl->now;
    const unsigned           i      = blockIdx.x * 256u + threadIdx.x;
    const bool               active = i < n && ticks[i] + ticks_of(levels[i], max_level) == now;
    const unsigned long long mask   = __builtin_amdgcn_ballot_w64(active);
    const unsigned           wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wave_count[wave] = static_cast<unsigned>(__builtin_popcountll(mask));
    __syncthreads();
    if (!active) return;
    unsigned at = offsets[blockIdx.x] + static_cast<unsigned>(__builtin_popcountll(mask & ((1ull << lane) - 1ull)));
    for (unsigned w = 0; w < wave; ++w) at += wave_count[w];
    active_list[at] = i;
}
