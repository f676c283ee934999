// hermite_ensemble_clock.inc -- the clock machinery of an ensemble that does not depend on the order of the scheme, one text for
// hermite_ensemble.hip (nb_hermite_ensemble_*) and hermite6_ensemble.hip (nb_hermite6_ensemble_*): the rule of *_advance_* as a function of
// a system's clock, the scalar loads of what is uniform over a workgroup, a system's dt and softening^2, the minimum over a workgroup, the
// tally behind the status record and the kernel that sums the blocks' tallies.  (What a clock kernel does with a system's next dt is
// hermite_ensemble_clock_update.inc, text inside that kernel.)  Included inside each translation unit's own anonymous
// namespace, after hermite_ensemble_kernels.h (EnsembleClock, EnsembleStatus, EnsembleSource) and softening_floor.h.

// The rule of nb_hermite_ensemble_advance_*, as far as it is a function of the clock before the call: does the system step, with which dt,
// and is that step its last?
enum : int { kSkip = 0, kFinish = 1, kStep = 2, kLastStep = 3 };
template <typename T> __device__ __forceinline__ int clock_decision(const EnsembleClock& c, double t_stop, double dt_max, T& dt) {
    if (c.flags & (kClockDone | kClockStalled)) return kSkip;
    const double remaining = t_stop - c.time;
    if (!(remaining > 0) || static_cast<T>(remaining) == T(0)) return kFinish;
    const double cand = dt_max < c.dt_next ? dt_max : c.dt_next;
    if (cand >= remaining) {
        dt = static_cast<T>(remaining);
        return kLastStep;
    }
    dt = static_cast<T>(cand);
    return kStep;
}

// (read-only for the whole launch -> scalar loads where the index is wave-uniform)
template <typename V> __device__ __forceinline__ V uniform_load(const V* p, size_t index) {
    typedef const V __attribute__((address_space(4)))* uniform_ptr;
    return reinterpret_cast<uniform_ptr>(reinterpret_cast<unsigned long long>(p))[index];
}

// dt and softening^2 of system s; false: the system takes no step in this call
template <typename T, bool STEP> __device__ __forceinline__ bool system_parameters(const EnsembleSource<T>& src, unsigned s, T& dt, T& eps2) {
    dt = src.dt, eps2 = src.eps2;
    if (src.params != nullptr) {
        dt   = uniform_load(src.params, 4 * static_cast<size_t>(s));
        eps2 = uniform_load(src.params, 4 * static_cast<size_t>(s) + 1);
    } else if (src.system_eps2 != nullptr) {
        eps2 = uniform_load(src.system_eps2, s);
    }
    eps2 = floored(eps2);
    if constexpr (STEP) {
        if (src.clocks != nullptr) {
            const double* const        words = reinterpret_cast<const double*>(src.clocks) + 4 * static_cast<size_t>(s);
            const std::uint32_t* const halves = reinterpret_cast<const std::uint32_t*>(words);
            EnsembleClock              c;
            c.time = uniform_load(words, 0), c.dt_next = uniform_load(words, 1), c.dt_last = 0, c.steps = 0, c.flags = uniform_load(halves, 7);
            return clock_decision<T>(c, src.t_stop, src.dt_max, dt) >= kStep;
        }
    }
    return true;
}

#include "block_min.inc"

// what one system, or a block of them, adds to the status record
struct Tally {
    unsigned long long systems, done, stalled, stepped, total_steps;
    double             min_time, min_dt_last;
};
__device__ __forceinline__ Tally block_tally(Tally t, unsigned long long (*sums)[256], double (*mins)[256]) {
    const int tid = threadIdx.x;
    sums[0][tid] = t.systems, sums[1][tid] = t.done, sums[2][tid] = t.stalled, sums[3][tid] = t.stepped, sums[4][tid] = t.total_steps;
    mins[0][tid] = t.min_time, mins[1][tid] = t.min_dt_last;
    __syncthreads();
#pragma unroll 1
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int q = 0; q < 5; ++q) sums[q][tid] += sums[q][tid + half];
#pragma unroll
            for (int q = 0; q < 2; ++q) mins[q][tid] = fmin(mins[q][tid], mins[q][tid + half]);
        }
        __syncthreads();
    }
    return Tally{sums[0][0], sums[1][0], sums[2][0], sums[3][0], sums[4][0], mins[0][0], mins[1][0]};
}
__device__ __forceinline__ void store_tally(const Tally& t, EnsembleStatus* out) {
    EnsembleStatus s{};
    s.systems = static_cast<std::uint32_t>(t.systems), s.done = static_cast<std::uint32_t>(t.done), s.stalled = static_cast<std::uint32_t>(t.stalled);
    s.stepped = static_cast<std::uint32_t>(t.stepped), s.total_steps = t.total_steps, s.min_time = t.min_time, s.min_dt_last = t.min_dt_last;
    *out = s;
}

// the blocks' tallies -> the status record (one workgroup)
__global__ __launch_bounds__(256) void hermite_ensemble_status(const EnsembleStatus* block_status, unsigned blocks, EnsembleStatus* status) {
    __shared__ unsigned long long sums[5][256];
    __shared__ double             mins[2][256];
    Tally                         t{0, 0, 0, 0, 0, __builtin_inf(), __builtin_inf()};
    for (unsigned i = threadIdx.x; i < blocks; i += 256u) {
        const EnsembleStatus r = block_status[i];
        t.systems += r.systems, t.done += r.done, t.stalled += r.stalled, t.stepped += r.stepped, t.total_steps += r.total_steps;
        t.min_time = fmin(t.min_time, r.min_time), t.min_dt_last = fmin(t.min_dt_last, r.min_dt_last);
    }
    t = block_tally(t, sums, mins);
    if (threadIdx.x == 0) store_tally(t, status);
}
