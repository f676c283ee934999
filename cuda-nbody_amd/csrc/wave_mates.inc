// wave_mates.inc -- SIMD-mate priority of the kernels on the wave-stream plan (wave_stream.h), as TEXT included inside the kernel body, in
// four parts.  The includer defines ONE of WAVE_MATES_SETUP / _CHUNK / _DONE / _LEAVE in front of each include (the fragment undefines it):
//   SETUP  once, before the chunk loop   requires tid, lane, wave; defines progress, simd, mine, done (a __syncthreads inside)
//   CHUNK  first thing of every chunk    requires S
//   DONE   last thing of every chunk
//   LEAVE  once, behind the chunk loop
//
// The SIMD arbiter is oldest-first: left alone, the waves that share a SIMD finish equal shares of work one after the other and
// the last runs alone at a lower issue rate (nbody_fast_stream.inc has the measurements).  As there, each wave publishes how many
// chunks it has done; one that is level with the slowest wave of ITS SIMD runs at priority 3, one that is ahead at 0.  The
// chunk -> wave assignment stays static, so no result bit depends on it.  (Plain LDS words, one writer each; a stale read only
// delays a priority change.)
#if defined(WAVE_MATES_SETUP)
#undef WAVE_MATES_SETUP
    __shared__ unsigned progress[4 * 8];  // [SIMD][wave of the workgroup]: chunks done; 0xffffffff: not on this SIMD, or finished
    if (tid < 32) progress[tid] = 0xffffffffu;
    __syncthreads();
    const unsigned           simd = static_cast<unsigned>(__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4));  // HW_REG_HW_ID[5:4] = SIMD_ID
    volatile unsigned* const mine = progress + simd * 8;
    unsigned                 done = 0;
    if (lane == 0) mine[wave] = 0;
#elif defined(WAVE_MATES_CHUNK)
#undef WAVE_MATES_CHUNK
        if constexpr (S > 1) {
            unsigned least = done;
#pragma unroll
            for (int q = 0; q < 8; ++q) least = min(least, mine[q]);
            if (static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(least))) >= done) {
                __builtin_amdgcn_s_setprio(3);
            } else {
                __builtin_amdgcn_s_setprio(0);
            }
        }
#elif defined(WAVE_MATES_DONE)
#undef WAVE_MATES_DONE
        ++done;
        if (lane == 0) mine[wave] = done;
#elif defined(WAVE_MATES_LEAVE)
#undef WAVE_MATES_LEAVE
    if (lane == 0) mine[wave] = 0xffffffffu;  // finished: never the one the others defer to
    __builtin_amdgcn_s_setprio(0);
#else
#error "wave_mates.inc: define WAVE_MATES_SETUP, WAVE_MATES_CHUNK, WAVE_MATES_DONE or WAVE_MATES_LEAVE in front of the include"
#endif
