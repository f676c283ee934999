// hermite6_block_kernels.h -- internal launch interface of libnbody_hip_hermite6_block.so (include/nbody_hip_hermite6_block.h) between
// its C-ABI unit (hermite6_block_boundary.hip) and its kernel unit (hermite6_block.hip, contraction on).  Parameters, status record,
// control record, limits and the tiles x ranges geometry are the 4th-order block library's (hermite_block_kernels.h); what differs is the
// body of three vec4, the nine partial planes and the stored snaps and crackles.
#pragma once

#include "hermite_block_kernels.h"

namespace nb {

inline constexpr unsigned kBlock6Sums = 9;  // ax ay az jx jy jz sx sy sz: block_layout's planes, with three vec4 per predicted body

template <typename T> struct Block6Args {
    T *                 pos, *vel, *acc, *jerk, *snap, *crackle;  // stored state T[4N]
    unsigned long long* ticks;                                    // [N]
    int*                levels;                                   // [N]
    BlockStatus*        status;
    T*                  state12;                                  // workspace sections
    T*                  partial;
    unsigned*           active;
    unsigned*           counts;
    unsigned long long* min_part;
    int*                lvl_part;
    BlockCtrl*          ctrl;
    unsigned            n;
    T                   eps2;  // > 0 (the C boundary replaces 0 by the floor of nbody_hip_hermite.h)
    BlockParams         p;
    double              t_stop;
};

template <typename T> hipError_t launch_block6_init(const Block6Args<T>& a, hipStream_t stream);  // after nb_hermite6_init's four launches
template <typename T> hipError_t launch_block6_step(const Block6Args<T>& a, hipStream_t stream);
template <typename T>
hipError_t launch_block6_sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const T* snap, const T* crackle, const unsigned long long* ticks,
                              const BlockStatus* status, unsigned n, const BlockParams& p, hipStream_t stream);

}  // namespace nb
