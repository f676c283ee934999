// hermite6_block_ensemble_kernels.h -- internal launch interface of libnbody_hip_hermite6_block_ensemble.so
// (include/nbody_hip_hermite6_block_ensemble.h) between its C-ABI unit (hermite6_block_ensemble_boundary.hip) and its kernel unit
// (hermite6_block_ensemble.hip, contraction on).  Limits, summary record, per-system geometry and workspace layout are the 4th-order block
// ensemble's (hermite_block_ensemble_kernels.h), the layout with three vec4 per predicted body and nine partial planes
// (hermite6_block_kernels.h); what differs in the arguments is the stored snaps and crackles.
#pragma once

#include "hermite6_block_kernels.h"
#include "hermite_block_ensemble_kernels.h"

namespace nb {

// The order-independent schedule kernels (hermite_block_ensemble_schedule.inc) read the base alone.
template <typename T> struct Block6EnsembleArgs : BlockEnsembleArgs<T> {
    T *snap, *crackle;  // stored state T[4 N B]
};

template <typename T> hipError_t launch_block6_ensemble_init(const Block6EnsembleArgs<T>& a, hipStream_t stream);  // after init's four evaluation launches
template <typename T> hipError_t launch_block6_ensemble_step(const Block6EnsembleArgs<T>& a, hipStream_t stream);
template <typename T>
hipError_t launch_block6_ensemble_sync(T* pos_out, T* vel_out, const T* pos, const T* vel, const T* acc, const T* jerk, const T* snap, const T* crackle,
                                       const unsigned long long* ticks, const BlockStatus* status, unsigned n, unsigned b, const BlockParams& p, hipStream_t stream);
hipError_t launch_block6_ensemble_summary(const BlockStatus* status, unsigned b, BlockEnsembleSummary* out, hipStream_t stream);

}  // namespace nb
