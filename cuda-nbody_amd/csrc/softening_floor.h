// softening_floor.h -- softening^2 == 0: the floor of nbody_hip_hermite.h (the i = j term contributes 0, not NaN).  One definition for
// the host boundaries (*_capi.hip) and for the two ensemble kernels, which floor a system's own softening^2 on the device.
#pragma once

#include <hip/hip_runtime.h>

namespace nb {

template <typename T> __host__ __device__ __forceinline__ T floored(T eps2) { return eps2 == T(0) ? (sizeof(T) == 4 ? T(0x1p-60) : T(0x1p-300)) : eps2; }

}  // namespace nb
