// nbody_pair_lead.h -- internal: the headline geometry's own forces kernel (nbody_pair_lead.hip: pair_forces_jpacked), as launch_pair
// of nbody_pair.hip sees it.  Nothing here is exported.
#pragma once

#include "nbody_kernels.h"

namespace nb {

// Does the one-GPU step launch pair_forces_jpacked in pair_forces<float, 8, 8>'s place?  Only the single full tournament of launch_pair
// in that geometry (R = 8, S = 8, one workgroup per block), and only while no clock words are lent (they ask for pair_forces_clocked) and no probe event is set (nb_set_pair_probe_event: the
// forces kernel timed on its own is set against the cycles pair_forces_clocked counts, so both are pair_forces');
// never in a variant build of nbody_pair.hip (NB_PAIR_STAMPS and the like: launch_pair does not ask then).  Unit ranges, rectangles,
// slices, the multi-GPU layer and fp64 keep pair_forces.
bool       pair_lead_takes(const PairArgs<float>& args, const PairGeom& g);
inline bool pair_lead_takes(const PairArgs<double>&, const PairGeom&) { return false; }

// The launch (prepare_only: arm the kernel's large-LDS attribute and return, as launch_pair_tile does).  Fills blocks / splits.
hipError_t       launch_pair_lead(const PairArgs<float>& args, hipStream_t stream, bool prepare_only);
inline hipError_t launch_pair_lead(const PairArgs<double>&, hipStream_t, bool) { return hipErrorInvalidValue; }

}  // namespace nb
