// energy_ensemble_kernels.h -- internal launch interface of libnbody_hip_energy_ensemble.so (include/nbody_hip_energy_ensemble.h) between its
// C-ABI unit (energy_ensemble_api.hip) and its kernel unit (energy_ensemble.hip).
#pragma once

#include "ensemble_kernels.h"  // the ensembles' limits and ensemble_systems_per_launch

struct nb_energy_ensemble_drift_record;  // include/nbody_hip_energy_ensemble.h

namespace nb {

// The geometry of a measurement: a function of (n, precision) alone.
struct EnergyEnsemblePlan {
    int      bodies_per_lane;  // I: a block is 64 * I bodies i
    int      waves;            // S
    unsigned blocks;           // NB; block a meets blocks a .. a + NB/2 (mod NB)
    unsigned splits;           // C: workgroups that share a block of bodies i and split its units
    unsigned units;            // per block: (NB/2 + 1) * I chunks of 64 bodies j
    unsigned groups;           // NB * C: workgroups (and records) per system
    unsigned block_threads;
    unsigned lds_bytes;
};
template <typename T> EnergyEnsemblePlan plan_energy_ensemble(unsigned n);

// Records (128 bytes each) the workspace holds per system, for either precision: at least plan_energy_ensemble<T>(n).groups, and
// monotone in n (groups itself is not: it steps down where the bodies per lane double).  NB * C <= (n / (64 I) + 1) * I <= n / 64 + 8.
inline unsigned energy_ensemble_records(unsigned n) { return (n + 63) / 64 + 8; }

template <typename T> struct EnergyEnsembleArgs {
    const T*           pos;
    const T*           vel;
    double*            records;      // [system][group][kRecord]
    nb_energy_t*       results;      // [system]
    const T*           system_eps2;  // null: eps2; else system s reads system_eps2[s * eps2_stride]
    unsigned           eps2_stride;
    unsigned           n, blocks, splits, units, groups;
    unsigned long long first_system;  // of this launch (a call whose grid would pass 2^31 threads is cut into several)
    T                  eps2;
};

// pairs then finish, each cut into launches of at most 2^31 threads
template <typename T> hipError_t launch_energy_ensemble(const EnergyEnsembleArgs<T>& a, unsigned long long systems, const EnergyEnsemblePlan& p, hipStream_t stream);
hipError_t launch_energy_ensemble_drift(const nb_energy_t* start, const nb_energy_t* end, unsigned systems, nb_energy_ensemble_drift_record* out, hipStream_t stream);

}  // namespace nb
