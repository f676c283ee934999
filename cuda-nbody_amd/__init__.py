"""cuda-nbody_amd -- MI355X-native all-pairs N-body hot path behind the reference's own seams.

The product is the C-ABI shared library ``libnbody_hip.so`` (include/nbody_hip.h) built from the hand-written
gfx950 HIP kernels in ``csrc/``, plus the C++23 host mirror of the reference's ``BodySystemCUDA`` /
``ComputeCUDA`` / ``Compute`` / CLI in ``host/``.  This Python module is the thin ctypes binding used by
tests/, bench.py and __graft_entry__.py: it mirrors the reference's ``BodySystemCUDADefault<T>`` interface
(/root/reference/src/nbody/bodysystemcuda.hpp:38-72, bodysystemcuda_default.cu:19-55) call for call.

There is NO CPU fallback: if libnbody_hip.so is missing or a HIP call fails, this module raises.

The directory name carries a hyphen, so import it with ``__graft_entry__.load_package()``.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NBODY_HIP_LIB", os.path.join(HERE, "libnbody_hip.so"))
# The lab bench (include/nbody_hip_lab.h: real-RCCL self-test, loopback rank, in-process world, allocation-failure hook) is a second
# library made of the SAME object files plus csrc/nbody_comm_lab.hip.  A process uses ONE of the two: use_lab() (or NBODY_HIP_LAB=1 in
# the environment) before the first lib() call makes lib() load libnbody_hip_lab.so instead -- tests/ and tools/ that need the lab
# do that in a process of their own; the product library never exports the lab's symbols.
LAB_LIB_PATH = os.environ.get("NBODY_HIP_LAB_LIB", os.path.join(HERE, "libnbody_hip_lab.so"))
# Ensembles (include/nbody_hip_ensemble.h: many independent systems of one size stepped in one launch) are a third library of their
# own objects; it shares no state with the other two and is loaded next to either of them by ensemble_lib().
ENSEMBLE_LIB_PATH = os.environ.get("NBODY_HIP_ENSEMBLE_LIB", os.path.join(HERE, "libnbody_hip_ensemble.so"))
# 4th-order Hermite steps (include/nbody_hip_hermite.h) are a fourth library on the same terms, loaded by hermite_lib().
HERMITE_LIB_PATH = os.environ.get("NBODY_HIP_HERMITE_LIB", os.path.join(HERE, "libnbody_hip_hermite.so"))
# 6th-order Hermite steps (include/nbody_hip_hermite6.h) are an eleventh, loaded by hermite6_lib().
HERMITE6_LIB_PATH = os.environ.get("NBODY_HIP_HERMITE6_LIB", os.path.join(HERE, "libnbody_hip_hermite6.so"))
# Hermite steps with block time steps (include/nbody_hip_hermite_block.h) are a fifth, loaded by hermite_block_lib().
HERMITE_BLOCK_LIB_PATH = os.environ.get("NBODY_HIP_HERMITE_BLOCK_LIB", os.path.join(HERE, "libnbody_hip_hermite_block.so"))
# Nearest neighbours, potentials and neighbour lists (include/nbody_hip_neighbour.h) are a sixth, loaded by neighbour_lib().
NEIGHBOUR_LIB_PATH = os.environ.get("NBODY_HIP_NEIGHBOUR_LIB", os.path.join(HERE, "libnbody_hip_neighbour.so"))
# Acceleration, jerk and potential of N sources at M points of the caller's own (include/nbody_hip_field.h) are a seventh, loaded by field_lib().
FIELD_LIB_PATH = os.environ.get("NBODY_HIP_FIELD_LIB", os.path.join(HERE, "libnbody_hip_field.so"))
# The K nearest neighbours, local densities and the density centre (include/nbody_hip_knn.h) are an eighth, loaded by knn_lib().
KNN_LIB_PATH = os.environ.get("NBODY_HIP_KNN_LIB", os.path.join(HERE, "libnbody_hip_knn.so"))
# Hermite steps of many independent systems, a time step per system (include/nbody_hip_hermite_ensemble.h) are a ninth, loaded by
# hermite_ensemble_lib().
HERMITE_ENSEMBLE_LIB_PATH = os.environ.get("NBODY_HIP_HERMITE_ENSEMBLE_LIB", os.path.join(HERE, "libnbody_hip_hermite_ensemble.so"))
# Block time steps of many independent systems, one launch per stage (include/nbody_hip_hermite_block_ensemble.h) are a tenth, loaded by
# hermite_block_ensemble_lib().
HERMITE_BLOCK_ENSEMBLE_LIB_PATH = os.environ.get("NBODY_HIP_HERMITE_BLOCK_ENSEMBLE_LIB", os.path.join(HERE, "libnbody_hip_hermite_block_ensemble.so"))
# 6th-order Hermite steps with block time steps (include/nbody_hip_hermite6_block.h) are a twelfth, loaded by hermite6_block_lib().
HERMITE6_BLOCK_LIB_PATH = os.environ.get("NBODY_HIP_HERMITE6_BLOCK_LIB", os.path.join(HERE, "libnbody_hip_hermite6_block.so"))
# 6th-order Hermite steps of many independent systems, a time step per system (include/nbody_hip_hermite6_ensemble.h) are a thirteenth,
# loaded by hermite6_ensemble_lib().
HERMITE6_ENSEMBLE_LIB_PATH = os.environ.get("NBODY_HIP_HERMITE6_ENSEMBLE_LIB", os.path.join(HERE, "libnbody_hip_hermite6_ensemble.so"))
# 6th-order block time steps of many systems in one launch per stage (include/nbody_hip_hermite6_block_ensemble.h): a library of its own
HERMITE6_BLOCK_ENSEMBLE_LIB_PATH = os.environ.get("NBODY_HIP_HERMITE6_BLOCK_ENSEMBLE_LIB", os.path.join(HERE, "libnbody_hip_hermite6_block_ensemble.so"))
# The energies of every system of an ensemble in one call, and the drift between two measurements (include/nbody_hip_energy_ensemble.h): a
# library of its own, loaded by energy_ensemble_lib().
ENERGY_ENSEMBLE_LIB_PATH = os.environ.get("NBODY_HIP_ENERGY_ENSEMBLE_LIB", os.path.join(HERE, "libnbody_hip_energy_ensemble.so"))

NB_MODE_STRICT, NB_MODE_FAST = 0, 1
NB_SHARD_ACC_IN, NB_SHARD_FINALIZE = 1, 2
NB_ERR_INVALID_ARGUMENT, NB_ERR_UNSUPPORTED, NB_ERR_RCCL_BASE = 10001, 10002, 20000
NB_ERR_OUT_OF_MEMORY = 2  # = hipErrorOutOfMemory: what nb_alloc answers when the device has no room

# enum class NBodyConfig, src/nbody/nbody_config.hpp:3
NBODY_CONFIG_RANDOM, NBODY_CONFIG_SHELL, NBODY_CONFIG_EXPAND = 0, 1, 2


@dataclass
class NBodyParams:
    """struct NBodyParams, src/nbody/params.hpp:8-16 (camera_origin dropped: display only)."""
    time_step: float = 0.016
    cluster_scale: float = 1.54
    velocity_scale: float = 8.0
    softening: float = 0.1
    damping: float = 1.0


# Compute::demo_params, src/nbody/compute.hpp:90-97
DEMO_PARAMS = (
    NBodyParams(0.016, 1.54, 8.0, 0.1, 1.0),
    NBodyParams(0.016, 0.68, 20.0, 0.1, 1.0),
    NBodyParams(0.0006, 0.16, 1000.0, 1.0, 1.0),
    NBodyParams(0.0006, 0.16, 1000.0, 1.0, 1.0),
    NBodyParams(0.0019, 0.32, 276.0, 1.0, 1.0),
    NBodyParams(0.0016, 0.32, 272.0, 0.145, 1.0),
    NBodyParams(0.016, 6.04, 0.0, 1.0, 1.0),
)


class NBodyHipError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what}: {code}")
        self.code = code


class DeviceInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 256), ("arch", ctypes.c_char * 64), ("compute_units", ctypes.c_int),
                ("wavefront_size", ctypes.c_int), ("clock_khz", ctypes.c_int), ("can_map_host_memory", ctypes.c_int),
                ("lds_bytes_per_cu", ctypes.c_int), ("total_memory", ctypes.c_size_t)]


class PairPlan(ctypes.Structure):
    _fields_ = [("applies", ctypes.c_int), ("bodies_per_lane", ctypes.c_int), ("waves_per_block", ctypes.c_int), ("splits", ctypes.c_uint),
                ("blocks", ctypes.c_uint), ("block_bodies", ctypes.c_uint), ("reaction_slots", ctypes.c_uint), ("grid_blocks", ctypes.c_uint),
                ("lds_bytes", ctypes.c_uint), ("workspace_bytes", ctypes.c_size_t), ("slices", ctypes.c_uint)]


class CommSelftest(ctypes.Structure):
    """nb_comm_selftest_t (include/nbody_hip_tuning.h): what the self-loop through the real RCCL reported"""
    _fields_ = [("rccl_version", ctypes.c_int), ("send_recv_status", ctypes.c_int), ("all_gather_status", ctypes.c_int),
                ("send_recv_ms", ctypes.c_float), ("all_gather_ms", ctypes.c_float),
                ("send_recv_wrong_bytes", ctypes.c_size_t), ("all_gather_wrong_bytes", ctypes.c_size_t),
                ("refused_call", ctypes.c_char * 64), ("library_path", ctypes.c_char * 256)]


class LaunchPlan(ctypes.Structure):
    _fields_ = [("bodies_per_lane", ctypes.c_int), ("lanes_per_body", ctypes.c_int), ("tile_bodies", ctypes.c_int),
                ("block_threads", ctypes.c_int), ("grid_blocks", ctypes.c_uint), ("lds_bytes", ctypes.c_uint)]


class Energy(ctypes.Structure):
    """nb_energy_t (include/nbody_hip.h): energy, momentum and angular momentum of a state, G = 1"""
    _fields_ = [("kinetic", ctypes.c_double), ("potential", ctypes.c_double), ("total", ctypes.c_double), ("mass", ctypes.c_double),
                ("momentum", ctypes.c_double * 3), ("angular_momentum", ctypes.c_double * 3), ("center_of_mass", ctypes.c_double * 3)]


# name -> (restype, argtypes); this table is also what tests/test_capi_symbols.py checks against the header
_vp, _ci, _cu, _cf, _cd, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
_P = ctypes.POINTER
SIGNATURES = {
    "nb_error_string": (ctypes.c_char_p, [_ci]),
    "nb_version": (ctypes.c_char_p, []),
    "nb_device_count": (_ci, [_P(_ci)]),
    "nb_set_device": (_ci, [_ci]),
    "nb_get_device": (_ci, [_P(_ci)]),
    "nb_device_info": (_ci, [_ci, _P(DeviceInfo)]),
    "nb_alloc": (_ci, [_P(_vp), _sz]),
    "nb_free": (_ci, [_vp]),
    "nb_memset": (_ci, [_vp, _ci, _sz, _vp]),
    "nb_h2d": (_ci, [_vp, _vp, _sz, _vp]),
    "nb_d2h": (_ci, [_vp, _vp, _sz, _vp]),
    "nb_d2d": (_ci, [_vp, _vp, _sz, _vp]),
    "nb_host_alloc_mapped": (_ci, [_P(_vp), _P(_vp), _sz]),
    "nb_host_free": (_ci, [_vp]),
    "nb_stream_create": (_ci, [_P(_vp)]),
    "nb_stream_destroy": (_ci, [_vp]),
    "nb_stream_synchronize": (_ci, [_vp]),
    "nb_stream_wait_event": (_ci, [_vp, _vp]),
    "nb_event_create": (_ci, [_P(_vp)]),
    "nb_event_destroy": (_ci, [_vp]),
    "nb_event_record": (_ci, [_vp, _vp]),
    "nb_event_synchronize": (_ci, [_vp]),
    "nb_event_elapsed_ms": (_ci, [_P(_cf), _vp, _vp]),
    "nb_device_synchronize": (_ci, []),
    "nb_set_softening_sq_f32": (_ci, [_cf]),
    "nb_set_softening_sq_f64": (_ci, [_cd]),
    "nb_get_softening_sq_f32": (_ci, [_P(_cf)]),
    "nb_get_softening_sq_f64": (_ci, [_P(_cd)]),
    "nb_integrate_f32": (_ci, [_vp, _vp, _vp, _cf, _cf, _cu, _ci, _ci, _vp]),
    "nb_integrate_f64": (_ci, [_vp, _vp, _vp, _cd, _cd, _cu, _ci, _ci, _vp]),
    "nb_integrate_shard_f32": (_ci, [_vp, _vp, _vp, _vp, _cu, _cu, _cu, _cu, _cu, _cf, _cf, _ci, _ci, _vp]),
    "nb_integrate_shard_f64": (_ci, [_vp, _vp, _vp, _vp, _cu, _cu, _cu, _cu, _cu, _cd, _cd, _ci, _ci, _vp]),
    "nb_graph_create_f32": (_ci, [_P(_vp), _vp, _vp, _vp, _cf, _cf, _cu, _ci, _ci, _cu]),
    "nb_graph_create_f64": (_ci, [_P(_vp), _vp, _vp, _vp, _cd, _cd, _cu, _ci, _ci, _cu]),
    "nb_graph_create_ws_f32": (_ci, [_P(_vp), _vp, _vp, _vp, _cf, _cf, _cu, _ci, _ci, _cu, _vp, _sz]),
    "nb_graph_create_ws_f64": (_ci, [_P(_vp), _vp, _vp, _vp, _cd, _cd, _cu, _ci, _ci, _cu, _vp, _sz]),
    "nb_workspace_bytes_f32": (_ci, [_cu, _ci, _P(_sz)]),
    "nb_workspace_bytes_f64": (_ci, [_cu, _ci, _P(_sz)]),
    "nb_workspace_bytes_capped_f32": (_ci, [_cu, _ci, _sz, _P(_sz)]),
    "nb_workspace_bytes_capped_f64": (_ci, [_cu, _ci, _sz, _P(_sz)]),
    "nb_integrate_ws_f32": (_ci, [_vp, _vp, _vp, _cf, _cf, _cu, _ci, _ci, _vp, _sz, _vp]),
    "nb_integrate_ws_f64": (_ci, [_vp, _vp, _vp, _cd, _cd, _cu, _ci, _ci, _vp, _sz, _vp]),
    "nb_pair_plan_f32": (_ci, [_cu, _P(PairPlan)]),
    "nb_pair_plan_f64": (_ci, [_cu, _P(PairPlan)]),
    "nb_graph_launch": (_ci, [_vp, _vp]),
    "nb_graph_destroy": (_ci, [_vp]),
    "nb_comm_unique_id": (_ci, [_vp]),
    "nb_comm_init_rank": (_ci, [_P(_vp), _vp, _ci, _ci]),
    "nb_comm_init_all": (_ci, [_P(_vp), _ci, _P(_ci)]),
    "nb_comm_destroy": (_ci, [_vp]),
    "nb_comm_info": (_ci, [_vp, _P(_ci), _P(_ci), _P(_ci)]),
    "nb_comm_stream_create": (_ci, [_vp, _P(_vp)]),
    "nb_stream_create_placed": (_ci, [_P(_vp)]),
    "nb_comm_set_workspace": (_ci, [_vp, _vp, _sz]),
    "nb_comm_layout_f32": (_ci, [_vp, _cu, _ci, _P(_ci)]),
    "nb_comm_layout_f64": (_ci, [_vp, _cu, _ci, _P(_ci)]),
    "nb_comm_set_exchange_grouping": (_ci, [_vp, _ci]),
    "nb_comm_get_exchange_grouping": (_ci, [_vp, _P(_ci)]),
    "nb_comm_workspace_bytes_f32": (_ci, [_vp, _cu, _ci, _P(_sz)]),
    "nb_comm_workspace_bytes_f64": (_ci, [_vp, _cu, _ci, _P(_sz)]),
    "nb_sharded_step_f32": (_ci, [_vp, _vp, _vp, _vp, _vp, _cu, _cf, _cf, _ci, _ci, _vp]),
    "nb_sharded_step_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _cu, _cd, _cd, _ci, _ci, _vp]),
    "nb_sharded_step_all_f32": (_ci, [_P(_vp), _ci, _P(_vp), _P(_vp), _P(_vp), _P(_vp), _cu, _cf, _cf, _ci, _ci, _P(_vp)]),
    "nb_sharded_step_all_f64": (_ci, [_P(_vp), _ci, _P(_vp), _P(_vp), _P(_vp), _P(_vp), _cu, _cd, _cd, _ci, _ci, _P(_vp)]),
    "nb_exchange_tiles_f32": (_ci, [_vp, _vp, _cu, _vp]),
    "nb_exchange_tiles_f64": (_ci, [_vp, _vp, _cu, _vp]),
    "nb_allgather_f32": (_ci, [_vp, _vp, _cu, _vp]),
    "nb_allgather_f64": (_ci, [_vp, _vp, _cu, _vp]),
    "nb_exchange_wait_tile": (_ci, [_vp, _ci, _vp]),
    "nb_exchange_wait_all": (_ci, [_vp, _vp]),
    "nb_energy_workspace_bytes": (_ci, [_cu, _P(_sz)]),
    "nb_energy_f32": (_ci, [_vp, _vp, _cu, _vp, _sz, _vp, _vp]),
    "nb_energy_f64": (_ci, [_vp, _vp, _cu, _vp, _sz, _vp, _vp]),
    "nb_plan_f32": (_ci, [_cu, _cu, _P(LaunchPlan)]),
    "nb_plan_f64": (_ci, [_cu, _cu, _P(LaunchPlan)]),
}

# include/nbody_hip_tuning.h: process-global tuning / test hooks, not part of the drop-in boundary
TUNING_SIGNATURES = {
    "nb_set_plan_override": (_ci, [_ci, _ci, _ci]),
    "nb_set_pair_plan_override": (_ci, [_ci, _ci, _ci, _ci]),
    "nb_set_pair_slices_override": (_ci, [_ci]),
    "nb_comm_set_pair_min_slice": (_ci, [_ci]),
    "nb_set_late_diagonal": (_ci, [_ci]),
    "nb_emulate_pair_rank_f32": (_ci, [_vp, _vp, _vp, _vp, _P(_sz), _cu, _ci, _ci, _cf, _cf, _vp]),
    "nb_emulate_pair_rank_f64": (_ci, [_vp, _vp, _vp, _vp, _P(_sz), _cu, _ci, _ci, _cd, _cd, _vp]),
    "nb_comm_reaction_exchange_f32": (_ci, [_vp, _cu, _vp]),
    "nb_comm_reaction_exchange_f64": (_ci, [_vp, _cu, _vp]),
    "nb_set_pair_probe_event": (_ci, [_vp]),
    "nb_set_memory_budget": (_ci, [_sz]),
    "nb_lds_optin_count": (_ci, [_P(_ci)]),
    "nb_comm_transport_info": (_ci, [_vp, _P(_ci), ctypes.c_char_p, _sz]),
    "nb_comm_last_step_trace": (_ci, [_vp, ctypes.c_char_p, _sz]),
    "nb_comm_side_stream_collisions": (_ci, [_vp, _P(_ci)]),
    "nb_comm_settle_side_stream": (_ci, [_vp, _vp]),
    "nb_comm_caller_stream_placement": (_ci, [_vp, _P(_ci)]),
    "nb_comm_pair_work_f32": (_ci, [_vp, _cu, _P(ctypes.c_ulonglong), _P(_ci)]),
    "nb_comm_pair_work_f64": (_ci, [_vp, _cu, _P(ctypes.c_ulonglong), _P(_ci)]),
    "nb_comm_last_enqueue_ms": (_ci, [_vp, _P(_cd)]),
    "nb_set_pair_clock_words": (_ci, [_vp, _sz]),
}

# include/nbody_hip_lab.h: exported by libnbody_hip_lab.so only
LAB_SIGNATURES = {
    "nb_clock_probe_launch": (_ci, [_vp, _ci, _cu, _vp]),
    "nb_set_alloc_limit": (_ci, [_sz]),
    "nb_comm_selftest_open": (_ci, [_P(_vp), _vp]),
    "nb_comm_loopback_open": (_ci, [_P(_vp), _vp, _ci, _ci]),
    "nb_comm_inprocess_open_all": (_ci, [_P(_vp), _ci, _vp]),
    "nb_comm_selftest_f32": (_ci, [_vp, _sz, _vp, _P(CommSelftest)]),
    "nb_comm_self_transfer_f32": (_ci, [_vp, _vp, _vp, _sz, _ci, _ci, _vp, _vp, _vp]),
    "nb_comm_replace_side_stream": (_ci, [_vp]),
}

# include/nbody_hip_ensemble.h: exported by libnbody_hip_ensemble.so, and nothing else is
class EnsemblePlan(ctypes.Structure):
    """nb_ensemble_plan_t: the FAST geometry of an ensemble (every field but grid_blocks a function of N and the precision)"""
    _fields_ = [("bodies_per_lane", ctypes.c_int), ("waves_per_group", ctypes.c_int), ("groups_per_system", ctypes.c_uint),
                ("block_threads", ctypes.c_uint), ("lds_bytes", ctypes.c_uint), ("grid_blocks", ctypes.c_ulonglong)]


ENSEMBLE_SIGNATURES = {
    "nb_ensemble_plan_f32": (_ci, [_cu, _cu, _P(EnsemblePlan)]),
    "nb_ensemble_plan_f64": (_ci, [_cu, _cu, _P(EnsemblePlan)]),
    "nb_ensemble_integrate_f32": (_ci, [_vp, _vp, _vp, _cu, _cu, _cf, _cf, _cf, _vp, _ci, _vp]),
    "nb_ensemble_integrate_f64": (_ci, [_vp, _vp, _vp, _cu, _cu, _cd, _cd, _cd, _vp, _ci, _vp]),
}


# include/nbody_hip_hermite.h: exported by libnbody_hip_hermite.so, and nothing else is
class HermitePlan(ctypes.Structure):
    """nb_hermite_plan_t: the geometry of the acceleration + jerk kernel, a function of N and the precision"""
    _fields_ = [("bodies_per_lane", ctypes.c_int), ("waves_per_group", ctypes.c_int), ("unroll", ctypes.c_int),
                ("groups", ctypes.c_uint), ("block_threads", ctypes.c_uint), ("lds_bytes", ctypes.c_uint)]


HERMITE_MAX_BODIES = 1 << 26
HERMITE_TIMESTEP_SCRATCH_BYTES = 8192
HERMITE_SIGNATURES = {
    "nb_hermite_workspace_bytes": (_ci, [_cu, _cu, _P(_sz)]),
    "nb_hermite_plan_f32": (_ci, [_cu, _P(HermitePlan)]),
    "nb_hermite_plan_f64": (_ci, [_cu, _P(HermitePlan)]),
    "nb_hermite_eval_f32": (_ci, [_vp, _vp, _vp, _vp, _cu, _cf, _vp]),
    "nb_hermite_eval_f64": (_ci, [_vp, _vp, _vp, _vp, _cu, _cd, _vp]),
    "nb_hermite_step_f32": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _cu, _cf, _cf, _vp]),
    "nb_hermite_step_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _cu, _cd, _cd, _vp]),
    "nb_hermite_timestep_f32": (_ci, [_vp, _vp, _cu, _cf, _vp, _vp, _sz, _vp]),
    "nb_hermite_timestep_f64": (_ci, [_vp, _vp, _cu, _cd, _vp, _vp, _sz, _vp]),
}


# include/nbody_hip_hermite6.h: exported by libnbody_hip_hermite6.so, and nothing else is
class Hermite6Plan(ctypes.Structure):
    """nb_hermite6_plan_t: the geometry of the acceleration + jerk + snap kernel, a function of N and the precision"""
    _fields_ = [("bodies_per_lane", ctypes.c_int), ("waves_per_group", ctypes.c_int), ("unroll", ctypes.c_int),
                ("groups", ctypes.c_uint), ("block_threads", ctypes.c_uint), ("lds_bytes", ctypes.c_uint)]


HERMITE6_MAX_BODIES = 1 << 26
HERMITE6_TIMESTEP_SCRATCH_BYTES = 8192
HERMITE6_SIGNATURES = {
    "nb_hermite6_workspace_bytes": (_ci, [_cu, _cu, _P(_sz)]),
    "nb_hermite6_plan_f32": (_ci, [_cu, _P(Hermite6Plan)]),
    "nb_hermite6_plan_f64": (_ci, [_cu, _P(Hermite6Plan)]),
    "nb_hermite6_eval_f32": (_ci, [_vp] * 7 + [_sz, _cu, _cf, _vp]),
    "nb_hermite6_eval_f64": (_ci, [_vp] * 7 + [_sz, _cu, _cd, _vp]),
    "nb_hermite6_init_f32": (_ci, [_vp] * 7 + [_sz, _cu, _cf, _vp]),
    "nb_hermite6_init_f64": (_ci, [_vp] * 7 + [_sz, _cu, _cd, _vp]),
    "nb_hermite6_step_f32": (_ci, [_vp] * 8 + [_sz, _cu, _cf, _cf, _vp]),
    "nb_hermite6_step_f64": (_ci, [_vp] * 8 + [_sz, _cu, _cd, _cd, _vp]),
    "nb_hermite6_timestep_f32": (_ci, [_vp] * 4 + [_cu, _cf, _vp, _vp, _sz, _vp]),
    "nb_hermite6_timestep_f64": (_ci, [_vp] * 4 + [_cu, _cd, _vp, _vp, _sz, _vp]),
}


# include/nbody_hip_hermite_block.h: exported by libnbody_hip_hermite_block.so, and nothing else is
class HermiteBlockParams(ctypes.Structure):
    """nb_hermite_block_params_t"""
    _fields_ = [("eta", _cd), ("eta_start", _cd), ("dt_max", _cd), ("max_level", _ci), ("reserved", _ci)]


class HermiteBlockStatus(ctypes.Structure):
    """nb_hermite_block_status_t: 64 bytes of device memory the block steps keep up to date"""
    _fields_ = [("now_ticks", ctypes.c_uint64), ("block_steps", ctypes.c_uint64), ("body_steps", ctypes.c_uint64), ("last_active", ctypes.c_uint32),
                ("deepest_level", ctypes.c_int32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 7)]


class HermiteBlockPlan(ctypes.Structure):
    """nb_hermite_block_plan_t: the geometry of one block step's evaluation, a function of N, n_act and the precision"""
    _fields_ = [("bodies_per_lane", _ci), ("waves_per_group", _ci), ("unroll", _ci), ("tiles", _cu), ("ranges", _cu), ("groups", _cu),
                ("launch_groups", _cu), ("block_threads", _cu), ("lds_bytes", _cu), ("slots", _cu), ("chunks", _cu), ("launches", _cu),
                ("partial_offset", ctypes.c_ulonglong), ("partial_bytes", ctypes.c_ulonglong)]


HERMITE_BLOCK_MAX_BODIES = 1 << 24
HERMITE_BLOCK_MAX_LEVEL = 40
HERMITE_BLOCK_STOPPED = 1
_block_state = [_vp] * 8 + [_sz, _cu]  # positions velocities accelerations jerks ticks levels status workspace, workspace_bytes, N
HERMITE_BLOCK_SIGNATURES = {
    "nb_hermite_block_workspace_bytes": (_ci, [_cu, _cu, _P(_sz)]),
    "nb_hermite_block_plan_f32": (_ci, [_cu, _cu, _P(HermiteBlockPlan)]),
    "nb_hermite_block_plan_f64": (_ci, [_cu, _cu, _P(HermiteBlockPlan)]),
    "nb_hermite_block_init_f32": (_ci, _block_state + [_cf, _P(HermiteBlockParams), _vp]),
    "nb_hermite_block_init_f64": (_ci, _block_state + [_cd, _P(HermiteBlockParams), _vp]),
    "nb_hermite_block_step_f32": (_ci, _block_state + [_cf, _P(HermiteBlockParams), _cd, _vp]),
    "nb_hermite_block_step_f64": (_ci, _block_state + [_cd, _P(HermiteBlockParams), _cd, _vp]),
    "nb_hermite_block_sync_f32": (_ci, [_vp] * 8 + [_cu, _P(HermiteBlockParams), _vp]),
    "nb_hermite_block_sync_f64": (_ci, [_vp] * 8 + [_cu, _P(HermiteBlockParams), _vp]),
}

# include/nbody_hip_hermite6_block.h: exported by libnbody_hip_hermite6_block.so, and nothing else is.  Parameters, status and plan
# records are the 4th-order block library's.
_block6_state = [_vp] * 10 + [_sz, _cu]  # positions velocities accelerations jerks snaps crackles ticks levels status workspace, workspace_bytes, N
HERMITE6_BLOCK_SIGNATURES = {
    "nb_hermite6_block_workspace_bytes": (_ci, [_cu, _cu, _P(_sz)]),
    "nb_hermite6_block_plan_f32": (_ci, [_cu, _cu, _P(HermiteBlockPlan)]),
    "nb_hermite6_block_plan_f64": (_ci, [_cu, _cu, _P(HermiteBlockPlan)]),
    "nb_hermite6_block_init_f32": (_ci, _block6_state + [_cf, _P(HermiteBlockParams), _vp]),
    "nb_hermite6_block_init_f64": (_ci, _block6_state + [_cd, _P(HermiteBlockParams), _vp]),
    "nb_hermite6_block_step_f32": (_ci, _block6_state + [_cf, _P(HermiteBlockParams), _cd, _vp]),
    "nb_hermite6_block_step_f64": (_ci, _block6_state + [_cd, _P(HermiteBlockParams), _cd, _vp]),
    "nb_hermite6_block_sync_f32": (_ci, [_vp] * 10 + [_cu, _P(HermiteBlockParams), _vp]),
    "nb_hermite6_block_sync_f64": (_ci, [_vp] * 10 + [_cu, _P(HermiteBlockParams), _vp]),
}


# include/nbody_hip_neighbour.h: exported by libnbody_hip_neighbour.so, and nothing else is
class NeighbourStatus(ctypes.Structure):
    """nb_neighbour_status_t: 64 bytes of device memory every survey and lists call writes"""
    _fields_ = [("total_neighbours", ctypes.c_uint64), ("closest_dist_sq", _cd), ("closest_i", ctypes.c_uint32), ("closest_j", ctypes.c_uint32),
                ("max_count", ctypes.c_uint32), ("max_count_body", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 7)]


class NeighbourPlan(ctypes.Structure):
    """nb_neighbour_plan_t: the geometry of the survey and the lists, a function of N and the precision"""
    _fields_ = [("bodies_per_lane", _ci), ("waves_per_group", _ci), ("unroll", _ci), ("tiles", _cu), ("block_threads", _cu), ("lds_bytes", _cu),
                ("chunks", _cu), ("list_ranges", _cu), ("list_groups", _cu), ("survey_launches", _cu), ("list_launches", _cu), ("reserved", _cu),
                ("planes_offset", ctypes.c_ulonglong), ("planes_bytes", ctypes.c_ulonglong)]


NEIGHBOUR_MAX_BODIES = 1 << 24
NEIGHBOUR_NONE = 0xFFFFFFFF
NEIGHBOUR_OVERFLOW = 1
_ull = ctypes.c_ulonglong
NEIGHBOUR_SIGNATURES = {
    "nb_neighbour_workspace_bytes": (_ci, [_cu, _cu, _P(_sz)]),
    "nb_neighbour_plan_f32": (_ci, [_cu, _P(NeighbourPlan)]),
    "nb_neighbour_plan_f64": (_ci, [_cu, _P(NeighbourPlan)]),
    # positions N radius_sq radii_sq softening_sq | nearest_index nearest_dist_sq counts potentials | status workspace workspace_bytes stream
    "nb_neighbour_survey_f32": (_ci, [_vp, _cu, _cf, _vp, _cf, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nb_neighbour_survey_f64": (_ci, [_vp, _cu, _cd, _vp, _cd, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # positions N radius_sq radii_sq | offsets indices capacity | status workspace workspace_bytes stream
    "nb_neighbour_lists_f32": (_ci, [_vp, _cu, _cf, _vp, _vp, _vp, _ull, _vp, _vp, _sz, _vp]),
    "nb_neighbour_lists_f64": (_ci, [_vp, _cu, _cd, _vp, _vp, _vp, _ull, _vp, _vp, _sz, _vp]),
}


# include/nbody_hip_field.h: exported by libnbody_hip_field.so, and nothing else is
class FieldPlan(ctypes.Structure):
    """nb_field_plan_t: the geometry of an evaluation, a function of N, M and the precision"""
    _fields_ = [("bodies_per_lane", _ci), ("waves_per_group", _ci), ("unroll", _ci), ("tiles", _cu), ("ranges", _cu), ("groups", _cu), ("block_threads", _cu),
                ("lds_bytes", _cu), ("launches", _cu), ("reserved", _cu), ("partial_offset", ctypes.c_ulonglong), ("partial_bytes", ctypes.c_ulonglong)]


FIELD_MAX_SOURCES = 1 << 26
FIELD_MAX_TARGETS = 1 << 24
FIELD_NONE = 0xFFFFFFFF
FIELD_SIGNATURES = {
    "nb_field_workspace_bytes": (_ci, [_cu, _cu, _cu, _P(_sz)]),
    "nb_field_plan_f32": (_ci, [_cu, _cu, _P(FieldPlan)]),
    "nb_field_plan_f64": (_ci, [_cu, _cu, _P(FieldPlan)]),
    # sources source_velocities N | targets target_velocities self_index M softening_sq | accelerations jerks potentials | workspace workspace_bytes stream
    "nb_field_eval_f32": (_ci, [_vp, _vp, _cu, _vp, _vp, _vp, _cu, _cf, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nb_field_eval_f64": (_ci, [_vp, _vp, _cu, _vp, _vp, _vp, _cu, _cd, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# include/nbody_hip_knn.h: exported by libnbody_hip_knn.so, and nothing else is
class KnnStructure(ctypes.Structure):
    """nb_knn_structure_t: 128 bytes of device memory a survey with the record writes"""
    _fields_ = [("sum_density", _cd), ("centre", _cd * 3), ("density_radius", _cd), ("core_radius", _cd), ("max_density", _cd), ("min_kth_dist_sq", _cd),
                ("max_kth_dist_sq", _cd), ("max_density_body", ctypes.c_uint32), ("defined", ctypes.c_uint32), ("degenerate", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 10)]


class KnnPlan(ctypes.Structure):
    """nb_knn_plan_t: the geometry of a survey, a function of N, K and the precision"""
    _fields_ = [("bodies_per_lane", _ci), ("waves_per_group", _ci), ("unroll", _ci), ("capacity", _ci), ("ranges", _cu), ("tiles", _cu), ("block_threads", _cu),
                ("lds_bytes", _cu), ("chunks", _cu), ("blocks", _cu), ("search_launches", _cu), ("structure_launches", _cu),
                ("density_offset", ctypes.c_ulonglong), ("density_bytes", ctypes.c_ulonglong)]


KNN_MAX_K = 16
KNN_SPHERE = 4.188790204786391
KNN_DEGENERATE = 1
KNN_NO_DENSITY = 2
KNN_SIGNATURES = {
    "nb_knn_workspace_bytes": (_ci, [_cu, _cu, _cu, _P(_sz)]),
    "nb_knn_plan_f32": (_ci, [_cu, _cu, _P(KnnPlan)]),
    "nb_knn_plan_f64": (_ci, [_cu, _cu, _P(KnnPlan)]),
    # positions N K | knn_index knn_dist_sq densities structure | workspace workspace_bytes stream
    "nb_knn_survey_f32": (_ci, [_vp, _cu, _cu, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nb_knn_survey_f64": (_ci, [_vp, _cu, _cu, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# include/nbody_hip_hermite_ensemble.h: exported by libnbody_hip_hermite_ensemble.so, and nothing else is
class HermiteEnsemblePlan(ctypes.Structure):
    """nb_hermite_ensemble_plan_t: nb_hermite_plan_t per system, and the grid"""
    _fields_ = [("bodies_per_lane", ctypes.c_int), ("waves_per_group", ctypes.c_int), ("unroll", ctypes.c_int), ("groups", ctypes.c_uint),
                ("block_threads", ctypes.c_uint), ("lds_bytes", ctypes.c_uint), ("groups_per_system", ctypes.c_uint), ("reserved", ctypes.c_uint),
                ("grid_blocks", ctypes.c_ulonglong)]


class HermiteEnsembleClock(ctypes.Structure):
    """nb_hermite_ensemble_clock_t: 32 bytes of device memory per system"""
    _fields_ = [("time", ctypes.c_double), ("dt_next", ctypes.c_double), ("dt_last", ctypes.c_double), ("steps", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class HermiteEnsembleStatus(ctypes.Structure):
    """nb_hermite_ensemble_status_t: 64 bytes of device memory nb_hermite_ensemble_advance_* writes"""
    _fields_ = [("systems", ctypes.c_uint32), ("done", ctypes.c_uint32), ("stalled", ctypes.c_uint32), ("stepped", ctypes.c_uint32),
                ("total_steps", ctypes.c_uint64), ("min_time", ctypes.c_double), ("min_dt_last", ctypes.c_double), ("reserved", ctypes.c_uint64 * 3)]


HERMITE_ENSEMBLE_CLOCK_DTYPE = np.dtype([("time", "<f8"), ("dt_next", "<f8"), ("dt_last", "<f8"), ("steps", "<u4"), ("flags", "<u4")])
HERMITE_ENSEMBLE_MAX_BODIES = 65536
HERMITE_ENSEMBLE_MAX_TOTAL = 1 << 28
HERMITE_ENSEMBLE_DONE, HERMITE_ENSEMBLE_STALLED = 1, 2
HERMITE_ENSEMBLE_SIGNATURES = {
    "nb_hermite_ensemble_workspace_bytes": (_ci, [_cu, _cu, _cu, _P(_sz)]),
    "nb_hermite_ensemble_plan_f32": (_ci, [_cu, _cu, _P(HermiteEnsemblePlan)]),
    "nb_hermite_ensemble_plan_f64": (_ci, [_cu, _cu, _P(HermiteEnsemblePlan)]),
    # accelerations jerks positions velocities | N B | softening_sq system_softening_sq | stream
    "nb_hermite_ensemble_eval_f32": (_ci, [_vp, _vp, _vp, _vp, _cu, _cu, _cf, _vp, _vp]),
    "nb_hermite_ensemble_eval_f64": (_ci, [_vp, _vp, _vp, _vp, _cu, _cu, _cd, _vp, _vp]),
    # new_positions old_positions velocities accelerations jerks | workspace workspace_bytes | N B | delta_time softening_sq system_params | stream
    "nb_hermite_ensemble_step_f32": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _cu, _cu, _cf, _cf, _vp, _vp]),
    "nb_hermite_ensemble_step_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _cu, _cu, _cd, _cd, _vp, _vp]),
    # accelerations jerks | N B | eta dt_out | workspace workspace_bytes | stream
    "nb_hermite_ensemble_timestep_f32": (_ci, [_vp, _vp, _cu, _cu, _cf, _vp, _vp, _sz, _vp]),
    "nb_hermite_ensemble_timestep_f64": (_ci, [_vp, _vp, _cu, _cu, _cd, _vp, _vp, _sz, _vp]),
    # accelerations jerks positions velocities clocks | N B | softening_sq system_softening_sq eta | workspace workspace_bytes | stream
    "nb_hermite_ensemble_begin_f32": (_ci, [_vp, _vp, _vp, _vp, _vp, _cu, _cu, _cf, _vp, _cf, _vp, _sz, _vp]),
    "nb_hermite_ensemble_begin_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _cu, _cu, _cd, _vp, _cd, _vp, _sz, _vp]),
    # new_positions old_positions velocities accelerations jerks clocks status | workspace workspace_bytes | N B | t_stop dt_max eta softening_sq
    # system_softening_sq | stream
    "nb_hermite_ensemble_advance_f32": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _cu, _cu, _cd, _cd, _cf, _cf, _vp, _vp]),
    "nb_hermite_ensemble_advance_f64": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _cu, _cu, _cd, _cd, _cd, _cd, _vp, _vp]),
}

# include/nbody_hip_hermite_block_ensemble.h: exported by libnbody_hip_hermite_block_ensemble.so, and nothing else is
# include/nbody_hip_hermite6_ensemble.h: exported by libnbody_hip_hermite6_ensemble.so, and nothing else is.  Plan, clock, status, flags and
# limits are nbody_hip_hermite_ensemble.h's.
HERMITE6_ENSEMBLE_SIGNATURES = {
    "nb_hermite6_ensemble_workspace_bytes": (_ci, [_cu, _cu, _cu, _P(_sz)]),
    "nb_hermite6_ensemble_plan_f32": (_ci, [_cu, _cu, _P(HermiteEnsemblePlan)]),
    "nb_hermite6_ensemble_plan_f64": (_ci, [_cu, _cu, _P(HermiteEnsemblePlan)]),
    # acc_out, jerk_out, snap_out, positions, velocities, acc_in, workspace, bytes, N, B, softening_sq, system_softening_sq, stream
    "nb_hermite6_ensemble_eval_f32": (_ci, [_vp] * 7 + [_sz, _cu, _cu, _cf, _vp, _vp]),
    "nb_hermite6_ensemble_eval_f64": (_ci, [_vp] * 7 + [_sz, _cu, _cu, _cd, _vp, _vp]),
    # accelerations, jerks, snaps, crackles, positions, velocities, workspace, bytes, N, B, softening_sq, system_softening_sq, stream
    "nb_hermite6_ensemble_init_f32": (_ci, [_vp] * 7 + [_sz, _cu, _cu, _cf, _vp, _vp]),
    "nb_hermite6_ensemble_init_f64": (_ci, [_vp] * 7 + [_sz, _cu, _cu, _cd, _vp, _vp]),
    # new_pos, old_pos, vel, acc, jerk, snap, crackle, workspace, bytes, N, B, delta_time, softening_sq, system_params, stream
    "nb_hermite6_ensemble_step_f32": (_ci, [_vp] * 8 + [_sz, _cu, _cu, _cf, _cf, _vp, _vp]),
    "nb_hermite6_ensemble_step_f64": (_ci, [_vp] * 8 + [_sz, _cu, _cu, _cd, _cd, _vp, _vp]),
    # acc, jerk, snap, crackle, N, B, eta, dt_out, workspace, bytes, stream
    "nb_hermite6_ensemble_timestep_f32": (_ci, [_vp] * 4 + [_cu, _cu, _cf, _vp, _vp, _sz, _vp]),
    "nb_hermite6_ensemble_timestep_f64": (_ci, [_vp] * 4 + [_cu, _cu, _cd, _vp, _vp, _sz, _vp]),
    # acc, jerk, snap, crackle, pos, vel, clocks, N, B, softening_sq, system_softening_sq, eta, workspace, bytes, stream
    "nb_hermite6_ensemble_begin_f32": (_ci, [_vp] * 7 + [_cu, _cu, _cf, _vp, _cf, _vp, _sz, _vp]),
    "nb_hermite6_ensemble_begin_f64": (_ci, [_vp] * 7 + [_cu, _cu, _cd, _vp, _cd, _vp, _sz, _vp]),
    # new_pos, old_pos, vel, acc, jerk, snap, crackle, clocks, status, workspace, bytes, N, B, t_stop, dt_max, eta, softening_sq,
    # system_softening_sq, stream
    "nb_hermite6_ensemble_advance_f32": (_ci, [_vp] * 10 + [_sz, _cu, _cu, _cd, _cd, _cf, _cf, _vp, _vp]),
    "nb_hermite6_ensemble_advance_f64": (_ci, [_vp] * 10 + [_sz, _cu, _cu, _cd, _cd, _cd, _cd, _vp, _vp]),
}


class HermiteBlockEnsemblePlan(ctypes.Structure):
    """nb_hermite_block_ensemble_plan_t: nb_hermite_block_plan_t of (N, n_act), and what the number of systems adds"""
    _fields_ = [("bodies_per_lane", _ci), ("waves_per_group", _ci), ("unroll", _ci), ("tiles", _cu), ("ranges", _cu), ("groups", _cu),
                ("launch_groups", _cu), ("block_threads", _cu), ("lds_bytes", _cu), ("slots", _cu), ("chunks", _cu), ("step_launches", _cu),
                ("partial_offset", ctypes.c_ulonglong), ("partial_bytes", ctypes.c_ulonglong), ("groups_per_system", _cu), ("blocks_per_system", _cu),
                ("eval_grid", ctypes.c_ulonglong), ("schedule_grid", ctypes.c_ulonglong), ("workspace_stride", ctypes.c_ulonglong)]


class HermiteBlockEnsembleSummary(ctypes.Structure):
    """nb_hermite_block_ensemble_summary_t: the B status records folded into 64 bytes of device memory"""
    _fields_ = [("min_now_ticks", ctypes.c_uint64), ("max_now_ticks", ctypes.c_uint64), ("block_steps", ctypes.c_uint64), ("body_steps", ctypes.c_uint64),
                ("systems", ctypes.c_uint32), ("stopped", ctypes.c_uint32), ("deepest_level", ctypes.c_int32), ("reserved", ctypes.c_uint32 * 5)]


HERMITE_BLOCK_ENSEMBLE_MAX_BODIES = 65536
HERMITE_BLOCK_ENSEMBLE_MAX_TOTAL = 1 << 28
# positions velocities accelerations jerks ticks levels status workspace, workspace_bytes, N, B
_block_ensemble_state = [_vp] * 8 + [_sz, _cu, _cu]
HERMITE_BLOCK_ENSEMBLE_SIGNATURES = {
    "nb_hermite_block_ensemble_workspace_bytes": (_ci, [_cu, _cu, _cu, _P(_sz)]),
    "nb_hermite_block_ensemble_plan_f32": (_ci, [_cu, _cu, _cu, _P(HermiteBlockEnsemblePlan)]),
    "nb_hermite_block_ensemble_plan_f64": (_ci, [_cu, _cu, _cu, _P(HermiteBlockEnsemblePlan)]),
    # ... softening_sq system_softening_sq params [t_stop] stream
    "nb_hermite_block_ensemble_init_f32": (_ci, _block_ensemble_state + [_cf, _vp, _P(HermiteBlockParams), _vp]),
    "nb_hermite_block_ensemble_init_f64": (_ci, _block_ensemble_state + [_cd, _vp, _P(HermiteBlockParams), _vp]),
    "nb_hermite_block_ensemble_step_f32": (_ci, _block_ensemble_state + [_cf, _vp, _P(HermiteBlockParams), _cd, _vp]),
    "nb_hermite_block_ensemble_step_f64": (_ci, _block_ensemble_state + [_cd, _vp, _P(HermiteBlockParams), _cd, _vp]),
    "nb_hermite_block_ensemble_sync_f32": (_ci, [_vp] * 8 + [_cu, _cu, _P(HermiteBlockParams), _vp]),
    "nb_hermite_block_ensemble_sync_f64": (_ci, [_vp] * 8 + [_cu, _cu, _P(HermiteBlockParams), _vp]),
    "nb_hermite_block_ensemble_summary": (_ci, [_vp, _cu, _vp, _vp]),
}

# include/nbody_hip_hermite6_block_ensemble.h: exported by libnbody_hip_hermite6_block_ensemble.so, and nothing else is.  Plan and summary
# records are the 4th-order block ensemble's.
# positions velocities accelerations jerks snaps crackles ticks levels status workspace, workspace_bytes, N, B
_block6_ensemble_state = [_vp] * 10 + [_sz, _cu, _cu]
HERMITE6_BLOCK_ENSEMBLE_SIGNATURES = {
    "nb_hermite6_block_ensemble_workspace_bytes": (_ci, [_cu, _cu, _cu, _P(_sz)]),
    "nb_hermite6_block_ensemble_plan_f32": (_ci, [_cu, _cu, _cu, _P(HermiteBlockEnsemblePlan)]),
    "nb_hermite6_block_ensemble_plan_f64": (_ci, [_cu, _cu, _cu, _P(HermiteBlockEnsemblePlan)]),
    # ... softening_sq system_softening_sq params [t_stop] stream
    "nb_hermite6_block_ensemble_init_f32": (_ci, _block6_ensemble_state + [_cf, _vp, _P(HermiteBlockParams), _vp]),
    "nb_hermite6_block_ensemble_init_f64": (_ci, _block6_ensemble_state + [_cd, _vp, _P(HermiteBlockParams), _vp]),
    "nb_hermite6_block_ensemble_step_f32": (_ci, _block6_ensemble_state + [_cf, _vp, _P(HermiteBlockParams), _cd, _vp]),
    "nb_hermite6_block_ensemble_step_f64": (_ci, _block6_ensemble_state + [_cd, _vp, _P(HermiteBlockParams), _cd, _vp]),
    "nb_hermite6_block_ensemble_sync_f32": (_ci, [_vp] * 10 + [_cu, _cu, _P(HermiteBlockParams), _vp]),
    "nb_hermite6_block_ensemble_sync_f64": (_ci, [_vp] * 10 + [_cu, _cu, _P(HermiteBlockParams), _vp]),
    "nb_hermite6_block_ensemble_summary": (_ci, [_vp, _cu, _vp, _vp]),
}

# include/nbody_hip_energy_ensemble.h: exported by libnbody_hip_energy_ensemble.so, and nothing else is
class EnergyEnsemblePlan(ctypes.Structure):
    """nb_energy_ensemble_plan_t: the geometry of a measurement, a function of (N, precision) but for the grid"""
    _fields_ = [("bodies_per_lane", _ci), ("waves_per_group", _ci), ("groups_per_system", _cu), ("block_threads", _cu), ("lds_bytes", _cu), ("reserved", _cu),
                ("grid_blocks", ctypes.c_ulonglong)]


class EnergyDrift(ctypes.Structure):
    """nb_energy_ensemble_drift_t: 64 bytes of device memory nb_energy_ensemble_drift writes"""
    _fields_ = [("worst_relative_drift", _cd), ("rms_relative_drift", _cd), ("worst_momentum_drift", _cd), ("systems", _cu), ("worst_system", _cu),
                ("worst_momentum_system", _cu), ("not_finite", _cu), ("reserved", ctypes.c_ulonglong * 3)]


ENERGY_ENSEMBLE_SIGNATURES = {
    "nb_energy_ensemble_plan_f32": (_ci, [_cu, _cu, _P(EnergyEnsemblePlan)]),
    "nb_energy_ensemble_plan_f64": (_ci, [_cu, _cu, _P(EnergyEnsemblePlan)]),
    "nb_energy_ensemble_workspace_bytes": (_ci, [_cu, _cu, _P(_sz)]),
    # positions velocities N B | softening_sq system_softening_sq softening_stride | workspace workspace_bytes | device_results stream
    "nb_energy_ensemble_f32": (_ci, [_vp, _vp, _cu, _cu, _cf, _vp, _cu, _vp, _sz, _vp, _vp]),
    "nb_energy_ensemble_f64": (_ci, [_vp, _vp, _cu, _cu, _cd, _vp, _cu, _vp, _sz, _vp, _vp]),
    # start end B | device_summary stream
    "nb_energy_ensemble_drift": (_ci, [_vp, _vp, _cu, _vp, _vp]),
}

_lib = None
_loaded = {}  # path -> the library at that path, its signatures set
_lab = os.environ.get("NBODY_HIP_LAB") == "1"


def use_lab() -> None:
    """This process works with the lab library (libnbody_hip_lab.so: everything libnbody_hip.so exports + include/nbody_hip_lab.h).
    Must come before the first lib() call: communicators, streams and the process-global settings belong to ONE loaded library."""
    global _lab
    if _lib is not None and not _lab:
        raise RuntimeError("use_lab() after libnbody_hip.so was loaded: a process uses one of the two libraries (set NBODY_HIP_LAB=1 or call it first)")
    _lab = True


def is_lab() -> bool:
    return _lab


def _load(path: str, signatures: dict) -> ctypes.CDLL:
    """The library at `path`, loaded once, every function of `signatures` given its types (fails loudly when it has not been built)."""
    if path not in _loaded:
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: build it with `make -C {os.path.join(HERE, 'csrc')}` "
                                    "(or __graft_entry__.build()); there is no CPU fallback")
        handle = ctypes.CDLL(path)
        for name, (restype, argtypes) in signatures.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = restype, argtypes
        _loaded[path] = handle
    return _loaded[path]


def lib() -> ctypes.CDLL:
    """Load libnbody_hip.so -- or, after use_lab(), libnbody_hip_lab.so (fails loudly when the HIP extension has not been built)."""
    global _lib
    if _lib is None:
        _lib = _load(LAB_LIB_PATH if _lab else LIB_PATH, {**SIGNATURES, **TUNING_SIGNATURES, **(LAB_SIGNATURES if _lab else {})})
    return _lib


def ensemble_lib() -> ctypes.CDLL:
    """Load libnbody_hip_ensemble.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(ENSEMBLE_LIB_PATH, ENSEMBLE_SIGNATURES)


def hermite_lib() -> ctypes.CDLL:
    """Load libnbody_hip_hermite.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(HERMITE_LIB_PATH, HERMITE_SIGNATURES)


def hermite6_lib() -> ctypes.CDLL:
    """Load libnbody_hip_hermite6.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(HERMITE6_LIB_PATH, HERMITE6_SIGNATURES)


def hermite_ensemble_lib() -> ctypes.CDLL:
    """Load libnbody_hip_hermite_ensemble.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(HERMITE_ENSEMBLE_LIB_PATH, HERMITE_ENSEMBLE_SIGNATURES)


def hermite6_ensemble_lib() -> ctypes.CDLL:
    """Load libnbody_hip_hermite6_ensemble.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(HERMITE6_ENSEMBLE_LIB_PATH, HERMITE6_ENSEMBLE_SIGNATURES)


def hermite_block_ensemble_lib() -> ctypes.CDLL:
    """Load libnbody_hip_hermite_block_ensemble.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(HERMITE_BLOCK_ENSEMBLE_LIB_PATH, HERMITE_BLOCK_ENSEMBLE_SIGNATURES)


def hermite6_block_ensemble_lib() -> ctypes.CDLL:
    """Load libnbody_hip_hermite6_block_ensemble.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(HERMITE6_BLOCK_ENSEMBLE_LIB_PATH, HERMITE6_BLOCK_ENSEMBLE_SIGNATURES)


def hermite_block_lib() -> ctypes.CDLL:
    """Load libnbody_hip_hermite_block.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(HERMITE_BLOCK_LIB_PATH, HERMITE_BLOCK_SIGNATURES)


def hermite6_block_lib() -> ctypes.CDLL:
    """Load libnbody_hip_hermite6_block.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(HERMITE6_BLOCK_LIB_PATH, HERMITE6_BLOCK_SIGNATURES)


def neighbour_lib() -> ctypes.CDLL:
    """Load libnbody_hip_neighbour.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(NEIGHBOUR_LIB_PATH, NEIGHBOUR_SIGNATURES)


def field_lib() -> ctypes.CDLL:
    """Load libnbody_hip_field.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(FIELD_LIB_PATH, FIELD_SIGNATURES)


def knn_lib() -> ctypes.CDLL:
    """Load libnbody_hip_knn.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(KNN_LIB_PATH, KNN_SIGNATURES)


def energy_ensemble_lib() -> ctypes.CDLL:
    """Load libnbody_hip_energy_ensemble.so (fails loudly when it has not been built).  Its errors are named by lib().nb_error_string."""
    return _load(ENERGY_ENSEMBLE_LIB_PATH, ENERGY_ENSEMBLE_SIGNATURES)


def check(code: int, what: str = "nbody_hip") -> None:
    if code != 0:
        name = lib().nb_error_string(code)
        raise NBodyHipError(code, f"{what}: {name.decode() if name else '?'}")


def device_count() -> int:
    n = _ci(0)
    check(lib().nb_device_count(ctypes.byref(n)), "nb_device_count")
    return n.value


def device_info(device: int = 0) -> DeviceInfo:
    info = DeviceInfo()
    check(lib().nb_device_info(device, ctypes.byref(info)), "nb_device_info")
    return info


def plan(i_count: int, j_count: int, dtype=np.float32) -> LaunchPlan:
    p = LaunchPlan()
    fn = lib().nb_plan_f32 if np.dtype(dtype) == np.float32 else lib().nb_plan_f64
    check(fn(i_count, j_count, ctypes.byref(p)), "nb_plan")
    return p


def pair_plan(num_bodies: int, dtype=np.float32) -> PairPlan:
    p = PairPlan()
    fn = lib().nb_pair_plan_f32 if np.dtype(dtype) == np.float32 else lib().nb_pair_plan_f64
    check(fn(num_bodies, ctypes.byref(p)), "nb_pair_plan")
    return p


def set_pair_plan_override(vectors_per_lane: int = 0, waves_per_block: int = 0, splits: int = 0, min_bodies: int = 0) -> None:
    check(lib().nb_set_pair_plan_override(vectors_per_lane, waves_per_block, splits, min_bodies), "nb_set_pair_plan_override")


def set_pair_slices_override(slices: int = 0) -> None:
    check(lib().nb_set_pair_slices_override(slices), "nb_set_pair_slices_override")


def set_plan_override(bodies_per_lane: int = 0, lanes_per_body: int = 0, tile_bodies: int = 0) -> None:
    check(lib().nb_set_plan_override(bodies_per_lane, lanes_per_body, tile_bodies), "nb_set_plan_override")


def set_softening_squared(value) -> None:
    """set_softening_squared(float|double), src/nbody/bodysystemcuda.cu:46-60 (overload chosen by dtype)."""
    if isinstance(value, np.float64) or type(value) is float:
        check(lib().nb_set_softening_sq_f64(float(value)), "nb_set_softening_sq_f64")
    else:
        check(lib().nb_set_softening_sq_f32(np.float32(value)), "nb_set_softening_sq_f32")


class DeviceBuffer:
    """A caller-owned device array (what thrust::device_vector<T> is to the reference)."""

    def __init__(self, nbytes: int):
        self.ptr = _vp()
        self.nbytes = nbytes
        check(lib().nb_alloc(ctypes.byref(self.ptr), nbytes), "nb_alloc")
        check(lib().nb_memset(self.ptr, 0, nbytes, None), "nb_memset")

    def upload(self, host: np.ndarray) -> None:
        assert host.flags.c_contiguous and host.nbytes <= self.nbytes
        check(lib().nb_h2d(self.ptr, host.ctypes.data_as(_vp), host.nbytes, None), "nb_h2d")

    def download(self, host: np.ndarray) -> np.ndarray:
        assert host.flags.c_contiguous and host.nbytes <= self.nbytes
        check(lib().nb_d2h(host.ctypes.data_as(_vp), self.ptr, host.nbytes, None), "nb_d2h")
        return host

    def free(self) -> None:
        if self.ptr:
            lib().nb_free(self.ptr)
            self.ptr = _vp()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _plan(load, stem: str, record, dtype, *sizes):
    """nb_<stem>_plan_f32 / _f64 of the library `load()` gives, for `sizes`: a filled `record`"""
    p = record()
    fn = getattr(load(), f"nb_{stem}_plan_" + ("f32" if np.dtype(dtype) == np.float32 else "f64"))
    check(fn(*sizes, ctypes.byref(p)), f"nb_{stem}_plan")
    return p


def _query_workspace_bytes(load, stem: str, dtype, *sizes) -> int:
    """nb_<stem>_workspace_bytes of the library `load()` gives, for `sizes` and the precision"""
    out = _sz(0)
    check(getattr(load(), f"nb_{stem}_workspace_bytes")(*sizes, np.dtype(dtype).itemsize, ctypes.byref(out)), f"nb_{stem}_workspace_bytes")
    return out.value


class _DeviceState:
    """What the classes of the small libraries share: a precision, the device buffers ``_buffers()`` lists, and the f32 / f64 entry
    points of one library (``_library``: its loader; ``_prefix``: how its symbols begin)."""

    _library, _prefix = None, "nb_"

    def __init__(self, dtype):
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError("float32 or float64")
        self._scalar = np.float32 if self.dtype == np.float32 else float
        self._suffix = "f32" if self.dtype == np.float32 else "f64"

    def _fn(self, name: str):
        return getattr(self._library(), f"{self._prefix}{name}_{self._suffix}")

    def _call(self, name: str, *args) -> None:
        check(self._fn(name)(*args), self._prefix + name)

    def _device(self, data, own: DeviceBuffer, shape, dtype=None):
        """the device address of `data`: its own when it is one, else a host array uploaded into `own`"""
        if isinstance(data, DeviceBuffer):
            return data.ptr
        if isinstance(data, (int, ctypes.c_void_p)):
            return data
        host = np.ascontiguousarray(data, dtype=dtype or self.dtype)
        if host.shape != shape:
            raise ValueError(f"expected an array of shape {shape}, got {host.shape}")
        own.upload(host)
        return own.ptr

    def _download(self, buf: DeviceBuffer) -> np.ndarray:
        return buf.download(np.empty(self.shape, dtype=self.dtype))

    def synchronize(self) -> None:
        check(lib().nb_device_synchronize(), "nb_device_synchronize")

    def free(self) -> None:
        for b in self._buffers():
            b.free()


class _HermiteState(_DeviceState):
    """... and what the four Hermite classes share on top: positions, velocities, accelerations and jerks of ``shape``, and softening^2."""

    def _softening_or_default(self, value):
        """None: 0.01, BodySystemHIP's default (T(0.1) * T(0.1))"""
        t = self.dtype.type
        return t(np.float32(0.1)) * t(np.float32(0.1)) if value is None else value

    def _set_system_softening(self, softening_sq) -> None:
        """`softening_sq` a scalar or one value per system: ``softening_sq`` (B values) and, for the latter, their device copy"""
        softening_sq = self._softening_or_default(softening_sq)
        if np.ndim(softening_sq) == 0:
            self.softening_sq = np.full(self.num_systems, softening_sq, self.dtype)
        else:
            self.softening_sq = np.ascontiguousarray(softening_sq, dtype=self.dtype)
            if self.softening_sq.shape != (self.num_systems,):
                self.free()
                raise ValueError(f"softening_sq: a scalar or {self.num_systems} values")
            self._system_eps2 = DeviceBuffer(self.softening_sq.nbytes)
            self._system_eps2.upload(self.softening_sq)

    def _softening(self):
        """(softening_sq, system_softening_sq) as the ensemble calls take them"""
        return self._scalar(self.softening_sq[0]), (self._system_eps2.ptr if self._system_eps2 is not None else None)

    def set_state(self, positions, velocities) -> None:
        for buf, data in ((self._pos, positions), (self._vel, velocities)):
            data = np.ascontiguousarray(data, dtype=self.dtype)
            if data.shape != self.shape:
                raise ValueError(f"expected an array of shape {self.shape}, got {data.shape}")
            buf.upload(data)

    def get_positions(self) -> np.ndarray:
        return self._download(self._pos)

    def get_velocities(self) -> np.ndarray:
        return self._download(self._vel)

    def get_accelerations(self) -> np.ndarray:
        return self._download(self._acc)

    def get_jerks(self) -> np.ndarray:
        return self._download(self._jerk)


def integrate_nbody_system(new_positions, old_positions, velocities, current_read: int, delta_time, damping,
                           num_bodies: int, block_size: int, dtype=np.float32, mode: int = NB_MODE_FAST, stream=None) -> None:
    """integrateNbodySystem<T>, src/nbody/integrate_nbody_cuda.hpp:5 (same argument order; `current_read` is
    unused there too).  Pointers are raw device addresses (int / c_void_p)."""
    del current_read
    if np.dtype(dtype) == np.float32:
        rc = lib().nb_integrate_f32(new_positions, old_positions, velocities, np.float32(delta_time), np.float32(damping),
                                    num_bodies, block_size, mode, stream)
    else:
        rc = lib().nb_integrate_f64(new_positions, old_positions, velocities, float(delta_time), float(damping),
                                    num_bodies, block_size, mode, stream)
    check(rc, "integrateNbodySystem")


class BodySystemHIP:
    """Mirror of BodySystemCUDADefault<T> (src/nbody/bodysystemcuda_default.hpp:28-36, .cu:8-55) on HIP.

    Two ping-pong position arrays + one velocity array of 4N T on the device; ``update`` writes
    pos[1-read] from pos[read] and swaps; ``set_*`` resets read=0/write=1; ``get_*`` are blocking D2H copies.
    ``reset`` needs initial conditions: pass ``randomise`` (a callable (config, n, cluster, velocity, dtype) ->
    (pos, vel)); the C++ host mirror owns the real randomise_bodies restatement.
    """

    def __init__(self, nb_bodies: int, block_size: int = 256, params: NBodyParams | None = None, dtype=np.float32,
                 positions: np.ndarray | None = None, velocities: np.ndarray | None = None, mode: int = NB_MODE_FAST,
                 workspace: bool = False, workspace_cap: int | None = None):
        """`workspace=True`: own the scratch memory nb_workspace_bytes_* asks for and step through nb_integrate_ws_* (FAST mode
        then takes the pairwise layout where it applies), as BodySystemHIPStored does in the C++ host."""
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError("float32 or float64")
        self.nb_bodies = int(nb_bodies)
        self.block_size = int(block_size)
        self.mode = mode
        params = params or NBodyParams()
        self.damping = self.dtype.type(np.float32(params.damping))  # float -> T, bodysystemcuda.cpp:56
        self.current_read, self.current_write = 0, 1
        nbytes = 4 * self.nb_bodies * self.dtype.itemsize
        self._pos = [DeviceBuffer(nbytes), DeviceBuffer(nbytes)]
        self._vel = DeviceBuffer(nbytes)
        self._host_pos = np.zeros(4 * self.nb_bodies, dtype=self.dtype)
        self._host_vel = np.zeros(4 * self.nb_bodies, dtype=self.dtype)
        self._workspace, self._workspace_bytes = None, 0
        if workspace:
            need = workspace_bytes(self.nb_bodies, self.dtype, self.mode, workspace_cap)  # (`workspace_cap`: spend at most that many bytes)
            if need:
                self._workspace, self._workspace_bytes = _vp(), need
                check(lib().nb_alloc(ctypes.byref(self._workspace), need), "nb_alloc(workspace)")
        self._set_softening(params.softening)
        if positions is not None:
            self.set_position(positions)
            self.set_velocity(velocities)

    def _set_softening(self, softening) -> None:
        # bodysystemcuda.cpp:42-46: softening2 = T(softening) * T(softening)
        s = self.dtype.type(np.float32(softening))
        self._softening_sq = s * s

    def _apply_softening(self) -> None:
        if self.dtype == np.float32:
            check(lib().nb_set_softening_sq_f32(self._softening_sq), "nb_set_softening_sq_f32")
        else:
            check(lib().nb_set_softening_sq_f64(float(self._softening_sq)), "nb_set_softening_sq_f64")

    def update_params(self, params: NBodyParams) -> None:
        self._set_softening(params.softening)
        self.damping = self.dtype.type(np.float32(params.damping))

    def reset(self, params: NBodyParams, config: int, randomise) -> None:
        pos, vel = randomise(config, self.nb_bodies, params.cluster_scale, params.velocity_scale, self.dtype)
        self.set_position(pos)
        self.set_velocity(vel)

    def update(self, delta_time, stream=None) -> None:
        self._apply_softening()
        if self._workspace is not None:
            f32 = self.dtype == np.float32
            fn, scalar = (lib().nb_integrate_ws_f32, np.float32) if f32 else (lib().nb_integrate_ws_f64, float)
            check(fn(self._pos[1 - self.current_read].ptr, self._pos[self.current_read].ptr, self._vel.ptr, scalar(delta_time), scalar(self.damping),
                     self.nb_bodies, self.block_size, self.mode, self._workspace, self._workspace_bytes, stream), "nb_integrate_ws")
        else:
            integrate_nbody_system(self._pos[1 - self.current_read].ptr, self._pos[self.current_read].ptr, self._vel.ptr,
                                   self.current_read, delta_time, self.damping, self.nb_bodies, self.block_size,
                                   self.dtype, self.mode, stream)
        self.current_read, self.current_write = self.current_write, self.current_read

    def update_many(self, delta_time, steps: int, stream=None) -> None:
        """`steps` (even) updates as ONE hipGraph launch (nb_graph_*): same kernels, same results as `steps` x update()."""
        # everything nb_graph_create_* bakes into the capture (damping and softening^2 are kernel arguments too)
        key = (float(delta_time), steps, self.current_read, self.mode, float(self.damping), float(self._softening_sq))
        if getattr(self, "_graph_key", None) != key:
            self._free_graph()
            self._apply_softening()
            g = _vp()
            a, b = self._pos[self.current_read].ptr, self._pos[1 - self.current_read].ptr
            if self.dtype == np.float32:
                rc = lib().nb_graph_create_ws_f32(ctypes.byref(g), a, b, self._vel.ptr, np.float32(delta_time), self.damping,
                                                  self.nb_bodies, self.block_size, self.mode, steps, self._workspace, self._workspace_bytes)
            else:
                rc = lib().nb_graph_create_ws_f64(ctypes.byref(g), a, b, self._vel.ptr, float(delta_time), float(self.damping),
                                                  self.nb_bodies, self.block_size, self.mode, steps, self._workspace, self._workspace_bytes)
            check(rc, "nb_graph_create")
            self._graph, self._graph_key = g, key
        check(lib().nb_graph_launch(self._graph, stream), "nb_graph_launch")  # even step count: read index unchanged

    def _free_graph(self) -> None:
        if getattr(self, "_graph", None):
            lib().nb_graph_destroy(self._graph)
        self._graph, self._graph_key = None, None

    def get_position(self) -> np.ndarray:
        return self._pos[self.current_read].download(self._host_pos)

    def get_velocity(self) -> np.ndarray:
        return self._vel.download(self._host_vel)

    def set_position(self, data: np.ndarray) -> None:
        data = np.ascontiguousarray(data, dtype=self.dtype)
        assert data.size == 4 * self.nb_bodies
        self.current_read, self.current_write = 0, 1
        self._pos[0].upload(data)

    def set_velocity(self, data: np.ndarray) -> None:
        data = np.ascontiguousarray(data, dtype=self.dtype)
        assert data.size == 4 * self.nb_bodies
        self.current_read, self.current_write = 0, 1
        self._vel.upload(data)

    def synchronize(self) -> None:
        check(lib().nb_device_synchronize(), "nb_device_synchronize")

    def free(self) -> None:
        self._free_graph()
        for b in self._pos + [self._vel]:
            b.free()
        if self._workspace is not None:
            lib().nb_free(self._workspace)
            self._workspace = None


def ensemble_plan(num_bodies: int, num_systems: int, dtype=np.float32) -> EnsemblePlan:
    """nb_ensemble_plan_*: the FAST geometry of `num_systems` systems of `num_bodies` bodies"""
    return _plan(ensemble_lib, "ensemble", EnsemblePlan, dtype, num_bodies, num_systems)


class BodyEnsembleHIP(_DeviceState):
    """B independent systems of N bodies on the device, stepped together by nb_ensemble_integrate_* (include/nbody_hip_ensemble.h).

    Two ping-pong position arrays + one velocity array of 4*N*B T; system s holds bodies [s*N, (s+1)*N).  Positions and velocities go
    in and out as (B, N, 4) arrays; ``update`` writes pos[1-read] from pos[read] and swaps; ``set_*`` resets read = 0."""

    _library, _prefix = staticmethod(ensemble_lib), "nb_ensemble_"

    def __init__(self, num_bodies: int, num_systems: int, dtype=np.float32, mode: int = NB_MODE_FAST):
        super().__init__(dtype)
        self.num_bodies, self.num_systems, self.mode = int(num_bodies), int(num_systems), mode
        ensemble_plan(self.num_bodies, self.num_systems, self.dtype)  # refuses the sizes the step refuses, before anything is allocated
        self.shape = (self.num_systems, self.num_bodies, 4)
        nbytes = 4 * self.num_bodies * self.num_systems * self.dtype.itemsize
        self._pos = [DeviceBuffer(nbytes), DeviceBuffer(nbytes)]
        self._vel = DeviceBuffer(nbytes)
        self._params = None
        self.current_read = 0

    def _upload(self, buf: DeviceBuffer, data) -> None:
        data = np.ascontiguousarray(data, dtype=self.dtype)
        if data.shape != self.shape:
            raise ValueError(f"expected an array of shape {self.shape}, got {data.shape}")
        buf.upload(data)

    def set_positions(self, data) -> None:
        self.current_read = 0
        self._upload(self._pos[0], data)

    def set_velocities(self, data) -> None:
        self.current_read = 0
        self._upload(self._vel, data)

    def get_positions(self) -> np.ndarray:
        return self._download(self._pos[self.current_read])

    def get_velocities(self) -> np.ndarray:
        return self._download(self._vel)

    def update(self, delta_time, damping=1.0, softening_sq=None, params=None, stream=None) -> None:
        """One step of every system.  `params`: None (every system uses delta_time, damping, softening_sq) or a (B, 4) array of
        {dt, damping, softening^2, ignored} per system (uploaded first; the scalars are then ignored).  softening_sq None: 0.01,
        BodySystemHIP's default (T(0.1) * T(0.1))."""
        t = self.dtype.type
        if softening_sq is None:
            softening_sq = t(np.float32(0.1)) * t(np.float32(0.1))
        table = None
        if params is not None:
            table = np.ascontiguousarray(params, dtype=self.dtype)
            if table.shape != (self.num_systems, 4):
                raise ValueError(f"params: expected shape {(self.num_systems, 4)}, got {table.shape}")
            if self._params is None:
                self._params = DeviceBuffer(table.nbytes)
            self._params.upload(table)
        self._call("integrate", self._pos[1 - self.current_read].ptr, self._pos[self.current_read].ptr, self._vel.ptr, self.num_bodies, self.num_systems,
                   self._scalar(delta_time), self._scalar(damping), self._scalar(softening_sq), self._params.ptr if table is not None else None, self.mode, stream)
        self.current_read = 1 - self.current_read

    def _buffers(self):
        return self._pos + [self._vel] + ([self._params] if self._params is not None else [])

    def free(self) -> None:
        super().free()
        self._params = None


def hermite_plan(num_bodies: int, dtype=np.float32) -> HermitePlan:
    """nb_hermite_plan_*: the geometry of the acceleration + jerk kernel for `num_bodies` bodies"""
    return _plan(hermite_lib, "hermite", HermitePlan, dtype, num_bodies)


def hermite_workspace_bytes(num_bodies: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(hermite_lib, "hermite", dtype, num_bodies)


class HermiteSystem(_HermiteState):
    """One system of N bodies on the device, stepped by the 4th-order Hermite scheme of include/nbody_hip_hermite.h.

    Positions (stepped in place: the call allows new == old), velocities, accelerations and jerks of 4*N T, the workspace and the
    time-step scalar are owned here.  ``set_state`` uploads (N, 4) positions {x, y, z, m} and velocities; ``eval`` fills the stored
    accelerations and jerks from the stored state (what starts a run); ``step(dt)`` takes one step; ``suggested_dt(eta)`` reads
    eta * min |a| / |jerk| of the stored derivatives back."""

    _library, _prefix = staticmethod(hermite_lib), "nb_hermite_"
    _query, _scratch_bytes = staticmethod(hermite_workspace_bytes), HERMITE_TIMESTEP_SCRATCH_BYTES
    _arrays = ("_pos", "_vel", "_acc", "_jerk")  # 4*N T each, allocated in this order

    def __init__(self, num_bodies: int, dtype=np.float32, softening_sq=None):
        super().__init__(dtype)
        self.num_bodies = int(num_bodies)
        self.softening_sq = self.dtype.type(self._softening_or_default(softening_sq))
        self._workspace_bytes = self._query(self.num_bodies, self.dtype)  # refuses the sizes the step refuses
        self.shape = (self.num_bodies, 4)
        for name in self._arrays:
            setattr(self, name, DeviceBuffer(4 * self.num_bodies * self.dtype.itemsize))
        self._workspace = DeviceBuffer(self._workspace_bytes)
        self._scratch = DeviceBuffer(self._scratch_bytes)
        self._dt = DeviceBuffer(8)

    def _buffers(self):
        return [self._pos, self._vel, self._acc, self._jerk, self._workspace, self._scratch, self._dt]

    def eval(self, stream=None) -> None:
        self._call("eval", self._acc.ptr, self._jerk.ptr, self._pos.ptr, self._vel.ptr, self.num_bodies, self._scalar(self.softening_sq), stream)

    def step(self, delta_time, stream=None) -> None:
        self._call("step", self._pos.ptr, self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._workspace.ptr, self._workspace_bytes, self.num_bodies,
                   self._scalar(delta_time), self._scalar(self.softening_sq), stream)

    def _derivatives(self):
        return self._acc.ptr, self._jerk.ptr

    def suggested_dt(self, eta, stream=None):
        self._call("timestep", *self._derivatives(), self.num_bodies, self._scalar(eta), self._dt.ptr, self._scratch.ptr, self._scratch_bytes, stream)
        out = np.empty(1, dtype=self.dtype)
        check(lib().nb_d2h(out.ctypes.data_as(_vp), self._dt.ptr, out.nbytes, stream), "nb_d2h")
        return out[0]


def hermite6_plan(num_bodies: int, dtype=np.float32) -> Hermite6Plan:
    """nb_hermite6_plan_*: the geometry of the acceleration + jerk + snap kernel for `num_bodies` bodies"""
    return _plan(hermite6_lib, "hermite6", Hermite6Plan, dtype, num_bodies)


def hermite6_workspace_bytes(num_bodies: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(hermite6_lib, "hermite6", dtype, num_bodies)


class Hermite6System(HermiteSystem):
    """One system of N bodies on the device, stepped by the 6th-order Hermite scheme of include/nbody_hip_hermite6.h.

    HermiteSystem's arrays and methods plus the snaps and crackles.  ``eval`` is nb_hermite6_init_*: it fills the stored accelerations,
    jerks and snaps from the stored state and zeroes the crackles (what starts a run); ``step(dt)`` takes one step;
    ``suggested_dt(eta)`` reads Aarseth's eta sqrt(min (|a||s| + |j|^2) / (|j||c| + |s|^2)) of the stored derivatives back."""

    _library, _prefix = staticmethod(hermite6_lib), "nb_hermite6_"
    _query, _scratch_bytes = staticmethod(hermite6_workspace_bytes), HERMITE6_TIMESTEP_SCRATCH_BYTES
    _arrays = HermiteSystem._arrays + ("_snap", "_crackle")

    def _buffers(self):
        return super()._buffers() + [self._snap, self._crackle]

    def eval(self, stream=None) -> None:
        self._call("init", self._acc.ptr, self._jerk.ptr, self._snap.ptr, self._crackle.ptr, self._pos.ptr, self._vel.ptr, self._workspace.ptr, self._workspace_bytes,
                   self.num_bodies, self._scalar(self.softening_sq), stream)

    def step(self, delta_time, stream=None) -> None:
        self._call("step", self._pos.ptr, self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._snap.ptr, self._crackle.ptr, self._workspace.ptr,
                   self._workspace_bytes, self.num_bodies, self._scalar(delta_time), self._scalar(self.softening_sq), stream)

    def _derivatives(self):
        return self._acc.ptr, self._jerk.ptr, self._snap.ptr, self._crackle.ptr

    def get_snaps(self) -> np.ndarray:
        return self._download(self._snap)

    def get_crackles(self) -> np.ndarray:
        return self._download(self._crackle)


def hermite_ensemble_plan(num_bodies: int, num_systems: int, dtype=np.float32) -> HermiteEnsemblePlan:
    """nb_hermite_ensemble_plan_*: the geometry of `num_systems` systems of `num_bodies` bodies"""
    return _plan(hermite_ensemble_lib, "hermite_ensemble", HermiteEnsemblePlan, dtype, num_bodies, num_systems)


def hermite_ensemble_workspace_bytes(num_bodies: int, num_systems: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(hermite_ensemble_lib, "hermite_ensemble", dtype, num_bodies, num_systems)


class HermiteEnsemble(_HermiteState):
    """B independent systems of N bodies on the device, stepped together by the 4th-order Hermite scheme of
    include/nbody_hip_hermite_ensemble.h.

    Positions (stepped in place: the calls allow new == old), velocities, accelerations and jerks of 4*N*B T, the workspace, the clocks and
    the status record are owned here; arrays go in and out as (B, N, 4).  ``set_state`` uploads positions {x, y, z, m} and velocities;
    ``eval`` fills the stored accelerations and jerks (what starts a fixed-dt run); ``step(dt)`` takes one step of every system, dt a
    scalar or one value per system; ``suggested_dt(eta)`` reads eta * min |a| / |jerk| of every system back.  The adaptive form:
    ``begin(eta)``, then ``advance(t_stop, eta, dt_max, calls)`` enqueues `calls` calls without reading anything back; ``clocks()`` and
    ``status()`` read the device records.  `softening_sq`: a scalar or one value per system."""

    _library, _prefix = staticmethod(hermite_ensemble_lib), "nb_hermite_ensemble_"
    _query = staticmethod(hermite_ensemble_workspace_bytes)

    def __init__(self, num_bodies: int, num_systems: int, dtype=np.float32, softening_sq=None):
        _DeviceState.__init__(self, dtype)
        self.num_bodies, self.num_systems = int(num_bodies), int(num_systems)
        self._workspace_bytes = self._query(self.num_bodies, self.num_systems, self.dtype)  # refuses the sizes the step refuses
        self.shape = (self.num_systems, self.num_bodies, 4)
        nbytes = 4 * self.num_bodies * self.num_systems * self.dtype.itemsize
        self._pos, self._vel, self._acc, self._jerk = (DeviceBuffer(nbytes) for _ in range(4))
        self._workspace = DeviceBuffer(self._workspace_bytes)
        self._clocks = DeviceBuffer(ctypes.sizeof(HermiteEnsembleClock) * self.num_systems)
        self._status = DeviceBuffer(ctypes.sizeof(HermiteEnsembleStatus))
        self._per_system = DeviceBuffer(self.num_systems * self.dtype.itemsize)  # dt_out
        self._params = DeviceBuffer(4 * self.num_systems * self.dtype.itemsize)
        self._system_eps2 = None
        self._set_system_softening(softening_sq)

    def _buffers(self):
        return [b for b in (self._pos, self._vel, self._acc, self._jerk, self._workspace, self._clocks, self._status, self._per_system, self._params, self._system_eps2)
                if b is not None]

    def _derivatives(self):
        return self._acc.ptr, self._jerk.ptr

    def _step_table(self, delta_time):
        """the {dt, softening^2, -, -} table of a step with a dt or a softening^2 per system, uploaded; None where the scalars do"""
        if np.ndim(delta_time) == 0 and self._system_eps2 is None:
            return None
        table = np.zeros((self.num_systems, 4), self.dtype)
        table[:, 0], table[:, 1] = delta_time, self.softening_sq
        self._params.upload(table)
        return table

    def eval(self, stream=None) -> None:
        self._call("eval", self._acc.ptr, self._jerk.ptr, self._pos.ptr, self._vel.ptr, self.num_bodies, self.num_systems, *self._softening(), stream)

    def step(self, delta_time, stream=None) -> None:
        """One step of every system: `delta_time` a scalar, or one dt per system (uploaded first, with the systems' softening^2)."""
        table = self._step_table(delta_time)
        self._call("step", self._pos.ptr, self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._workspace.ptr, self._workspace_bytes, self.num_bodies,
                   self.num_systems, self._scalar(0 if table is not None else delta_time), self._scalar(self.softening_sq[0]),
                   self._params.ptr if table is not None else None, stream)

    def suggested_dt(self, eta, stream=None) -> np.ndarray:
        self._call("timestep", *self._derivatives(), self.num_bodies, self.num_systems, self._scalar(eta), self._per_system.ptr, self._workspace.ptr,
                   self._workspace_bytes, stream)
        out = np.empty(self.num_systems, dtype=self.dtype)
        check(lib().nb_d2h(out.ctypes.data_as(_vp), self._per_system.ptr, out.nbytes, stream), "nb_d2h")
        return out

    def begin(self, eta, stream=None) -> None:
        self._call("begin", self._acc.ptr, self._jerk.ptr, self._pos.ptr, self._vel.ptr, self._clocks.ptr, self.num_bodies, self.num_systems, *self._softening(),
                   self._scalar(eta), self._workspace.ptr, self._workspace_bytes, stream)

    def advance(self, t_stop, eta, dt_max=float("inf"), calls: int = 1, stream=None) -> None:
        """`calls` calls of nb_hermite_ensemble_advance_*: every system that can still move takes `calls` steps towards t_stop; nothing is read back."""
        for _ in range(calls):
            self._call("advance", self._pos.ptr, self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._clocks.ptr, self._status.ptr, self._workspace.ptr,
                       self._workspace_bytes, self.num_bodies, self.num_systems, float(t_stop), float(dt_max), self._scalar(eta), *self._softening(), stream)

    def clocks(self) -> np.ndarray:
        """the systems' clocks as a structured array (HERMITE_ENSEMBLE_CLOCK_DTYPE)"""
        return self._clocks.download(np.empty(self.num_systems, dtype=HERMITE_ENSEMBLE_CLOCK_DTYPE))

    def status(self) -> HermiteEnsembleStatus:
        """the status record of the last advance"""
        raw = self._status.download(np.empty(ctypes.sizeof(HermiteEnsembleStatus), dtype=np.uint8))
        return HermiteEnsembleStatus.from_buffer_copy(raw.tobytes())


def hermite6_ensemble_plan(num_bodies: int, num_systems: int, dtype=np.float32) -> HermiteEnsemblePlan:
    """nb_hermite6_ensemble_plan_*: the geometry of `num_systems` systems of `num_bodies` bodies"""
    return _plan(hermite6_ensemble_lib, "hermite6_ensemble", HermiteEnsemblePlan, dtype, num_bodies, num_systems)


def hermite6_ensemble_workspace_bytes(num_bodies: int, num_systems: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(hermite6_ensemble_lib, "hermite6_ensemble", dtype, num_bodies, num_systems)


class Hermite6Ensemble(HermiteEnsemble):
    """B independent systems of N bodies on the device, stepped together by the 6th-order Hermite scheme of
    include/nbody_hip_hermite6_ensemble.h.

    HermiteEnsemble's arrays and methods plus the snaps and crackles.  ``eval`` is nb_hermite6_ensemble_init_*: it fills the stored
    accelerations, jerks and snaps and zeroes the crackles (what starts a fixed-dt run); ``suggested_dt(eta)`` reads Aarseth's
    eta sqrt(min (|a||s| + |j|^2) / (|j||c| + |s|^2)) of every system back; ``begin`` / ``advance`` are the adaptive form with that step."""

    _library, _prefix = staticmethod(hermite6_ensemble_lib), "nb_hermite6_ensemble_"
    _query = staticmethod(hermite6_ensemble_workspace_bytes)

    def __init__(self, num_bodies: int, num_systems: int, dtype=np.float32, softening_sq=None):
        super().__init__(num_bodies, num_systems, dtype, softening_sq)
        nbytes = 4 * self.num_bodies * self.num_systems * self.dtype.itemsize
        self._snap, self._crackle = DeviceBuffer(nbytes), DeviceBuffer(nbytes)

    def _buffers(self):
        return super()._buffers() + [b for b in (getattr(self, "_snap", None), getattr(self, "_crackle", None)) if b is not None]

    def _derivatives(self):
        return self._acc.ptr, self._jerk.ptr, self._snap.ptr, self._crackle.ptr

    def eval(self, stream=None) -> None:
        self._call("init", *self._derivatives(), self._pos.ptr, self._vel.ptr, self._workspace.ptr, self._workspace_bytes, self.num_bodies, self.num_systems,
                   *self._softening(), stream)

    def step(self, delta_time, stream=None) -> None:
        """One step of every system: `delta_time` a scalar, or one dt per system (uploaded first, with the systems' softening^2)."""
        table = self._step_table(delta_time)
        self._call("step", self._pos.ptr, self._pos.ptr, self._vel.ptr, *self._derivatives(), self._workspace.ptr, self._workspace_bytes, self.num_bodies,
                   self.num_systems, self._scalar(0 if table is not None else delta_time), self._scalar(self.softening_sq[0]),
                   self._params.ptr if table is not None else None, stream)

    def begin(self, eta, stream=None) -> None:
        self._call("begin", *self._derivatives(), self._pos.ptr, self._vel.ptr, self._clocks.ptr, self.num_bodies, self.num_systems, *self._softening(),
                   self._scalar(eta), self._workspace.ptr, self._workspace_bytes, stream)

    def advance(self, t_stop, eta, dt_max=float("inf"), calls: int = 1, stream=None) -> None:
        """`calls` calls of nb_hermite6_ensemble_advance_*: every system that can still move takes `calls` steps towards t_stop; nothing is read back."""
        for _ in range(calls):
            self._call("advance", self._pos.ptr, self._pos.ptr, self._vel.ptr, *self._derivatives(), self._clocks.ptr, self._status.ptr, self._workspace.ptr,
                       self._workspace_bytes, self.num_bodies, self.num_systems, float(t_stop), float(dt_max), self._scalar(eta), *self._softening(), stream)

    def get_snaps(self) -> np.ndarray:
        return self._download(self._snap)

    def get_crackles(self) -> np.ndarray:
        return self._download(self._crackle)


def hermite_block_plan(num_bodies: int, num_active: int, dtype=np.float32) -> HermiteBlockPlan:
    """nb_hermite_block_plan_*: the geometry of a block step of `num_active` of `num_bodies` bodies"""
    return _plan(hermite_block_lib, "hermite_block", HermiteBlockPlan, dtype, num_bodies, num_active)


def hermite_block_workspace_bytes(num_bodies: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(hermite_block_lib, "hermite_block", dtype, num_bodies)


class HermiteBlockSystem(_HermiteState):
    """One system of N bodies on the device, stepped by the Hermite scheme with block time steps of include/nbody_hip_hermite_block.h.

    The state (positions, velocities, accelerations, jerks, ticks, levels), the status record and the workspace are owned here.
    ``set_state`` uploads (N, 4) positions {x, y, z, m} and velocities; ``init`` evaluates and assigns the first levels; ``step(t_stop)``
    enqueues one block step; ``advance(t_stop, batch)`` enqueues batches of block steps and reads the status between them until a
    step would pass t_stop; ``snapshot()`` is the synchronised state at the status time; ``status()`` the status record."""

    _library, _prefix = staticmethod(hermite_block_lib), "nb_hermite_block_"
    _query = staticmethod(hermite_block_workspace_bytes)

    def __init__(self, num_bodies: int, dtype=np.float32, softening_sq=None, eta=0.02, eta_start=0.01, dt_max=0.125, max_level=30):
        super().__init__(dtype)
        self.num_bodies = int(num_bodies)
        self.softening_sq = self.dtype.type(self._softening_or_default(softening_sq))
        self.params = HermiteBlockParams(float(eta), float(eta_start), float(dt_max), int(max_level), 0)
        self.tick = float(dt_max) * 2.0 ** -int(max_level)
        self._workspace_bytes = self._query(self.num_bodies, self.dtype)  # refuses the sizes the step refuses
        self.shape = (self.num_bodies, 4)
        nbytes = 4 * self.num_bodies * self.dtype.itemsize
        self._pos, self._vel, self._acc, self._jerk, self._pos_out, self._vel_out = (DeviceBuffer(nbytes) for _ in range(6))
        self._ticks, self._levels = DeviceBuffer(8 * self.num_bodies), DeviceBuffer(4 * self.num_bodies)
        self._status = DeviceBuffer(ctypes.sizeof(HermiteBlockStatus))
        self._workspace = DeviceBuffer(self._workspace_bytes)

    def _buffers(self):
        return [self._pos, self._vel, self._acc, self._jerk, self._pos_out, self._vel_out, self._ticks, self._levels, self._status, self._workspace]

    def _state_args(self):
        return (self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._ticks.ptr, self._levels.ptr, self._status.ptr, self._workspace.ptr,
                self._workspace_bytes, self.num_bodies, self._scalar(self.softening_sq), ctypes.byref(self.params))

    def init(self, stream=None) -> None:
        self._call("init", *self._state_args(), stream)

    def step(self, t_stop=float("inf"), stream=None) -> None:
        self._call("step", *self._state_args(), float(t_stop), stream)

    def status(self, stream=None) -> HermiteBlockStatus:
        out = HermiteBlockStatus()
        check(lib().nb_d2h(ctypes.byref(out), self._status.ptr, ctypes.sizeof(out), stream), "nb_d2h(status)")
        return out

    def time(self) -> float:
        return self.status().now_ticks * self.tick

    def advance(self, t_stop, batch: int = 64, stream=None) -> HermiteBlockStatus:
        """block steps until the next one would pass t_stop: `batch` calls are enqueued, then the status is read"""
        while True:
            for _ in range(batch):
                self.step(t_stop, stream)
            status = self.status(stream)
            if status.flags & HERMITE_BLOCK_STOPPED:
                return status

    def snapshot(self, stream=None):
        """(positions, velocities) of every body predicted to the status time (nb_hermite_block_sync_*)"""
        self.sync(stream)
        check(lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
        return self._download(self._pos_out), self._download(self._vel_out)

    def sync(self, stream=None) -> None:
        """the synchronised snapshot, left on the device: snapshot_ptrs() for nb_energy_*"""
        self._call("sync", self._pos_out.ptr, self._vel_out.ptr, self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._ticks.ptr, self._status.ptr,
                   self.num_bodies, ctypes.byref(self.params), stream)

    def snapshot_ptrs(self):
        return self._pos_out.ptr, self._vel_out.ptr

    def get_ticks(self) -> np.ndarray:
        return self._ticks.download(np.empty(self.num_bodies, dtype=np.uint64))

    def get_levels(self) -> np.ndarray:
        return self._levels.download(np.empty(self.num_bodies, dtype=np.int32))


def hermite6_block_plan(num_bodies: int, num_active: int, dtype=np.float32) -> HermiteBlockPlan:
    """nb_hermite6_block_plan_*: the geometry of a 6th-order block step of `num_active` of `num_bodies` bodies"""
    return _plan(hermite6_block_lib, "hermite6_block", HermiteBlockPlan, dtype, num_bodies, num_active)


def hermite6_block_workspace_bytes(num_bodies: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(hermite6_block_lib, "hermite6_block", dtype, num_bodies)


class Hermite6BlockSystem(HermiteBlockSystem):
    """One system of N bodies on the device, stepped by the 6th-order Hermite scheme with block time steps of
    include/nbody_hip_hermite6_block.h.

    HermiteBlockSystem's arrays and methods plus the snaps and crackles.  eta sits inside the root of dt_A as there, and eta = 0.2 here
    does what eta = 0.02 does in the 4th-order scheme."""

    _library, _prefix = staticmethod(hermite6_block_lib), "nb_hermite6_block_"
    _query = staticmethod(hermite6_block_workspace_bytes)

    def __init__(self, num_bodies: int, dtype=np.float32, softening_sq=None, eta=0.2, eta_start=0.01, dt_max=0.125, max_level=30):
        super().__init__(num_bodies, dtype, softening_sq, eta, eta_start, dt_max, max_level)
        nbytes = 4 * self.num_bodies * self.dtype.itemsize
        self._snap, self._crackle = DeviceBuffer(nbytes), DeviceBuffer(nbytes)

    def _buffers(self):
        return super()._buffers() + [self._snap, self._crackle]

    def _state_args(self):
        return (self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._snap.ptr, self._crackle.ptr, self._ticks.ptr, self._levels.ptr, self._status.ptr,
                self._workspace.ptr, self._workspace_bytes, self.num_bodies, self._scalar(self.softening_sq), ctypes.byref(self.params))

    def sync(self, stream=None) -> None:
        """the synchronised snapshot, left on the device: snapshot_ptrs() for nb_energy_*"""
        self._call("sync", self._pos_out.ptr, self._vel_out.ptr, self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._snap.ptr, self._crackle.ptr,
                   self._ticks.ptr, self._status.ptr, self.num_bodies, ctypes.byref(self.params), stream)

    def get_snaps(self) -> np.ndarray:
        return self._download(self._snap)

    def get_crackles(self) -> np.ndarray:
        return self._download(self._crackle)


def hermite_block_ensemble_plan(num_bodies: int, num_systems: int, num_active: int, dtype=np.float32) -> HermiteBlockEnsemblePlan:
    """nb_hermite_block_ensemble_plan_*: the solo geometry of a block step of `num_active` of `num_bodies` bodies, and the grids of `num_systems` systems"""
    return _plan(hermite_block_ensemble_lib, "hermite_block_ensemble", HermiteBlockEnsemblePlan, dtype, num_bodies, num_systems, num_active)


def hermite_block_ensemble_workspace_bytes(num_bodies: int, num_systems: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(hermite_block_ensemble_lib, "hermite_block_ensemble", dtype, num_bodies, num_systems)


class HermiteBlockEnsemble(_HermiteState):
    """B independent systems of N bodies on the device, each stepped by the Hermite scheme with block time steps of
    include/nbody_hip_hermite_block.h, all of them in the launches of one call (include/nbody_hip_hermite_block_ensemble.h).

    The state (positions, velocities, accelerations, jerks, ticks, levels), one status record per system, the summary record and the
    workspace are owned here; arrays go in and out as (B, N, 4), ticks and levels as (B, N).  ``set_state`` uploads positions
    {x, y, z, m} and velocities; ``init`` evaluates and assigns the first levels; ``step(t_stop)`` enqueues one block step of every system
    that has not reached t_stop; ``advance(t_stop, batch)`` enqueues batches of calls and one summary, reads 64 bytes, and repeats until
    every system is stopped; ``summary()`` and ``statuses()`` read the device records; ``snapshot()`` is every system synchronised at its
    own status time.  `params`: a HermiteBlockParams (default: eta 0.02, eta_start 0.01, dt_max 0.125, 30 levels); `softening_sq`: a
    scalar or one value per system."""

    _library, _prefix = staticmethod(hermite_block_ensemble_lib), "nb_hermite_block_ensemble_"
    _query = staticmethod(hermite_block_ensemble_workspace_bytes)
    _default_params = (0.02, 0.01, 0.125, 30, 0)

    def __init__(self, num_bodies: int, num_systems: int, dtype=np.float32, params=None, softening_sq=None):
        super().__init__(dtype)
        self.num_bodies, self.num_systems = int(num_bodies), int(num_systems)
        self.params = HermiteBlockParams(*self._default_params) if params is None else params
        self.tick = float(self.params.dt_max) * 2.0 ** -int(self.params.max_level)
        self._workspace_bytes = self._query(self.num_bodies, self.num_systems, self.dtype)  # refuses the sizes the step refuses
        self.shape = (self.num_systems, self.num_bodies, 4)
        count = self.num_bodies * self.num_systems
        nbytes = 4 * count * self.dtype.itemsize
        self._system_eps2 = None
        self._pos, self._vel, self._acc, self._jerk, self._pos_out, self._vel_out = (DeviceBuffer(nbytes) for _ in range(6))
        self._ticks, self._levels = DeviceBuffer(8 * count), DeviceBuffer(4 * count)
        self._status = DeviceBuffer(ctypes.sizeof(HermiteBlockStatus) * self.num_systems)
        self._summary = DeviceBuffer(ctypes.sizeof(HermiteBlockEnsembleSummary))
        self._workspace = DeviceBuffer(self._workspace_bytes)
        self._set_system_softening(softening_sq)

    def _buffers(self):
        return [b for b in (self._pos, self._vel, self._acc, self._jerk, self._pos_out, self._vel_out, self._ticks, self._levels, self._status, self._summary,
                            self._workspace, self._system_eps2) if b is not None]

    def _state_args(self):
        return (self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._ticks.ptr, self._levels.ptr, self._status.ptr, self._workspace.ptr,
                self._workspace_bytes, self.num_bodies, self.num_systems, *self._softening(), ctypes.byref(self.params))

    def init(self, stream=None) -> None:
        self._call("init", *self._state_args(), stream)

    def step(self, t_stop=float("inf"), stream=None) -> None:
        self._call("step", *self._state_args(), float(t_stop), stream)

    def summary(self, stream=None) -> HermiteBlockEnsembleSummary:
        """the status records folded on the device (one launch), then 64 bytes read"""
        out = HermiteBlockEnsembleSummary()
        check(getattr(self._library(), self._prefix + "summary")(self._status.ptr, self.num_systems, self._summary.ptr, stream), self._prefix + "summary")
        check(lib().nb_d2h(ctypes.byref(out), self._summary.ptr, ctypes.sizeof(out), stream), "nb_d2h(summary)")
        return out

    def statuses(self, stream=None):
        """the B status records"""
        out = (HermiteBlockStatus * self.num_systems)()
        check(lib().nb_d2h(ctypes.byref(out), self._status.ptr, ctypes.sizeof(out), stream), "nb_d2h(status)")
        return list(out)

    def times(self) -> np.ndarray:
        return np.array([s.now_ticks * self.tick for s in self.statuses()])

    def advance(self, t_stop, batch: int = 64, stream=None) -> HermiteBlockEnsembleSummary:
        """block steps until every system's next one would pass t_stop: `batch` calls and a summary are enqueued, then 64 bytes are read"""
        while True:
            for _ in range(batch):
                self.step(t_stop, stream)
            summary = self.summary(stream)
            if summary.stopped == summary.systems:
                return summary

    def sync(self, stream=None) -> None:
        """the synchronised snapshots, left on the device: snapshot_ptrs() for nb_energy_* (system s at byte offset s * 4 N sizeof T)"""
        self._call("sync", self._pos_out.ptr, self._vel_out.ptr, self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._ticks.ptr, self._status.ptr,
                   self.num_bodies, self.num_systems, ctypes.byref(self.params), stream)

    def snapshot(self, stream=None):
        """(positions, velocities) of every body predicted to its system's status time (nb_hermite_block_ensemble_sync_*)"""
        self.sync(stream)
        check(lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
        return self._download(self._pos_out), self._download(self._vel_out)

    def snapshot_ptrs(self):
        return self._pos_out.ptr, self._vel_out.ptr

    def get_ticks(self) -> np.ndarray:
        return self._ticks.download(np.empty(self.shape[:2], dtype=np.uint64))

    def get_levels(self) -> np.ndarray:
        return self._levels.download(np.empty(self.shape[:2], dtype=np.int32))


def hermite6_block_ensemble_plan(num_bodies: int, num_systems: int, num_active: int, dtype=np.float32) -> HermiteBlockEnsemblePlan:
    """nb_hermite6_block_ensemble_plan_*: the solo geometry of a 6th-order block step of `num_active` of `num_bodies` bodies, and the grids of `num_systems` systems"""
    return _plan(hermite6_block_ensemble_lib, "hermite6_block_ensemble", HermiteBlockEnsemblePlan, dtype, num_bodies, num_systems, num_active)


def hermite6_block_ensemble_workspace_bytes(num_bodies: int, num_systems: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(hermite6_block_ensemble_lib, "hermite6_block_ensemble", dtype, num_bodies, num_systems)


class Hermite6BlockEnsemble(HermiteBlockEnsemble):
    """B independent systems of N bodies on the device, each stepped by the 6th-order Hermite scheme with block time steps of
    include/nbody_hip_hermite6_block.h, all of them in the launches of one call (include/nbody_hip_hermite6_block_ensemble.h).

    HermiteBlockEnsemble's arrays and methods plus the snaps and crackles.  `params` defaults to Hermite6BlockSystem's: eta 0.2 (inside
    the root of dt_A; it does what eta = 0.02 does in the 4th-order scheme), eta_start 0.01, dt_max 0.125, 30 levels."""

    _library, _prefix = staticmethod(hermite6_block_ensemble_lib), "nb_hermite6_block_ensemble_"
    _query = staticmethod(hermite6_block_ensemble_workspace_bytes)
    _default_params = (0.2, 0.01, 0.125, 30, 0)

    def __init__(self, num_bodies: int, num_systems: int, dtype=np.float32, params=None, softening_sq=None):
        self._snap = self._crackle = None
        super().__init__(num_bodies, num_systems, dtype, params, softening_sq)
        nbytes = 4 * self.num_bodies * self.num_systems * self.dtype.itemsize
        self._snap, self._crackle = DeviceBuffer(nbytes), DeviceBuffer(nbytes)

    def _buffers(self):
        return super()._buffers() + [b for b in (self._snap, self._crackle) if b is not None]

    def _state_args(self):
        return (self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._snap.ptr, self._crackle.ptr, self._ticks.ptr, self._levels.ptr, self._status.ptr,
                self._workspace.ptr, self._workspace_bytes, self.num_bodies, self.num_systems, *self._softening(), ctypes.byref(self.params))

    def sync(self, stream=None) -> None:
        """the synchronised snapshots, left on the device: snapshot_ptrs() for nb_energy_* (system s at byte offset s * 4 N sizeof T)"""
        self._call("sync", self._pos_out.ptr, self._vel_out.ptr, self._pos.ptr, self._vel.ptr, self._acc.ptr, self._jerk.ptr, self._snap.ptr, self._crackle.ptr,
                   self._ticks.ptr, self._status.ptr, self.num_bodies, self.num_systems, ctypes.byref(self.params), stream)

    def get_snaps(self) -> np.ndarray:
        return self._download(self._snap)

    def get_crackles(self) -> np.ndarray:
        return self._download(self._crackle)


def neighbour_plan(num_bodies: int, dtype=np.float32) -> NeighbourPlan:
    """nb_neighbour_plan_*: the geometry of a survey and of the lists of `num_bodies` bodies"""
    return _plan(neighbour_lib, "neighbour", NeighbourPlan, dtype, num_bodies)


def neighbour_workspace_bytes(num_bodies: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(neighbour_lib, "neighbour", dtype, num_bodies)


def neighbour_status_dict(status: NeighbourStatus) -> dict:
    return {name: getattr(status, name) for name, _ in NeighbourStatus._fields_ if name != "reserved"}


class NeighbourSurvey(_DeviceState):
    """Nearest neighbours, counts, potentials and neighbour lists of states of N bodies (include/nbody_hip_neighbour.h).

    The outputs, the status record, the workspace and a staging copy of the positions are device buffers owned here.  ``positions`` is
    a device address (a DeviceBuffer, its ``ptr`` or an int: T[4 N], only read) or a host array of shape (N, 4) {x, y, z, m};
    ``radii_sq`` likewise (T[N]).  ``survey`` and ``lists`` enqueue on `stream`, wait for it and return numpy arrays plus the status
    record as a dict; ``enqueue_survey`` / ``enqueue_lists`` only enqueue (outputs stay on the device: see the ``*_ptr`` attributes)."""

    _library, _prefix = staticmethod(neighbour_lib), "nb_neighbour_"

    def __init__(self, num_bodies: int, dtype=np.float32, softening_sq=0.0):
        super().__init__(dtype)
        self.num_bodies = n = int(num_bodies)
        self.softening_sq = self.dtype.type(softening_sq)
        self._workspace_bytes = neighbour_workspace_bytes(n, self.dtype)  # refuses the sizes the calls refuse
        size = self.dtype.itemsize
        self._pos, self._radii = DeviceBuffer(4 * n * size), DeviceBuffer(n * size)
        self._nearest, self._counts = DeviceBuffer(4 * n), DeviceBuffer(4 * n)
        self._nearest_d2, self._potentials = DeviceBuffer(n * size), DeviceBuffer(n * size)
        self._offsets = DeviceBuffer(8 * (n + 1))
        self._indices = None
        self._status = DeviceBuffer(ctypes.sizeof(NeighbourStatus))
        self._workspace = DeviceBuffer(self._workspace_bytes)

    def _buffers(self):
        return [b for b in (self._pos, self._radii, self._nearest, self._counts, self._nearest_d2, self._potentials, self._offsets, self._indices, self._status,
                            self._workspace) if b is not None]

    def _radius(self, radius_sq, radii_sq):
        if (radius_sq is None) == (radii_sq is None):
            raise ValueError("give radius_sq or radii_sq")
        if radii_sq is None:
            return self._scalar(radius_sq), None
        return self._scalar(0), self._device(radii_sq, self._radii, (self.num_bodies,))

    def enqueue_survey(self, positions, radius_sq=None, radii_sq=None, potentials=False, stream=None) -> None:
        radius, radii = self._radius(radius_sq, radii_sq)
        self._call("survey", self._device(positions, self._pos, (self.num_bodies, 4)), self.num_bodies, radius, radii, self._scalar(self.softening_sq), self._nearest.ptr,
                   self._nearest_d2.ptr, self._counts.ptr, self._potentials.ptr if potentials else None, self._status.ptr, self._workspace.ptr,
                   self._workspace_bytes, stream)

    def enqueue_lists(self, positions, radius_sq=None, radii_sq=None, capacity: int = 0, stream=None) -> None:
        radius, radii = self._radius(radius_sq, radii_sq)
        capacity = int(capacity)
        if capacity > 0 and (self._indices is None or self._indices.nbytes < 4 * capacity):
            if self._indices is not None:
                self._indices.free()
            self._indices = DeviceBuffer(4 * capacity)
        self._call("lists", self._device(positions, self._pos, (self.num_bodies, 4)), self.num_bodies, radius, radii, self._offsets.ptr,
                   self._indices.ptr if capacity > 0 else None, capacity, self._status.ptr, self._workspace.ptr, self._workspace_bytes, stream)

    def status(self, stream=None) -> dict:
        out = NeighbourStatus()
        check(lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
        check(lib().nb_d2h(ctypes.byref(out), self._status.ptr, ctypes.sizeof(out), stream), "nb_d2h(status)")
        return neighbour_status_dict(out)

    def survey(self, positions, radius_sq=None, radii_sq=None, potentials=False, stream=None) -> dict:
        self.enqueue_survey(positions, radius_sq, radii_sq, potentials, stream)
        n = self.num_bodies
        out = {"status": self.status(stream)}
        out["nearest_index"] = self._nearest.download(np.empty(n, dtype=np.uint32))
        out["nearest_dist_sq"] = self._nearest_d2.download(np.empty(n, dtype=self.dtype))
        out["counts"] = self._counts.download(np.empty(n, dtype=np.uint32))
        out["potentials"] = self._potentials.download(np.empty(n, dtype=self.dtype)) if potentials else None
        return out

    def lists(self, positions, radius_sq=None, radii_sq=None, capacity: int = 0, stream=None) -> dict:
        """offsets (N + 1), indices (the total's entries; None when they exceed `capacity`: status['total_neighbours'] says what is needed)"""
        self.enqueue_lists(positions, radius_sq, radii_sq, capacity, stream)
        out = {"status": self.status(stream)}
        out["offsets"] = self._offsets.download(np.empty(self.num_bodies + 1, dtype=np.uint64))
        total = out["status"]["total_neighbours"]
        if out["status"]["flags"] & NEIGHBOUR_OVERFLOW:
            out["indices"] = None
        else:
            out["indices"] = self._indices.download(np.empty(total, dtype=np.uint32)) if total > 0 else np.empty(0, dtype=np.uint32)
        return out

    @property
    def nearest_index_ptr(self):
        return self._nearest.ptr

    @property
    def nearest_dist_sq_ptr(self):
        return self._nearest_d2.ptr

    @property
    def counts_ptr(self):
        return self._counts.ptr

    @property
    def potentials_ptr(self):
        return self._potentials.ptr

    @property
    def status_ptr(self):
        return self._status.ptr


def knn_plan(num_bodies: int, k: int, dtype=np.float32) -> KnnPlan:
    """nb_knn_plan_*: the geometry of a survey of the `k` nearest neighbours of `num_bodies` bodies"""
    return _plan(knn_lib, "knn", KnnPlan, dtype, num_bodies, k)


def knn_workspace_bytes(num_bodies: int, k: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(knn_lib, "knn", dtype, num_bodies, k)


def knn_structure_dict(record: KnnStructure) -> dict:
    out = {name: getattr(record, name) for name, _ in KnnStructure._fields_ if name not in ("reserved", "centre")}
    out["centre"] = tuple(record.centre)
    return out


class KnnSurvey(_DeviceState):
    """The K nearest neighbours of every body, local densities and the structure record of states of N bodies (include/nbody_hip_knn.h).

    The outputs, the record, the workspace and a staging copy of the positions are device buffers owned here, sized for `max_k`.
    ``positions`` is a device address (a DeviceBuffer, its ``ptr`` or an int: T[4 N], only read) or a host array of shape (N, 4)
    {x, y, z, m}.  ``survey`` enqueues on `stream`, waits for it and returns numpy arrays plus the record as a dict; ``enqueue_survey``
    only enqueues (outputs stay on the device: see the ``*_ptr`` attributes)."""

    _library, _prefix = staticmethod(knn_lib), "nb_knn_"

    def __init__(self, num_bodies: int, dtype=np.float32, max_k: int = KNN_MAX_K):
        super().__init__(dtype)
        self.num_bodies = n = int(num_bodies)
        self.max_k = int(max_k)
        self._workspace_bytes = knn_workspace_bytes(n, self.max_k, self.dtype)  # refuses the sizes the calls refuse; the same for every K
        size = self.dtype.itemsize
        self._pos = DeviceBuffer(4 * n * size)
        self._index, self._dist_sq = DeviceBuffer(4 * n * self.max_k), DeviceBuffer(size * n * self.max_k)
        self._densities = DeviceBuffer(n * size)
        self._structure = DeviceBuffer(ctypes.sizeof(KnnStructure))
        self._workspace = DeviceBuffer(self._workspace_bytes)
        self._positions = None  # what the last survey looked at: a host copy, or the device address
        self._centre = None  # the density centre of the last survey with the record

    def _buffers(self):
        return [self._pos, self._index, self._dist_sq, self._densities, self._structure, self._workspace]

    def enqueue_survey(self, positions, k: int, densities=None, structure=None, stream=None) -> None:
        """`densities` and `structure` default to k >= 2 (the calls refuse them with k = 1)"""
        k = int(k)
        if not 1 <= k <= self.max_k:
            raise ValueError(f"k must be in 1 .. {self.max_k}")
        densities = k >= 2 if densities is None else bool(densities)
        structure = k >= 2 if structure is None else bool(structure)
        address = self._device(positions, self._pos, (self.num_bodies, 4))
        self._positions = address if isinstance(positions, (DeviceBuffer, int, ctypes.c_void_p)) else np.array(positions, dtype=self.dtype)
        self._call("survey", address, self.num_bodies, k, self._index.ptr, self._dist_sq.ptr, self._densities.ptr if densities else None,
                   self._structure.ptr if structure else None, self._workspace.ptr, self._workspace_bytes, stream)

    def structure(self, stream=None) -> dict:
        out = KnnStructure()
        check(lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
        check(lib().nb_d2h(ctypes.byref(out), self._structure.ptr, ctypes.sizeof(out), stream), "nb_d2h(structure)")
        return knn_structure_dict(out)

    def survey(self, positions, k: int, densities=None, structure=None, stream=None) -> dict:
        self.enqueue_survey(positions, k, densities, structure, stream)
        n, k = self.num_bodies, int(k)
        densities = k >= 2 if densities is None else bool(densities)
        structure = k >= 2 if structure is None else bool(structure)
        check(lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
        out = {"knn_index": self._index.download(np.empty((n, k), dtype=np.uint32)), "knn_dist_sq": self._dist_sq.download(np.empty((n, k), dtype=self.dtype))}
        out["densities"] = self._densities.download(np.empty(n, dtype=self.dtype)) if densities else None
        out["structure"] = self.structure(stream) if structure else None
        self._centre = out["structure"]["centre"] if structure else None
        return out

    def lagrangian_radii(self, fractions, centre=None) -> np.ndarray:
        """For each fraction f the distance from the density centre of the last ``survey`` (or from `centre`) at which the cumulative mass,
        bodies taken by distance, first reaches f M.  Host work: the positions are downloaded, distances are float64, one sort."""
        centre = self._centre if centre is None else centre
        if centre is None or self._positions is None:
            raise RuntimeError("lagrangian_radii needs a survey with the structure record (or a centre) first")
        if isinstance(self._positions, np.ndarray):
            pos = self._positions
        else:
            pos = np.empty((self.num_bodies, 4), dtype=self.dtype)
            address = self._positions if isinstance(self._positions, (int, ctypes.c_void_p)) else self._positions.value
            check(lib().nb_d2h(pos.ctypes.data_as(_vp), address, pos.nbytes, None), "nb_d2h(positions)")
        return lagrangian_radii(pos, centre, fractions)

    @property
    def knn_index_ptr(self):
        return self._index.ptr

    @property
    def knn_dist_sq_ptr(self):
        return self._dist_sq.ptr

    @property
    def densities_ptr(self):
        return self._densities.ptr

    @property
    def structure_ptr(self):
        return self._structure.ptr


def lagrangian_radii(positions, centre, fractions) -> np.ndarray:
    """positions (N, 4) {x, y, z, m}: for each fraction f the smallest distance from `centre` whose bodies (all within it, in float64) hold
    at least f times the total mass"""
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 4)
    r = np.sqrt(((pos[:, :3] - np.asarray(centre, dtype=np.float64)) ** 2).sum(axis=1))
    order = np.argsort(r, kind="stable")
    cumulative = np.cumsum(pos[order, 3])
    at = np.searchsorted(cumulative, np.asarray(fractions, dtype=np.float64) * cumulative[-1], side="left")
    return r[order][np.minimum(at, len(r) - 1)]


def field_plan(num_sources: int, num_targets: int, dtype=np.float32) -> FieldPlan:
    """nb_field_plan_*: the geometry of an evaluation of `num_sources` sources at `num_targets` points"""
    return _plan(field_lib, "field", FieldPlan, dtype, num_sources, num_targets)


def field_workspace_bytes(num_sources: int, num_targets: int, dtype=np.float32) -> int:
    return _query_workspace_bytes(field_lib, "field", dtype, num_sources, num_targets)


class FieldProbe(_DeviceState):
    """Acceleration, jerk and potential of N sources at up to `max_targets` points of the caller's own (include/nbody_hip_field.h).

    The outputs, the workspace (sized for every M up to `max_targets`) and staging copies of the inputs are device buffers owned here.
    ``sources`` / ``source_velocities`` are device addresses (a DeviceBuffer, its ``ptr`` or an int: T[4 N], only read) or host arrays of
    shape (N, 4); ``targets`` / ``target_velocities`` likewise with (M, 4), ``self_index`` with (M,) of uint32.  A device address for
    ``targets`` needs ``num_targets``.  ``eval`` enqueues on `stream`, waits for it and returns numpy arrays; ``enqueue`` only enqueues
    (outputs stay on the device: see the ``*_ptr`` attributes)."""

    _library, _prefix = staticmethod(field_lib), "nb_field_"

    def __init__(self, num_sources: int, max_targets: int, dtype=np.float32, softening_sq=0.0):
        super().__init__(dtype)
        self.num_sources, self.max_targets = n, m = int(num_sources), int(max_targets)
        self.softening_sq = self.dtype.type(softening_sq)
        size, per_tile = self.dtype.itemsize, 128 if self.dtype == np.float32 else 64
        # the workspace of the largest call: the partial planes exist while tiles * J is short of the geometry's target, so the tile
        # counts up to that target (and the largest M) cover every M; the query refuses the sizes the calls refuse
        tiles_max = -(-m // per_tile)
        sizes = {min(m, t * per_tile) for t in range(1, min(tiles_max, 1024) + 1)} | {m}
        self._workspace_bytes = max(field_workspace_bytes(n, count, self.dtype) for count in sizes)
        self._src, self._src_vel = DeviceBuffer(4 * n * size), DeviceBuffer(4 * n * size)
        self._tgt, self._tgt_vel, self._self = DeviceBuffer(4 * m * size), DeviceBuffer(4 * m * size), DeviceBuffer(4 * m)
        self._acc, self._jerk, self._pot = DeviceBuffer(4 * m * size), DeviceBuffer(4 * m * size), DeviceBuffer(m * size)
        self._workspace = DeviceBuffer(max(self._workspace_bytes, 256))

    def _buffers(self):
        return [self._src, self._src_vel, self._tgt, self._tgt_vel, self._self, self._acc, self._jerk, self._pot, self._workspace]

    def _device(self, data, own: DeviceBuffer, shape, dtype=None):
        """... and None (an input left out) stays None"""
        return None if data is None else super()._device(data, own, shape, dtype)

    def enqueue(self, sources, targets, source_velocities=None, target_velocities=None, self_index=None, num_targets=None, accelerations=True, jerks=False,
                potentials=True, stream=None) -> int:
        """-> M.  `num_targets` is needed when `targets` is a device address, else it is the host array's length."""
        if num_targets is None:
            if isinstance(targets, (DeviceBuffer, int, ctypes.c_void_p)):
                raise ValueError("targets given as a device address: say num_targets")
            num_targets = np.shape(targets)[0]
        m = int(num_targets)
        if not 1 <= m <= self.max_targets:
            raise ValueError(f"1 <= num_targets <= {self.max_targets}")
        if jerks and (source_velocities is None or target_velocities is None):
            raise ValueError("jerks need source_velocities and target_velocities")
        n = self.num_sources
        self._call("eval", self._device(sources, self._src, (n, 4)), self._device(source_velocities, self._src_vel, (n, 4)), n, self._device(targets, self._tgt, (m, 4)),
                   self._device(target_velocities, self._tgt_vel, (m, 4)), self._device(self_index, self._self, (m,), np.uint32), m, self._scalar(self.softening_sq),
                   self._acc.ptr if accelerations else None, self._jerk.ptr if jerks else None, self._pot.ptr if potentials else None, self._workspace.ptr,
                   self._workspace.nbytes, stream)
        return m

    def eval(self, sources, targets, source_velocities=None, target_velocities=None, self_index=None, jerks=False, potentials=True, stream=None, num_targets=None) -> dict:
        """accelerations (M, 4); jerks (M, 4) or None; potentials (M,) or None"""
        m = self.enqueue(sources, targets, source_velocities, target_velocities, self_index, num_targets, True, jerks, potentials, stream)
        check(lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
        out = {"accelerations": self._acc.download(np.empty((m, 4), dtype=self.dtype))}
        out["jerks"] = self._jerk.download(np.empty((m, 4), dtype=self.dtype)) if jerks else None
        out["potentials"] = self._pot.download(np.empty(m, dtype=self.dtype)) if potentials else None
        return out

    @property
    def accelerations_ptr(self):
        return self._acc.ptr

    @property
    def jerks_ptr(self):
        return self._jerk.ptr

    @property
    def potentials_ptr(self):
        return self._pot.ptr

    @property
    def workspace_ptr(self):
        return self._workspace.ptr


class Event:
    def __init__(self):
        self.h = _vp()
        check(lib().nb_event_create(ctypes.byref(self.h)), "nb_event_create")

    def record(self, stream=None) -> None:
        check(lib().nb_event_record(self.h, stream), "nb_event_record")

    def synchronize(self) -> None:
        check(lib().nb_event_synchronize(self.h), "nb_event_synchronize")

    def elapsed_ms(self, stop: "Event") -> float:
        ms = _cf(0)
        check(lib().nb_event_elapsed_ms(ctypes.byref(ms), self.h, stop.h), "nb_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            if self.h:
                lib().nb_event_destroy(self.h)
        except Exception:
            pass


class ShardedRank:
    """One rank of the body-sharded system THROUGH THE C-ABI: nb_comm_init_rank + nb_sharded_step_* (csrc/nbody_comm.hip),
    i.e. the product's own multi-GPU path -- RCCL send/recv rounds of position tiles on the communicator's side stream,
    the kernel of tile k waiting on tile k's event.  One process (or thread) per GPU; `unique_id` is rank 0's
    ``comm_unique_id()`` shipped to the other ranks by any means (bench.py: the torch.distributed store over gloo).

    The caller owns the arrays, exactly as with nb_integrate_*: `positions` = the two full-size ping-pong arrays (device
    addresses), `velocities`, `acc` (partial accelerations), all 4N T.  Python mirror of host/bodysystemhip_sharded.cpp's
    use of the same entry points (that class drives all local devices from one thread through the *_all form)."""

    def __init__(self, unique_id, world: int, rank: int, positions, velocities, acc, num_bodies: int, dtype=np.float32,
                 mode: int = NB_MODE_FAST, block_size: int = 256, stream=None, comm=None):
        """`comm`: an existing communicator to step ANOTHER system with (a communicator is not tied to a system size; the rank that
        created it keeps the ownership) -- otherwise nb_comm_init_rank makes one from `unique_id`."""
        self.dtype = np.dtype(dtype)
        self.world, self.rank, self.n = int(world), int(rank), int(num_bodies)
        if self.n % self.world:
            raise ValueError(f"{self.n} bodies do not shard evenly over {self.world} ranks; pad with zero-mass bodies")
        self.pos, self.vel, self.acc = [int(positions[0]), int(positions[1])], int(velocities), int(acc)
        self.mode, self.block_size, self.stream = mode, block_size, stream
        self.read = 0
        self.owns_comm = comm is None
        if comm is None:
            self.comm = _vp()
            check(lib().nb_comm_init_rank(ctypes.byref(self.comm), unique_id, self.world, self.rank), "nb_comm_init_rank")
        else:
            self.comm = comm
        f32 = self.dtype == np.float32
        self._step = lib().nb_sharded_step_f32 if f32 else lib().nb_sharded_step_f64
        self._tiles = lib().nb_exchange_tiles_f32 if f32 else lib().nb_exchange_tiles_f64
        self._scalar = np.float32 if f32 else float

    def workspace_bytes(self) -> int:
        """nb_comm_workspace_bytes_*: the scratch memory this rank can use in its mode (one rank: the single-GPU pairwise step;
        several: pairs once across the ranks, reaction sums sent to their owners); 0 = none."""
        need = _sz(0)
        fn = lib().nb_comm_workspace_bytes_f32 if self.dtype == np.float32 else lib().nb_comm_workspace_bytes_f64
        check(fn(self.comm, self.n, self.mode, ctypes.byref(need)), "nb_comm_workspace_bytes")
        return need.value

    def set_workspace(self, workspace, nbytes: int) -> None:
        """nb_comm_set_workspace: lend this rank the scratch memory of workspace_bytes().  With several ranks this is a COLLECTIVE
        over the communicator (every rank calls it; a rank without memory passes None, 0): the ranks learn the smallest amount
        lent anywhere, and the step is pairwise only if that suffices -- on every rank or on none."""
        check(lib().nb_comm_set_workspace(self.comm, workspace, nbytes), "nb_comm_set_workspace")

    def pairwise(self) -> bool:
        """nb_comm_layout_*: does nb_sharded_step_* of this communicator evaluate every pair once (the same answer on every rank)?"""
        flag = _ci(0)
        fn = lib().nb_comm_layout_f32 if self.dtype == np.float32 else lib().nb_comm_layout_f64
        check(fn(self.comm, self.n, self.mode, ctypes.byref(flag)), "nb_comm_layout")
        return bool(flag.value)

    def set_exchange_grouping(self, one_group: bool) -> None:
        """nb_comm_set_exchange_grouping: all G-1 position rounds of a step in one RCCL group (True) or a group and
        an event per round (False, the default since round 5); every rank must choose the same."""
        check(lib().nb_comm_set_exchange_grouping(self.comm, 1 if one_group else 0), "nb_comm_set_exchange_grouping")

    def exchange_grouping(self) -> bool:
        flag = _ci(0)
        check(lib().nb_comm_get_exchange_grouping(self.comm, ctypes.byref(flag)), "nb_comm_get_exchange_grouping")
        return bool(flag.value)

    def info(self) -> dict:
        """nb_comm_info + nb_comm_transport_info: what the communicator itself says about this rank and the RCCL it is bound to"""
        r, w, d = _ci(-1), _ci(-1), _ci(-1)
        check(lib().nb_comm_info(self.comm, ctypes.byref(r), ctypes.byref(w), ctypes.byref(d)), "nb_comm_info")
        out = {"rank": r.value, "world": w.value, "device": d.value}
        out.update(comm_transport_info(self.comm))
        hits = _ci(-1)
        check(lib().nb_comm_side_stream_collisions(self.comm, ctypes.byref(hits)), "nb_comm_side_stream_collisions")
        out["side_stream_collisions"] = hits.value  # (-1: never probed -- no pairwise step with two partners yet)
        bad = _ci(-1)
        check(lib().nb_comm_caller_stream_placement(self.comm, ctypes.byref(bad)), "nb_comm_caller_stream_placement")
        out["caller_stream_badly_placed"] = bad.value  # 1: stepping on the null stream or on its hardware queue (~40 % slower with RCCL active)
        return out

    def pair_work(self):
        """nb_comm_pair_work_* (tuning header): (pair evaluations, force launches) of this rank per pairwise step; None when the
        communicator steps one-sidedly"""
        evals, launches = ctypes.c_ulonglong(0), _ci(0)
        fn = lib().nb_comm_pair_work_f32 if self.dtype == np.float32 else lib().nb_comm_pair_work_f64
        rc = fn(self.comm, self.n, ctypes.byref(evals), ctypes.byref(launches))
        if rc == NB_ERR_UNSUPPORTED:
            return None
        check(rc, "nb_comm_pair_work")
        return evals.value, launches.value

    def make_step_stream(self):
        """nb_comm_stream_create: a well-placed non-blocking stream to step on, which becomes this rank's stream (the caller destroys
        it with nb_stream_destroy); returns it as a ctypes.c_void_p"""
        made = _vp()
        check(lib().nb_comm_stream_create(self.comm, ctypes.byref(made)), "nb_comm_stream_create")
        self.stream = made
        return made

    def update(self, delta_time, damping) -> None:
        """pos[1-read][own slice], vel[own slice] <- one step from pos[read]; then the tiles of pos[1-read] start moving."""
        check(self._step(self.comm, self.pos[1 - self.read], self.pos[self.read], self.vel, self.acc, self.n, self._scalar(delta_time),
                         self._scalar(damping), self.block_size, self.mode, self.stream), "nb_sharded_step")
        self.read = 1 - self.read

    def exchange_once(self, which: int | None = None) -> None:
        """One exchange of a position array outside any step (bring-up / diagnostics); the stream waits for all its tiles."""
        array = self.pos[self.read if which is None else which]
        check(self._tiles(self.comm, array, self.n, self.stream), "nb_exchange_tiles")
        self.finish()

    def finish(self) -> None:
        """Make the compute stream wait for every tile still in flight (asynchronous; synchronise the stream to block)."""
        check(lib().nb_exchange_wait_all(self.comm, self.stream), "nb_exchange_wait_all")

    def reaction_exchange_once(self) -> None:
        """nb_comm_reaction_exchange_* (tuning header): the reaction leg of a pairwise step alone; the stream waits for it."""
        fn = lib().nb_comm_reaction_exchange_f32 if self.dtype == np.float32 else lib().nb_comm_reaction_exchange_f64
        check(fn(self.comm, self.n, self.stream), "nb_comm_reaction_exchange")

    def destroy(self) -> None:
        if self.comm and self.owns_comm:
            lib().nb_comm_destroy(self.comm)
        self.comm = _vp()


def workspace_bytes(num_bodies: int, dtype=np.float32, mode: int = NB_MODE_FAST, max_bytes: int | None = None) -> int:
    """nb_workspace_bytes_* (max_bytes: nb_workspace_bytes_capped_*): scratch memory nb_integrate_ws_* wants for this system (0 = none)."""
    need = _sz(0)
    f32 = np.dtype(dtype) == np.float32
    if max_bytes is None:
        check((lib().nb_workspace_bytes_f32 if f32 else lib().nb_workspace_bytes_f64)(num_bodies, mode, ctypes.byref(need)), "nb_workspace_bytes")
    else:
        check((lib().nb_workspace_bytes_capped_f32 if f32 else lib().nb_workspace_bytes_capped_f64)(num_bodies, mode, max_bytes, ctypes.byref(need)), "nb_workspace_bytes_capped")
    return need.value


def energy_workspace_bytes(num_bodies: int) -> int:
    """nb_energy_workspace_bytes: scratch memory nb_energy_* needs for this many bodies (either precision)"""
    need = _sz(0)
    check(lib().nb_energy_workspace_bytes(num_bodies, ctypes.byref(need)), "nb_energy_workspace_bytes")
    return need.value


def energy(positions, velocities, num_bodies: int, dtype=np.float32, workspace=None, stream=None) -> dict:
    """nb_energy_* of the device arrays `positions` / `velocities` (raw device addresses) with the softening^2 set for `dtype`:
    {"kinetic", "potential", "total", "mass", "momentum", "angular_momentum", "center_of_mass"} (vectors as 3-tuples).
    `workspace`: a DeviceBuffer of at least energy_workspace_bytes(num_bodies) bytes; None = one is allocated for the call.
    Blocks until the result is back on the host."""
    own = workspace is None
    if own:
        workspace = DeviceBuffer(energy_workspace_bytes(num_bodies))
    result = DeviceBuffer(ctypes.sizeof(Energy))
    check(lib().nb_stream_synchronize(None), "nb_stream_synchronize")  # (DeviceBuffer clears on the null stream; `stream` may not wait for it)
    try:
        fn = lib().nb_energy_f32 if np.dtype(dtype) == np.float32 else lib().nb_energy_f64
        check(fn(positions, velocities, num_bodies, workspace.ptr, workspace.nbytes, result.ptr, stream), "nb_energy")
        out = Energy()
        check(lib().nb_d2h(ctypes.byref(out), result.ptr, ctypes.sizeof(Energy), stream), "nb_d2h(energy)")
    finally:
        result.free()
        if own:
            workspace.free()
    return energy_dict(out)


def energy_dict(out: Energy) -> dict:
    return {"kinetic": out.kinetic, "potential": out.potential, "total": out.total, "mass": out.mass, "momentum": tuple(out.momentum),
            "angular_momentum": tuple(out.angular_momentum), "center_of_mass": tuple(out.center_of_mass)}


def energy_ensemble_plan(num_bodies: int, num_systems: int, dtype=np.float32) -> EnergyEnsemblePlan:
    """nb_energy_ensemble_plan_*: the geometry of a measurement of `num_systems` systems of `num_bodies` bodies"""
    return _plan(energy_ensemble_lib, "energy_ensemble", EnergyEnsemblePlan, dtype, num_bodies, num_systems)


def energy_ensemble_workspace_bytes(num_bodies: int, num_systems: int) -> int:
    """nb_energy_ensemble_workspace_bytes: scratch memory nb_energy_ensemble_* needs (either precision)"""
    need = _sz(0)
    check(energy_ensemble_lib().nb_energy_ensemble_workspace_bytes(num_bodies, num_systems, ctypes.byref(need)), "nb_energy_ensemble_workspace_bytes")
    return need.value


def energy_ensemble(positions, velocities, num_bodies: int, num_systems: int, dtype=np.float32, softening_sq=0.0, system_softening_sq=None,
                    softening_stride: int = 1, workspace=None, results=None, stream=None) -> list:
    """nb_energy_ensemble_* of the device arrays `positions` / `velocities` (raw device addresses, 4 * num_bodies * num_systems elements):
    one dict per system with the keys of energy().  `softening_sq`: the scalar; `system_softening_sq`: a device address, system s reads
    element s * softening_stride of it.  `workspace`: a DeviceBuffer of at least energy_ensemble_workspace_bytes(...) bytes; `results`: a
    DeviceBuffer of 104 * num_systems bytes that keeps the records on the device (for energy_ensemble_drift); None = allocated for the
    call.  Blocks until the results are back on the host."""
    own_workspace, own_results = workspace is None, results is None
    if own_workspace:
        workspace = DeviceBuffer(energy_ensemble_workspace_bytes(num_bodies, num_systems))
    if own_results:
        results = DeviceBuffer(ctypes.sizeof(Energy) * num_systems)
    check(lib().nb_stream_synchronize(None), "nb_stream_synchronize")  # (DeviceBuffer clears on the null stream; `stream` may not wait for it)
    try:
        f32 = np.dtype(dtype) == np.float32
        fn = energy_ensemble_lib().nb_energy_ensemble_f32 if f32 else energy_ensemble_lib().nb_energy_ensemble_f64
        check(fn(positions, velocities, num_bodies, num_systems, np.float32(softening_sq) if f32 else float(softening_sq), system_softening_sq, softening_stride,
                 workspace.ptr, workspace.nbytes, results.ptr, stream), "nb_energy_ensemble")
        out = (Energy * num_systems)()
        check(lib().nb_d2h(ctypes.byref(out), results.ptr, ctypes.sizeof(out), stream), "nb_d2h(energy_ensemble)")
        check(lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
    finally:
        if own_results:
            results.free()
        if own_workspace:
            workspace.free()
    return [energy_dict(e) for e in out]


def energy_ensemble_drift(start, end, num_systems: int, stream=None) -> dict:
    """nb_energy_ensemble_drift of two device arrays of `num_systems` nb_energy_t (DeviceBuffers or raw addresses): the 64-byte record as a
    dict.  Blocks until it is back on the host."""
    summary = DeviceBuffer(ctypes.sizeof(EnergyDrift))
    check(lib().nb_stream_synchronize(None), "nb_stream_synchronize")
    try:
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        check(energy_ensemble_lib().nb_energy_ensemble_drift(ptr(start), ptr(end), num_systems, summary.ptr, stream), "nb_energy_ensemble_drift")
        out = EnergyDrift()
        check(lib().nb_d2h(ctypes.byref(out), summary.ptr, ctypes.sizeof(out), stream), "nb_d2h(energy_ensemble_drift)")
        check(lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
    finally:
        summary.free()
    return {name: getattr(out, name) for name, _ in EnergyDrift._fields_ if name != "reserved"}


def comm_transport_info(comm) -> dict:
    """nb_comm_transport_info (tuning header): {"rccl_version": 22204, "rccl_library": ".../librccl.so.1"}; 0 / "" when the
    communicator has no transport bound (a world of one)."""
    version, path = _ci(0), ctypes.create_string_buffer(512)
    check(lib().nb_comm_transport_info(comm, ctypes.byref(version), path, len(path)), "nb_comm_transport_info")
    return {"rccl_version": version.value, "rccl_library": path.value.decode()}


def comm_unique_id() -> bytes:
    """nb_comm_unique_id: the 128 bytes rank 0 hands to every other rank."""
    buf = ctypes.create_string_buffer(128)
    check(lib().nb_comm_unique_id(buf), "nb_comm_unique_id")
    return buf.raw
