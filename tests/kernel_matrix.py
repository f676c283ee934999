"""The kernel matrix: every __global__ function the fifteen registered listings of `make -C cuda-nbody_amd/csrc asm` hold (LISTINGS), and
what checks it.  The Makefile builds nineteen listings: the other four (field.s, knn.s, hermite_ensemble.s, hermite6_ensemble.s) have a
registry of their own, on the same terms, in the test module of their library: REGISTERED_ELSEWHERE names the listing, the module and the
registry function (as strings: those modules import this one), and the test module asserts that each exists and that the two tables are
all the Makefile builds.

A kernel is (listing, (function name, template arguments)): the block-step units share kernel text by include (hermite_block_schedule.inc,
hermite_block_ensemble_schedule.inc), so block_scan and its like are compiled into two listings under one symbol -- two code objects, two
libraries, each with a test of its own.  SHARED_TEXT names those kernels and their listings; the test module asserts that no listing holds
a symbol twice and that SHARED_TEXT is exactly what is compiled more than once.

Three lists, which together must equal the set of `.amdhsa_kernel` symbols (tests/test_kernel_matrix.py asserts it in both directions):

  CASES        the shape-dispatched families -- a kernel picked from a family of template instantiations by N or by a plan.  A case
               names the instantiation it claims (template arguments), the public entry point that reaches it, the override that
               forces it (where one is needed), the shape, and the plan fields that select it as the plan QUERY reports them.  The GPU
               part of tests/test_kernel_matrix.py runs every case and first asserts that the query, read on that device, selects the
               claimed instantiation.
  OTHER        every other kernel (schedule, scan, reduce, finish, predict, pack, sync, STRICT, pair_forces_clocked, pair_forces_jpacked),
               once per listing, with the existing test that checks it.
  UNREACHABLE  instantiations no public call can launch, each with the host-side reason, which is asserted.  None of them can be
               selected by a default plan (no override) for any N: that is asserted too.

A plain helper module: no fixture, no pytest setting.  Kernels are identified as (function name, template arguments), the arguments parsed
from the mangled symbol with a regex (as tests/test_ensemble.py does); `c++filt` is only asked when that regex does not match."""
import re
import subprocess
from dataclasses import dataclass

import numpy as np

F32, F64 = np.float32, np.float64
TYPE_NAME = {F32: "float", F64: "double"}
DTYPE_OF = {"float": F32, "double": F64}
LANE_WIDTH = {F32: 2, F64: 1}  # W: bodies i per vector (fp32 travels in packed pairs)

LISTINGS = ("nbody_fast.s", "nbody_strict.s", "nbody_pair.s", "nbody_energy.s", "ensemble_fast.s", "ensemble_strict.s", "hermite_eval.s", "hermite_block.s",
            "neighbour.s", "energy_ensemble.s", "hermite6_eval.s", "hermite6_block.s", "hermite_block_ensemble.s", "hermite6_block_ensemble.s", "nbody_pair_lead.s")
# listing -> (test module, the function that returns its registry); the module also has test_every_kernel_of_the_listing_is_in_the_registry
REGISTERED_ELSEWHERE = {
    "field.s": ("tests.test_field", "field_registry"),
    "knn.s": ("tests.test_knn", "knn_registry"),
    "hermite_ensemble.s": ("tests.test_hermite_ensemble", "ensemble_registry"),
    "hermite6_ensemble.s": ("tests.test_hermite6_ensemble", "ensemble6_registry"),
}
LISTING_TEST = "test_every_kernel_of_the_listing_is_in_the_registry"

# ---------------------------------------------------------------------------------------------------------------- symbols
_PREFIX = re.compile(r"^_ZN2nb12_GLOBAL__N_1(\d+)")
_TEMPLATE = re.compile(r"^I([fd]?)((?:L[ib]\d+E)*)E")  # (no T: pair_forces_jpacked<8>)
_ARGUMENT = re.compile(r"L([ib])(\d+)E")
_DEMANGLED = re.compile(r"nb::\(anonymous namespace\)::(\w+)(?:<([^>]*)>)?\(")


def parse_symbol(symbol):
    """(function name, template arguments) of a kernel symbol: ("integrate_bodies_fast", ("float", 2, 8, 4)), ("block_scan", ())"""
    m = _PREFIX.match(symbol)
    if m:
        start, length = m.end(), int(m.group(1))
        name, rest = symbol[start:start + length], symbol[start + length:]
        t = _TEMPLATE.match(rest)
        if t and (t.group(1) or t.group(2)):
            args = [TYPE_NAME[F32 if t.group(1) == "f" else F64]] if t.group(1) else []
            args += [bool(int(v)) if k == "b" else int(v) for k, v in _ARGUMENT.findall(t.group(2))]
            return name, tuple(args)
        if rest.startswith("E"):
            return name, ()
    # fallback: the demangler's text, read with a regex of the same meaning
    kernel = parse_demangled(subprocess.run(["c++filt", symbol], capture_output=True, text=True, check=True).stdout)
    if kernel is None:
        raise ValueError(f"cannot read the kernel symbol {symbol!r}")
    return kernel


def parse_demangled(text):
    """the same from a demangled name, "void nb::(anonymous namespace)::hermite_eval<float, 4, false>(nb::HermiteArgs<float>)"; None if it is not one"""
    d = _DEMANGLED.search(text)
    if d is None:
        return None
    args = []
    for a in (d.group(2) or "").split(","):
        a = a.strip()
        if a in ("float", "double"):
            args.append(a)
        elif a in ("true", "false"):
            args.append(a == "true")
        elif a:
            args.append(int(re.sub(r"^\(\w+\)", "", a)))
    return d.group(1), tuple(args)


def kernel_name(kernel):
    name, args = kernel
    if not args:
        return name
    return name + "<" + ", ".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in args) + ">"


def listed_kernels(text):
    """the kernels of one listing: every `.amdhsa_kernel` symbol, parsed"""
    return [parse_symbol(s) for s in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)]


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    family: str        # the kernel's function name
    dtype: type        # np.float32 / np.float64
    args: tuple        # the template arguments after T
    entry: str         # the public entry point that launches it
    override: tuple    # (setter of the package, arguments) or ()
    plan: tuple        # ((field of the plan query, value), ...): what selects the instantiation
    shape: tuple = ()  # ((name, value), ...): N, or how the ranges are sized
    note: str = ""

    @property
    def kernel(self):
        return self.family, (TYPE_NAME[self.dtype], *self.args)

    @property
    def listing(self):
        return FAMILY_LISTING[self.family]

    @property
    def id(self):
        shape = "".join(f" {k}={v}" for k, v in self.shape if k in ("n", "systems"))
        return kernel_name(self.kernel).replace(" ", "") + shape


# The wave-stream kernel: integrate_bodies_fast<T, R, S, LPT>.  R vectors of bodies i per lane (I = R W), S waves split j, chunks of
# 64 LPT bodies j per wave.  nb_set_plan_override(I, S, tile) with tile = 64 S LPT forces each one; plan_fast reports them back as
# bodies_per_lane, lanes_per_body, tile_bodies.  The ranges of a case are sized from (I, S, LPT) by test_kernel_matrix.stream_launches.
def _stream_cases():
    out = []
    for dtype in (F32, F64):
        w = LANE_WIDTH[dtype]
        for r in ((1, 2) if dtype == F32 else (1, 2, 4)):
            for s in (4, 8, 16):
                for lpt in (1, 2, 4):
                    if (s, lpt) == (16, 4):
                        continue  # UNREACHABLE, below
                    i, tile = r * w, 64 * s * lpt
                    out.append(Case("integrate_bodies_fast", dtype, (r, s, lpt), "nb_integrate_shard", ("set_plan_override", (i, s, tile)),
                                    (("bodies_per_lane", i), ("lanes_per_body", s), ("tile_bodies", tile), ("block_threads", 64 * s))))
    return out


# The wave-split kernel: integrate_bodies_wavesplit<T, R, LPT, BLOCK>.  A wave owns I = R W bodies i, a workgroup of BLOCK threads stages
# tiles of LPT BLOCK bodies j.  nb_set_plan_override(I, 64, tile) fixes I and the tile; the workgroup size is plan_fast's own choice from
# i_count and the device's CU count, so a case offers i_counts in units of the CU count and takes the first the query answers with its
# BLOCK ("cu_multiples": i_count = CUs x multiple + 29; 0: a small range, 301 bodies).
WAVESPLIT_FORMS = ((2, 256), (4, 256), (1, 512), (2, 512), (1, 1024))  # (LPT, BLOCK), the switch of dispatch_wavesplit


def _wavesplit_cases():
    out = []
    for dtype in (F32, F64):
        w = LANE_WIDTH[dtype]
        for r in (1, 2):
            for lpt, block in WAVESPLIT_FORMS:
                i, tile = r * w, lpt * block
                waves = block // 64
                multiples = (0,) if block == 256 else tuple(k * i for k in (waves, waves * 3 // 2, waves // 2 * 3 // 2, waves // 2, waves * 2, waves * 3))
                out.append(Case("integrate_bodies_wavesplit", dtype, (r, lpt, block), "nb_integrate_shard", ("set_plan_override", (i, 64, tile)),
                                (("bodies_per_lane", i), ("lanes_per_body", 64), ("tile_bodies", tile), ("block_threads", block)),
                                (("cu_multiples", multiples),)))
    return out


# The pairwise kernel: pair_forces<T, R, S>.  nb_set_pair_plan_override(R, S, splits, min_bodies = 1) forces each one at any size; the
# query reports bodies_per_lane = R W and waves_per_block = S.  Whole systems of a ragged N step through nb_integrate_ws_*.
PAIR_N = 3000  # fp32: 24 / 12 / 6 / 3 blocks (R = 1, 2, 4, 8); fp64: 47 / 24 / 12 / 6; the last block partly empty every time


def _pair_cases():
    out = []
    for dtype in (F32, F64):
        for r in (1, 2, 4, 8):
            for s in (4, 8, 12, 16):
                if (r, s) == (8, 16):
                    continue  # UNREACHABLE, below
                out.append(Case("pair_forces", dtype, (r, s), "nb_integrate_ws", ("set_pair_plan_override", (r, s, 2, 1)),
                                (("applies", 1), ("slices", 1), ("bodies_per_lane", r * LANE_WIDTH[dtype]), ("waves_per_block", s)), (("n", PAIR_N),)))
    return out


# The libraries dispatched by N alone: S, the waves that split j, is 1 below 256 bodies, 2 from 256, 4 from 512, 8 from 1 024
# (plan_ensemble_fast, plan_stream, block_waves, neighbour_waves; the 6th-order and block-ensemble units take plan_stream and block_waves).  The sizes sit on and around every switch point -- a wave gets exactly
# one chunk, then one chunk and one ragged body -- and inside the S = 4 window.
N_BY_WAVES = {1: (255,), 2: (256, 257, 511), 4: (512, 513, 700, 1023), 8: (1024, 1025)}
MASSES = ("equal", "species", "random")
ENSEMBLE_LARGE = ((8192 + 37, 3), (65536, 2))  # (bodies, systems), S = 8: the fp32 second-level sums fire from 8 192 bodies; the API's largest N
BLOCK_ENSEMBLE_SYSTEMS = 3  # one system per kind of MASSES, with 1, 129 and all bodies due


def ensemble_vectors(dtype, waves):
    """R of ensemble_fast<T, R, S>: I = min(S, 4) bodies i per lane, at least one vector"""
    return max(min(waves, 4), LANE_WIDTH[dtype]) // LANE_WIDTH[dtype]


def _n_dispatched_cases():
    out = []
    for dtype in (F32, F64):
        w = LANE_WIDTH[dtype]
        for s, sizes in N_BY_WAVES.items():
            r = ensemble_vectors(dtype, s)
            for n, systems in [(n, 3) for n in sizes] + (list(ENSEMBLE_LARGE) if s == 8 else []):
                out.append(Case("ensemble_fast", dtype, (r, s), "nb_ensemble_integrate", (), (("bodies_per_lane", r * w), ("waves_per_group", s)),
                                (("n", n), ("systems", systems))))
            for n in sizes:
                for step in (False, True):
                    out.append(Case("hermite_eval", dtype, (s, step), "nb_hermite_step" if step else "nb_hermite_eval", (), (("waves_per_group", s),), (("n", n),)))
                out.append(Case("hermite_block_eval", dtype, (s,), "nb_hermite_block_step", (), (("waves_per_group", s),), (("n", n),)))
                for pot in (False, True):
                    out.append(Case("neighbour_survey", dtype, (s, pot), "nb_neighbour_survey", (), (("waves_per_group", s),), (("n", n),),
                                    "POT = false: the survey of distances and counts (and the lists built on it); true: with potentials"))
                # the 6th-order scheme: the same driver text with nine sums, an interaction and a finish of its own
                for step in (False, True):
                    out.append(Case("hermite6_eval", dtype, (s, step), "nb_hermite6_step" if step else "nb_hermite6_eval", (), (("waves_per_group", s),), (("n", n),)))
                out.append(Case("hermite6_block_eval", dtype, (s,), "nb_hermite6_block_step", (), (("waves_per_group", s),), (("n", n),)))
                # the block steps of many systems: three systems of n bodies, bit for bit the solo steps (which the cases above hold to long double)
                for family, entry in (("hermite_block_ensemble_eval", "nb_hermite_block_ensemble_step"), ("hermite6_block_ensemble_eval", "nb_hermite6_block_ensemble_step")):
                    out.append(Case(family, dtype, (s,), entry, (), (("waves_per_group", s),), (("n", n), ("systems", BLOCK_ENSEMBLE_SYSTEMS))))
    return out


# The energies of an ensemble: energy_ensemble_pairs<T, R, S>.  R vectors of bodies i per lane (a block is 64 R W bodies) and S waves per
# workgroup follow N alone (plan_energy_ensemble); the query reports them as bodies_per_lane = R W and waves_per_group = S.  Each window
# of N that selects one instantiation is ((R, S), first n, last n).  fp32 (2, 1) and (4, 2) are compiled (the dispatch switch is one text
# for both precisions, and fp64 reaches those lines) but selected by no N: UNREACHABLE, below.  A case sits at the first and at the last
# n of its window (65 536 is the API's largest N).
ENERGY_ENSEMBLE_WINDOWS = {
    F32: (((1, 1), 1, 128), ((1, 2), 129, 255), ((2, 2), 256, 256), ((2, 4), 257, 511), ((4, 4), 512, 65536)),
    F64: (((1, 1), 1, 127), ((2, 1), 128, 128), ((2, 2), 129, 255), ((4, 2), 256, 256), ((4, 4), 257, 65536)),
}


def _energy_ensemble_cases():
    out = []
    for dtype in (F32, F64):
        for (r, s), first, last in ENERGY_ENSEMBLE_WINDOWS[dtype]:
            for n in sorted({first, last}):
                out.append(Case("energy_ensemble_pairs", dtype, (r, s), "nb_energy_ensemble", (),
                                (("bodies_per_lane", r * LANE_WIDTH[dtype]), ("waves_per_group", s)), (("n", n),)))
    return out


CASES = _stream_cases() + _wavesplit_cases() + _pair_cases() + _n_dispatched_cases() + _energy_ensemble_cases()
# family -> the one listing that holds its instantiations
FAMILY_LISTING = {"integrate_bodies_fast": "nbody_fast.s", "integrate_bodies_wavesplit": "nbody_fast.s", "pair_forces": "nbody_pair.s", "ensemble_fast": "ensemble_fast.s",
                  "hermite_eval": "hermite_eval.s", "hermite_block_eval": "hermite_block.s", "neighbour_survey": "neighbour.s", "energy_ensemble_pairs": "energy_ensemble.s",
                  "hermite6_eval": "hermite6_eval.s", "hermite6_block_eval": "hermite6_block.s", "hermite_block_ensemble_eval": "hermite_block_ensemble.s",
                  "hermite6_block_ensemble_eval": "hermite6_block_ensemble.s"}
FAMILIES = tuple(FAMILY_LISTING)
# the families whose S follows N alone (N_BY_WAVES), with the position of S among the template arguments after T
N_DISPATCHED = {"ensemble_fast": 1, "hermite_eval": 0, "hermite_block_eval": 0, "neighbour_survey": 0, "hermite6_eval": 0, "hermite6_block_eval": 0,
                "hermite_block_ensemble_eval": 0, "hermite6_block_ensemble_eval": 0}


def cases_of(family):
    return [c for c in CASES if c.family == family]


def claimed_kernels():
    return {(c.listing, c.kernel) for c in CASES}


# ---------------------------------------------------------------------------------------------------------------- every other kernel
def _both(name, test):
    return {(name, ("float",)): test, (name, ("double",)): test}


def _in(listing, kernels):
    return {(listing, kernel): test for kernel, test in kernels.items()}


_BLOCK4 = "tests.test_hermite_block::test_one_block_step_stage_by_stage_against_long_double"
_BLOCK6 = "tests.test_hermite6_block::test_one_block6_step_stage_by_stage_against_long_double"
# a block-ensemble kernel outside the evaluation is held to the solo call's bits, array by array and status by status, and the solo kernels to
# long double by the solo entries above it; the summary is recomputed from the statuses in the same test (check_against_solo)
_ENSEMBLE4, _ENSEMBLE6 = "tests.test_hermite_block_ensemble", "tests.test_hermite6_block_ensemble"
_STEP_BITS, _INIT_SYNC_BITS = "test_three_systems_take_the_solo_steps_bit_for_bit", "test_init_and_sync_are_the_solo_calls_per_system"


def _block_ensemble(module, predict_count, finish, sync):
    return {
        ("block_ensemble_summary", ()): f"{module}::{_STEP_BITS}",
        **_both("block_ensemble_init_levels", f"{module}::{_INIT_SYNC_BITS}"),
        **_both("block_ensemble_min_partial", f"{module}::{_STEP_BITS}"),
        **_both(predict_count, f"{module}::{_STEP_BITS}"),
        **_both("block_ensemble_scatter", f"{module}::{_STEP_BITS}"),
        **_both(finish, f"{module}::{_STEP_BITS}"),
        **_both(sync, f"{module}::{_INIT_SYNC_BITS}"),
    }


OTHER = {
    **_in("nbody_strict.s", _both("integrate_bodies_strict", "tests.test_gpu_parity::test_strict_matches_oracle_bitwise_ragged")),
    **_in("ensemble_strict.s", _both("ensemble_strict", "tests.test_ensemble::test_strict_every_system_matches_the_oracle")),
    **_in("nbody_energy.s", {
        **_both("energy_pairs", "tests.test_energy::test_energy_matches_fp64_numpy"),
        ("energy_finish", ()): "tests.test_energy::test_energy_matches_fp64_numpy",
    }),
    **_in("nbody_pair.s", {
        **_both("pair_finish", "tests.test_pairwise::test_pair_mass_forms"),
        **_both("pair_reduce", "tests.test_pairwise::test_sliced_pairwise_force_error"),
        ("pair_forces_clocked", ("float", 8, 8)): "tests.test_pairwise::test_clocked_variant_of_the_forces_kernel_changes_no_bit",
        ("pair_forces_clocked", ("double", 8, 8)): "tests.test_pairwise::test_clocked_variant_of_the_forces_kernel_changes_no_bit",
    }),
    # one S is compiled (launch_pair_lead): not a family.  What selects it is JPACKED_PLAN, asserted on the host at JPACKED_N
    **_in("nbody_pair_lead.s", {("pair_forces_jpacked", (8,)): "tests.test_pair_jpacked::test_jpacked_shapes"}),
    **_in("hermite_eval.s", {
        **_both("hermite_predict", "tests.test_hermite::test_one_step_against_long_double"),
        **_both("hermite_timestep_partial", "tests.test_hermite::test_shared_time_step"),
        **_both("hermite_timestep_final", "tests.test_hermite::test_shared_time_step"),
    }),
    **_in("hermite_block.s", {
        ("block_min_partial", ()): _BLOCK4,
        **_both("block_predict_count", _BLOCK4),
        ("block_scan", ()): _BLOCK4,
        ("block_scatter", ()): _BLOCK4,
        **_both("hermite_block_finish", _BLOCK4),
        **_both("block_init_levels", "tests.test_hermite_block::test_init_levels_against_long_double"),
        **_both("block_sync", "tests.test_hermite_block::test_python_class_gives_the_c_calls_bits"),
    }),
    **_in("neighbour.s", {
        ("neighbour_status", ()): "tests.test_neighbour::test_exact_lattices",
        **_both("neighbour_count", "tests.test_neighbour::test_exact_lattices"),
        ("list_block", ()): "tests.test_neighbour::test_exact_lattices",
        ("list_scan", ()): "tests.test_neighbour::test_exact_lattices",
        ("list_offsets", ()): "tests.test_neighbour::test_exact_lattices",
        **_both("neighbour_fill", "tests.test_neighbour::test_exact_lattices"),
    }),
    **_in("energy_ensemble.s", {
        ("energy_ensemble_finish", ()): "tests.test_energy_ensemble::test_every_system_matches_fp64_numpy",
        ("energy_ensemble_drift_summary", ()): "tests.test_energy_ensemble::test_drift_summary_agrees_with_numpy",
    }),
    **_in("hermite6_eval.s", {
        **_both("hermite6_pack", "tests.test_hermite6::test_eval_against_long_double_sums"),
        **_both("hermite6_predict", "tests.test_hermite6::test_one_step_against_long_double"),
        **_both("hermite6_timestep_partial", "tests.test_hermite6::test_time_step"),
        **_both("hermite6_timestep_final", "tests.test_hermite6::test_time_step"),
    }),
    **_in("hermite6_block.s", {
        ("block_min_partial", ()): _BLOCK6,
        **_both("block6_predict_count", _BLOCK6),
        ("block_scan", ()): _BLOCK6,
        ("block_scatter", ()): _BLOCK6,
        **_both("hermite6_block_finish", _BLOCK6),
        **_both("block6_init_levels", "tests.test_hermite6_block::test_block6_init_is_hermite6_init_and_levels_against_long_double"),
        **_both("block6_sync", "tests.test_hermite6_block::test_block6_python_class_gives_the_c_calls_bits"),
    }),
    **_in("hermite_block_ensemble.s", _block_ensemble(_ENSEMBLE4, "block_ensemble_predict_count", "hermite_block_ensemble_finish", "block_ensemble_sync")),
    **_in("hermite6_block_ensemble.s", _block_ensemble(_ENSEMBLE6, "block6_ensemble_predict_count", "hermite6_block_ensemble_finish", "block6_ensemble_sync")),
}

# pair_forces_jpacked: the geometry nb_set_pair_plan_override(8, 8, 1, 1) forces, as the plan query reports it -- what one_step of
# tests/test_pair_jpacked.py asserts before every launch -- at the size of test_jpacked_shapes whose last tile's second half holds one body
JPACKED_OVERRIDE = ("set_pair_plan_override", (8, 8, 1, 1))
JPACKED_PLAN = (("applies", 1), ("slices", 1), ("bodies_per_lane", 16), ("waves_per_block", 8), ("splits", 1))
JPACKED_N = 3072 + 65

# the kernels compiled into more than one listing, under one symbol: whole kernels shared as text by the block-step units
SHARED_TEXT = {
    **{(name, ()): ("hermite_block.s", "hermite6_block.s") for name in ("block_min_partial", "block_scan", "block_scatter")},  # hermite_block_schedule.inc
    **{kernel: ("hermite_block_ensemble.s", "hermite6_block_ensemble.s")  # hermite_block_ensemble_schedule.inc
       for kernel in (("block_ensemble_summary", ()), *_both("block_ensemble_init_levels", ""), *_both("block_ensemble_min_partial", ""), *_both("block_ensemble_scatter", ""))},
}


# ---------------------------------------------------------------------------------------------------------------- unreachable
GFX950_LDS_BYTES = 160 * 1024  # the LDS of one CU, the most a workgroup can be given (kPairLdsLimit, nbody_kernels.h)


@dataclass(frozen=True)
class Unreachable:
    kernel: tuple
    kind: str      # which host-side reason test_kernel_matrix.test_unreachable_reasons_hold asserts
    reason: str
    override: tuple  # what a caller would have to set to ask for it


PAIR_SIZES = (129, 517, 3000, 4160, 8193, 20000, 65536, 262144, 1048576)

# pair_forces<T, 8, 16>: sixteen waves each folding 3 x 8 vectors of 64 W-wide lanes need 16 * 3 * 8 * W * 64 * sizeof(T) + 256 = 196 864
# bytes of LDS in either precision, whatever N and however the units are dealt (pair_lds_bytes with no tail sums) -- more than a CU has, so
# the runtime refuses the launch and the step reports the error.  The default plan never asks for it: S is 8 unless the override sets it.
#
# integrate_bodies_fast<T, R, 16, 4>: sixteen waves with chunks of 256 bodies j are tile_bodies = 4 096.  plan_fast itself gives sixteen
# waves 128 bodies each (2 048), and nb_set_plan_override takes no tile above 2 048 (NB_ERR_INVALID_ARGUMENT, the previous override stays).
UNREACHABLE = [
    Unreachable(("pair_forces", (TYPE_NAME[dtype], 8, 16)), "pair_lds",
                "needs 196 864 bytes of LDS per workgroup for every N: more than the 160 KiB of a gfx950 CU; default plans keep S = 8",
                ("set_pair_plan_override", (8, 16, 1, 1)))
    for dtype in (F32, F64)
] + [
    Unreachable(("integrate_bodies_fast", (TYPE_NAME[dtype], r, 16, 4)), "tile_refused",
                "tile_bodies = 4 096: nb_set_plan_override refuses it, and plan_fast gives 16 waves tiles of 2 048 bodies",
                ("set_plan_override", (r * LANE_WIDTH[dtype], 16, 4096)))
    for dtype in (F32, F64) for r in ((1, 2) if dtype == F32 else (1, 2, 4))
] + [
    # energy_ensemble_pairs<float, 2, 1> and <float, 4, 2>: the (R, S) fp64 takes at 128 and at 256 bodies, where a system is one block of
    # I = R units.  In fp32 a lane holds packed pairs, so one block of R vectors is 2 R units, and S -- the most waves that leave each two
    # units -- is already 2 (R = 2) or 4 (R = 4) there.  There is no override: the plan is a function of N alone.
    Unreachable(("energy_ensemble_pairs", ("float", r, s)), "energy_plan",
                f"no n in [1, 65 536] makes nb_energy_ensemble_plan_f32 answer bodies_per_lane = {2 * r} with waves_per_group = {s}", ())
    for r, s in ((2, 1), (4, 2))
]


def registry():
    """(listing, kernel) -> what the registry says about it; raises if a kernel of a listing is named twice"""
    out = {}
    for key in sorted(claimed_kernels()):
        out[key] = "cases"
    for key in OTHER:
        assert key not in out, (key[0], kernel_name(key[1]))
        out[key] = "other"
    for u in UNREACHABLE:
        key = (FAMILY_LISTING[u.kernel[0]], u.kernel)
        assert key not in out, kernel_name(u.kernel)
        out[key] = "unreachable"
    return out
