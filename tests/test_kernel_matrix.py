"""Every compiled kernel instantiation against a long double sum (the registry: tests/kernel_matrix.py).

CPU part: the fifteen registered listings of `make asm` (the step, pairwise, Hermite, block-step, block-ensemble and neighbour kernels of
both orders, and energy_ensemble.s) hold exactly the kernels the registry names, listing by listing -- a new `case` in a dispatch switch,
or a case taken out of the registry, fails here with the kernel's name -- and every case's shape makes the plan query select the
instantiation it claims (the one-sided and pairwise queries with the CU count a machine without a device reports; the GPU part reads them
again on the device).  The Makefile's other four listings (field.s, knn.s, hermite_ensemble.s, hermite6_ensemble.s) are registered in the
test modules of their libraries: kernel_matrix.REGISTERED_ELSEWHERE names module and registry function, resolved and asserted here.

GPU part: one parametrised test per shape-dispatched family, one parameter per case: set the override, assert that the plan query selects
the claimed instantiation, run it through the public entry point, restore the override, and compare with long double sums -- the
project's own references and bounds, imported from the modules that define them (test_gpu_parity.direct_sum_f64, test_fast_domain's TOL,
UNIT_ROUNDOFF and check_step, the checkers of test_hermite, test_hermite_block, test_hermite6, test_hermite6_block and test_neighbour;
for energy_ensemble_pairs the probe pairs and probe bodies of test_energy_domain, which count every pair and every body once, bit for
bit; for the two block ensembles the solo block steps' bits, the solo kernels being held to long double at the same sizes by the cases
of hermite_block_eval and hermite6_block_eval).

How a one-sided case sizes its ranges (nb_integrate_shard_*, i and j independent) is in stream_launches / wavesplit_launches below: each
instantiation meets a ragged i range that does not start at 0, a j range that starts off a multiple of 4, a ragged last chunk with an odd
number of groups, fewer chunks than waves, in fp32 enough chunks per wave for the second-level sums, chunks of all three mass forms and a
first body j of mass zero."""
import ctypes
import hashlib
import importlib
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import kernel_matrix as km
import test_hermite6 as hermite6
import test_hermite6_block as block6
import test_hermite6_block_ensemble as block6_ensemble
import test_hermite_block_ensemble as block_ensemble
from conftest import ROOT
from test_ensemble import T as as_T
from test_ensemble import eps2_of, step as ensemble_step, systems as ensemble_systems
from test_energy_domain import ensemble_probe_bodies, ensemble_probe_pairs
from test_fast_domain import TOL, UNIT_ROUNDOFF, check_step
from test_gpu_parity import direct_sum_f64, gpu_accel, run_gpu
from test_hermite import check_eval, check_one_step, cloud, evaluate
from test_hermite_block import check_block_stages
from test_neighbour import check_cloud

gpu_only = pytest.mark.gpu
CSRC = os.path.join(ROOT, "cuda-nbody_amd", "csrc")
LD = np.longdouble
F32, F64 = km.F32, km.F64
EPS2 = 0.01
PAIR_TERMS = 2 * 10 ** 7  # the most long double pair terms one case's reference may take


def ids(cases):
    return [c.id for c in cases]


# ---------------------------------------------------------------------------------------------------------------- the listings
_LISTED = {}


def listed():
    """{listing: [kernels]} of `make asm`, built once per session"""
    if not _LISTED:
        subprocess.run(["make", "-s", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "asm"], check=True, capture_output=True)
        for name in km.LISTINGS:
            with open(os.path.join(CSRC, name)) as f:
                _LISTED[name] = km.listed_kernels(f.read())
    return _LISTED


def test_symbol_parser_reads_template_arguments():
    assert km.parse_symbol("_ZN2nb12_GLOBAL__N_121integrate_bodies_fastIdLi4ELi16ELi2EEEvNS_5ShardIT_EE") == ("integrate_bodies_fast", ("double", 4, 16, 2))
    assert km.parse_symbol("_ZN2nb12_GLOBAL__N_116neighbour_surveyIfLi8ELb1EEEvPKT_S4_S2_S2_jPjPS2_S5_S6_PNS_13NeighbourTileE") == ("neighbour_survey", ("float", 8, True))
    assert km.parse_symbol("_ZN2nb12_GLOBAL__N_110block_scanEPjjPNS_9BlockCtrlEPNS_11BlockStatusE") == ("block_scan", ())
    assert km.parse_symbol("_ZN2nb12_GLOBAL__N_113energy_finishEPKdjP9nb_energy") == ("energy_finish", ())
    assert km.kernel_name(("hermite_eval", ("float", 4, False))) == "hermite_eval<float, 4, false>"
    assert km.parse_symbol("_ZN2nb12_GLOBAL__N_119pair_forces_jpackedILi8EEEvNS_8PairArgsIfEE") == ("pair_forces_jpacked", (8,))
    assert km.parse_demangled("void nb::(anonymous namespace)::pair_forces_jpacked<8>(nb::PairArgs<float>)") == ("pair_forces_jpacked", (8,))
    assert km.parse_symbol("_ZN2nb12_GLOBAL__N_113hermite6_evalIdLi8ELb1EEEvNS_12Hermite6ArgsIT_EE") == ("hermite6_eval", ("double", 8, True))


def named(keys):
    return sorted(f"{listing}: {km.kernel_name(kernel)}" for listing, kernel in keys)


def test_the_listings_and_the_registry_name_the_same_kernels():
    """both directions, by listing and name: a compiled kernel the registry does not know; a kernel the registry names that is not compiled"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        built = next(line for line in f if line.startswith("ASM :=")).split()[2:]
    assert not hasattr(km, "UNREGISTERED"), "every listing is registered, here or in its library's module"
    assert len(km.LISTINGS) == 15 and len(km.REGISTERED_ELSEWHERE) == 4 and not set(km.LISTINGS) & set(km.REGISTERED_ELSEWHERE)
    assert sorted(km.LISTINGS + tuple(km.REGISTERED_ELSEWHERE)) == sorted(built), "a listing in neither table, or a table naming a listing the Makefile does not build"
    compiled = [(listing, k) for listing, kernels in listed().items() for k in kernels]
    twice = {key: count for key, count in Counter(compiled).items() if count > 1}
    assert not twice, f"a listing holds a symbol twice: {named(twice)}"
    # the same symbol in two listings: whole kernels shared as text, each copy registered with a test of its own library -- exactly SHARED_TEXT
    where = {}
    for listing, kernel in compiled:
        where.setdefault(kernel, []).append(listing)
    shared = {kernel: tuple(sorted(listings)) for kernel, listings in where.items() if len(listings) > 1}
    assert shared == {kernel: tuple(sorted(listings)) for kernel, listings in km.SHARED_TEXT.items()}, \
        f"compiled into more than one listing, against kernel_matrix.SHARED_TEXT: {sorted(km.kernel_name(k) for k in set(shared) ^ set(km.SHARED_TEXT))}"
    assert not any(kernel[0] in km.FAMILIES for kernel in shared), "an instantiation of a shape-dispatched family belongs to one listing"
    registry = km.registry()
    unknown = named(set(compiled) - set(registry))
    assert not unknown, f"compiled, but in no list of tests/kernel_matrix.py (CASES, OTHER, UNREACHABLE): {unknown}"
    missing = named(set(registry) - set(compiled))
    assert not missing, f"named by tests/kernel_matrix.py, but not in that listing: {missing}"
    # every instantiation of a shape-dispatched family is claimed by a case, unless UNREACHABLE says why not
    unreachable = {u.kernel for u in km.UNREACHABLE}
    for listing, kernel in compiled:
        if kernel[0] in km.FAMILIES and kernel not in unreachable:
            assert listing == km.FAMILY_LISTING[kernel[0]], (listing, km.kernel_name(kernel))
            assert registry[listing, kernel] == "cases", f"{km.kernel_name(kernel)}: an instantiation of a shape-dispatched family without a case"
        if kernel[0] not in km.FAMILIES:
            assert registry[listing, kernel] == "other", (listing, km.kernel_name(kernel))
    sizes = {family: sum(1 for _, k in compiled if k[0] == family) for family in km.FAMILIES}
    assert sizes == {"integrate_bodies_fast": 45, "integrate_bodies_wavesplit": 20, "pair_forces": 32, "ensemble_fast": 8, "hermite_eval": 16,
                     "hermite_block_eval": 8, "neighbour_survey": 16, "energy_ensemble_pairs": 12, "hermite6_eval": 16, "hermite6_block_eval": 8,
                     "hermite_block_ensemble_eval": 8, "hermite6_block_ensemble_eval": 8}, sizes
    # pair_forces_jpacked: one S, so a kernel of OTHER; a second S would make it a family with cases
    assert [k for k in listed()["nbody_pair_lead.s"] if k[0] == "pair_forces_jpacked"] == [("pair_forces_jpacked", (8,))]


def test_the_other_four_listings_have_registries_of_their_own():
    """field.s, knn.s, hermite_ensemble.s and hermite6_ensemble.s: the module and the registry function kernel_matrix.REGISTERED_ELSEWHERE
    names exist, the registry is not empty, and the module holds the test that compares it with its listing"""
    for listing, (module_name, function) in km.REGISTERED_ELSEWHERE.items():
        assert module_name.startswith("tests.") and os.path.exists(os.path.join(ROOT, *module_name.split(".")) + ".py"), (listing, module_name)
        module = importlib.import_module(module_name.split(".", 1)[1])
        assert callable(getattr(module, function, None)), f"{listing}: {module_name} has no {function}()"
        assert len(getattr(module, function)()) > 0, f"{listing}: {module_name}.{function}() names no kernel"
        assert callable(getattr(module, km.LISTING_TEST, None)), f"{listing}: {module_name} has no {km.LISTING_TEST}"
        with open(module.__file__) as f:
            text = f.read()
        assert f'"{listing}"' in text, f"{module_name} does not read {listing}"


def test_every_other_kernel_names_an_existing_test():
    for (listing, kernel), test in km.OTHER.items():
        assert listing in km.LISTINGS, (listing, km.kernel_name(kernel))
        module, name = test.split("::")
        path = os.path.join(ROOT, *module.split(".")) + ".py"
        with open(path) as f:
            assert f"\ndef {name}(" in f.read(), f"{listing}: {km.kernel_name(kernel)}: {test} does not exist"


def plan_fields(plan, case):
    return tuple((name, getattr(plan, name)) for name, _ in case.plan)


def query(pkg, case, n=None, i_count=None, j_count=None):
    """the plan query of the case's library"""
    if case.family in ("integrate_bodies_fast", "integrate_bodies_wavesplit"):
        return pkg.plan(i_count, j_count, case.dtype)
    if case.family == "pair_forces":
        return pkg.pair_plan(n, case.dtype)
    if case.family == "ensemble_fast":
        return pkg.ensemble_plan(n, dict(case.shape)["systems"], case.dtype)
    if case.family == "hermite_eval":
        return pkg.hermite_plan(n, case.dtype)
    if case.family == "hermite_block_eval":
        return pkg.hermite_block_plan(n, n, case.dtype)
    if case.family == "hermite6_eval":
        return pkg.hermite6_plan(n, case.dtype)
    if case.family == "hermite6_block_eval":
        return pkg.hermite6_block_plan(n, n, case.dtype)
    if case.family == "hermite_block_ensemble_eval":
        return pkg.hermite_block_ensemble_plan(n, dict(case.shape)["systems"], n, case.dtype)
    if case.family == "hermite6_block_ensemble_eval":
        return pkg.hermite6_block_ensemble_plan(n, dict(case.shape)["systems"], n, case.dtype)
    if case.family == "energy_ensemble_pairs":
        return pkg.energy_ensemble_plan(n, 1, case.dtype)
    return pkg.neighbour_plan(n, case.dtype)


class forced:
    """the case's override for the duration of a block"""
    RESET = {"set_plan_override": (0, 0, 0), "set_pair_plan_override": (0, 0, 0, 0)}

    def __init__(self, pkg, override):
        self.pkg, self.override = pkg, override

    def __enter__(self):
        if self.override:
            getattr(self.pkg, self.override[0])(*self.override[1])

    def __exit__(self, *exc):
        if self.override:
            getattr(self.pkg, self.override[0])(*self.RESET[self.override[0]])


def test_n_dispatched_cases_select_their_instantiation_on_the_host(pkg):
    """ensemble, Hermite and block steps of both orders, block ensembles, neighbours: the plan is host logic of (N, precision) alone"""
    assert set(km.N_DISPATCHED) <= set(km.FAMILIES)
    for case in km.CASES:
        if case.family not in km.N_DISPATCHED:
            continue
        n = dict(case.shape)["n"]
        assert plan_fields(query(pkg, case, n=n), case) == case.plan, (case.id, n)
        s = case.args[km.N_DISPATCHED[case.family]]
        assert n in km.N_BY_WAVES[s] or (case.family == "ensemble_fast" and (n, dict(case.shape)["systems"]) in km.ENSEMBLE_LARGE)
    # every instantiation the listing holds has a case at every size of its wave count: one taken out is missed by the kernel's name
    for family, position in km.N_DISPATCHED.items():
        compiled = sorted(k for k in listed()[km.FAMILY_LISTING[family]] if k[0] == family)
        assert compiled, family
        for kernel in compiled:
            s = kernel[1][1 + position]
            with_systems = {"ensemble_fast": 3, "hermite_block_ensemble_eval": km.BLOCK_ENSEMBLE_SYSTEMS, "hermite6_block_ensemble_eval": km.BLOCK_ENSEMBLE_SYSTEMS}.get(family)
            want = set(km.N_BY_WAVES[s]) if with_systems is None else {(n, with_systems) for n in km.N_BY_WAVES[s]}
            if family == "ensemble_fast" and s == 8:
                want |= set(km.ENSEMBLE_LARGE)
            have = {dict(c.shape)["n"] if with_systems is None else (dict(c.shape)["n"], dict(c.shape)["systems"]) for c in km.cases_of(family) if c.kernel == kernel}
            assert have == want, f"{km.kernel_name(kernel)}: cases at {sorted(have)}, wanted at {sorted(want)}"
    # the switch points of S, and both neighbours of each
    for n in (255, 256, 257, 511, 512, 513, 1023, 1024, 1025):
        want = 1 if n < 256 else 2 if n < 512 else 4 if n < 1024 else 8
        for dtype in (F32, F64):
            got = (pkg.ensemble_plan(n, 1, dtype).waves_per_group, pkg.hermite_plan(n, dtype).waves_per_group, pkg.hermite_block_plan(n, 1, dtype).waves_per_group,
                   pkg.neighbour_plan(n, dtype).waves_per_group, pkg.hermite6_plan(n, dtype).waves_per_group, pkg.hermite6_block_plan(n, 1, dtype).waves_per_group,
                   pkg.hermite_block_ensemble_plan(n, 1, 1, dtype).waves_per_group, pkg.hermite6_block_ensemble_plan(n, 1, 1, dtype).waves_per_group)
            assert got == (want,) * 8, (n, got)
            for n_act in (1, 65, 129, n):  # ... whatever part of the system is due
                got = (pkg.hermite6_block_plan(n, n_act, dtype).waves_per_group, pkg.hermite_block_ensemble_plan(n, km.BLOCK_ENSEMBLE_SYSTEMS, n_act, dtype).waves_per_group,
                       pkg.hermite6_block_ensemble_plan(n, km.BLOCK_ENSEMBLE_SYSTEMS, n_act, dtype).waves_per_group)
                assert got == (want,) * 3, (n, n_act, got)
    # the energies of an ensemble: every case at the first or the last n of its window, every window with both, and every n from 1 to
    # 65 536 inside the window of the instantiation its plan selects -- so of the twelve compiled kernels only the ten with a case are ever
    # asked for (the other two: UNREACHABLE, test_unreachable_reasons_hold)
    for dtype in (F32, F64):
        cases = [c for c in km.cases_of("energy_ensemble_pairs") if c.dtype == dtype]
        for case in cases:
            assert plan_fields(query(pkg, case, n=dict(case.shape)["n"]), case) == case.plan, case.id
        assert sorted((c.args, dict(c.shape)["n"]) for c in cases) == sorted({(shape, n) for shape, first, last in km.ENERGY_ENSEMBLE_WINDOWS[dtype] for n in (first, last)})
        w = km.LANE_WIDTH[dtype]
        for shape, first, last in km.ENERGY_ENSEMBLE_WINDOWS[dtype]:
            for n in range(first, last + 1):
                p = pkg.energy_ensemble_plan(n, 1, dtype)
                assert (p.bodies_per_lane // w, p.waves_per_group) == shape, (km.TYPE_NAME[dtype], n, shape)
        windows = km.ENERGY_ENSEMBLE_WINDOWS[dtype]
        assert windows[0][1] == 1 and windows[-1][2] == 65536 and all(a[2] + 1 == b[1] for a, b in zip(windows, windows[1:]))
        idle = {u.kernel[1][1:] for u in km.UNREACHABLE if u.kind == "energy_plan" and u.kernel[1][0] == km.TYPE_NAME[dtype]}
        compiled = {k[1][1:] for k in listed()["energy_ensemble.s"] if k[0] == "energy_ensemble_pairs" and k[1][0] == km.TYPE_NAME[dtype]}
        assert {shape for shape, _, _ in windows} == {c.args for c in cases} == compiled - idle and idle <= compiled


def test_overridden_cases_select_their_instantiation_on_the_host(pkg):
    """one-sided and pairwise: the same query the GPU part reads, here with the CU count the library assumes without a device"""
    for case in km.cases_of("integrate_bodies_fast"):
        for launch in stream_launches(case):
            with forced(pkg, case.override):
                assert plan_fields(query(pkg, case, i_count=launch["i_count"], j_count=launch["j_count"]), case) == case.plan, (case.id, launch["name"])
    for case in km.cases_of("integrate_bodies_wavesplit"):
        with forced(pkg, case.override):
            for launch in wavesplit_launches(pkg, case, cu_count=256):
                assert plan_fields(query(pkg, case, i_count=launch["i_count"], j_count=launch["j_count"]), case) == case.plan, (case.id, launch["name"])
    for case in km.cases_of("pair_forces"):
        with forced(pkg, case.override):
            assert plan_fields(query(pkg, case, n=dict(case.shape)["n"]), case) == case.plan, case.id
    # pair_forces_jpacked (OTHER): the geometry its test forces is the one launch_pair hands to it -- fp32, R = 8, eight waves, one split, one slice
    assert km.OTHER["nbody_pair_lead.s", ("pair_forces_jpacked", (8,))] == "tests.test_pair_jpacked::test_jpacked_shapes"
    import test_pair_jpacked  # (every test of it is marked gpu; its constants are plain)
    sizes = next(mark.args[1] for mark in test_pair_jpacked.test_jpacked_shapes.pytestmark if mark.name == "parametrize")
    assert km.JPACKED_OVERRIDE[1] == (*test_pair_jpacked.LEAD, 1) and km.JPACKED_N in sizes, "the override and a size of test_jpacked_shapes"
    with forced(pkg, km.JPACKED_OVERRIDE):
        for n in sizes:
            p = pkg.pair_plan(n, F32)
            assert tuple((name, getattr(p, name)) for name, _ in km.JPACKED_PLAN) == km.JPACKED_PLAN, f"{n} bodies: the forced headline geometry is not the j-packed kernel's"


def test_unreachable_reasons_hold(pkg):
    """pair_forces<T, 8, 16>: asked for through the override, every size needs more LDS than a CU has; no default plan has 16 waves.
    integrate_bodies_fast<T, R, 16, 4>: the override refuses the tile, and no plan with 16 waves -- default or forced -- has it.
    energy_ensemble_pairs<float, 2, 1> and <float, 4, 2>: the plan query, which nothing overrides, selects them for no n in [1, 65 536]."""
    assert {u.kernel for u in km.UNREACHABLE} == ({("pair_forces", (t, 8, 16)) for t in ("float", "double")} |
                                                  {("integrate_bodies_fast", (t, r, 16, 4)) for t, rs in (("float", (1, 2)), ("double", (1, 2, 4))) for r in rs} |
                                                  {("energy_ensemble_pairs", ("float", 2, 1)), ("energy_ensemble_pairs", ("float", 4, 2))})
    shapes = [(i, j) for i in (1, 63, 300, 1000, 4096, 8193, 20000, 32768, 40001, 65536, 131072, 262144, 1048576) for j in (i, 37, 2048, 5000, 1048576)]
    for u in km.UNREACHABLE:
        dtype = km.DTYPE_OF[u.kernel[1][0]]
        name = km.kernel_name(u.kernel)
        if u.kind == "energy_plan":
            assert not u.override and dtype == F32
            r, s = u.kernel[1][1:]
            for n in range(1, 65537):
                p = pkg.energy_ensemble_plan(n, 1, dtype)
                assert (p.bodies_per_lane // km.LANE_WIDTH[dtype], p.waves_per_group) != (r, s), f"{name}: n = {n} selects it now -- give the kernel a case"
            plan = pkg.EnergyEnsemblePlan()  # past the last n the query answers nothing
            assert pkg.energy_ensemble_lib().nb_energy_ensemble_plan_f32(65537, 1, ctypes.byref(plan)) == 10001
        elif u.kind == "pair_lds":
            with forced(pkg, u.override):
                for n in km.PAIR_SIZES:
                    p = pkg.pair_plan(n, dtype)
                    assert (p.bodies_per_lane // km.LANE_WIDTH[dtype], p.waves_per_block) == u.kernel[1][1:], (n, "the override does ask for it")
                    assert p.lds_bytes > km.GFX950_LDS_BYTES, (name, n, p.lds_bytes)
            for n in sorted(set(km.PAIR_SIZES) | set(range(6145, 300000, 4099))):  # no default plan selects it, whatever N
                assert pkg.pair_plan(n, dtype).waves_per_block == 8, (name, n)
        else:
            assert u.kind == "tile_refused"
            i, s, tile = u.override[1]
            with forced(pkg, ("set_plan_override", (i, s, 2048))):
                assert pkg.lib().nb_set_plan_override(i, s, tile) == 10001, f"{name}: the override takes the tile now -- give the kernel a case"
                before = pkg.plan(5000, 5000, dtype)
                assert (before.bodies_per_lane, before.lanes_per_body, before.tile_bodies) == (i, s, 2048), "a refused override changes nothing"
            for forced_plan in ((0, 0, 0), (0, 16, 0), (i, 16, 0), (i, 16, 2048), (i, 16, 1024)):
                with forced(pkg, ("set_plan_override", forced_plan)):
                    for i_count, j_count in shapes:
                        p = pkg.plan(i_count, j_count, dtype)
                        assert p.lanes_per_body != 16 or p.tile_bodies <= 2048, (name, forced_plan, i_count, j_count, p.tile_bodies)


# ---------------------------------------------------------------------------------------------------------------- one-sided shapes
def stream_unroll(dtype, r):
    """U of nbody_fast_stream.inc: bodies j per group"""
    return 4 if (dtype == F64 and r == 1) else (8 // r if r >= 2 else 8)


def stream_launches(case):
    """The two launches of a wave-stream case <T, R, S, LPT> (I = R W bodies i per lane, chunks of CH = 64 LPT bodies j, groups of U):

    long   i = [37, 37 + 64 I + 29): two workgroups, the second ragged.  j from 3: P S + 2 whole chunks and a last chunk of 3 U + 1
           bodies (three groups, one body over), which wave 2 streams; P chunks per wave = 9 in fp32 or, where a register sum takes more
           chunks than that before it is flushed (LPT = 1: 16), one more than that; 3 in fp64.  The first body j has mass 0, so the sums
           are in units of 1: chunk c is unit (every mass 1), one species (0.25) or mixed as c mod 3 = 0, 1, 2; chunk 0 is mixed by its
           first body.
    short  i = [5, 5 + 128 I + 1): three workgroups.  j from 6: S - 2 whole chunks and a last chunk of 3 U + 1 bodies: S - 1 chunks, the
           last wave has nothing to do.  The first body j has mass 0.5, the unit of this launch: unit chunks are 0.5, species 2."""
    r, s, lpt = case.args
    i, ch, u = r * km.LANE_WIDTH[case.dtype], 64 * lpt, stream_unroll(case.dtype, r)
    per_wave = max(9, 1024 // ch + 1) if case.dtype == F32 else 3
    return [dict(name="long", i_begin=37, i_count=64 * i + 29, j_begin=3, j_count=(per_wave * s + 2) * ch + 3 * u + 1, chunk=ch, first_mass=0.0, unit=1.0, species=0.25),
            dict(name="short", i_begin=5, i_count=128 * i + 1, j_begin=6, j_count=(s - 2) * ch + 3 * u + 1, chunk=ch, first_mass=0.5, unit=0.5, species=2.0)]


def wavesplit_launches(pkg, case, cu_count):
    """The two launches of a wave-split case <T, R, LPT, BLOCK> (a wave owns I = R W bodies i, tiles of TILE = LPT BLOCK bodies j consumed
    in rounds of 64 U, U = 8 / R).  The override must be set.  The i range starts at 37 / 5 and holds CUs x multiple + 29 bodies, the first
    multiple of the case for which the plan query answers with the case's BLOCK (kernel_matrix._wavesplit_cases).

    long   j from 3: three whole tiles and a last one of 64 U + 13 bodies (a whole round, then a partial one)
    short  j from 6: one tile of 32 U + 13 bodies, less than a round
    Masses by spans of 64 bodies j as the wave-stream launches have them by chunk."""
    r, lpt, block = case.args
    i, tile, u = r * km.LANE_WIDTH[case.dtype], lpt * block, 8 // r
    out = []
    for name, i_begin, j_begin, j_count, first_mass, unit, species in (("long", 37, 3, 3 * tile + 64 * u + 13, 0.0, 1.0, 0.25), ("short", 5, 6, 32 * u + 13, 0.5, 0.5, 2.0)):
        counts = [301 if m == 0 else cu_count * m + 29 for m in dict(case.shape)["cu_multiples"]]
        chosen = next((c for c in counts if plan_fields(pkg.plan(c, j_count, case.dtype), case) == case.plan), None)
        assert chosen is not None, f"{case.id}, {name}: no i_count of {counts} makes the plan query answer {dict(case.plan)} on {cu_count} CUs"
        assert chosen % (block // 64 * i) != 0
        out.append(dict(name=name, i_begin=i_begin, i_count=chosen, j_begin=j_begin, j_count=j_count, chunk=64, first_mass=first_mass, unit=unit, species=species))
    return out


def shard_system(dtype, launch, seed):
    """(n, 4) bodies for one launch: standard normal positions; the masses of the j range by spans of `chunk` bodies from j_begin -- unit,
    one species, mixed (0.5 .. 2), in turn -- the first body j `first_mass`; every body outside the j range has a random mass"""
    rng = np.random.default_rng(seed)
    j0, nj, ch = launch["j_begin"], launch["j_count"], launch["chunk"]
    n = max(launch["i_begin"] + launch["i_count"], j0 + nj) + 11
    pos = np.zeros((n, 4), dtype)
    pos[:, :3] = rng.standard_normal((n, 3))
    pos[:, 3] = rng.uniform(0.5, 2.0, n)
    span = (np.arange(nj) // ch) % 3
    pos[j0:j0 + nj, 3] = np.where(span == 0, launch["unit"], np.where(span == 1, launch["species"], pos[j0:j0 + nj, 3]))
    pos[j0, 3] = launch["first_mass"]
    return pos


def sample_ranges(begin, count, budget_rows):
    """[(first, count)] within [begin, begin + count): all of it when it fits the budget, else its first 64 bodies, 61 in the middle and its last 93"""
    if count <= max(budget_rows, 218):
        return [(begin, count)]
    return [(begin, 64), (begin + count // 2 - 30, 61), (begin + count - 93, 93)]


_SUMS = {}  # (dtype, bodies, eps^2, range) -> (a, F): the long double sums, once per (system, range)


def sums(pos, i0, ni, j0, nj, eps2):
    key = (pos.dtype.name, hashlib.sha1(pos.tobytes()).hexdigest(), float(eps2), i0, ni, j0, nj)
    if key not in _SUMS:
        _SUMS[key] = direct_sum_f64(pos, i0, ni, j0, nj, eps2)
    return _SUMS[key]


def check_partial_sums(acc, pos, launch, eps2, what):
    """the accelerations a launch without NB_SHARD_FINALIZE left, against the long double sums over its j range: |a_gpu - a| <= tol F_i per
    body (tol of test_fast_domain: 5e-6 fp32, 1e-14 fp64); nothing outside the i range written, .w zero"""
    dtype = pos.dtype.type
    n = pos.shape[0]
    acc = acc.reshape(n, 4)
    i0, ni, j0, nj = launch["i_begin"], launch["i_count"], launch["j_begin"], launch["j_count"]
    worst = 0.0
    for a, count in sample_ranges(i0, ni, PAIR_TERMS // (2 * nj)):
        ref, size = sums(pos, a, count, j0, nj, eps2)
        err = np.linalg.norm(acc[a:a + count, :3].astype(np.float64) - ref, axis=1) / size
        worst = max(worst, float(err.max()))
    print(f"{what}: i [{i0}, {i0 + ni}) x j [{j0}, {j0 + nj}): max |da| / F = {worst:.3e} (tol {TOL[dtype]:.0e})")
    assert np.isfinite(acc).all() and worst < TOL[dtype], f"{what}: {worst:.3e} of F_i"
    assert not acc[:i0].any() and not acc[i0 + ni:].any(), f"{what}: wrote outside its i range"
    assert not acc[:, 3].any(), f"{what}: .w of the partial sums"


def run_shard_case(gpu, case, launches):
    for k, launch in enumerate(launches):
        pos = shard_system(case.dtype, launch, 1000 * len(case.args) + 17 * sum(case.args) + k)
        p = gpu.plan(launch["i_count"], launch["j_count"], case.dtype)
        assert plan_fields(p, case) == case.plan, f"{case.id}, {launch['name']}: the plan query selects {plan_fields(p, case)}"
        acc = gpu_accel(gpu, pos.reshape(-1), case.dtype, launch["i_begin"], launch["i_count"], launch["j_begin"], launch["j_count"], gpu.NB_MODE_FAST)
        check_partial_sums(acc, pos, launch, case.dtype(EPS2), f"{case.id} {launch['name']}")


def test_stream_launches_meet_every_shape_condition():
    """what the issue asks each wave-stream instantiation to meet at least once, asserted on the shapes themselves"""
    for case in km.cases_of("integrate_bodies_fast"):
        r, s, lpt = case.args
        i, u = r * km.LANE_WIDTH[case.dtype], stream_unroll(case.dtype, r)
        long, short = stream_launches(case)
        for launch in (long, short):
            ch = launch["chunk"]
            chunks = -(-launch["j_count"] // ch)
            last = launch["j_count"] - (chunks - 1) * ch
            assert launch["i_count"] % (64 * i) != 0 and launch["i_begin"] != 0 and launch["j_begin"] % 4 != 0
            assert last % u != 0 and (last // u) % 2 == 1, "a last chunk off a multiple of U, with an odd number of groups"
            assert launch["i_count"] * launch["j_count"] <= PAIR_TERMS
            masses = shard_system(case.dtype, launch, 1)[launch["j_begin"]:launch["j_begin"] + launch["j_count"], 3]
            forms = set()
            for c in range(chunks):
                m = masses[c * ch:(c + 1) * ch]
                forms.add("mixed" if len(set(m)) > 1 else "unit" if m[0] == launch["unit"] else "species")
            assert forms == {"unit", "species", "mixed"}, (case.id, launch["name"], forms)
        assert -(-short["j_count"] // short["chunk"]) < s, "fewer chunks than waves"
        assert long["first_mass"] == 0.0 and short["first_mass"] != 0.0
        if case.dtype == F32:
            per_wave = (long["j_count"] // long["chunk"]) // s
            assert per_wave >= 9 and per_wave > 1024 // long["chunk"], "the second-level sums are flushed at least once"


# ---------------------------------------------------------------------------------------------------------------- GPU: one-sided
@gpu_only
@pytest.mark.parametrize("case", km.cases_of("integrate_bodies_fast"), ids=ids(km.cases_of("integrate_bodies_fast")))
def test_integrate_bodies_fast(gpu, case):
    gpu.set_softening_squared(case.dtype(EPS2))
    with forced(gpu, case.override):
        run_shard_case(gpu, case, stream_launches(case))


@gpu_only
@pytest.mark.parametrize("case", km.cases_of("integrate_bodies_wavesplit"), ids=ids(km.cases_of("integrate_bodies_wavesplit")))
def test_integrate_bodies_wavesplit(gpu, case):
    gpu.set_softening_squared(case.dtype(EPS2))
    with forced(gpu, case.override):
        run_shard_case(gpu, case, wavesplit_launches(gpu, case, gpu.device_info(0).compute_units))


def step_rows(pos, vel, a, size, rows, dt, damping, dtype):
    """test_fast_domain.step_bounds for the bodies `rows`, from their long double sums (a, F): (v1, p1, bound_v, bound_p)"""
    tol, u = TOL[dtype], UNIT_ROUNDOFF[dtype]
    dt_l, damp_l = LD(dt), LD(damping)
    v0, p0 = vel[rows, :3].astype(LD), pos[rows, :3].astype(LD)
    v1 = (v0 + a.astype(LD) * dt_l) * damp_l
    p1 = p0 + v1 * dt_l
    a_dt = np.abs(a.astype(LD)) * abs(dt_l)
    bound_v = abs(damp_l) * (abs(dt_l) * tol * size.astype(LD)[:, None] + 2 * u * (np.abs(v0) + a_dt))
    bound_p = abs(dt_l) * bound_v + 2 * u * (np.abs(p0) + np.abs(v1) * abs(dt_l))
    return v1, p1, bound_v, bound_p


def check_step_rows(got_pos, got_vel, pos, vel, ranges, j0, nj, dt, damping, eps2, what):
    """check_step of test_fast_domain for the bodies of `ranges` only (a system too large to sum whole), the bodies j [j0, j0 + nj)"""
    dtype = pos.dtype.type
    for a0, count in ranges:
        a, size = sums(pos, a0, count, j0, nj, eps2)
        rows = np.arange(a0, a0 + count)
        v1, p1, bound_v, bound_p = step_rows(pos, vel, a, size, rows, dt, damping, dtype)
        err_v, err_p = np.abs(got_vel[rows, :3].astype(LD) - v1), np.abs(got_pos[rows, :3].astype(LD) - p1)
        print(f"{what}: bodies [{a0}, {a0 + count}): velocity at {float((err_v / bound_v).max()):.3g}, position at {float((err_p / bound_p).max()):.3g} of their bounds")
        assert (err_v <= bound_v).all(), f"{what}: velocity {float((err_v / bound_v).max()):.3g} x its bound in [{a0}, {a0 + count})"
        assert (err_p <= bound_p).all(), f"{what}: position {float((err_p / bound_p).max()):.3g} x its bound in [{a0}, {a0 + count})"
    assert got_pos[:, 3].tobytes() == pos[:, 3].tobytes() and got_vel[:, 3].tobytes() == vel[:, 3].tobytes(), f"{what}: .w changed"


@gpu_only
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("family", ["integrate_bodies_fast", "integrate_bodies_wavesplit"])
def test_shard_flags_compose_off_the_first_body(gpu, family, dtype):
    """The same ranges twice, i_begin = 37: acc-out over the first part of j, then NB_SHARD_ACC_IN | NB_SHARD_FINALIZE over the rest (the
    wave-stream kernel divides the sums it takes in by the second part's reference mass, 0.375, and multiplies on the way out); then one
    finalize call.  Each against the long double step, and against each other within twice the bounds both meet."""
    w = km.LANE_WIDTH[dtype]
    override = (4, 8, 2048) if family == "integrate_bodies_fast" else (w, 64, 512)
    i0, ni, j0, nj, cut = 37, 2 * 64 * 4 + 29, 3, 5000 + 77, 1900 + 3
    n = j0 + nj + 11
    rng = np.random.default_rng(53)
    pos, vel = np.zeros((n, 4), dtype), np.zeros((n, 4), dtype)
    pos[:, :3], vel[:, :3] = rng.standard_normal((n, 3)), rng.standard_normal((n, 3)) * 0.3
    pos[:, 3], vel[:, 3] = rng.uniform(0.5, 2.0, n), rng.uniform(0.01, 0.5, n)
    pos[j0, 3], pos[cut, 3] = 1.25, 0.375
    dt, damping, eps2 = dtype(np.float32(0.016)), dtype(np.float32(0.995)), dtype(EPS2)
    gpu.set_softening_squared(eps2)
    fn = gpu.lib().nb_integrate_shard_f32 if dtype == F32 else gpu.lib().nb_integrate_shard_f64
    d_old, d_new, d_vel, d_acc = (gpu.DeviceBuffer(pos.nbytes) for _ in range(4))
    results = []
    with forced(gpu, ("set_plan_override", override)):
        p = gpu.plan(ni, nj - (cut - j0), dtype)
        assert (p.bodies_per_lane, p.lanes_per_body, p.tile_bodies) == override
        try:
            for parts in (((j0, cut - j0, 0), (cut, j0 + nj - cut, gpu.NB_SHARD_ACC_IN | gpu.NB_SHARD_FINALIZE)), ((j0, nj, gpu.NB_SHARD_FINALIZE),)):
                d_old.upload(pos.reshape(-1)), d_vel.upload(vel.reshape(-1)), d_new.upload(np.zeros(4 * n, dtype)), d_acc.upload(np.full(4 * n, 7.0, dtype))
                for first, count, flags in parts:
                    gpu.check(fn(d_new.ptr, d_old.ptr, d_vel.ptr, d_acc.ptr, i0, ni, first, count, flags, dt, damping, 256, gpu.NB_MODE_FAST, None), "nb_integrate_shard")
                results.append((d_new.download(np.zeros(4 * n, dtype)).reshape(n, 4).copy(), d_vel.download(np.zeros(4 * n, dtype)).reshape(n, 4).copy()))
        finally:
            for buf in (d_old, d_new, d_vel, d_acc):
                buf.free()
    rows = np.arange(i0, i0 + ni)
    outside = np.ones(n, bool)
    outside[rows] = False
    for name, (new_pos, new_vel) in zip(("acc-out, then acc-in + finalize", "one finalize call"), results):
        assert not new_pos[outside].any() and new_vel[outside].tobytes() == vel[outside].tobytes(), f"{name}: wrote outside its i range"
        full_pos = pos.copy()
        full_pos[rows] = new_pos[rows]
        check_step_rows(full_pos, new_vel, pos, vel, [(i0, ni)], j0, nj, dt, damping, eps2, f"{family} {np.dtype(dtype).name}, {name}")
    a, size = sums(pos, i0, ni, j0, nj, eps2)
    _, _, bound_v, bound_p = step_rows(pos, vel, a, size, rows, dt, damping, dtype)
    assert (np.abs(results[0][1][rows, :3].astype(LD) - results[1][1][rows, :3].astype(LD)) <= 2 * bound_v).all(), "the two velocities differ by more than both bounds"
    assert (np.abs(results[0][0][rows, :3].astype(LD) - results[1][0][rows, :3].astype(LD)) <= 2 * bound_p).all(), "the two positions differ by more than both bounds"


# ---------------------------------------------------------------------------------------------------------------- GPU: pairwise
def set_masses(bodies, kind, seed):
    """masses of an (n, 4) system in place: "equal" as they are; "species": three contiguous species whose borders fall inside chunks, tiles and
    blocks; "random": 2^-3 .. 2^3"""
    n = bodies.shape[0]
    if kind == "species":
        bodies[:, 3] = 1.0
        bodies[n // 3 + 5:, 3] = 2.0
        bodies[2 * n // 3 + 11:, 3] = 0.25
    elif kind == "random":
        bodies[:, 3] = 2.0 ** np.random.default_rng(seed).uniform(-3, 3, n)
    return bodies


@gpu_only
@pytest.mark.parametrize("case", km.cases_of("pair_forces"), ids=ids(km.cases_of("pair_forces")))
def test_pair_forces(gpu, oracle, case):
    """one step of a whole system of 3 000 bodies (a last block that is partly empty in every geometry), three species with borders inside
    blocks and tiles and velocities with a .w, against check_step (one long double reference per precision, whatever the geometry)"""
    n, dtype = dict(case.shape)["n"], case.dtype
    oracle.srand(3)
    pos, vel = oracle.randomise(1, n, 1.54, 8.0, dtype)
    set_masses(pos.reshape(n, 4), "species", 0)
    vel.reshape(n, 4)[:, 3] = np.random.default_rng(3).uniform(0.01, 0.5, n)
    params = gpu.NBodyParams(softening=0.1, damping=0.995)
    dt, damping = dtype(np.float32(0.016)), dtype(np.float32(0.995))
    with forced(gpu, case.override):
        p = gpu.pair_plan(n, dtype)
        assert plan_fields(p, case) == case.plan, f"{case.id}: the plan query selects {plan_fields(p, case)}"
        assert p.lds_bytes <= gpu.device_info(0).lds_bytes_per_cu
        got_pos, got_vel = run_gpu(gpu, pos, vel, 1, gpu.NB_MODE_FAST, dt=dt, params=params, workspace=True)
    check_step(got_pos, got_vel, pos, vel, dt, damping, eps2_of(dtype, 0.1), case.id)


@gpu_only
def test_unreachable_kernels_exceed_this_devices_lds(gpu):
    lds = gpu.device_info(0).lds_bytes_per_cu
    for u in km.UNREACHABLE:
        if u.kind != "pair_lds":
            continue
        dtype = km.DTYPE_OF[u.kernel[1][0]]
        with forced(gpu, u.override):
            for n in km.PAIR_SIZES:
                assert gpu.pair_plan(n, dtype).lds_bytes > lds, (km.kernel_name(u.kernel), n, lds)


# ---------------------------------------------------------------------------------------------------------------- GPU: dispatched by N
@gpu_only
@pytest.mark.parametrize("case", km.cases_of("ensemble_fast"), ids=ids(km.cases_of("ensemble_fast")))
def test_ensemble_fast(gpu, oracle, case):
    """systems of equal, species and random masses in one launch; up to 1 025 bodies every body against check_step, the large systems on
    sampled bodies (their first, middle and last workgroups) within the same bounds"""
    shape = dict(case.shape)
    n, count, dtype = shape["n"], shape["systems"], case.dtype
    p = gpu.ensemble_plan(n, count, dtype)
    assert plan_fields(p, case) == case.plan, f"{case.id}: the plan query selects {plan_fields(p, case)}"
    pos, vel = ensemble_systems(oracle, dtype, n, count, seed0=61 + n % 7)
    for s in range(count):
        set_masses(pos[s], km.MASSES[s % 3], n + s)
    dt, damping = 0.016, 0.995
    got_pos, got_vel = ensemble_step(gpu, pos, vel, gpu.NB_MODE_FAST, dt=dt, damping=damping)
    for s in range(count):
        what = f"{case.id} system {s} ({km.MASSES[s % 3]})"
        if n * n * count <= PAIR_TERMS:
            check_step(got_pos[s].reshape(-1), got_vel[s].reshape(-1), pos[s].reshape(-1), vel[s].reshape(-1), as_T(dtype, dt), as_T(dtype, damping), eps2_of(dtype, 0.1), what)
            continue
        rows = PAIR_TERMS // (count * n)
        ranges = [(0, rows // 3), (n // 2 - 30, rows // 3), (n - rows // 3, rows // 3)]
        check_step_rows(got_pos[s], got_vel[s], pos[s], vel[s], ranges, 0, n, as_T(dtype, dt), as_T(dtype, damping), eps2_of(dtype, 0.1), what)
        assert np.isfinite(got_pos[s]).all() and np.isfinite(got_vel[s]).all(), what


@gpu_only
@pytest.mark.parametrize("case", km.cases_of("hermite_eval"), ids=ids(km.cases_of("hermite_eval")))
def test_hermite_eval(gpu, case):
    n, dtype = dict(case.shape)["n"], case.dtype
    assert plan_fields(gpu.hermite_plan(n, dtype), case) == case.plan, case.id
    step = case.args[1]
    for mass in km.MASSES:
        if step:
            check_one_step(gpu, dtype, n, mass, 0.01, 1.0 / 64)
        else:
            pos, vel = cloud(n, dtype, 1000 + n, mass)
            acc, jerk = evaluate(gpu, pos, vel, dtype(0.01))
            check_eval(acc, jerk, pos, vel, dtype(0.01), f"{case.id} {mass}")


@gpu_only
@pytest.mark.parametrize("case", km.cases_of("hermite_block_eval"), ids=ids(km.cases_of("hermite_block_eval")))
def test_hermite_block_eval(gpu, case):
    """block-step stages with all, 129 and 65 of the bodies due (one, some and few tiles of active bodies)"""
    n, dtype = dict(case.shape)["n"], case.dtype
    for k, (mass, n_act) in enumerate(zip(km.MASSES, (n, 129, 65))):
        assert plan_fields(gpu.hermite_block_plan(n, n_act, dtype), case) == case.plan, (case.id, n_act)
        check_block_stages(gpu, dtype, n, n_act, mass, (2e-5, 3e-4, 4e-3, 0.05)[(n + k) % 4])


def step6_masses(case):
    """The mass kinds of a hermite6_eval<T, S, true> case: one kind, rotating with the place of n among the sizes of its S -- or as many more
    as it takes for the S with fewer than three sizes to meet all three (S = 1: one size, three kinds; S = 8: two sizes, two kinds each)."""
    sizes = km.N_BY_WAVES[case.args[0]]
    place = sizes.index(dict(case.shape)["n"])
    return tuple(km.MASSES[(place + k) % 3] for k in range(-(-3 // len(sizes))))


def test_every_wave_count_of_the_sixth_order_step_meets_every_mass_kind():
    for dtype in (F32, F64):
        for s in km.N_BY_WAVES:
            cases = [c for c in km.cases_of("hermite6_eval") if c.dtype == dtype and c.args == (s, True)]
            assert {m for c in cases for m in step6_masses(c)} == set(km.MASSES), (km.TYPE_NAME[dtype], s)
            assert all(len(step6_masses(c)) == 1 for c in cases) or len(cases) < 3


@gpu_only
@pytest.mark.parametrize("case", km.cases_of("hermite6_eval"), ids=ids(km.cases_of("hermite6_eval")))
def test_hermite6_eval(gpu, case):
    """STEP = false: nb_hermite6_eval_* on the fp32-representable states of tests/test_hermite6.py (a random acc_in) with all three mass kinds,
    against reference6 under check_eval.  STEP = true: the second step of a run, every stage against ld_step (check_one_step6), the mass
    kinds in rotation over the sizes of an S (step6_masses).

    What these cases found: with the corrector as first written (v + fma(h/2, a0 + a1, fma(h^3/120, s0 + s1, -h^2/10 (j1 - j0)))) the fp64
    step with random masses had its worst velocity at 1.22 (n = 255) and 1.12 (n = 1025) of ld_step's bound, the evaluation being at 0.16
    of its own; the module's case at n = 1000 passed at 0.984.  In these clouds (masses up to 8, softening 0.1, h = 1/64) a few bodies are
    in encounters so tight that h^3/120 |s0 + s1| is the largest term of their velocity increment and larger than |v|, and every operation
    on that term's path left a rounding of its size: four, against the 2u of the term magnitudes ld_step allows.  csrc/hermite6_correct.inc
    now sums the increments of v1 and x1 in twice T's precision (fp32 in fp64, fp64 in double-double), so each takes one rounding of its
    own size."""
    n, dtype = dict(case.shape)["n"], case.dtype
    assert plan_fields(gpu.hermite6_plan(n, dtype), case) == case.plan, case.id
    if case.args[1]:
        for mass in step6_masses(case):
            hermite6.check_one_step6(gpu, dtype, n, mass)
        return
    eps2 = dtype(np.float32(EPS2))  # (the same eps^2 in both precisions: they share one long double reference)
    for mass in km.MASSES:
        pos, vel, acc = hermite6.state32(n, dtype, 6000 + n, mass, 0.3)
        hermite6.check_eval(hermite6.evaluate(gpu, pos, vel, acc, eps2), pos, vel, acc, eps2, f"{case.id} {mass}")


@gpu_only
@pytest.mark.parametrize("case", km.cases_of("hermite6_block_eval"), ids=ids(km.cases_of("hermite6_block_eval")))
def test_hermite6_block_eval(gpu, case):
    """6th-order block-step stages with all, 129 and 65 of the bodies due (one, some and few tiles of active bodies): the predictor, the nine
    sums against reference6, the corrector, the planes in range order bit for bit and the level decisions (check_block6_stages_of, whose
    cap on decisions near a threshold counts these cases with the module's own)"""
    n, dtype = dict(case.shape)["n"], case.dtype
    for k, (mass, n_act) in enumerate(zip(km.MASSES, (n, 129, 65))):
        assert plan_fields(gpu.hermite6_block_plan(n, n_act, dtype), case) == case.plan, (case.id, n_act)
        pos, vel = cloud(n, dtype, 1000 + n + n_act, mass)
        block6.check_block6_stages_of(gpu, pos, vel, dtype(0.01), n_act, mass, block6.STAGE_ETAS[(n + k) % 4])


def check_block_ensemble_case(gpu, case, module, plan_query):
    """Three systems of n bodies with equal, species and random masses and 1, 129 and n bodies due, each with a `now` of its own, in one call:
    after 1 and after 12 block steps every array and the status of every system are the solo calls' bit for bit (check_against_solo of the
    library's module)."""
    n, systems, dtype = dict(case.shape)["n"], dict(case.shape)["systems"], case.dtype
    actives = [1, min(129, n), n]
    assert len(actives) == systems
    for n_act in actives:
        assert plan_fields(plan_query(n, systems, n_act, dtype), case) == case.plan, (case.id, n_act)
    module.check_against_solo(gpu, dtype, n, actives)


@gpu_only
@pytest.mark.parametrize("case", km.cases_of("hermite_block_ensemble_eval"), ids=ids(km.cases_of("hermite_block_ensemble_eval")))
def test_hermite_block_ensemble_eval(gpu, case):
    """The solo block steps' bits (check_block_ensemble_case).  What makes bit equality a reference here: the solo kernels are held to long
    double at these same sizes -- the predictor, the sums, the corrector and the level decisions -- by the cases of hermite_block_eval
    above, so an ensemble instantiation that agrees with them bit for bit meets the same bounds, and one that folds its waves or ends its
    last chunk otherwise does not agree."""
    check_block_ensemble_case(gpu, case, block_ensemble, gpu.hermite_block_ensemble_plan)


@gpu_only
@pytest.mark.parametrize("case", km.cases_of("hermite6_block_ensemble_eval"), ids=ids(km.cases_of("hermite6_block_ensemble_eval")))
def test_hermite6_block_ensemble_eval(gpu, case):
    """The solo 6th-order block steps' bits (check_block_ensemble_case).  What makes bit equality a reference here: the solo kernels are
    held to long double at these same sizes -- S = 4 and every switch of S included -- by the cases of hermite6_block_eval above; before
    those cases the solo bits were themselves unreferenced between 512 and 1 023 bodies."""
    check_block_ensemble_case(gpu, case, block6_ensemble, gpu.hermite6_block_ensemble_plan)


@gpu_only
@pytest.mark.parametrize("case", km.cases_of("neighbour_survey"), ids=ids(km.cases_of("neighbour_survey")))
def test_neighbour_survey(gpu, case):
    """POT = false: nearest neighbours, distances, counts and the lists built on them; POT = true: the potentials of clouds of all three
    mass kinds, softened and not"""
    n, dtype = dict(case.shape)["n"], case.dtype
    assert plan_fields(gpu.neighbour_plan(n, dtype), case) == case.plan, case.id
    if case.args[1]:
        check_cloud(gpu, dtype, n, km.MASSES, (0.01, 0.0))
    else:
        check_cloud(gpu, dtype, n, ("equal",), ())


@gpu_only
@pytest.mark.parametrize("case", km.cases_of("energy_ensemble_pairs"), ids=ids(km.cases_of("energy_ensemble_pairs")))
def test_energy_ensemble_pairs(gpu, case):
    """the probe pairs and the probe bodies of test_energy_domain at the first and the last size of the instantiation's window: every pair
    among the geometry's edge indices (every pair at all up to 130 bodies) and each of those bodies' O(N) terms counted once, bit for bit"""
    n, dtype = dict(case.shape)["n"], case.dtype
    assert plan_fields(gpu.energy_ensemble_plan(n, 1, dtype), case) == case.plan, f"{case.id}: the plan query selects {plan_fields(gpu.energy_ensemble_plan(n, 1, dtype), case)}"
    ensemble_probe_pairs(gpu, dtype, n, case.id)
    ensemble_probe_bodies(gpu, dtype, n, case.id)
