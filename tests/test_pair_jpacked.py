"""pair_forces_jpacked (csrc/nbody_pair_lead.hip): the forces kernel the one-GPU pairwise step launches in pair_forces<float, 8, 8>'s
place for the headline geometry -- fp32, R = 8, eight waves, one workgroup per block, the single full tournament, no clock words
lent and no probe event set.  It packs two bodies J into a register pair (a tile is 128 bodies), so every case here is a shape at which that can go wrong:
even and odd block counts, a last 128-tile with one real body, with 65 (the second half just begins), ragged in both halves, and a
size with several units per wave and a second-level flush.

Every case is forced with nb_set_pair_plan_override(8, 8, 1, 1), runs one whole step, and is held per body to the long double step
of tests/test_fast_domain.py (its helpers, its bounds: the FAST contract, 5e-6 F_i on the force, 2u more on velocity and position).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_fast_domain as domain
from test_gpu_parity import DT, direct_sum_f64, rel_err, run_gpu
from test_pairwise_trajectory import assert_fp32_envelope, forced_pairwise

pytestmark = pytest.mark.gpu

LEAD = (8, 8, 1)   # the geometry pair_forces_jpacked takes
OLD = (8, 8, 2)    # the nearest geometry that keeps pair_forces
BIG = 16384
PARAMS = dict(softening=0.1, damping=0.995)


def bodies(oracle, n, seed=41):
    oracle.srand(seed)
    pos, vel = oracle.randomise(1, n, 1.54, 8.0, np.float32)
    return pos, vel


def seed_yardstick(pos, eps2):
    """test_fast_domain.forces() for a large system: forces() itself is called (its key, its cache), with the direct_sum_f64 it calls
    cut into row ranges over a few threads for that one call (numpy drops the lock inside its loops).  The same sums: a row's
    do not depend on how the rows are cut."""
    def by_row_ranges(p, i0, ni, j0, nj, softening_sq):
        rows = [(i0 + a, min(512, ni - a)) for a in range(0, ni, 512)]
        with ThreadPoolExecutor(8) as pool:
            parts = list(pool.map(lambda r: direct_sum_f64(p, r[0], r[1], j0, nj, softening_sq), rows))
        return np.concatenate([a for a, _ in parts]), np.concatenate([f for _, f in parts])

    plain = domain.direct_sum_f64
    domain.direct_sum_f64 = by_row_ranges
    try:
        domain.forces(pos, eps2)
    finally:
        domain.direct_sum_f64 = plain


def one_step(gpu, pos, vel, plan=LEAD):
    params = gpu.NBodyParams(**PARAMS)
    with forced_pairwise(gpu, plan):
        p = gpu.pair_plan(pos.size // 4, np.float32)
        assert p.applies == 1 and p.slices == 1 and (p.bodies_per_lane, p.waves_per_block, p.splits) == (16, plan[1], plan[2])
        return run_gpu(gpu, pos, vel, 1, gpu.NB_MODE_FAST, dt=DT, params=params, workspace=True)


def held_to_the_yardstick(gpu, got, pos, vel, what):
    eps2 = domain.eps2_of(np.float32, PARAMS["softening"])
    if pos.size // 4 >= 8192:
        seed_yardstick(pos, eps2)
    domain.check_step(got[0], got[1], pos, vel, np.float32(DT), np.float32(PARAMS["damping"]), eps2, what)


@pytest.fixture(scope="module")
def big(gpu, oracle):
    """the 16 384-body system, one species, and its step through both kernels: shared by the three tests that need it"""
    pos, vel = bodies(oracle, BIG)
    return {"pos": pos, "vel": vel, "lead": one_step(gpu, pos, vel), "lead again": one_step(gpu, pos, vel), "old": one_step(gpu, pos, vel, OLD)}


@pytest.mark.parametrize("n", [2048, 3072, 3072 + 1, 3072 + 65, 2048 + 127])
def test_jpacked_shapes(gpu, oracle, n):
    """NB = 2 (even: the antipodal unit q = Q keeps no reaction), NB = 3 (odd), and the ragged last tiles"""
    pos, vel = bodies(oracle, n)
    held_to_the_yardstick(gpu, one_step(gpu, pos, vel), pos, vel, f"{n} bodies")


def test_jpacked_sixteen_blocks(gpu, big):
    """16 blocks: nine units per wave, so the register sums join the second-level sums once on the way"""
    held_to_the_yardstick(gpu, big["lead"], big["pos"], big["vel"], "16 384 bodies")


MASSES = ["one species", "two species by block", "alternating in a tile", "a zero mass", "2^20", "2^-20", "2^21", "2^-21"]


@pytest.mark.parametrize("form", MASSES)
def test_jpacked_masses(gpu, oracle, form):
    """The one-species loop (in units of the species' mass), the general loop, and the edge of the masses a sum may be kept in
    units of (usable_unit: 2^+-20 inside, 2^+-21 outside), on the size whose last tile's second half holds one body."""
    n = 3072 + 65
    pos, vel = bodies(oracle, n, seed=43)
    m = pos.reshape(n, 4)[:, 3]
    if form == "one species":
        m[:] = 0.75
    elif form == "two species by block":
        m[:1024], m[1024:] = 0.5, 2.0
    elif form == "alternating in a tile":
        m[0::2], m[1::2] = 0.5, 2.0
    elif form == "a zero mass":
        m[1500] = 0.0
    else:
        m[:] = np.float32(2.0) ** int(form[2:])
    held_to_the_yardstick(gpu, one_step(gpu, pos, vel), pos, vel, form)


def test_jpacked_is_what_runs(gpu, big):
    """(8, 8, 1) takes another kernel than (8, 8, 2): other bits (another summation order), both inside the bound."""
    assert big["lead"][0].tobytes() != big["old"][0].tobytes()
    held_to_the_yardstick(gpu, big["old"], big["pos"], big["vel"], "16 384 bodies, pair_forces")


def test_jpacked_steps_aside_for_the_clocked_kernel(gpu, big):
    """While clock words are lent, or a probe event is set, the step is pair_forces' again: with room for the launch's workgroups pair_forces_clocked runs,
    one workgroup short pair_forces itself -- the same bits (tests/test_pairwise.py holds the two to that), and not jpacked's."""
    lib = gpu.lib()
    with forced_pairwise(gpu, LEAD):
        grid = gpu.pair_plan(BIG, np.float32).grid_blocks
    words = gpu.DeviceBuffer(grid * 16)
    gpu.check(lib.nb_memset(words.ptr, 0, grid * 16, None))
    try:
        gpu.check(lib.nb_set_pair_clock_words(words.ptr, grid * 16), "nb_set_pair_clock_words")
        clocked = one_step(gpu, big["pos"], big["vel"])
        gpu.check(lib.nb_device_synchronize())
        assert words.download(np.zeros(grid * 2, np.uint64)).all()  # (pair_forces_clocked ran)
        gpu.check(lib.nb_memset(words.ptr, 0, grid * 16, None))
        gpu.check(lib.nb_set_pair_clock_words(words.ptr, grid * 16 - 16), "nb_set_pair_clock_words")
        plain = one_step(gpu, big["pos"], big["vel"])
        gpu.check(lib.nb_device_synchronize())
        assert not words.download(np.zeros(grid * 2, np.uint64)).any()  # (pair_forces ran)
        gpu.check(lib.nb_set_pair_clock_words(None, 0), "nb_set_pair_clock_words")
        probe = gpu.Event()  # ... and while a probe event times the forces kernel on its own (the figure set against those cycles)
        gpu.check(lib.nb_set_pair_probe_event(probe.h), "nb_set_pair_probe_event")
        probed = one_step(gpu, big["pos"], big["vel"])
    finally:
        gpu.check(lib.nb_set_pair_probe_event(None), "nb_set_pair_probe_event")
        gpu.check(lib.nb_set_pair_clock_words(None, 0), "nb_set_pair_clock_words")
        words.free()
    assert clocked[0].tobytes() == plain[0].tobytes() and clocked[1].tobytes() == plain[1].tobytes()
    assert probed[0].tobytes() == plain[0].tobytes() and probed[1].tobytes() == plain[1].tobytes()
    assert clocked[0].tobytes() != big["lead"][0].tobytes()
    assert one_step(gpu, big["pos"], big["vel"])[0].tobytes() == big["lead"][0].tobytes()  # the words returned: jpacked again


def test_jpacked_is_reproducible(big):
    assert big["lead"][0].tobytes() == big["lead again"][0].tobytes() and big["lead"][1].tobytes() == big["lead again"][1].tobytes()


def test_jpacked_trajectory(gpu, oracle):
    """100 steps at 4 096 + 65 bodies against the CPU path, to the bars every FAST kernel is held to (tests/test_gpu_parity.py
    test_fast_fp32_vs_golden, as tests/test_pairwise_trajectory.py states them for the pairwise layout)."""
    n = 4096 + 65
    pos0, vel0 = oracle.startup_state(n, np.float32)
    ref, p, v, done = {}, pos0.copy(), vel0.copy(), 0
    for s in (1, 10, 100):
        oracle.update(p, v, DT, steps=s - done)
        ref[s], done = p.copy(), s
    with forced_pairwise(gpu, LEAD):
        system = gpu.BodySystemHIP(n, 256, gpu.NBodyParams(), np.float32, pos0, vel0, mode=gpu.NB_MODE_FAST, workspace=True)
        assert system._workspace is not None
        errs, done = {}, 0
        for s in (1, 10, 100):
            for _ in range(s - done):
                system.update(DT)
            errs[s], done = rel_err(system.get_position(), ref[s]), s
        system.free()
    assert_fp32_envelope(errs)
