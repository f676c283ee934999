"""FAST over the operand range STRICT is tested on.  Every FAST path -- the one-sided kernel (default plan, wave-split and tile
layouts forced, a shard chained over uneven j chunks), the pairwise layout (R = 1, 2, 8) and its sliced form (2 and 3 slices) --
takes one whole step, and the result is held to a long double (x86 80-bit) step computed from the same T-typed inputs:

    a_i  = sum_j m_j d_ij / (|d_ij|^2 + eps^2)^(3/2)   (self term included: eps = 0 gives NaN, as the reference does)
    F_i  = sum_j |term_ij|                              (what a sum's rounding error scales with)
    v1   = (v0 + a dt) damping,   p1 = p0 + v1 dt

per body and component:  |v1_gpu - v1| <= |damping| (|dt| tol F_i + 2u (|v0| + |a dt|)),
                         |p1_gpu - p1| <= |dt| bound(v1) + 2u (|p0| + |v1 dt|),
tol = 5e-6 (fp32) / 1e-14 (fp64), u the unit roundoff.  Velocity .w and the masses must come through bit for bit.

Besides: the coupling m d2^(-3/2) per term across the exponent range (fp32 d^2 in 2^+-84, fp64 2^+-600, through the three chunk
forms of the wave-stream kernel), the energy kernel's pair potential over the same range, and non-finite inputs, which must give
non-finite results at exactly the bodies where STRICT gives them.
"""
import hashlib

import numpy as np
import pytest

from conftest import xyz
from test_gpu_parity import direct_sum_f64, gpu_accel, run_gpu
from test_pairwise import sliced

gpu_only = pytest.mark.gpu

TOL = {np.float32: 5e-6, np.float64: 1e-14}
UNIT_ROUNDOFF = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
N = 2048 + 37  # ragged: a partly empty last block, tile and chunk in every layout


# ---------------------------------------------------------------------------------------------- the yardstick
_FORCES = {}  # (dtype, bodies, eps^2) -> (a, F): the long double sums are the expensive part, shared by every path and step case


def forces(pos, eps2):
    """a_i and F_i (float64 arrays, summed in long double) of the T-typed bodies `pos` (4n), softening^2 `eps2` (a T)"""
    key = (pos.dtype.name, hashlib.sha1(pos.tobytes()).hexdigest(), float(eps2))
    if key not in _FORCES:
        n = pos.size // 4
        with np.errstate(all="ignore"):
            _FORCES[key] = direct_sum_f64(pos.reshape(n, 4), 0, n, 0, n, eps2)
    return _FORCES[key]


def yardstick(pos, vel, dt, damping, eps2):
    """one step in long double from T-typed inputs: (a, F, v1, p1), v1 / p1 as (n, 3) long double"""
    a, size = forces(pos, eps2)
    n = pos.size // 4
    dt, damping = np.longdouble(dt), np.longdouble(damping)
    with np.errstate(all="ignore"):
        v1 = (xyz(vel).astype(np.longdouble) + a.astype(np.longdouble) * dt) * damping
        p1 = xyz(pos).astype(np.longdouble) + v1 * dt
    return a, size, v1.reshape(n, 3), p1.reshape(n, 3)


def step_bounds(pos, vel, dt, damping, eps2, tol, u):
    """the yardstick's step and the per-body, per-component allowances (module docstring) for a kernel held to `tol`"""
    a, size, v1, p1 = yardstick(pos, vel, dt, damping, eps2)
    dt_, damp = abs(np.longdouble(dt)), abs(np.longdouble(damping))
    a_dt = np.abs(a.astype(np.longdouble)) * dt_
    bound_v = damp * (dt_ * tol * size.astype(np.longdouble)[:, None] + 2 * u * (np.abs(xyz(vel).astype(np.longdouble)) + a_dt))
    bound_p = dt_ * bound_v + 2 * u * (np.abs(xyz(pos).astype(np.longdouble)) + np.abs(v1) * dt_)
    return v1, p1, bound_v, bound_p


def check_step(got_pos, got_vel, pos, vel, dt, damping, eps2, what):
    dtype = pos.dtype.type
    v1, p1, bound_v, bound_p = step_bounds(pos, vel, dt, damping, eps2, TOL[dtype], UNIT_ROUNDOFF[dtype])
    assert np.isfinite(v1).all() and np.isfinite(p1).all(), f"{what}: the yardstick itself is not finite"
    err_v = np.abs(xyz(got_vel).astype(np.longdouble) - v1)
    err_p = np.abs(xyz(got_pos).astype(np.longdouble) - p1)
    with np.errstate(all="ignore"):
        ratio_v, ratio_p = np.nan_to_num(err_v / bound_v, nan=np.inf), np.nan_to_num(err_p / bound_p, nan=np.inf)
    worst_v, worst_p = np.unravel_index(np.argmax(ratio_v), ratio_v.shape), np.unravel_index(np.argmax(ratio_p), ratio_p.shape)
    assert (err_v <= bound_v).all(), f"{what}: velocity {float(ratio_v[worst_v]):.3g} x its bound at body {worst_v[0]}"
    assert (err_p <= bound_p).all(), f"{what}: position {float(ratio_p[worst_p]):.3g} x its bound at body {worst_p[0]}"
    n = pos.size // 4
    assert got_pos.reshape(n, 4)[:, 3].tobytes() == pos.reshape(n, 4)[:, 3].tobytes(), f"{what}: masses changed"
    assert got_vel.reshape(n, 4)[:, 3].tobytes() == vel.reshape(n, 4)[:, 3].tobytes(), f"{what}: velocity .w changed"


def eps2_of(dtype, softening):
    """softening^2 as BodySystemHIP sets it: T(float(softening)) squared in T"""
    s = dtype(np.float32(softening))
    return s * s


def test_yardstick_matches_the_cpu_path(oracle):
    """The yardstick against the reference's own fp64 step (oracle.update): equal to fp64 rounding -- the CPU path's sums of n
    terms held to n u F_i -- at damping != 1 and dt of both signs; and too tight to let a step that drops the damping pass."""
    u = 2.0 ** -53
    for n, seed, dt, damping in ((64, 1, 0.016, 0.995), (200, 2, -0.016, 0.5), (129, 3, 0.0019, 0.9), (97, 4, -0.0006, 1.0)):
        oracle.srand(seed)
        pos, vel = oracle.randomise(seed % 3, n, 1.54, 8.0, np.float64)
        pos.reshape(n, 4)[:, 3] = np.linspace(0.5, 2.0, n)
        vel.reshape(n, 4)[:, 3] = 0.25  # (the CPU path keeps .w too)
        eps2 = oracle.softening_sq(0.1, np.float64)
        dt64, damp64 = np.float64(np.float32(dt)), np.float64(np.float32(damping))
        got_p, got_v = pos.copy(), vel.copy()
        oracle.update(got_p, got_v, dt, steps=1, softening=0.1, damping=damping)
        v1, p1, bound_v, bound_p = step_bounds(pos, vel, dt64, damp64, eps2, (n + 8) * u, u)
        assert (np.abs(xyz(got_v) - v1) <= bound_v).all(), (n, dt, damping)
        assert (np.abs(xyz(got_p) - p1) <= bound_p).all(), (n, dt, damping)
        if damping != 1:
            v_undamped = yardstick(pos, vel, dt64, 1.0, eps2)[2]
            assert not (np.abs(xyz(got_v) - v_undamped) <= bound_v).all()


# ---------------------------------------------------------------------------------------------- the paths under test
def one_sided(plan):
    def run(gpu, pos, vel, dt, params):
        gpu.set_plan_override(*plan)
        try:
            return run_gpu(gpu, pos, vel, 1, gpu.NB_MODE_FAST, dt=dt, params=params)
        finally:
            gpu.set_plan_override(0, 0, 0)
    return run


def shard_chain(cuts, plan=(2, 8, 1024)):
    """the step as a chain of shard launches over the j chunks [cuts[k], cuts[k+1]) (NB_SHARD_ACC_IN, NB_SHARD_FINALIZE on the
    last), the tile layout forced: each launch expresses its sums in units of ITS first body's mass"""
    def run(gpu, pos, vel, dt, params):
        n, dtype = pos.size // 4, pos.dtype.type
        lib = gpu.lib()
        gpu.set_softening_squared(eps2_of(dtype, params.softening))
        fn = lib.nb_integrate_shard_f32 if dtype == np.float32 else lib.nb_integrate_shard_f64
        d_old, d_new, d_vel, d_acc = (gpu.DeviceBuffer(pos.nbytes) for _ in range(4))
        d_old.upload(pos), d_vel.upload(vel)
        ends = [c for c in cuts if c < n] + [n]
        gpu.set_plan_override(*plan)
        try:
            for k, (a, b) in enumerate(zip(ends[:-1], ends[1:])):
                flags = (gpu.NB_SHARD_ACC_IN if k else 0) | (gpu.NB_SHARD_FINALIZE if b == n else 0)
                gpu.check(fn(d_new.ptr, d_old.ptr, d_vel.ptr, d_acc.ptr, 0, n, a, b - a, flags, dtype(dt), dtype(np.float32(params.damping)), 256, gpu.NB_MODE_FAST, None), "nb_integrate_shard")
            out = d_new.download(np.zeros_like(pos)).copy(), d_vel.download(np.zeros_like(vel)).copy()
        finally:
            gpu.set_plan_override(0, 0, 0)
            for buf in (d_old, d_new, d_vel, d_acc):
                buf.free()
        return out
    return run


def pairwise(plan, slices=0):
    def run(gpu, pos, vel, dt, params):
        with sliced(gpu, slices, plan):
            p = gpu.pair_plan(pos.size // 4, pos.dtype)
            assert p.applies == 1 and (p.slices >= 2 if slices else p.slices == 1), (plan, slices, p.slices)
            return run_gpu(gpu, pos, vel, 1, gpu.NB_MODE_FAST, dt=dt, params=params, workspace=True)
    return run


PATHS = {
    "one-sided": one_sided((0, 0, 0)),
    "one-sided wave-split": one_sided((0, 64, 0)),
    "one-sided tiles": one_sided((2, 8, 1024)),
    "one-sided tiles 16 waves": one_sided((4, 16, 2048)),
    "shard chain": shard_chain([0, 700, 1301, 1302, 1900]),
    "pairwise R=1": pairwise((1, 8, 1)),
    "pairwise R=2": pairwise((2, 8, 1)),
    "pairwise R=8": pairwise((8, 8, 1)),
    "pairwise 2 slices": pairwise((2, 8, 1), 2),
    "pairwise 3 slices": pairwise((1, 4, 2), 3),
}


def check_all_paths(gpu, pos, vel, dt, params, what):
    dtype = pos.dtype.type
    dt = dtype(np.float32(dt))
    damping = dtype(np.float32(params.damping))
    eps2 = eps2_of(dtype, params.softening)
    for name, run in PATHS.items():
        got_pos, got_vel = run(gpu, pos, vel, dt, params)
        check_step(got_pos, got_vel, pos, vel, dt, damping, eps2, f"{what}, {name}")


# ---------------------------------------------------------------------------------------------- a. parameters
@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("row", range(7))
def test_fast_demo_rows(gpu, oracle, dtype, row):
    """All seven demo parameter rows of the reference (their dt, softening, cluster and velocity scales) from random, shell and
    expand starts."""
    params = gpu.DEMO_PARAMS[row]
    for config in (0, 1, 2):
        oracle.srand(100 * row + config)
        pos, vel = oracle.randomise(config, N, params.cluster_scale, params.velocity_scale, dtype)
        check_all_paths(gpu, pos, vel, params.time_step, params, f"row {row} config {config}")


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dt,damping", [(0.016, 0.995), (0.016, 0.5), (0.0, 0.995), (-0.016, 0.5), (-0.0019, 1.0)])
def test_fast_damping_dt_and_velocity_w(gpu, oracle, dtype, dt, damping):
    """Damping != 1, dt = 0 (then p1 == p0 bitwise, v1 == v0 damping), negative dt; masses from 0.5 to 2 and a nonzero velocity
    .w (the tipsy softening slot) that must come through untouched."""
    oracle.srand(17)
    pos, vel = oracle.randomise(1, N, 1.54, 8.0, dtype)
    pos.reshape(N, 4)[:, 3] = np.linspace(0.5, 2.0, N).astype(dtype)
    vel.reshape(N, 4)[:, 3] = np.random.default_rng(3).uniform(0.01, 0.5, N).astype(dtype)
    params = gpu.NBodyParams(softening=0.1, damping=damping)
    check_all_paths(gpu, pos, vel, dt, params, f"dt {dt} damping {damping}")
    if dt == 0:
        damp = dtype(np.float32(damping))
        for name, run in PATHS.items():
            got_pos, got_vel = run(gpu, pos, vel, dtype(0), params)
            assert got_pos.tobytes() == pos.tobytes(), name
            assert np.array_equal(xyz(got_vel), xyz(vel) * damp), name


# ---------------------------------------------------------------------------------------------- b. STRICT's window, for FAST
def strict_window_cases(dtype):
    """the systems of test_gpu_parity.test_strict_fast_form_window_edges_bitwise, cases (a)-(e), drawn the same way"""
    rng = np.random.default_rng(7)
    n = 128 * 9 + 17
    f32 = dtype == np.float32
    cexp, mexp = (18, 40) if f32 else (100, 100)
    ulp = 2.0 ** -23 if f32 else 2.0 ** -52
    soft_lo, soft_hi = (2.0 ** -39, 2.0 ** 38) if f32 else (2.0 ** -100, 2.0 ** 100)

    def system(coord_scale, mass_lo, mass_hi):
        pos = np.zeros((n, 4), dtype)
        pos[:, :3] = (rng.uniform(-1, 1, (n, 3)) * coord_scale).astype(dtype)
        pos[:, 3] = (2.0 ** rng.uniform(mass_lo, mass_hi, n)).astype(dtype)
        vel = (rng.standard_normal((n, 4)) * 0.1).astype(dtype)
        vel[:, 3] = 0
        return pos, vel

    cases = []
    pos, vel = system(2.0 ** cexp, -mexp, mexp)
    pos[0, :3], pos[1, :3] = 2.0 ** cexp, -(2.0 ** cexp)
    pos[2, 3], pos[3, 3] = 2.0 ** -mexp, 2.0 ** mexp
    cases.append(("edges", pos, vel, 0.1))
    pos, vel = system(100.0, -3, 3)
    pos[128 * 2 + 5, 0] = dtype(2.0 ** cexp) * dtype(1 + ulp)
    pos[128 * 4 + 1, 3] = 2.0 ** (mexp + 1)
    pos[128 * 6 + 9, 3] = -0.0
    pos[128 * 7 + 2, 3] = 0.0
    pos[128 * 8 + 3, 3] = -1.5
    cases.append(("mixed chunks", pos, vel, 0.1))
    pos, vel = system(1.0, -2, 2)
    pos[1::2, :3] = pos[0::2, :3][: pos[1::2].shape[0]] + dtype(2.0 ** -70)
    pos[5, :3] = pos[4, :3] * dtype(1 + ulp)
    cases.append(("tiny separations", pos, vel, float(np.sqrt(np.float32(soft_lo))) if f32 else 2.0 ** -50))
    pos, vel = system(10.0, -2, 2)
    cases.append(("softening below window", pos, vel, 2.0 ** -21 if f32 else 2.0 ** -60))
    cases.append(("softening above window", pos, vel, 2.0 ** 19.5 if f32 else 2.0 ** 60))
    pos, vel = system(2.0 ** min(cexp, 18), 0, 0)
    pos[:, 3] = 1
    pos[0, :3], pos[1, :3] = 2.0 ** min(cexp, 18), -(2.0 ** min(cexp, 18))
    pos[128 * 1 + 63, 3] = dtype(1) + dtype(ulp)
    pos[128 * 3 + 0, 3] = dtype(1) - dtype(ulp / 2)
    pos[128 * 5 + 31, 3] = 2
    pos[128 * 7 + 7, 3] = -1
    cases.append(("unit-mass chunks among others", pos, vel, 0.1))
    pos, vel = system(1.0, 0, 0)
    pos[:, 3] = 1
    pos[1::2, :3] = pos[0::2, :3][: pos[1::2].shape[0]] + dtype(2.0 ** -70)
    cases.append(("unit masses, tiny separations", pos, vel, float(np.sqrt(np.float32(soft_lo))) if f32 else 2.0 ** -50))
    cases.append(("unit masses, softening at the upper edge", pos, vel, float(np.sqrt(np.float32(soft_hi))) * 0.999 if f32 else 2.0 ** 49))
    return cases


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fast_on_strict_window_cases(gpu, dtype):
    """STRICT's window-edge systems (coordinates and masses on the edges, chunks just outside, tiny separations, softening at and
    beyond the window, unit-mass chunks among others): FAST to the yardstick's bounds instead of 0 ulp."""
    for name, pos, vel, softening in strict_window_cases(dtype):
        check_all_paths(gpu, pos.reshape(-1).copy(), vel.reshape(-1).copy(), 0.016, gpu.NBodyParams(softening=softening, damping=0.999), name)


def shell_bodies(oracle, dtype, n=N, seed=23):
    oracle.srand(seed)
    pos, vel = oracle.randomise(1, n, 1.54, 8.0, dtype)
    pos.reshape(n, 4)[:, 3] = np.linspace(0.5, 2.0, n).astype(dtype)
    return pos, vel


@gpu_only
@pytest.mark.parametrize("dtype,e", [(np.float32, e) for e in (20, -20, 21, -21, 40, -40)] + [(np.float64, e) for e in (60, -60, 61, -61)])
def test_fast_reference_mass_at_the_unit_window(gpu, oracle, dtype, e):
    """The mass the kernels keep their sums in units of (the first body of a j range; a tile's species) on the edge of the window a
    unit is taken from (usable_unit, nbody_lane.h: 2^+-20 in fp32, 2^+-60 in fp64) and just outside it, and in fp32 at STRICT's mass
    edges 2^+-40: the first body alone, and the whole system one species."""
    params = gpu.NBodyParams(softening=0.1, damping=0.995)
    pos, vel = shell_bodies(oracle, dtype)
    pos.reshape(N, 4)[0, 3] = dtype(2.0 ** e)
    check_all_paths(gpu, pos, vel, 0.016, params, f"first body 2^{e}")
    pos.reshape(N, 4)[:, 3] = dtype(2.0 ** e)
    check_all_paths(gpu, pos, vel, 0.016, params, f"species 2^{e}")


@gpu_only
@pytest.mark.parametrize("dtype,mexp", [(np.float32, 40), (np.float32, 60), (np.float64, 60), (np.float64, 100)])
def test_fast_contiguous_species_at_opposite_mass_edges(gpu, oracle, dtype, mexp):
    """Contiguous species of masses 2^mexp and 2^-mexp taking turns, borders inside tiles, chunks and blocks: the pairwise kernel
    re-expresses its sums at every change of species (ratios 2^+-2mexp), the one-sided kernel scales whole chunks."""
    pos, vel = shell_bodies(oracle, dtype, seed=29)
    borders = [0, 300, 371, 700, 1090, 1500, 1501, 1800, N]
    m = pos.reshape(N, 4)[:, 3]
    for k, (a, b) in enumerate(zip(borders[:-1], borders[1:])):
        m[a:b] = dtype(2.0 ** (mexp if k % 2 else -mexp))
    check_all_paths(gpu, pos, vel, 0.016, gpu.NBodyParams(softening=0.1, damping=0.995), f"species 2^+-{mexp}")


def close_pair_system(dtype, lo):
    """A small reference mass against heavy bodies at the softening floor: 128 bodies of mass 2^lo spread out, then two clumps of
    heavy bodies (one species, then mixed masses) of the largest mass of STRICT's window a distance eps/sqrt(2) apart -- each heavy
    body feels ~2 000 coherent terms of the largest size the window allows: in units of 2^-40, far beyond fp32's range."""
    f32 = dtype == np.float32
    hi, eps2_exp = (40, -39) if f32 else (100, -100)
    n = 4096
    rng = np.random.default_rng(31)
    pos = np.zeros((n, 4), dtype)
    vel = np.zeros((n, 4), dtype)
    pos[:128, :3] = rng.uniform(0.5, 1.0, (128, 3)).astype(dtype)
    pos[:128, 3] = dtype(2.0 ** lo)
    half = (n - 128) // 2
    pos[128 + half:, 0] = dtype(2.0 ** ((eps2_exp - 1) / 2))  # eps / sqrt(2): where d / (d^2 + eps^2)^(3/2) peaks
    pos[128:, 3] = dtype(2.0 ** hi)
    pos[128 + half + 1::2, 3] = dtype(2.0 ** hi) * dtype(1 - UNIT_ROUNDOFF[dtype])  # the second clump's masses mixed
    vel[:, :3] = (rng.standard_normal((n, 3)) * 0.1).astype(dtype)
    softening = float(np.sqrt(np.float32(2.0 ** eps2_exp))) if f32 else 2.0 ** (eps2_exp / 2)
    return pos.reshape(-1), vel.reshape(-1), softening


@gpu_only
@pytest.mark.parametrize("dtype,lo", [(np.float32, -40), (np.float32, -20), (np.float64, -60)])
def test_fast_small_reference_mass_against_heavy_close_pairs(gpu, dtype, lo):
    """The reference-mass headroom: a first body (and a first tile) of mass 2^lo while heavy bodies (fp32: 2^40) sit at the softening
    floor of STRICT's window (eps^2 = 2^-39).  fp32 2^-40 overflowed while sums could be kept in units of it; 2^-20 is the smallest
    unit the window still admits.  The exact result and every intermediate of the reference formula are finite and normal, so FAST
    must meet the bound."""
    pos, vel, softening = close_pair_system(dtype, lo)
    check_all_paths(gpu, pos, vel, 0.016, gpu.NBodyParams(softening=softening, damping=0.995), "small reference mass, heavy close pairs")


# ---------------------------------------------------------------------------------------------- c. the coupling across the exponent range
# Measured maxima (MI355X) of the relative error of ONE term m d / (d^2 + eps^2)^(3/2) against the exact term rounded to T, and of
# the energy kernel's pair potential; the bars are twice these and never looser than 1e-6 (fp32) / 1e-14 (fp64).
COUPLING_MEASURED = {
    ("float32", "unit"): 3.489e-7, ("float32", "uniform"): 3.489e-7, ("float32", "mixed"): 3.489e-7,
    ("float64", "unit"): 4.402e-16, ("float64", "uniform"): 4.402e-16, ("float64", "mixed"): 6.303e-16,
}
ENERGY_MEASURED = {"float32": 1.122e-7, "float64": 2.382e-16}
# The same pair potential with both bodies off the origin (the probe pairs of tests/test_energy_domain.py: a cloud in [-1, 1]^3, so the
# coordinate differences round too), eps^2 = 0.01 and 0; the maximum over nb_energy_* and nb_energy_ensemble_* at every size of that
# module's MI355X run.  Not a bar of its own: those tests are held to min(2 x ENERGY_MEASURED, CAP) as the sweep below is.
ENERGY_PROBE_MEASURED = {"float32": 1.675e-7, "float64": 3.359e-16}
CAP = {"float32": 1e-6, "float64": 1e-14}


def sweep_probes(dtype):
    """[(eps^2, squared distances)]: eps = 0 over the whole range, and eps-dominated launches (d^2 from eps^2 2^-24 to eps^2);
    mantissas off the powers of two, every d^2 + eps^2 inside the range"""
    f32 = dtype == np.float32
    top, step = (84, 0.25) if f32 else (600, 2.0)
    rng = np.random.default_rng(41)
    whole = 2.0 ** np.arange(-top, top, step)
    out = [(0.0, whole * rng.uniform(1.0, 2.0, whole.size))]
    for e in ((-80, -40, 0, 40, 80) if f32 else (-600, -200, 0, 200, 600)):
        near = 2.0 ** (e + np.arange(-24, 0, 0.5))
        out.append((2.0 ** e, near * rng.uniform(1.0, 2.0, near.size)))
    return out


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("form", ["unit", "uniform", "mixed"])
def test_fast_coupling_across_the_exponent_range(gpu, dtype, form):
    """K bodies i against ONE full chunk of 64 bodies j (tile layout, 64 bodies j per wave and chunk) of which one sits at the origin
    and 63 so far away (2^62 fp32, 2^400 fp64) that their coupling underflows to exactly 0: every body i's sum holds a single nonzero
    term, so no summation rounding is left and the result is held to the exact term rounded to T.  fp32 d^2 in 2^+-84, fp64 2^+-600,
    eps = 0 and eps-dominated, through the chunk forms kUnit (every mass the reference mass), kUniform (one species in a chunk of its
    own, after a chunk of zero masses) and kMixed (the far bodies' masses differ)."""
    ch = 64
    name = np.dtype(dtype).name
    far = 2.0 ** (62 if dtype == np.float32 else 400)
    worst = 0.0
    for eps2, d2 in sweep_probes(dtype):
        d = np.sqrt(d2 / 1.25)  # (the body i sits at (d, d/2, 0))
        k = d.size
        nj = ch if form != "uniform" else 2 * ch
        near = nj - ch  # the one body j that counts: first of its chunk
        pos = np.zeros((nj + k, 4), dtype)
        pos[:nj, 0] = dtype(far)
        pos[near, 0] = 0
        pos[:, 3] = dtype(1.5)
        if form == "uniform":
            pos[:ch, 3] = 0
        if form == "mixed":
            pos[near + 1:nj:2, 3] = dtype(0.75)
            pos[near + 2:nj:2, 3] = dtype(3.0)
        pos[nj:, 0] = d.astype(dtype)
        pos[nj:, 1] = (d * 0.5).astype(dtype)
        flat = pos.reshape(-1).copy()
        gpu.set_softening_squared(dtype(eps2))
        gpu.set_plan_override(2, 8, 512)
        try:
            assert gpu.plan(k, nj, dtype).tile_bodies // 8 == ch
            acc = gpu_accel(gpu, flat, dtype, nj, k, 0, nj, gpu.NB_MODE_FAST)
        finally:
            gpu.set_plan_override(0, 0, 0)
        # (the far bodies' exact terms are below 2^-40 (fp32) / 2^-200 (fp64) of the near body's: left out of the yardstick)
        p = pos.astype(np.longdouble)
        r2 = p[nj:, 0] ** 2 + p[nj:, 1] ** 2 + np.longdouble(dtype(eps2))
        want = (-p[near, 3] * p[nj:, :2] / (r2 * np.sqrt(r2))[:, None]).astype(dtype).astype(np.longdouble)
        got = xyz(acc)[nj:, :2].astype(np.longdouble)
        err = np.sqrt(((got - want) ** 2).sum(axis=1)) / np.sqrt((want ** 2).sum(axis=1))  # (long double: no overflow at 2^+-600)
        assert np.isfinite(err).all(), (eps2, d2[~np.isfinite(err)][:4])
        worst = max(worst, float(err.max()))
    print(f"coupling {name} {form}: max relative error of one term {worst:.3e}")
    assert worst <= min(2 * COUPLING_MEASURED[(name, form)], CAP[name]), worst


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_energy_pair_potential_across_the_exponent_range(gpu, dtype):
    """nb_energy_* on two-body systems: the potential against -m1 m2 / sqrt(d^2 + eps^2) over the same range."""
    name = np.dtype(dtype).name
    worst = 0.0
    work = gpu.DeviceBuffer(gpu.energy_workspace_bytes(2))
    d_pos, d_vel = gpu.DeviceBuffer(8 * np.dtype(dtype).itemsize), gpu.DeviceBuffer(8 * np.dtype(dtype).itemsize)
    d_vel.upload(np.zeros(8, dtype))
    try:
        for eps2, d2 in sweep_probes(dtype):
            gpu.set_softening_squared(dtype(eps2))
            for dd in d2[:: 4 if dtype == np.float32 else 2]:
                x = dtype(np.sqrt(dd / 1.25))
                pos = np.array([0, 0, 0, 1.5, x, x * dtype(0.5), 0, 0.75], dtype)
                d_pos.upload(pos)
                e = gpu.energy(d_pos.ptr, d_vel.ptr, 2, dtype, workspace=work)
                r2 = np.longdouble(x) ** 2 + np.longdouble(x * dtype(0.5)) ** 2 + np.longdouble(dtype(eps2))
                want = -np.longdouble(1.5) * np.longdouble(0.75) / np.sqrt(r2)
                err = float(abs((np.longdouble(e["potential"]) - want) / want))
                assert np.isfinite(err), (eps2, dd, e["potential"])
                worst = max(worst, err)
    finally:
        work.free(), d_pos.free(), d_vel.free()
    print(f"energy {name}: max relative error of the pair potential {worst:.3e}")
    assert worst <= min(2 * ENERGY_MEASURED[name], CAP[name]), worst


# ---------------------------------------------------------------------------------------------- d. non-finite inputs
def nonfinite_bodies(pos, vel):
    return ~(np.isfinite(xyz(pos)).all(axis=1) & np.isfinite(xyz(vel)).all(axis=1))


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", ["eps 0", "eps 0, no ragged block", "NaN coordinate", "inf mass first", "NaN mass", "inf mass last", "NaN velocity"])
def test_fast_nonfinite_where_strict_is(gpu, oracle, dtype, case):
    """Non-finite inputs are ordinary data: every FAST path gives non-finite results at exactly the bodies where STRICT does (eps = 0:
    every body's self term is 0 * inf; a NaN coordinate or an inf / NaN mass reaches every body; a NaN velocity only its own), and
    the masses come through bit for bit."""
    n = 2048 if case == "eps 0, no ragged block" else N
    pos, vel = shell_bodies(oracle, dtype, n=n, seed=37)
    p, v = pos.reshape(n, 4), vel.reshape(n, 4)
    softening = 0.0 if case.startswith("eps 0") else 0.1
    if case == "NaN coordinate":
        p[777, 1] = np.nan
    elif case == "inf mass first":
        p[0, 3] = np.inf
    elif case == "NaN mass":
        p[1000, 3] = np.nan
    elif case == "inf mass last":
        p[n - 1, 3] = -np.inf
    elif case == "NaN velocity":
        v[5, 2] = np.nan
    params = gpu.NBodyParams(softening=softening, damping=0.995)
    dt = dtype(np.float32(0.016))
    with np.errstate(all="ignore"):
        strict = nonfinite_bodies(*run_gpu(gpu, pos, vel, 1, gpu.NB_MODE_STRICT, dt=dt, params=params))
    assert strict.sum() == (1 if case == "NaN velocity" else n), strict.sum()
    for name, run in PATHS.items():
        got_pos, got_vel = run(gpu, pos, vel, dt, params)
        fast = nonfinite_bodies(got_pos, got_vel)
        assert np.array_equal(fast, strict), (name, np.flatnonzero(fast != strict)[:8])
        assert got_pos.reshape(n, 4)[:, 3].tobytes() == p[:, 3].tobytes(), name
