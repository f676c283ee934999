"""The 6th-order block and ensemble kernels over their operand range (the "Operand range" and "Range of h" paragraphs of
include/nbody_hip_hermite6_block.h, and include/nbody_hip_hermite6_ensemble.h's pointer to nbody_hip_hermite6.h), as
tests/test_hermite_domain.py holds hermite_eval, hermite_block_eval, field_eval, hermite6_eval and the 4th-order ensembles to theirs.

CPU part: the headers' constants; every system below has a long double reference whose results and sums of term magnitudes are finite
and normal in T; the corrector of csrc/hermite6_correct.inc restated in numpy T arithmetic, over the steps h = dt_max 2^-k the block
scheme admits: the crackle is finite and within the long double bound wherever h^3 is normal in T, and not finite where h^3 rounds to 0.
GPU part (MI355X):
  A. ONE term through hermite6_block_eval and hermite6_block_finish across the exponent range (ONE_TERM6_MEASURED);
  B. check_block6_stages_of with first bodies on and around the unit window, and species at opposite mass edges;
  C. the sums on both sides of their cap 2^126 |m_0| (2^1022 |m_0|);
  D. the levels on both sides of the range of dt_A, and init's want;
  E. the corrector with the deepest level's h on both sides of the range of h^3;
  F. an ensemble of three systems with first bodies of their own against the solo calls;
  G. the escape to plain units in one system of an ensemble;
  H. the per-system time steps at extreme magnitudes;
  I. non-finite inputs stay in their system, and go through a block step as the formulas say.
The references, bounds and device wrappers are those of the sister modules."""
import ctypes
import functools

import numpy as np
import pytest

from test_fast_domain import CAP, TOL, UNIT_ROUNDOFF
from test_hermite import LD, cloud
from test_hermite6 import Device as Device6
from test_hermite6 import check_eval as check_eval6
from test_hermite6 import reference6
from test_hermite6_block import Block6Device, aarseth6, check_block6_stages_of, correct6, corrector6_bounds, evaluate6_rows, predict6
from test_hermite6_block import fns as block6_fns
from test_hermite6_ensemble import Ensemble as Ensemble6
from test_hermite6_ensemble import same_bits
from test_hermite6_ensemble import solo_timestep as solo_timestep6
from test_hermite_block import first_levels, new_levels
from test_hermite_domain import (ONE_TERM_MEASURED, TIMESTEP6_ALLOWED, TIMESTEP6_CASES, WINDOW, acc_in_for, close_pair_system, formula_rows, header_text, mass_system,
                                 mass_values, norm, normal_in, one_sided_system, one_term, poisoned_system, probe_sets, probes, species_system, term_errors, timestep6_arrays,
                                 timestep6_rule, two_bodies)

gpu_only = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
N = 128 * 9 + 17  # tests/test_hermite_domain.py's: S = 8, a ragged last chunk and tile
N_SMALL = 200     # S = 1
ERR = 10001       # NB_ERR_INVALID_ARGUMENT

# The range of h (include/nbody_hip_hermite6.h, _hermite6_block.h): h^3, formed in T as (h h) h, is a normal T from 2^-42 (fp32) /
# 2^-340 (fp64) up; it rounds to 0 from 2^-50 / 2^-359 down.
H_NORMAL = {np.float32: -42, np.float64: -340}
H_ZERO = {np.float32: -50, np.float64: -359}
# A step so short that the predictor returns the stored x and v (v h is below half an ulp of x), with h^3 normal: section A
SHORT_STEP = {np.float32: 2.0 ** -40, np.float64: 2.0 ** -300}


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_the_block6_and_ensemble6_headers_state_the_window():
    """the twin of test_the_window_is_the_one_the_headers_state for the two headers that came after it"""
    f32, f64 = WINDOW[np.float32], WINDOW[np.float64]
    block = header_text("nbody_hip_hermite6_block.h")
    paragraph = block[block.index("Operand range."):block.index("Status.")]
    assert f"2^-{f32['unit']} <= |m_0| <= 2^{f32['unit']} (fp32; 2^+-{f64['unit']} fp64)" in paragraph
    assert f"2^{f32['sums']} min(1, |m_0|) (fp32) / 2^{f64['sums']} min(1, |m_0|) (fp64)" in paragraph
    assert "no escape to plain units" in paragraph and "[2^-250, 2^250]" in paragraph and 'nbody_hip_hermite6.h, "Operand range"' in paragraph
    assert '"Operand range"' in header_text("nbody_hip_hermite6_ensemble.h")
    # the range of h, in the three headers
    lo32, lo64 = -H_NORMAL[np.float32], -H_NORMAL[np.float64]
    solo, ens = header_text("nbody_hip_hermite6.h"), header_text("nbody_hip_hermite6_ensemble.h")
    assert f"2^-{lo32} <= |h| <= 2^42 (fp32) / 2^-{lo64} <= |h| <= 2^341 (fp64)" in solo and "must be a normal T" in solo and "must not be 0" not in solo
    assert f"|h| <= 2^{H_ZERO[np.float32]} / 2^{H_ZERO[np.float64]}" in solo and "c1 is infinite or NaN" in solo
    assert f"2^-{lo32} <= |dt| <= 2^42 (fp32) / 2^-{lo64} <= |dt| <= 2^341 (fp64)" in ens and "ends STALLED" in ens and "A dt of 0" not in ens
    assert f"2^-{lo32} <= q and dt_max <= 2^42 (fp32) / 2^-{lo64} <= q and dt_max <= 2^341 (fp64)" in paragraph
    assert "init, step and sync refuse parameters outside that range" in paragraph
    for dtype in DTYPES:  # ... and they are the format's: the cube of 2^H_NORMAL is normal, that of half of it is not; 2^H_ZERO's is 0
        h = dtype(2.0) ** dtype(H_NORMAL[dtype])
        assert cube(h) >= np.finfo(dtype).tiny and 0 < cube(h / 2) < np.finfo(dtype).tiny
        zero = dtype(2.0) ** dtype(H_ZERO[dtype])
        assert cube(zero) == 0 and cube(zero * 2) > 0
        assert np.isfinite(cube(dtype(2.0) ** dtype(42 if dtype == np.float32 else 341))) and np.isinf(cube(dtype(2.0) ** dtype(43 if dtype == np.float32 else 342)))


def cube(h):
    """h^3 as the corrector forms it in T"""
    with np.errstate(all="ignore"):
        return (h * h) * h


def own_acc(pos, eps2):
    """the bodies' own accelerations as an (n, 4) T array, from plain fp64 sums: what init stores, to 1e-13 or so -- the acc_in of a block
    step's evaluation"""
    return own_acc_and_size(pos, eps2)[0]


def own_acc_and_size(pos, eps2):
    """(own_acc, the largest sum of term magnitudes A_i = sum |m_j| |r| / s^3 of any body and component)"""
    x, m = pos[:, :3].astype(np.float64), pos[:, 3].astype(np.float64)
    acc, size = np.zeros_like(pos), 0.0
    for i in range(0, pos.shape[0], 256):
        r = x[None] - x[i:i + 256, None]
        s2 = (r * r).sum(axis=2) + np.float64(eps2)
        k = (m[None] / (s2 * np.sqrt(s2)))[:, :, None]
        acc[i:i + 256, :3] = (k * r).sum(axis=1)
        size = max(size, float((np.abs(k) * np.abs(r)).sum(axis=1).max()))
    return acc, size


def true_state(pos, vel, eps2):
    """(acc, jerk, snap) of every body as (n, 4) T arrays, from plain fp64 sums"""
    n = pos.shape[0]
    acc = own_acc(pos, eps2)
    x, v, a, m = pos[:, :3].astype(np.float64), vel[:, :3].astype(np.float64), acc[:, :3].astype(np.float64), pos[:, 3].astype(np.float64)
    with np.errstate(all="ignore"):
        js = [evaluate6_rows(x[i:i + 128], v[i:i + 128], a[i:i + 128], x, v, a, m, np.float64(eps2))[1:] for i in range(0, n, 128)]
    out = [acc]
    for q in (np.concatenate([q[0] for q in js]), np.concatenate([q[1] for q in js])):
        t = np.zeros_like(pos)
        t[:, :3] = q
        out.append(t)
    return out


def species6_system(dtype, mexp):
    """species_system for the block step, whose acc_in is the bodies' own acceleration: fp32 masses of 2^60 at distances of order 1 give
    accelerations of 2^67 and snap terms m a / r^3 beyond FLT_MAX, and 256-fold further apart the crackle's 60 tol A_i / h^3 still passes
    FLT_MAX at the steps the predicted coordinates allow: that system is spread out 4096-fold (accelerations of 2^43, as 2^+-40 has)"""
    pos, vel = species_system(dtype, mexp)
    if dtype == np.float32 and mexp == 60:
        pos[:, :3] *= 4096
    return pos, vel


SPECIES = [(np.float32, 40), (np.float32, 60), (np.float64, 60), (np.float64, 100)]


@functools.lru_cache(maxsize=None)
def species6_dt_max(name, mexp):
    """the largest power of two up to 1/8 that keeps every PREDICTED coordinate (the oldest body is 600 ticks = 2.35 dt_max behind)
    within 2^40 in fp32, as test_block_stages_with_species_at_opposite_mass_edges chooses it, with the snap and the crackle the stage
    test stores (4 |s| |j| / |a| at the most); (dt_max, the largest sum of term magnitudes A_i)"""
    pos, vel = species6_system(np.dtype(name).type, mexp)
    acc, jerk, snap = true_state(pos, vel, pos.dtype.type(0.01))
    a, j, s = (norm(q[:, :3].astype(np.float64)) for q in (acc, jerk, snap))
    with np.errstate(all="ignore"):
        c = np.where(a > 0, s * j / a, 1.0)
    a, j, s, c = own_acc_and_size(pos, pos.dtype.type(0.01))[1], j.max(), s.max(), 4 * c.max()
    dt_max = 0.125
    while pos.dtype == np.float32:
        t = 2.35 * dt_max
        if 2.0 ** 16 + 2 * t + a * t ** 2 / 2 + j * t ** 3 / 6 + s * t ** 4 / 24 + c * t ** 5 / 120 <= 2.0 ** 40:
            break
        dt_max /= 2
    return dt_max, a


def sample_rows(n):
    """every 9th body, the bodies round every border of species_system and the last one"""
    borders = [b + d for b in (0, 300, 371, 640, 897, 1024, 1025, 1100, n - 1) for d in (-1, 0, 1)]
    return np.array(sorted({i for i in list(range(0, n, 9)) + borders if 0 <= i < n}))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_block6_systems_have_finite_normal_references(dtype):
    """Sections B, E, F and I: the first-body systems, the species and the clean poisoned system with the bodies' own accelerations as
    acc_in (what a block step's evaluation sees, to the predictor's move): the acceleration of EVERY body is finite and normal in T, and
    on a sample of the bodies so are the long double a, jerk, snap and the sums of their term magnitudes, none of which passes the block
    header's cap 2^sums min(1, |m_ref|).  The three systems of section F also with acc_in_for's acc_in.  The species' dt_max leaves the
    deepest step's cube normal and the crackle's 60 tol A_i / h^3 far below the largest T."""
    win = WINDOW[dtype]
    systems = [(f"first {value}", *mass_system(dtype, N, "first", value)) for value in mass_values(dtype)]
    systems += [(f"species 2^+-{mexp}", *species6_system(dtype, mexp)) for t, mexp in SPECIES if t == dtype]
    systems += [("poisoned, clean", *poisoned_system(dtype)[:2]), ("small", *mass_system(dtype, N_SMALL, "first", 1.0))]
    for what, pos, vel in systems:
        eps2, rows = dtype(0.01), sample_rows(pos.shape[0])
        acc = own_acc(pos, eps2)
        assert normal_in(dtype, acc[:, :3]).all() and acc[:, :3].any(axis=1).all(), what
        m0 = abs(float(pos[0, 3]))
        m_ref = m0 if 2.0 ** -win["unit"] <= m0 <= 2.0 ** win["unit"] else 1.0
        variants = [acc] + ([acc_in_for(pos)] if what in [f"first {v}" for v in (2.0 ** win["unit"], 2.0 ** -(win["unit"] + 1), 0.0)] else [])
        for acc_in in variants:
            ref = reference6(pos, vel, acc_in, eps2, rows=rows)
            for q in ref:
                assert normal_in(dtype, q).all(), what
            assert max(float(q.max()) for q in ref[3:]) <= 2.0 ** win["sums"] * min(1.0, m_ref), what
    for t, mexp in SPECIES:
        if t == dtype:
            dt_max, a = species6_dt_max(np.dtype(dtype).name, mexp)
            h = dt_max * 2.0 ** -8
            print(f"species 2^+-{mexp}: dt_max 2^{int(np.log2(dt_max))}, largest A_i 2^{np.log2(a):.1f}")
            # (the crackle's bound bc holds 60 tol A_i / h^3: a c1 within it must be representable)
            assert cube(dtype(h)) >= np.finfo(dtype).tiny and 60 * TOL[dtype] * a / LD(h) ** 3 < LD(np.finfo(dtype).max) / 2 ** 10, mexp


# ---- C: the close pairs of tests/test_hermite_domain.py through a block step -------------------------------------------------------------
# A block step evaluates the PREDICTED state, and every due body is at least one tick from its stored one.  fp32: a tick of 2^-40 moves
# no body (velocities up to 2^4).  fp64: the velocities that put S_i on 2^1022 are 2^353, and the shortest tick whose cube is normal,
# 2^-340, moves a body 2^13 -- the clumps, 2^-50 apart, cannot be held in a stored fp64 position then.  So the stored positions are
# the wanted ones moved BACK by v h (the predictor returns the wanted ones to an ulp of v h), and the largest fp64 velocities are those a
# legal step holds the clumps at: 2^-22 of section 3's (v h <= 2^-9: an ulp of 2^-62 against a softening length of 2^-50), S_i up to
# 2^977 = 2^15 beyond the block cap.
CAP_TICK = {np.float32: 2.0 ** -40, np.float64: 2.0 ** -340}
CAP_FASTEST = {np.float32: 1.0, np.float64: 2.0 ** -22}


def capped_velocities(name, lo):
    """close_pair_system(name, lo, 6) with its largest velocities (see above) and with them scaled by 2^(lo/2) rounded down to a power of
    two: the snap is quadratic in them, so S_i comes down from 2^126 (2^1022) to the block cap 2^126 |m_0| (2^1022 |m_0|)"""
    dtype = np.dtype(name).type
    pos, vel, eps2, scale = close_pair_system(name, lo, 6)
    fast, slow = vel.copy(), vel.copy()
    fast[:, :3] = vel[:, :3] * dtype(CAP_FASTEST[dtype])
    slow[:, :3] = vel[:, :3] * dtype(2.0 ** np.floor(lo / 2))
    return pos, fast, slow, eps2, scale


def moved_back(pos, vel, h):
    """the stored positions whose prediction over h is `pos`, to an ulp of v h"""
    out = pos.copy()
    out[:, :3] = (pos[:, :3].astype(LD) - vel[:, :3].astype(LD) * LD(h)).astype(pos.dtype)
    return out


@pytest.mark.parametrize("name,lo", [("float32", -20), ("float64", -60)])
def test_the_capped_close_pairs_have_finite_normal_references(name, lo):
    """Section C before it runs, on the state the predictor returns (restated: stored + v h, rounded to T): it is the wanted one to
    2^-10 of the softening length; with the scaled velocities every S_i is at or below the block cap and the largest within a factor
    16 of it, and every reference is finite and normal in T; with the largest velocities at least 64 bodies are under the cap and 64
    are 2^10 beyond it."""
    dtype = np.dtype(name).type
    pos, fast, slow, eps2, _ = capped_velocities(name, lo)
    cap = LD(2.0) ** (WINDOW[dtype]["sums"] + lo)
    zero, h = np.zeros_like(pos), CAP_TICK[dtype]
    assert cube(dtype(h)) >= np.finfo(dtype).tiny
    sizes = {}
    for what, vel in (("slow", slow), ("fast", fast)):
        predicted = pos.copy()
        predicted[:, :3] = (moved_back(pos, vel, h)[:, :3].astype(LD) + vel[:, :3].astype(LD) * LD(h)).astype(dtype)
        assert np.abs(predicted[:, :3].astype(LD) - pos[:, :3].astype(LD)).max() <= np.sqrt(LD(eps2)) * 2.0 ** -10, what
        ref = reference6(predicted, vel, zero, eps2)
        sizes[what] = ref[5].max(axis=1)
        if what == "slow":
            for q in ref:
                assert normal_in(dtype, q).all()
    assert cap / 16 < sizes["slow"].max() <= cap * (1 + 1e-6), float(np.log2(sizes["slow"].max()))
    assert (sizes["fast"] <= cap).sum() >= 64 and (sizes["fast"] > cap * 2.0 ** 10).sum() >= 64


# ---- D: two bodies whose derivatives sit at 2^e -----------------------------------------------------------------------------------------
def falling_pair(e):
    """Two fp64 bodies of 2^100 whose LARGEST derivative, the crackle after a step, is about 2^e.  Within the mass window a pair with
    |a| = 2^240 has a dynamical time of 2^-155 and every derivative is the one before it over that time, so the 6th-order norms cannot
    all sit at 2^240: the pair is r = 2^((253.6 - e) / 6.5) apart instead (e = 240: |a| 2^96, |j| 2^142, |s| 2^191, |c1| 2^240).
    (pos, vel, eps2, dt_max, eta_start): dt_max is a quarter of the dynamical time, eta_start puts init's want at 0.64 dt_max."""
    m, r = 2.0 ** 100, 2.0 ** ((253.6 - e) / 6.5)
    pos, vel = np.zeros((2, 4)), np.zeros((2, 4))
    pos[:, 3], pos[1, 0], vel[1, 1] = m, r, r / 8
    dt_max = 2.0 ** (np.floor(np.log2(np.sqrt(r ** 3 / m))) - 2)
    return pos, vel, np.float64(r * r * 2.0 ** -60), dt_max, 0.08 * dt_max


def level_case(e):
    """(pos, vel, eps2, dt_max, eta_start, eta) of section D: e > 0 the falling pair, e < 0 two_bodies of tests/test_hermite_domain.py"""
    if e > 0:
        return (*falling_pair(e), 0.002)
    return (*two_bodies(e), 0.125, 0.01, 0.2)


def ld_block_step_of_two(e, max_level=8):
    """the first block step of level_case(e) in long double: (levels after init, a1, j1, s1, c1)"""
    pos, vel, eps2, dt_max, eta_start, _ = level_case(e)
    x, v, m, z = pos[:, :3].astype(LD), vel[:, :3].astype(LD), pos[:, 3].astype(LD), np.zeros((2, 3), LD)
    a, j, _ = evaluate6_rows(x, v, z, x, v, z, m, LD(eps2))
    s = evaluate6_rows(x, v, a, x, v, a, m, LD(eps2))[2]
    k = first_levels(a, j, LD(eta_start), LD(dt_max), max_level)[0]
    h = (LD(dt_max) * LD(2.0) ** -k)[:, None]
    xp, vp, ap = predict6(x, v, a, j, s, z, h)
    a1, j1, s1 = evaluate6_rows(xp, vp, ap, xp, vp, ap, m, LD(eps2))
    return k, a1, j1, s1, correct6(x, v, a, j, s, a1, j1, s1, h)[2]


@pytest.mark.parametrize("e", [240, -240, 600, -600])
def test_the_level_cases_sit_where_they_should(e):
    """Section D before it runs: inside the range (|e| = 240) every norm of the step's a1, j1, s1, c1 is in [2^-250, 2^250] with the
    extreme one within 2^10 of 2^e, and the long double dt_A is not near a threshold; beyond it (|e| = 600) a square overflows (the
    crackle's: the plain fp64 expression is NaN or has an infinite denominator) or every square underflows; the tick's cube is normal."""
    pos, vel, eps2, dt_max, eta_start, eta = level_case(e)
    k, a1, j1, s1, c1 = ld_block_step_of_two(e)
    norms = np.array([np.log2(norm(q)).astype(np.float64) for q in (a1, j1, s1, c1)])
    extreme = norms.max() if e > 0 else norms.min()
    print(f"e {e}: levels {k}, log2 norms of a1, j1, s1, c1 {norms[:, 0]}, dt_max 2^{np.log2(dt_max)}")
    assert abs(extreme - e) < 10 and (k == 1).all()
    assert cube(np.float64(dt_max * 2.0 ** -8)) >= np.finfo(np.float64).tiny
    if abs(e) <= 250:
        assert (np.abs(norms) <= 250).all()
        dt_a = aarseth6(a1, j1, s1, c1, LD(eta), LD(dt_max))
        assert (new_levels(k, dt_a, 128, dt_max, 8)[1] > 1e-3).all()
    else:
        assert (2 * norms.max() > 1024) if e > 0 else (2 * norms.max() < -1080)


# ---- the h^3 range ----------------------------------------------------------------------------------------------------------------------
def fma_in(dtype, a, b, c):
    """fma in T through the next wider format (fp32: exact product in fp64; fp64: long double), one rounding to T but for double rounding"""
    wide = np.float64 if dtype == np.float32 else LD
    with np.errstate(all="ignore"):
        return (np.asarray(a, wide) * np.asarray(b, wide) + np.asarray(c, wide)).astype(dtype)


def correct6_in(dtype, x, v, a0, j0, s0, a1, j1, s1, h):
    """csrc/hermite6_correct.inc in numpy T arithmetic, operation for operation: (x1, v1, c1) from T-typed (n, 3) arrays and a T h"""
    T = dtype
    with np.errstate(all="ignore"):
        h = T(h)
        h2, hh = h * T(0.5), h * h
        t10, h3 = hh * T(0.1), hh * h
        t120 = h3 * (T(1) / T(120))
        v1 = v + fma_in(T, h2, a0 + a1, fma_in(T, t120, s0 + s1, -t10 * (j1 - j0)))
        x1 = x + fma_in(T, h2, v + v1, fma_in(T, t120, j0 + j1, -t10 * (a1 - a0)))
        d0 = fma_in(T, -h2 * h, s0, fma_in(T, -h, j0, a1 - a0))
        d1 = fma_in(T, -h, s0, j1 - j0) * h
        d2 = (s1 - s0) * hh
        c1 = fma_in(T, T(9), d2, fma_in(T, T(-36), d1, T(60) * d0)) / h3
    assert all(q.dtype == T for q in (x1, v1, c1))
    return x1, v1, c1


def smooth_pair(dtype, h):
    """A smooth two-body state and its exact continuation: masses 1 and 0.75 about 1.3 apart at softening^2 0.01, in T; the stored x,
    v, a0, j0, s0 (long double sums rounded to T), and a1, j1, s1 = the long double sums over the long double predicted state at h,
    rounded to T -- what an evaluation within its tolerance returns.  ((n, 3) arrays: x, v, a0, j0, s0, a1, j1, s1)"""
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.75, -0.375]], dtype)
    v = np.array([[0.125, -0.25, 0.0], [-0.5, 0.375, 0.25]], dtype)
    m, eps2, z = np.array([1.0, 0.75], LD), LD(dtype(0.01)), np.zeros((2, 3), LD)
    xl, vl = x.astype(LD), v.astype(LD)
    a0 = evaluate6_rows(xl, vl, z, xl, vl, z, m, eps2)[0].astype(dtype)
    _, j0, s0 = (q.astype(dtype) for q in evaluate6_rows(xl, vl, a0.astype(LD), xl, vl, a0.astype(LD), m, eps2))
    xp, vp, ap = (q.astype(dtype).astype(LD) for q in predict6(xl, vl, a0.astype(LD), j0.astype(LD), s0.astype(LD), z, LD(h)))
    a1, j1, s1 = (q.astype(dtype) for q in evaluate6_rows(xp, vp, ap, xp, vp, ap, m, eps2))
    return x, v, a0, j0, s0, a1, j1, s1


def crackle_check(dtype, h):
    """(finite, within bc, c1 in T, bc) of the restated corrector at step h against correct6 in long double from the same T-typed inputs;
    bc is corrector6_bounds' with the evaluation's tolerance on the pair's single term"""
    tol, u = LD(TOL[dtype]), LD(UNIT_ROUNDOFF[dtype])
    x, v, a0, j0, s0, a1, j1, s1 = smooth_pair(dtype, h)
    c1 = correct6_in(dtype, x, v, a0, j0, s0, a1, j1, s1, h)[2]
    ld = [q.astype(LD) for q in (x, v, a0, j0, s0, a1, j1, s1)]
    hl = np.full((2, 1), LD(dtype(h)))
    _, v1, want = correct6(*ld, hl)
    ba, bj, bs = (tol * np.abs(q) for q in ld[5:8])
    bc = corrector6_bounds(*ld, v1, hl, ba, bj, bs, u)[2]
    finite = bool(np.isfinite(c1).all())
    return finite, finite and bool((np.abs(c1.astype(LD) - want) <= bc).all()), c1, bc


def h_cases(dtype):
    """h = dt_max 2^-k, k = 0 .. 40, over the dt_max the block header admits: 1, 2^-3, 2^-10 and a dt_max that is no power of two
    (0.016) in both precisions; fp64 also 2^-300, 2^-305 (h down to 2^-345) and 2^-320 (the subnormal cubes and the first that are 0)"""
    tops = [1.0, 2.0 ** -3, 2.0 ** -10, 0.016] + ([2.0 ** -300, 2.0 ** -305, 2.0 ** -320, 0.016 * 2.0 ** -300] if dtype == np.float64 else [])
    return [top * 2.0 ** -k for top in tops for k in range(41)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_crackle_over_the_range_of_h(dtype):
    """The defect the range of h is stated for, on the CPU: wherever h^3 is a normal T the restated corrector's crackle is finite and
    within bc; where h^3 rounds to 0 it is not finite (x / 0); between the two -- a subnormal cube, which the headers give no bound for --
    it is finite here (counted, not asserted to be within bc).  The limits are the headers': 2^-42 / 2^-340 and 2^-50 / 2^-359."""
    tiny = np.finfo(dtype).tiny
    seen = {"normal": 0, "subnormal": 0, "subnormal outside bc": 0, "zero": 0}
    lowest_normal, highest_zero = np.inf, 0.0
    for h in h_cases(dtype):
        h3 = cube(dtype(h))
        finite, within, c1, bc = crackle_check(dtype, h)
        if h3 >= tiny:
            assert finite and within, (h, c1)
            seen["normal"] += 1
            lowest_normal = min(lowest_normal, h)
        elif h3 > 0:
            assert finite, (h, c1)
            seen["subnormal"] += 1
            seen["subnormal outside bc"] += not within
        else:
            assert not finite, (h, c1)
            seen["zero"] += 1
            highest_zero = max(highest_zero, h)
    print(f"{np.dtype(dtype).name}: {seen}; lowest h with a normal cube 2^{np.log2(lowest_normal):.2f}, highest h with a cube of 0 2^{np.log2(highest_zero):.2f}")
    assert seen["normal"] > 100 and seen["subnormal"] >= 8 and seen["zero"] >= 1
    assert 2.0 ** H_NORMAL[dtype] <= lowest_normal < 2.0 ** (H_NORMAL[dtype] + 1) and 2.0 ** (H_ZERO[dtype] - 1) < highest_zero <= 2.0 ** H_ZERO[dtype]
    # the legal fp32 call of the issue: dt_max = 2^-10 with max_level = 40 has a deepest step whose cube is 0
    if dtype == np.float32:
        assert not crackle_check(dtype, 2.0 ** -50)[0] and crackle_check(dtype, 2.0 ** -42)[1]


# ---------------------------------------------------------------------------------------------------------------- GPU
# A. Measured maxima (MI355X) of |got - want| over the term's magnitude, as ONE_TERM_MEASURED of tests/test_hermite_domain.py holds them.
# Acceleration and jerk are hermite_block_eval's figures to the digit (the same text streams them).  The snap is 0.46e-7 (fp32: 0.8 u)
# and 0.87e-16 (fp64: 0.8 u) above hermite6_eval's 3.617e-7 / 5.347e-16: the planes' divide and multiply by m_0, within the 2u they
# may add.  The bars are twice these, and never looser than CAP (acc) or TOL (jerk, snap).
ONE_TERM6_MEASURED = {  # (kernel, precision, output): the maximum over the layouts and probe sets
    ("hermite6_block_eval", "float32", "acc"): 3.483e-7, ("hermite6_block_eval", "float32", "jerk"): 3.739e-7, ("hermite6_block_eval", "float32", "snap"): 4.081e-7,
    ("hermite6_block_eval", "float64", "acc"): 4.801e-16, ("hermite6_block_eval", "float64", "jerk"): 4.986e-16, ("hermite6_block_eval", "float64", "snap"): 6.216e-16,
}


def bar6(name, output):
    limit = CAP[name] if output == "acc" else TOL[np.dtype(name).type]
    return min(2 * ONE_TERM6_MEASURED[("hermite6_block_eval", name, output)], limit)


def block6_sums(gpu, pos, vel, acc, eps2, h):
    """a1, j1, s1 of every body from ONE block step in which all bodies are due (max_level 0, tick 0, the stored acceleration `acc`,
    stored jerk = snap = crackle = 0), through the partial planes and the finish kernel, and the predicted state they are the sums of"""
    n = pos.shape[0]
    d = Block6Device(gpu, pos, vel, eps2, gpu.HermiteBlockParams(0.2, 0.01, h, 0, 0))
    d.put("acc", acc)
    d.step()
    status = d.status()
    assert (status.now_ticks, status.last_active, status.flags) == (1, n, 0)
    out = d.get("acc"), d.get("jerk"), d.get("snap"), d.get("ws")
    d.free()
    return out


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_term_block6(gpu, dtype):
    """hermite6_block_eval and hermite6_block_finish: the one-term sweep of test_one_term_block with the snap, the near body in a unit
    chunk (the nine planes are in units of its mass) and in a mixed one.  The probes' acc_in is the stored acceleration; the step is
    2^-40 / 2^-300, whose cube is normal."""
    name, h = np.dtype(dtype).name, SHORT_STEP[dtype]
    assert cube(dtype(h)) >= np.finfo(dtype).tiny
    worst = {}
    for eps2, d2 in probe_sets(dtype):
        pos_p, vel_p, acc_p = probes(dtype, d2)
        for layout in ("unit", "mixed"):
            pos, vel, acc = one_sided_system(dtype, layout, pos_p, vel_p, acc_p)
            a1, j1, s1, predicted = block6_sums(gpu, pos, vel, acc, dtype(eps2), h)
            # the sums are those of the PREDICTED state: the stored x, v and a, but for z = 0 + v_z h of the probes
            assert predicted[:, [0, 1, 3]].tobytes() == pos[:, [0, 1, 3]].tobytes() and predicted[:, 4:7].tobytes() == np.ascontiguousarray(vel[:, :3]).tobytes()
            assert predicted[:, 8:11].tobytes() == np.ascontiguousarray(acc[:, :3]).tobytes() and not predicted[:, 7].any() and not predicted[:, 11].any()
            assert not predicted[:128, 2].any() and (np.abs(predicted[128:, 2]) <= np.abs(pos_p[:, 0]) * h).all()
            terms, sizes, _ = one_term(dtype, predicted[128:, 0:4], predicted[128:, 4:8], predicted[128:, 8:12], eps2)
            for output, err in term_errors(dtype, dict(acc=a1[128:, :3], jerk=j1[128:, :3], snap=s1[128:, :3]), terms, sizes).items():
                assert np.isfinite(err).all(), (eps2, layout, output)
                worst[output] = max(worst.get(output, 0.0), float(err.max()))
    for output, value in worst.items():
        print(f"one term hermite6_block_eval {name} {output}: max error over the term's magnitude {value:.3e} (bar {bar6(name, output):.3e}; hermite6_eval "
              f"{ONE_TERM_MEASURED[('hermite6_eval', name, output)]:.3e})")
    for output, value in worst.items():
        assert value <= bar6(name, output), (output, value)


# ---- B ---------------------------------------------------------------------------------------------------------------------------------
@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(7))
def test_block6_stages_with_first_bodies_around_the_unit_window(gpu, dtype, index):
    """check_block6_stages_of on the first-body systems: the nine planes are in units of the first body's mass on the window's edge, in
    plain units just outside it and at 0, -0.0 and a negative mass; "planes added in range order, times m_ref" bit for bit on both sides"""
    value = mass_values(dtype)[index]
    pos, vel = mass_system(dtype, N, "first", value)
    check_block6_stages_of(gpu, pos, vel, dtype(0.01), 129, f"first {value}", 0.04)


@gpu_only
@pytest.mark.parametrize("dtype,mexp", SPECIES)
def test_block6_stages_with_species_at_opposite_mass_edges(gpu, dtype, mexp):
    """... and on the contiguous species (fp32 2^+-60: spread out, species6_system), with the dt_max of species6_dt_max"""
    pos, vel = species6_system(dtype, mexp)
    dt_max, _ = species6_dt_max(np.dtype(dtype).name, mexp)
    check_block6_stages_of(gpu, pos, vel, dtype(0.01), 129, f"species 2^+-{mexp}", 0.04, dt_max=dt_max)


# ---- C ---------------------------------------------------------------------------------------------------------------------------------
@gpu_only
@pytest.mark.parametrize("name,lo", [("float32", -20), ("float64", -60)])
def test_block6_sums_on_both_sides_of_their_cap(gpu, name, lo):
    """The nine planes are in units of the first body's mass with no escape to plain units: the header caps the sums of term magnitudes
    at 2^126 |m_0| (2^1022 |m_0|).  With the velocities that put S_i on that cap every body meets check_eval6's bound; with the largest
    ones the bodies under the cap still meet it, and the bodies 2^10 beyond it have infinite or NaN snaps, as the header says."""
    dtype = np.dtype(name).type
    pos, fast, slow, eps2, _ = capped_velocities(name, lo)
    cap = LD(2.0) ** (WINDOW[dtype]["sums"] + lo)
    zero, h = np.zeros_like(pos), CAP_TICK[dtype]
    a1, j1, s1, predicted = block6_sums(gpu, moved_back(pos, slow, h), slow, zero, eps2, h)
    assert np.abs(predicted[:, :3].astype(LD) - pos[:, :3].astype(LD)).max() <= np.sqrt(LD(eps2)) * 2.0 ** -10 and not predicted[:, 8:12].any()
    assert reference6(predicted[:, 0:4], predicted[:, 4:8], zero, eps2)[5].max() <= cap * (1 + 1e-6)
    check_eval6((a1, j1, s1), predicted[:, 0:4], predicted[:, 4:8], zero, eps2, f"block sums on their cap behind 2^{lo}")
    a1, j1, s1, predicted = block6_sums(gpu, moved_back(pos, fast, h), fast, zero, eps2, h)
    assert np.abs(predicted[:, :3].astype(LD) - pos[:, :3].astype(LD)).max() <= np.sqrt(LD(eps2)) * 2.0 ** -10
    size = reference6(predicted[:, 0:4], predicted[:, 4:8], zero, eps2)[5].max(axis=1)
    under, beyond = np.flatnonzero(size <= cap), np.flatnonzero(size > cap * 2.0 ** 10)
    assert under.size >= 64 and beyond.size >= 64
    check_eval6((a1, j1, s1), predicted[:, 0:4], predicted[:, 4:8], zero, eps2, f"block sums under their cap behind 2^{lo}", rows=under)
    assert not np.isfinite(s1[beyond, :3]).all(axis=1).any()


# ---- D ---------------------------------------------------------------------------------------------------------------------------------
def plain_norm(q):
    """|.| = sqrt(x^2 + y^2 + z^2) in plain fp64, as the header states it"""
    q = q.astype(np.float64)
    with np.errstate(all="ignore"):
        return np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2])


@gpu_only
@pytest.mark.parametrize("e", [240, -240, 600, -600])
def test_block6_levels_on_both_sides_of_the_range_of_dt_a(gpu, e):
    """init's want and the step's dt_A are plain fp64 expressions of products of two norms.  With every norm of a1, j1, s1, c1 inside
    [2^-250, 2^250] the levels are the long double rule's, recomputed from the GPU's stored a1, j1, s1, c1; with norms of 2^+-600 they
    are what the fp64 expression gives -- dt_max where it is NaN, the deepest level where an infinite denominator makes it 0 -- and never
    out of [0, max_level]."""
    pos, vel, eps2, dt_max, eta_start, eta = level_case(e)
    params = gpu.HermiteBlockParams(eta, eta_start, dt_max, 8, 0)
    d = Block6Device(gpu, pos, vel, eps2, params)
    d.init()
    acc, jerk, levels0 = d.get("acc"), d.get("jerk"), d.get("levels").astype(np.int64)
    assert all(np.isfinite(d.get(k)).all() for k in ("acc", "jerk", "snap", "crackle"))
    inside = abs(e) <= 250
    rule = first_levels(acc[:, :3].astype(LD), jerk[:, :3].astype(LD), LD(eta_start), LD(dt_max), 8)[0]
    with np.errstate(all="ignore"):
        want0 = eta_start * plain_norm(acc) / plain_norm(jerk)
    want0 = np.where(np.isfinite(want0) & (want0 > 0), want0, dt_max)
    plain = (dt_max * 2.0 ** -np.arange(8)[None, :] > want0[:, None]).sum(axis=1)
    assert (levels0 == plain).all() and (rule == 1).all(), (levels0, plain, rule)
    assert (plain == (0 if e == -600 else rule)).all()  # (2^-600: the squares underflow, 0 / 0: dt_max; 2^600 is the crackle's norm, |a|^2 and |j|^2 are in range)
    d.step()
    got = [d.get(k) for k in ("acc", "jerk", "snap", "crackle")]
    levels1, status = d.get("levels").astype(np.int64), d.status()
    d.free()
    assert status.last_active == 2 and all(np.isfinite(q).all() for q in got)
    norms = np.array([np.log2(norm(q[:, :3].astype(LD))).astype(np.float64) for q in got])
    if inside:
        assert (np.abs(norms) <= 250).all()
        dt_a = aarseth6(*(q[:, :3].astype(LD) for q in got), LD(eta), LD(dt_max))
    else:
        with np.errstate(all="ignore"):
            n_a, n_j, n_s, n_c = (plain_norm(q) for q in got)
            dt_a = np.sqrt(eta * (n_a * n_s + n_j * n_j) / (n_j * n_c + n_s * n_s))
        dt_a = np.where(np.isfinite(dt_a), dt_a, dt_max)
        # 2^600: |c|^2 overflows, the denominator is infinite and dt_A = 0 -- the header's "finite value that can be too small, down to 0
        # (the deepest level)", where the exact rule asks for level 4; 2^-600: every square underflows, 0 / 0, dt_max
        assert (dt_a == (0 if e > 0 else dt_max)).all()
        exact = aarseth6(*(q[:, :3].astype(LD) for q in got), LD(eta), LD(dt_max))
        assert e < 0 or (new_levels(levels0, exact, status.now_ticks, dt_max, 8)[0] == 4).all()
    want, rel = new_levels(levels0, dt_a, status.now_ticks, dt_max, 8)
    print(f"norms of 2^{e}: log2 norms {norms[:, 0]}, levels {levels0} -> {levels1}, dt_A / dt_max {(dt_a / dt_max).astype(np.float64)}, rule {want} (distance from a threshold {rel})")
    if inside:
        assert (rel > 1e-6).all()
    elif e > 0:
        assert (want == 8).all()
    assert (levels1 == want).all() and ((0 <= levels1) & (levels1 <= 8)).all()


# ---- E ---------------------------------------------------------------------------------------------------------------------------------
AT_THE_LIMIT = {np.float32: (2.0 ** -10, 32), np.float64: (2.0 ** -300, 40)}     # the tick is 2^-42 / 2^-340: its cube is the smallest normal one of a power of two
BELOW_THE_LIMIT = {np.float32: (2.0 ** -10, 33), np.float64: (2.0 ** -301, 40)}  # 2^-43 / 2^-341: refused


def smooth_system(dtype, n):
    if n == 2:
        pos, vel = np.zeros((2, 4), dtype), np.zeros((2, 4), dtype)
        pos[1, :3], pos[:, 3] = (1.0, 0.75, -0.375), (1.0, 0.75)
        vel[0, :3], vel[1, :3] = (0.125, -0.25, 0.0), (-0.5, 0.375, 0.25)
        return pos, vel
    return mass_system(dtype, n, "first", 1.0)


def check_corrected(stored, got, predicted, h, eps2, what):
    """the six arrays after a step of h from `stored` against long double: a1, j1, s1 to the evaluation's tolerance over the predicted
    state, x1, v1, c1 to corrector6_bounds; everything finite"""
    dtype = stored[0].dtype.type
    tol, u = LD(TOL[dtype]), LD(UNIT_ROUNDOFF[dtype])
    a1, j1, s1, mag_a, mag_j, mag_s = reference6(predicted[:, 0:4], predicted[:, 4:8], predicted[:, 8:12], eps2)
    x, v, a0, j0, s0 = (q[:, :3].astype(LD) for q in stored[:5])
    hl = np.full((x.shape[0], 1), LD(dtype(h)))
    x1, v1, c1 = correct6(x, v, a0, j0, s0, a1, j1, s1, hl)
    ba, bj, bs = tol * mag_a, tol * mag_j, tol * mag_s
    bx, bv, bc = corrector6_bounds(x, v, a0, j0, s0, a1, j1, s1, v1, hl, ba, bj, bs, u)
    for name, g, w, b in zip(("position", "velocity", "acceleration", "jerk", "snap", "crackle"), got, (x1, v1, a1, j1, s1, c1), (bx, bv, ba, bj, bs, bc)):
        assert np.isfinite(g).all(), (what, name)
        assert (np.abs(g[:, :3].astype(LD) - w) <= b).all(), (what, name)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [2, N_SMALL])
def test_the_corrector_on_both_sides_of_the_range_of_h(gpu, dtype, n):
    """The headers' "Range of h".  Block calls: with every body on the deepest level and a tick of 2^-42 (2^-340), the smallest power
    of two whose cube is normal, one block step leaves all eight arrays finite and c1 within bc; with a tick of 2^-43 (2^-341) init,
    step and sync refuse the parameters and touch nothing.  (fp64 takes the parameters fp32 refuses.)  nb_hermite6_step_*, which does
    not check: the same at the limit; at 2^-50 (2^-359), where the cube rounds to 0, every crackle is infinite or NaN and the rest
    finite, as the header says."""
    pos, vel = smooth_system(dtype, n)
    eps2 = dtype(0.01)
    dt_max, max_level = AT_THE_LIMIT[dtype]
    h = dt_max * 2.0 ** -max_level
    assert cube(dtype(h)) >= np.finfo(dtype).tiny > cube(dtype(h / 2)) and h == 2.0 ** H_NORMAL[dtype]
    params = gpu.HermiteBlockParams(0.2, 0.01, dt_max, max_level, 0)
    d = Block6Device(gpu, pos, vel, eps2, params, ws_fill=np.nan)
    d.init()
    d.put("levels", np.full(n, max_level, np.int32))
    stored = d.state()
    assert not stored[6].any() and all(np.isfinite(q).all() for q in stored[:6])
    d.step()
    got, predicted, status = d.state(), d.get("ws"), d.status()
    assert d.canaries_intact() and (status.now_ticks, status.last_active, status.flags, status.deepest_level) == (1, n, 0, max_level)
    check_corrected(stored, got, predicted, h, eps2, f"block step at 2^{H_NORMAL[dtype]}")
    assert (got[6] == 1).all() and ((0 <= got[7]) & (got[7] <= max_level)).all()
    # below the limit: refused by init, step and sync, before any launch
    f, scalar = block6_fns(gpu, dtype)
    before = d.everything()
    for bad in (gpu.HermiteBlockParams(0.2, 0.01, *BELOW_THE_LIMIT[dtype], 0), gpu.HermiteBlockParams(0.2, 0.01, 2.0 ** (43 if dtype == np.float32 else 342), 0, 0)):
        args = [d.ptr(k) for k in ("pos", "vel", "acc", "jerk", "snap", "crackle", "ticks", "levels", "status", "ws")] + [d.ws_bytes, n, scalar(eps2), ctypes.byref(bad)]
        assert f["init"](*args, None) == ERR and f["step"](*args, float("inf"), None) == ERR
        assert f["sync"](*[d.ptr(k) for k in ("pos_out", "vel_out", "pos", "vel", "acc", "jerk", "snap", "crackle", "ticks", "status")], n, ctypes.byref(bad), None) == ERR
    assert d.everything() == before
    d.free()
    if dtype == np.float64:  # what fp32 refuses is in range here
        d = Block6Device(gpu, pos, vel, eps2, gpu.HermiteBlockParams(0.2, 0.01, *BELOW_THE_LIMIT[np.float32], 0))
        d.init(), d.step()
        assert all(np.isfinite(q).all() for q in d.state()[:6])
        d.free()
    # the solo step does not check
    s = Device6(gpu, pos, vel, eps2)
    s.init()
    start = s.state()
    s.step(dtype(h), new="pos2", old="pos")
    check_corrected(start, s.state("pos2"), s.get("ws"), h, eps2, f"nb_hermite6_step at 2^{H_NORMAL[dtype]}")
    s.free()
    s = Device6(gpu, pos, vel, eps2)
    s.init()
    zero = dtype(2.0 ** H_ZERO[dtype])
    assert cube(zero) == 0
    s.step(zero, new="pos2", old="pos")
    after = s.state("pos2")
    s.free()
    assert not np.isfinite(after[5][:, :3]).any() and not after[5][:, 3].any() and all(np.isfinite(q).all() for q in after[:5])


# ---- F, G ------------------------------------------------------------------------------------------------------------------------------
@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_ensemble6_systems_with_first_bodies_of_their_own(gpu, dtype):
    """One launch of three systems whose first bodies weigh 2^20 (2^60), 2^-21 (2^-61: no unit) and 0; system 0 has a unit chunk of its
    own.  The unit mass is per system: eval with a non-zero acc_in, init, the time step and one step have the bits of the solo calls."""
    e = WINDOW[dtype]["unit"]
    systems = [mass_system(dtype, N, "first", value) for value in (2.0 ** e, 2.0 ** -(e + 1), 0.0)]
    systems[0][0][128:256, 3] = 2.0 ** e
    pos, vel = np.stack([s[0] for s in systems]), np.stack([s[1] for s in systems])
    acc_in = np.stack([acc_in_for(pos[s], 71 + s) for s in range(3)]).astype(dtype)
    eps2, dt, eta = dtype(0.01), dtype(1.0 / 128), dtype(0.02)
    ens = Ensemble6(gpu, pos, vel, eps2)
    ens.put("accin", acc_in)
    ens.eval()
    evaluated = ens.get("acc"), ens.get("jerk"), ens.get("snap")
    ens.init()
    begun, dt0 = ens.state(), ens.timestep(eta)
    ens.step(dt, new="pos2", old="pos")
    stepped, predicted = ens.state("pos2"), ens.predicted()
    ens.free()
    for s in range(3):
        d = Device6(gpu, pos[s], vel[s], eps2)
        d.put("accin", acc_in[s])
        d.eval()
        for g, k in zip(evaluated, ("acc", "jerk", "snap")):
            assert g[s].tobytes() == d.get(k).tobytes(), ("eval", k, s)
            assert np.isfinite(g[s]).all(), ("eval", k, s)
        d.init()
        same_bits([q[s] for q in begun], d.state(), ("init", s))
        assert dt0[s].tobytes() == solo_timestep6(gpu, d, eta).tobytes() and np.isfinite(dt0[s]) and dt0[s] > 0, ("timestep", s)
        d.step(dt, new="pos2", old="pos")
        same_bits([q[s] for q in stepped], d.state("pos2"), ("step", s))
        assert predicted[s].tobytes() == d.get("ws").tobytes(), ("predicted", s)
        d.free()
    # (that the bits are RIGHT, not only equal: system 0, whose unit is 2^20 / 2^60, against long double)
    check_eval6([q[0] for q in evaluated], pos[0], vel[0], acc_in[0], eps2, "ensemble system 0, first body on the window's edge")
    # Scaling by a power of two is exact, so the launch above has the same bits whichever of its first bodies is the unit.  A second
    # launch with first bodies of 1.5, 1.7 and 0.3, each with a unit chunk of its own: 1.7 / 1.5 rounds.
    for s, value in enumerate((1.5, 1.7, 0.3)):
        pos[s, 0, 3] = pos[s, 128:256, 3] = value
    ens = Ensemble6(gpu, pos, vel, eps2)
    ens.put("accin", acc_in)
    ens.eval()
    evaluated = ens.get("acc"), ens.get("jerk"), ens.get("snap")
    ens.free()
    for s in range(3):
        d = Device6(gpu, pos[s], vel[s], eps2)
        d.put("accin", acc_in[s])
        d.eval()
        for g, k in zip(evaluated, ("acc", "jerk", "snap")):
            assert g[s].tobytes() == d.get(k).tobytes(), ("eval, units that are no powers of two", k, s)
        d.free()
        check_eval6([q[s] for q in evaluated], pos[s], vel[s], acc_in[s], eps2, f"ensemble system {s}, first body {pos[s, 0, 3]}")


@gpu_only
@pytest.mark.parametrize("name,lo", [("float32", -20), ("float64", -60)])
def test_the_escape_to_plain_units_in_the_ensemble6(gpu, name, lo):
    """The heavy close pairs behind a light first body (S_i up to 2^126 / 2^1022) as system 1 of an ensemble launch beside an ordinary
    system 0 with another softening: check_eval6's bound, and the bits of the solo call."""
    dtype = np.dtype(name).type
    pos, vel, eps2, _ = close_pair_system(name, lo, 6)
    other = mass_system(dtype, N, "first", 0.75)
    zero = np.zeros_like(pos)
    ens = Ensemble6(gpu, np.stack([other[0], pos]), np.stack([other[1], vel]), np.array([0.01, eps2], dtype))
    ens.eval()
    got = ens.get("acc"), ens.get("jerk"), ens.get("snap")
    ens.free()
    check_eval6([q[1] for q in got], pos, vel, zero, eps2, f"ensemble, 6th order, heavy close pairs behind 2^{lo}")
    check_eval6([q[0] for q in got], other[0], other[1], zero, dtype(0.01), "ensemble, the ordinary system beside them")
    d = Device6(gpu, pos, vel, eps2)
    d.eval()
    for g, k in zip(got, ("acc", "jerk", "snap")):
        assert g[1].tobytes() == d.get(k).tobytes(), k
    d.free()


# ---- H ---------------------------------------------------------------------------------------------------------------------------------
@gpu_only
@pytest.mark.parametrize("dtype,e", TIMESTEP6_CASES)
def test_ensemble6_time_steps_at_extreme_magnitudes(gpu, dtype, e):
    """nb_hermite6_ensemble_timestep_*: the arrays of test_hermite6_time_step_on_both_sides_of_its_range as the middle system of three
    with different e.  Each system's dt is the solo call's bits; inside the range it is the long double rule to the solo test's bound,
    beyond it the plain fp64 outcome, never NaN; a system whose every body is left out gets +inf and its neighbours keep their bits."""
    others = [x for x in ((50, 80) if dtype == np.float32 else (100, 245, 600)) if x != e][:2]
    cases = [others[0], e, others[1]]
    arrays = [timestep6_arrays(dtype, x) for x in cases]
    n, eta = arrays[0][0].shape[0], dtype(0.02)
    zeros = np.zeros((3, n, 4), dtype)
    ens = Ensemble6(gpu, zeros, zeros, dtype(0.01))
    for k, key in enumerate(("acc", "jerk", "snap", "crackle")):
        ens.put(key, np.stack([q[k] for q in arrays]))
    dts = ens.timestep(eta)
    # every body of the middle system left out: |s| = |c| = 0 makes every denominator 0
    ens.put("snap", np.stack([arrays[0][2], np.zeros((n, 4), dtype), arrays[2][2]]))
    ens.put("crackle", np.stack([arrays[0][3], np.zeros((n, 4), dtype), arrays[2][3]]))
    emptied = ens.timestep(eta)
    ens.free()
    assert np.isposinf(emptied[1]) and emptied[[0, 2]].tobytes() == dts[[0, 2]].tobytes()
    for s, x in enumerate(cases):
        d = Device6(gpu, zeros[0], zeros[0], dtype(0.01))
        for key, q in zip(("acc", "jerk", "snap", "crackle"), arrays[s]):
            d.put(key, q)
        solo = solo_timestep6(gpu, d, eta)
        d.free()
        want, _ = timestep6_rule(arrays[s], x, eta)
        print(f"system {s} (2^+-{x}): dt {dts[s]!r}, rule {float(want):.17g}")
        assert dts[s].tobytes() == solo.tobytes(), (s, x)
        assert np.isfinite(dts[s]) and dts[s] > 0 and abs(LD(dts[s]) - want) <= TIMESTEP6_ALLOWED[dtype] * want, (s, x, dts[s], want)


# ---- I ---------------------------------------------------------------------------------------------------------------------------------
POISONS = ["NaN coordinate", "inf mass", "NaN mass", "NaN velocity", "NaN acc_in"]
PLACES = {"body 0": 0, "ragged tail": N - 1}


def poison_one(pos, vel, acc_in, k, poison):
    if poison == "NaN coordinate":
        pos[k, 1] = np.nan
    elif poison == "inf mass":
        pos[k, 3] = np.inf
    elif poison == "NaN mass":
        pos[k, 3] = np.nan
    elif poison == "NaN velocity":
        vel[k, 2] = np.nan
    else:
        acc_in[k, 0] = np.nan


def three_systems(dtype):
    """(pos, vel, acc_in) of three systems (3, N, 4): poisoned_system in the middle of two first-body systems; velocity .w carries a pattern"""
    middle = poisoned_system(dtype)
    sides = [mass_system(dtype, N, "first", value) for value in (0.75, 1.25)]
    pos, vel = np.stack([sides[0][0], middle[0], sides[1][0]]), np.stack([sides[0][1], middle[1], sides[1][1]])
    vel[:, :, 3] = (np.arange(3 * N).reshape(3, N) % 251 + 1).astype(dtype)
    acc_in = np.stack([acc_in_for(pos[0], 72), middle[2], acc_in_for(pos[2], 73)]).astype(dtype)
    return pos, vel, acc_in


def ensemble6_launches(gpu, pos, vel, acc_in):
    """eval with acc_in, then init and one step of 1/128: (acc, jerk, snap of the eval; the six arrays after the step)"""
    dtype = pos.dtype.type
    ens = Ensemble6(gpu, pos, vel, dtype(0.01))
    ens.put("accin", acc_in)
    ens.eval()
    evaluated = ens.get("acc"), ens.get("jerk"), ens.get("snap")
    ens.init()
    ens.step(dtype(1.0 / 128), new="pos2", old="pos")
    stepped = ens.state("pos2")
    ens.free()
    return evaluated, stepped


_CLEAN = {}


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("poison", POISONS)
def test_nonfinite_inputs_stay_in_their_system(gpu, dtype, place, poison):
    """One non-finite input in system 1 of three: systems 0 and 2 keep the bits of the clean launch (eval, and init + one step); system
    1's acceleration, jerk and snap become non-finite exactly where formula_rows says -- everywhere or nowhere per output --, output .w
    stays 0, and the step leaves masses and velocity .w bit for bit."""
    k = PLACES[place]
    pos, vel, acc_in = three_systems(dtype)
    if dtype not in _CLEAN:
        _CLEAN[dtype] = ensemble6_launches(gpu, pos, vel, acc_in)
        assert all(np.isfinite(q).all() for part in _CLEAN[dtype] for q in part)
    clean = _CLEAN[dtype]
    poison_one(pos[1], vel[1], acc_in[1], k, poison)
    rows = np.array(sorted({0, 1, 5, 130, 400, 777, N - 1, k}))
    rule = formula_rows(pos[1], vel[1], acc_in[1], dtype(0.01), rows)
    reached = {}
    for q, name in zip(rule, ("acc", "jerk", "snap")):
        bad = ~np.isfinite(q)
        assert bad.all() or not bad.any(), name
        reached[name] = bool(bad.all())
    assert reached == {"acc": poison in ("NaN coordinate", "inf mass", "NaN mass"), "jerk": poison != "NaN acc_in", "snap": True}
    evaluated, stepped = ensemble6_launches(gpu, pos, vel, acc_in)
    for s in (0, 2):
        for g, w, name in zip(evaluated + stepped, clean[0] + clean[1], ("acc", "jerk", "snap", "x1", "v1", "a1", "j1", "s1", "c1")):
            assert g[s].tobytes() == w[s].tobytes(), (s, name)
    for q, name in zip(evaluated, ("acc", "jerk", "snap")):
        bad = ~np.isfinite(q[1][:, :3])
        assert bad.all() if reached[name] else not bad.any(), (name, int(bad.sum()))
        assert q[1][:, 3].tobytes() == np.zeros(N, dtype).tobytes(), name
    assert stepped[0][1][:, 3].tobytes() == pos[1][:, 3].tobytes() and stepped[1][1][:, 3].tobytes() == vel[1][:, 3].tobytes()
    assert not any(q[1][:, 3].any() for q in stepped[2:])


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("poison", POISONS)
def test_nonfinite_inputs_through_a_block6_step(gpu, dtype, place, poison):
    """nb_hermite6_block_step_* with all bodies due (every body on level 8 at tick 0; the stored acceleration is acc_in, jerk = snap =
    crackle = 0).  The evaluation sees the PREDICTED state, into which the poisoned body's velocity and acceleration enter: formula_rows
    on the workspace's predicted state is the rule, everywhere or nowhere per output.  Output .w stays 0, masses and velocity .w come
    through bit for bit, every level stays in [0, max_level], the canaries hold."""
    k = PLACES[place]
    pos, vel, acc_in = poisoned_system(dtype)
    vel[:, 3] = (np.arange(N) % 251 + 1).astype(dtype)
    poison_one(pos, vel, acc_in, k, poison)
    eps2 = dtype(0.01)
    d = Block6Device(gpu, pos, vel, eps2, gpu.HermiteBlockParams(0.2, 0.01, 0.125, 8, 0), ws_fill=np.nan)
    d.put("acc", acc_in), d.put("levels", np.full(N, 8, np.int32))
    d.step()
    got, predicted, status = d.state(), d.get("ws"), d.status()
    assert d.canaries_intact() and (status.now_ticks, status.last_active) == (1, N)
    d.free()
    rows = np.array(sorted({0, 1, 5, 130, 400, 777, N - 1, k}))
    rule = formula_rows(predicted[:, 0:4], predicted[:, 4:8], predicted[:, 8:12], eps2, rows)
    for q, g, name in zip(rule, got[2:5], ("acc", "jerk", "snap")):
        want = ~np.isfinite(q)
        assert want.all() or not want.any(), name
        bad = ~np.isfinite(g[:, :3])
        assert bad.all() if want.all() else not bad.any(), (name, int(bad.sum()))
    assert not np.isfinite(got[4][:, :3]).any()  # (every poison reaches the snap)
    assert got[0][:, 3].tobytes() == pos[:, 3].tobytes() and got[1][:, 3].tobytes() == vel[:, 3].tobytes()
    assert not any(g[:, 3].any() for g in got[2:6])
    assert (got[6] == 1).all() and ((0 <= got[7]) & (got[7] <= 8)).all()
