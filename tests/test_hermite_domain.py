"""The Hermite, field and 6th-order kernels over their operand range (the "Operand range" paragraphs of include/nbody_hip_hermite.h,
_hermite6.h, _hermite_block.h and _field.h), as tests/test_fast_domain.py holds the FAST step to its own.

CPU part: the window's constants against the headers' text; every probe set and system below has a long double reference whose
results and formula intermediates (s^2, s^-2, s^-3, r.w, w.w + r.b, alpha, beta, each term) are finite and normal in T.
GPU part (MI355X):
  1. ONE term across the exponent range, per kernel and output, against the exact term rounded to T (ONE_TERM_MEASURED);
  2. masses on and around the window a unit mass is taken from, species at opposite mass edges, the ensemble against the solo calls;
  3. a small first body against heavy close pairs with the largest velocities the window admits (fp32: the jerk sums reach 2^126);
  4. softening: the floor, coincident pairs, softening^2 on and beyond the edges of the range of s^2;
  5. non-finite inputs, which reach exactly the outputs the formulas say;
  6. the time-step rules on hand-made arrays of magnitudes up to 2^+-100 (fp32) / 2^+-900 (fp64);
  7. the block scheme: one term through the planes and the finish kernel, check_block_stages on the systems of 2, the sums on both
     sides of their cap, the block ensemble against the solo block steps, the levels on both sides of the range of dt_A.
The references, bounds and device wrappers are those of the sister modules."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_fast_domain import CAP, TOL, UNIT_ROUNDOFF
from test_field import FLOOR, NONE
from test_field_gpu import check_field, field_reference
from test_field_gpu import run as field_run
from test_hermite import LD, Device, check_eval, check_step_of, cloud, reference
from test_hermite_block import BlockDevice, aarseth, check_block_stages, check_block_stages_of, first_levels, hand_made_schedule, new_levels
from test_hermite_block_ensemble import load_ensemble, solo_bytes, solo_start
from test_hermite6 import Device as Device6
from test_hermite6 import check_eval as check_eval6
from test_hermite6 import evaluate as evaluate6
from test_hermite6 import fns as hermite6_fns
from test_hermite6 import reference6
from test_hermite_ensemble import Ensemble, same_bits, solo_timestep

gpu_only = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
N = 128 * 9 + 17  # S = 8; a ragged last chunk (17 bodies: four groups and one body) and a ragged last tile
N_SMALL = 200     # S = 1: no fold

# The window of the headers' "Operand range" paragraphs, as exponents of two: s^2 = r.r + eps^2 within 2^+-s2; masses 0 or within
# 2^+-mass, with softening^2 >= 2^eps2_lo when they are at the edge; every sum of term magnitudes at most 2^sums; the floor s^2 takes
# at softening 0; the window a first body's mass is the unit in (usable_unit, csrc/nbody_lane.h).
WINDOW = {np.float32: dict(s2=84, mass=40, eps2_lo=-39, sums=126, floor=-60, unit=20),
          np.float64: dict(s2=600, mass=100, eps2_lo=-100, sums=1022, floor=-300, unit=60)}
HEADERS = ("nbody_hip_hermite.h", "nbody_hip_hermite_block.h", "nbody_hip_hermite6.h", "nbody_hip_field.h")
POINTERS = ("nbody_hip_hermite_ensemble.h", "nbody_hip_hermite_block_ensemble.h")


def header_text(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return " ".join(text.replace("\n *", " ").split())


def test_the_window_is_the_one_the_headers_state():
    f32, f64 = WINDOW[np.float32], WINDOW[np.float64]
    for name in HEADERS:
        text = header_text(name)
        paragraph = text[text.index("Operand range."):]
        assert f"[2^-{f32['s2']}, 2^{f32['s2']}] (fp32) / [2^-{f64['s2']}, 2^{f64['s2']}] (fp64)" in paragraph, name
        assert re.search(rf"\[2\^-{f32['mass']}, 2\^{f32['mass']}\]( \(fp32\))? / \[2\^-{f64['mass']}, 2\^{f64['mass']}\]", paragraph), name
        assert f"2^{f32['sums']}" in paragraph and f"2^{f64['sums']}" in paragraph, name
        assert "5e-6 (fp32) / 1e-14 (fp64)" in paragraph or name == "nbody_hip_hermite_block.h", name
    hermite = header_text("nbody_hip_hermite.h")
    assert f"2^{f32['floor']} (fp32) / 2^{f64['floor']} (fp64)" in hermite
    assert f"masses of 2^{f32['mass']} at softening_sq = 2^{f32['eps2_lo']} (fp32); 2^{f64['mass']} at 2^{f64['eps2_lo']} (fp64)" in hermite
    assert f"2^-{f32['unit']} <= |m_0| <= 2^{f32['unit']} (fp32; 2^+-{f64['unit']} fp64)" in header_text("nbody_hip_hermite_block.h")
    for name in POINTERS:
        assert '"Operand range"' in header_text(name), name
    lane = open(os.path.join(ROOT, "cuda-nbody_amd", "csrc", "nbody_lane.h")).read()
    assert f"T(0x1p-{f32['unit']}) : T(0x1p-{f64['unit']})" in lane and f"T(0x1p{f32['unit']}) : T(0x1p{f64['unit']})" in lane
    assert TOL == {np.float32: 5e-6, np.float64: 1e-14} and CAP == {"float32": 1e-6, "float64": 1e-14}
    assert FLOOR == {t: 2.0 ** WINDOW[t]["floor"] for t in DTYPES}


def normal_in(dtype, x):
    """x (long double), rounded to T, is finite and normal -- or exactly 0 where x is"""
    x = np.asarray(x, LD)
    with np.errstate(all="ignore"):
        t = x.astype(dtype)
    return np.isfinite(t) & (((t == 0) & (x == 0)) | (np.abs(t) >= np.finfo(dtype).tiny))


def norm(q):
    return np.sqrt((q * q).sum(axis=-1))


# ---------------------------------------------------------------------------------------------- 1. one term across the exponent range
# Measured maxima (MI355X) of |got - want| over the term's magnitude, want the exact term rounded to T: |want| for the acceleration and
# the potential, k (|w| + 3 |r.w| s^-2 |r|) for the jerk, k (|b| + 6 |alpha| |J'| + 3 |beta| |r|) for the snap (w - 3 alpha r cancels).
# The bars are twice these, and never looser than CAP (acc, pot: 1e-6 / 1e-14) or TOL (jerk, snap: 5e-6 / 1e-14).
ONE_TERM_MEASURED = {  # (kernel, precision, output): the maximum over the layouts and probe sets
    ("hermite_eval", "float32", "acc"): 3.483e-7, ("hermite_eval", "float32", "jerk"): 3.091e-7,
    ("hermite_eval", "float64", "acc"): 4.317e-16, ("hermite_eval", "float64", "jerk"): 4.026e-16,
    ("hermite6_eval", "float32", "acc"): 3.483e-7, ("hermite6_eval", "float32", "jerk"): 3.091e-7, ("hermite6_eval", "float32", "snap"): 3.617e-7,
    ("hermite6_eval", "float64", "acc"): 4.317e-16, ("hermite6_eval", "float64", "jerk"): 4.026e-16, ("hermite6_eval", "float64", "snap"): 5.347e-16,
    ("hermite_block_eval", "float32", "acc"): 3.483e-7, ("hermite_block_eval", "float32", "jerk"): 3.739e-7,
    ("hermite_block_eval", "float64", "acc"): 4.801e-16, ("hermite_block_eval", "float64", "jerk"): 4.986e-16,
    ("field_eval", "float32", "acc"): 3.483e-7, ("field_eval", "float32", "jerk"): 3.022e-7, ("field_eval", "float32", "pot"): 1.190e-7,
    ("field_eval", "float64", "acc"): 4.238e-16, ("field_eval", "float64", "jerk"): 4.000e-16, ("field_eval", "float64", "pot"): 3.703e-16,
}
# (fp32, s^2 in (2^84, 2^84.75], where s^-3 is subnormal: acc 2.69e-7, jerk 2.27e-7 -- no worse than inside the range)
NEAR_MASS = 1.5
W_PER_D = np.array([0.5, -1.25, 0.75])  # the near body's velocity and acc_in relative to a probe's, per unit of d: every exact term is
B_PER_D = np.array([-0.75, 0.5, 1.5])   # of the order 1 / d^2


def probe_sets(dtype):
    """[(eps^2, squared distances |r|^2)]: eps = 0 over the whole range of s^2 (below 2^-36 / 2^-248 the floor is what counts), and
    five eps-dominated launches (|r|^2 from eps^2 2^-24 to eps^2 2^-1/2); mantissas off the powers of two; every s^2 in the window"""
    win = WINDOW[dtype]
    top, step = win["s2"], 0.25 if dtype == np.float32 else 2.0
    rng = np.random.default_rng(43)
    whole = 2.0 ** np.arange(-top, top, step)
    whole = whole * rng.uniform(1.0, 2.0, whole.size)
    out = [(0.0, whole[whole <= 2.0 ** top])]
    for e in ((-80, -40, 0, 40, 80) if dtype == np.float32 else (-600, -200, 0, 200, 599)):
        near = 2.0 ** (e + np.arange(-24, -1, 0.5))
        out.append((2.0 ** e, near * rng.uniform(1.0, 2.0, near.size)))
    return out


def probes(dtype, d2):
    """K probes at (d, d/2, 0), |r|^2 = d2, moving and accelerating against the near body at rest at the origin in proportion to d:
    T-typed (K, 4) position (mass 0), velocity and acc_in"""
    d = np.sqrt(d2 / 1.25)
    pos, vel, acc = (np.zeros((d.size, 4), dtype) for _ in range(3))
    pos[:, 0], pos[:, 1] = d, d * 0.5
    vel[:, :3] = -d[:, None] * W_PER_D
    acc[:, :3] = -d[:, None] * B_PER_D
    return pos, vel, acc


def one_term(dtype, pos, vel, acc, eps2, mass=NEAR_MASS):
    """the exact terms a source of `mass` at rest at the origin adds to the probes, in long double from the T-typed inputs, with the
    floor at eps^2 = 0: (terms, magnitudes, intermediates)"""
    s2_add = LD(dtype(eps2)) if eps2 != 0 else LD(FLOOR[dtype])
    r, w, b = -pos[:, :3].astype(LD), -vel[:, :3].astype(LD), -acc[:, :3].astype(LD)
    s2 = (r * r).sum(axis=1) + s2_add
    inv2 = 1 / s2
    inv3 = inv2 / np.sqrt(s2)
    k = LD(mass) * inv3
    rw, wwrb = (r * w).sum(axis=1), (w * w).sum(axis=1) + (r * b).sum(axis=1)
    alpha = rw * inv2
    beta = wwrb * inv2 + alpha * alpha
    jp = w - 3 * alpha[:, None] * r
    sp = b - 6 * alpha[:, None] * jp - 3 * beta[:, None] * r
    terms = dict(acc=k[:, None] * r, jerk=k[:, None] * jp, snap=k[:, None] * sp, pot=-LD(mass) / np.sqrt(s2))
    sizes = dict(acc=norm(terms["acc"]), jerk=np.abs(k) * (norm(w) + 3 * np.abs(rw) * inv2 * norm(r)),
                 snap=np.abs(k) * (norm(b) + 6 * np.abs(alpha) * norm(jp) + 3 * np.abs(beta) * norm(r)), pot=np.abs(terms["pot"]))
    return terms, sizes, dict(s2=s2, inv2=inv2, inv3=inv3, rw=rw, wwrb=wwrb, alpha=alpha, beta=beta)


def term_errors(dtype, got, terms, sizes):
    """{output: |got - want| / magnitude per probe}, want the exact term rounded to T"""
    out = {}
    for name, g in got.items():
        want = terms[name].astype(dtype).astype(LD)
        diff = g.astype(LD) - want
        out[name] = (np.abs(diff) if diff.ndim == 1 else norm(diff)) / sizes[name]
    return out


def far_of(dtype):
    return 2.0 ** (62 if dtype == np.float32 else 400)  # (the distances of test_fast_coupling_across_the_exponent_range)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_probe_has_a_finite_normal_reference(dtype):
    """No probe is dropped: every quantity of the documented formulas is finite and normal in T for every probe of every launch, and
    the pairs that must contribute exactly 0 -- probe with probe (mass 0), anything with a far body (s^-3 underflows) -- do so
    without an infinity on the way (0 * inf is NaN)."""
    win, far = WINDOW[dtype], far_of(dtype)
    count = 0
    for eps2, d2 in probe_sets(dtype):
        assert d2.size <= 700
        pos, vel, acc = probes(dtype, d2)
        terms, sizes, inter = one_term(dtype, pos, vel, acc, eps2)
        assert (inter["s2"] >= LD(2.0) ** -win["s2"]).all() and (inter["s2"] <= LD(2.0) ** win["s2"]).all(), eps2
        for name, q in {**terms, **sizes, **inter}.items():
            assert normal_in(dtype, q).all(), (eps2, name, d2[~normal_in(dtype, q).reshape(d2.size, -1).all(axis=1)][:4])
        assert (sizes["jerk"] > 0).all() and (sizes["snap"] > 0).all()
        # probe against probe: s^-3 and the brackets stay finite in T, so a mass of 0 gives a term of exactly 0
        s2_add = LD(dtype(eps2)) if eps2 != 0 else LD(FLOOR[dtype])
        p, v, a = pos[:, :3].astype(LD), vel[:, :3].astype(LD), acc[:, :3].astype(LD)
        r, w, b = p[None] - p[:, None], v[None] - v[:, None], a[None] - a[:, None]
        s2 = (r * r).sum(axis=2) + s2_add
        alpha, beta = (r * w).sum(axis=2) / s2, ((w * w).sum(axis=2) + (r * b).sum(axis=2)) / s2
        big = LD(np.finfo(dtype).max) / 8
        for q in (s2 ** LD(-1.5), alpha, alpha * alpha, beta, norm(w) + 3 * np.abs(alpha) * norm(r), norm(b) + 6 * np.abs(alpha) * (norm(w) + 3 * np.abs(alpha) * norm(r)) + 3 * np.abs(beta) * norm(r)):
            assert (np.abs(q) < big).all(), eps2
        # probe against far body: m s^-3 rounds to 0 in T (below half the smallest subnormal), the brackets stay finite
        d_far = LD(far) - np.abs(p).max()
        assert (LD(8.0) * d_far ** -3).astype(dtype) == 0
        assert far * np.abs(np.concatenate([v, a])).max() * 3 < big and d_far ** 2 > LD(2.0) ** -win["s2"]
        count += d2.size
    assert count == sum(d2.size for _, d2 in probe_sets(dtype)) and count > 700


def one_sided_system(dtype, layout, pos_p, vel_p, acc_p):
    """chunk 0: the near body (body 0: the unit mass) and 127 far bodies -- of the unit mass ("unit": the chunk takes the loop without
    the mass multiply) or of other masses ("mixed"); then the probes, mass 0, in chunks of their own (mixed form)"""
    k = pos_p.shape[0]
    pos, vel, acc = (np.zeros((128 + k, 4), dtype) for _ in range(3))
    pos[1:128, 0] = far_of(dtype)
    pos[:128, 3] = NEAR_MASS
    if layout == "mixed":
        pos[1:128:2, 3], pos[2:128:2, 3] = 0.75, 3.0
    pos[128:], vel[128:], acc[128:] = pos_p, vel_p, acc_p
    return pos, vel, acc


def hermite_results(gpu, pos, vel, acc, eps2):
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    out = [dict(acc=d.get("acc")[128:, :3], jerk=d.get("jerk")[128:, :3])]
    d.step(pos.dtype.type(0), new="pos2", old="pos")  # dt = 0 predicts the stored state: the STEP kernel's sums of the same bodies
    assert d.get("ws")[:, :3].tobytes() == pos[:, :3].tobytes()
    out.append(dict(acc=d.get("acc")[128:, :3], jerk=d.get("jerk")[128:, :3]))
    d.free()
    return out


def hermite6_results(gpu, pos, vel, acc, eps2):
    a, j, s = evaluate6(gpu, pos, vel, acc, eps2)
    return [dict(acc=a[128:, :3], jerk=j[128:, :3], snap=s[128:, :3])]


def bar(kernel, name, output):
    limit = CAP[name] if output in ("acc", "pot") else TOL[np.dtype(name).type]
    return min(2 * ONE_TERM_MEASURED[(kernel, name, output)], limit)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", ["hermite_eval", "hermite6_eval"])
def test_one_term_across_the_exponent_range(gpu, dtype, kernel):
    """Every probe's sums hold a single nonzero term: no summation rounding is left.  hermite_eval: the evaluation and the STEP
    kernel (dt = 0), near body in a unit chunk and in a mixed one; hermite6_eval: the evaluation, both layouts."""
    name = np.dtype(dtype).name
    results = hermite_results if kernel == "hermite_eval" else hermite6_results
    worst = {}
    for eps2, d2 in probe_sets(dtype):
        pos_p, vel_p, acc_p = probes(dtype, d2)
        terms, sizes, _ = one_term(dtype, pos_p, vel_p, acc_p, eps2)
        for layout in ("unit", "mixed"):
            pos, vel, acc = one_sided_system(dtype, layout, pos_p, vel_p, acc_p)
            for got in results(gpu, pos, vel, acc, dtype(eps2)):
                for output, err in term_errors(dtype, got, terms, sizes).items():
                    assert np.isfinite(err).all(), (eps2, layout, output, d2[~np.isfinite(err)][:4])
                    worst[output] = max(worst.get(output, 0.0), float(err.max()))
    for output, value in worst.items():
        print(f"one term {kernel} {name} {output}: max error over the term's magnitude {value:.3e} (bar {bar(kernel, name, output):.3e})")
    for output, value in worst.items():
        assert value <= bar(kernel, name, output), (output, value)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_term_field(gpu, dtype):
    """field_eval: the probes are targets of one chunk of 128 sources, the near one at the origin; without and with the jerk; a few
    probes exclude a far source of the chunk (the MASK form of the chunk).  The far sources of mass 0, of the near source's mass (their
    acceleration and jerk terms underflow to 0) and of other masses: a source's term has the same bits whatever the other sources of
    its chunk weigh, and with mass 0 the potential holds one term too."""
    name = np.dtype(dtype).name
    worst = {}
    for eps2, d2 in probe_sets(dtype):
        tgt, tgt_vel, acc_p = probes(dtype, d2)
        terms, sizes, _ = one_term(dtype, tgt, tgt_vel, acc_p, eps2)
        k = tgt.shape[0]
        self_index = np.full(k, NONE, np.uint32)
        self_index[3::7] = 5
        src, src_vel = np.zeros((128, 4), dtype), np.zeros((128, 4), dtype)
        src[1:, 0] = far_of(dtype)
        src[0, 3] = NEAR_MASS
        seen = {}
        for far_masses in ("zero", "equal", "mixed"):
            if far_masses == "equal":
                src[1:, 3] = NEAR_MASS
            elif far_masses == "mixed":
                src[1::2, 3], src[2::2, 3] = 0.75, -3.0
            for with_jerk in (False, True):
                outputs = ("acc", "jerk", "pot") if with_jerk else ("acc", "pot")
                out = field_run(gpu, src, tgt, src_vel if with_jerk else None, tgt_vel if with_jerk else None, self_index, dtype(eps2), outputs)
                got = {o: (out[o][:, :3] if o != "pot" else out[o]) for o in outputs if o != "pot" or far_masses == "zero"}
                for output, err in term_errors(dtype, got, terms, sizes).items():
                    assert np.isfinite(err).all(), (eps2, far_masses, output)
                    worst[output] = max(worst.get(output, 0.0), float(err.max()))
                for o in got:
                    if o != "pot":
                        assert seen.setdefault((o, with_jerk), got[o].tobytes()) == got[o].tobytes(), (eps2, far_masses, o)
        assert seen[("acc", False)] == seen[("acc", True)]  # (which outputs are stored changes no bit of the others)
    for output, value in worst.items():
        print(f"one term field_eval {name} {output}: max error over the term's magnitude {value:.3e} (bar {bar('field_eval', name, output):.3e})")
    for output, value in worst.items():
        assert value <= bar("field_eval", name, output), (output, value)


@gpu_only
def test_one_term_above_the_fp32_range(gpu):
    """The last 3/4 binade FAST's sweep reaches and the header leaves out: s^2 in (2^84, 2^84.75], where s^-3 = s^-1 s^-2 is subnormal
    in fp32.  The header's statement: the term is off by up to two units of 2^-149 in s^-3, on top of the bar inside the range."""
    dtype = np.float32
    d2 = 2.0 ** (84 + np.arange(0.02, 0.75, 0.01))
    pos_p, vel_p, acc_p = probes(dtype, d2)
    terms, sizes, inter = one_term(dtype, pos_p, vel_p, acc_p, 0.0)
    assert normal_in(dtype, terms["acc"]).all() and normal_in(dtype, terms["jerk"]).all() and not normal_in(dtype, inter["inv3"]).any()
    extra = 2 * LD(2.0) ** -149 / inter["inv3"]
    for layout in ("unit", "mixed"):
        pos, vel, acc = one_sided_system(dtype, layout, pos_p, vel_p, acc_p)
        for got in hermite_results(gpu, pos, vel, acc, dtype(0)):
            err = term_errors(dtype, got, terms, sizes)
            print(f"above the range, {layout}: acc {float(err['acc'].max()):.3e}, jerk {float(err['jerk'].max()):.3e} (two subnormal units: up to {float(extra.max()):.3e})")
            assert (err["acc"] <= bar("hermite_eval", "float32", "acc") + extra).all()
            assert (err["jerk"] <= bar("hermite_eval", "float32", "jerk") + extra).all()


# ---------------------------------------------------------------------------------------------- 2. masses on and around the unit window
def mass_values(dtype):
    e = WINDOW[dtype]["unit"]
    return [2.0 ** e, 2.0 ** -e, 2.0 ** (e + 1), 2.0 ** -(e + 1), 0.0, -0.0, -1.5]


def mass_system(dtype, n, kind, value):
    """a cloud with masses from 0.5 to 2 whose first body ("first"), or every body ("species"), has mass `value`"""
    pos, vel = cloud(n, dtype, 61 + n, "equal")
    pos[:, 3] = np.linspace(0.5, 2.0, n)
    if kind == "first":
        pos[0, 3] = value
    else:
        pos[:, 3] = value
    return pos, vel


def species_system(dtype, mexp):
    """contiguous species of 2^mexp and 2^-mexp taking turns, borders inside chunks, groups and tiles: unit and mixed chunks alternate"""
    pos, vel = cloud(N, dtype, 67, "equal")
    borders = [0, 300, 371, 640, 897, 1024, 1025, 1100, N]
    for k, (a, b) in enumerate(zip(borders[:-1], borders[1:])):
        pos[a:b, 3] = 2.0 ** (mexp if k % 2 else -mexp)
    return pos, vel


def acc_in_for(pos, seed=71):
    acc = np.zeros_like(pos)
    acc[:, :3] = (np.random.default_rng(seed).standard_normal((pos.shape[0], 3)) * 2).astype(np.float32)
    return acc


def check_all_evaluations(gpu, pos, vel, eps2, what, step=True, dt=1.0 / 128):
    """nb_hermite_eval_* (check_eval), nb_hermite_step_* stage by stage (ld_step), nb_hermite6_eval_* (reference6)"""
    dtype = pos.dtype.type
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    acc, jerk = d.get("acc"), d.get("jerk")
    d.free()
    check_eval(acc, jerk, pos, vel, eps2, what)
    if step:
        check_step_of(gpu, pos, vel, eps2, dtype(dt), what)
    acc_in = acc_in_for(pos)
    check_eval6(evaluate6(gpu, pos, vel, acc_in, eps2), pos, vel, acc_in, eps2, what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_mass_systems_have_finite_normal_references(dtype):
    """every system of section 2 -- 7 masses x (first body, species) x both sizes, and the species at opposite edges: the sums and
    the sums of term magnitudes are finite and normal in T (or exactly 0: a species of mass 0)"""
    systems = [(f"{kind} {value} n {n}", mass_system(dtype, n, kind, value)) for kind in ("first", "species") for value in mass_values(dtype) for n in (N, N_SMALL)]
    systems += [(f"species 2^+-{mexp}", species_system(dtype, mexp)) for mexp in ((40, 60) if dtype == np.float32 else (60, 100))]
    for what, (pos, vel) in systems:
        for q in reference(pos, vel, dtype(0.01)):
            assert normal_in(dtype, q).all(), what


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(7))
@pytest.mark.parametrize("kind", ["first", "species"])
def test_masses_on_and_around_the_unit_window(gpu, dtype, kind, index):
    """The first body -- the mass the unit chunks are recognised by -- on the edge of the window (2^+-20 / 2^+-60), just outside
    (2^+-21 / 2^+-61: the unit falls back to 1), 0, -0.0 and negative; alone among other masses (every chunk mixed), and as the
    whole system's species (every chunk unit, the last one ragged)."""
    value = mass_values(dtype)[index]
    for n in (N, N_SMALL):
        pos, vel = mass_system(dtype, n, kind, value)
        check_all_evaluations(gpu, pos, vel, dtype(0.01), f"{kind} {value} n {n}", step=kind == "first" or n == N_SMALL)


@gpu_only
@pytest.mark.parametrize("dtype,mexp", [(np.float32, 40), (np.float32, 60), (np.float64, 60), (np.float64, 100)])
def test_contiguous_species_at_opposite_mass_edges(gpu, dtype, mexp):
    """Masses at the edge of the window and, as FAST is tested, 2^20 beyond it.  The step's evaluation sees the PREDICTED state, which
    a dt^2 / 2 moves: fp32 masses of 2^60 (accelerations of 2^67) at dt = 1/128 throw the bodies 2^52 apart -- s^2 = 2^104, beyond the
    range of s^2.  So dt is the largest power of two up to 1/128 that keeps every predicted coordinate within 2^40 (s^2 <= 2^84)."""
    pos, vel = species_system(dtype, mexp)
    eps2 = dtype(0.01)
    a, j = (float(np.abs(q).max()) for q in reference(pos, vel, eps2)[:2])
    dt = 2.0 ** -7
    while dtype == np.float32 and 4 + 2 * dt + a * dt * dt / 2 + j * dt ** 3 / 6 > 2.0 ** 40:
        dt /= 2
    assert dt >= 2.0 ** -20
    check_all_evaluations(gpu, pos, vel, eps2, f"species 2^+-{mexp}", dt=dt)
    # the field has no unit form: targets are the sources, each excluding itself
    self_index = np.arange(N, dtype=np.uint32)
    out = field_run(gpu, pos, pos, vel, vel, self_index, eps2, ("acc", "jerk", "pot"))
    check_field(out, field_reference(pos, vel, pos, vel, self_index, eps2), dtype, f"field, species 2^+-{mexp}")


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_act", [129, N])
def test_block_stages_at_this_modules_size(gpu, dtype, n_act):
    """One block step of the block scheme at N = 1 169 (S = 8, a ragged last chunk), stage by stage against long double, with masses
    of 2^+-10 drawn per body: the partial planes are in units of the FIRST body's mass, which the finish kernel multiplies back."""
    check_block_stages(gpu, dtype, N, n_act, "random", 4e-3)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_ensemble_systems_with_first_bodies_of_their_own(gpu, dtype):
    """One launch of three systems whose first bodies weigh 2^20 (2^60), 2^-21 (2^-61: no unit) and 0: the unit mass is per system,
    so every system has the bits of the solo calls."""
    e = WINDOW[dtype]["unit"]
    systems = [mass_system(dtype, N, "first", value) for value in (2.0 ** e, 2.0 ** -(e + 1), 0.0)]
    systems[0][0][128:256, 3] = 2.0 ** e  # (a unit chunk of its own in system 0)
    pos, vel = np.stack([s[0] for s in systems]), np.stack([s[1] for s in systems])
    eps2, dt, eta = dtype(0.01), dtype(1.0 / 128), dtype(0.02)
    ens = Ensemble(gpu, pos, vel, eps2)
    ens.eval()
    acc0, jerk0, dt0 = ens.get("acc"), ens.get("jerk"), ens.timestep(eta)
    ens.step(dt, new="pos2", old="pos")
    stepped = ens.state("pos2")
    ens.free()
    for s in range(3):
        d = Device(gpu, pos[s], vel[s], eps2)
        d.eval()
        assert acc0[s].tobytes() == d.get("acc").tobytes() and jerk0[s].tobytes() == d.get("jerk").tobytes(), ("eval", s)
        assert dt0[s].tobytes() == solo_timestep(gpu, d, eta).tobytes(), ("timestep", s)
        d.step(dt, new="pos2", old="pos")
        same_bits([q[s] for q in stepped], d.state("pos2"), ("step", s))
        d.free()


# ---------------------------------------------------------------------------------------------- 3. small reference mass, heavy close pairs
@functools.lru_cache(maxsize=None)
def close_pair_system(name, lo, order):
    """close_pair_system of tests/test_fast_domain.py at N = 1 169, with velocities: 128 bodies of mass 2^lo spread out (the first body
    among them), then two clumps of heavy bodies (one species, then mixed masses) of the largest mass of the window, eps / sqrt(2)
    apart at the window's softening floor.  Every velocity is a random direction times the largest power of two that keeps the sums
    of term magnitudes -- J_i for the 4th order, S_i for the 6th (acc_in = 0) -- at or below 2^126 (fp32) / 2^1022 (fp64)."""
    dtype = np.dtype(name).type
    win = WINDOW[dtype]
    hi, eps2_exp = win["mass"], win["eps2_lo"]
    rng = np.random.default_rng(31)
    pos, vel = np.zeros((N, 4), dtype), np.zeros((N, 4), dtype)
    pos[:128, :3] = rng.uniform(0.5, 1.0, (128, 3))
    pos[:128, 3] = 2.0 ** lo
    half = (N - 128) // 2
    pos[128 + half:, 0] = 2.0 ** ((eps2_exp - 1) / 2)  # eps / sqrt(2): where d / (d^2 + eps^2)^(3/2) peaks
    pos[128:, 3] = 2.0 ** hi
    pos[128 + half + 1::2, 3] = dtype(2.0 ** hi) * dtype(1 - UNIT_ROUNDOFF[dtype])
    direction = rng.standard_normal((N, 3))
    eps2 = dtype(2.0 ** eps2_exp)
    unit_vel = vel.astype(LD)
    unit_vel[:, :3] = direction
    zero_acc = np.zeros((N, 4), LD)
    if order == 4:
        size = reference(pos.astype(LD), unit_vel, eps2)[3]  # J_i at velocities of order 1: linear in their scale
        scale = 2.0 ** np.floor(win["sums"] - np.log2(float(size.max())))
    else:
        size = reference6(pos.astype(LD), unit_vel, zero_acc, eps2)[5]  # S_i: quadratic
        scale = 2.0 ** np.floor((win["sums"] - np.log2(float(size.max()))) / 2)
    vel[:, :3] = direction * scale
    return pos, vel, eps2, scale


CLOSE_PAIRS = [("float32", -20), ("float32", -40), ("float64", -60)]


@pytest.mark.parametrize("name,lo", CLOSE_PAIRS)
@pytest.mark.parametrize("order", [4, 6])
def test_close_pair_systems_have_finite_normal_references(name, lo, order):
    """Before anything runs on the GPU: the exact acceleration, jerk and snap of every body, and the sums of their term magnitudes,
    are finite and normal in T, and the largest sum is within a factor of 4 (6th order: 16) of the window's edge."""
    dtype = np.dtype(name).type
    pos, vel, eps2, scale = close_pair_system(name, lo, order)
    if order == 4:
        ref = reference(pos, vel, eps2)
        size = ref[3]
    else:
        ref = reference6(pos, vel, np.zeros_like(pos), eps2)
        size = ref[5]
    for q in ref:
        assert normal_in(dtype, q).all()
    top = LD(2.0) ** WINDOW[dtype]["sums"]
    assert top / (4 if order == 4 else 16) < size.max() <= top * (1 + 1e-6), (float(np.log2(size.max())), scale)


@gpu_only
@pytest.mark.parametrize("name,lo", CLOSE_PAIRS)
def test_small_reference_mass_against_heavy_close_pairs(gpu, name, lo):
    """A first body of 2^-20 (fp64: 2^-60) is the unit mass; 2^-40 is FAST's other case carried over.  Kept in units of it, the mixed
    chunks' jerk sums -- up to 2^126 (2^1022) here -- passed FLT_MAX (DBL_MAX) by 2^18 (2^58) while the exact jerk was representable:
    a wave whose sums outgrow that unit now goes over to plain units (csrc/hermite_stream.inc).  The exact result and every
    intermediate of the documented formula are finite and normal, so the bound holds."""
    pos, vel, eps2, scale = close_pair_system(name, lo, 4)
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    acc, jerk = d.get("acc"), d.get("jerk")
    d.free()
    check_eval(acc, jerk, pos, vel, eps2, f"heavy close pairs behind 2^{lo}, velocities of 2^{int(np.log2(scale))}")
    pos, vel, eps2, scale = close_pair_system(name, lo, 6)
    acc_in = np.zeros_like(pos)
    check_eval6(evaluate6(gpu, pos, vel, acc_in, eps2), pos, vel, acc_in, eps2, f"6th order, heavy close pairs behind 2^{lo}, velocities of 2^{int(np.log2(scale))}")


# ---------------------------------------------------------------------------------------------- 4. softening
@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_floor_at_no_softening(gpu, dtype):
    """softening^2 = 0.  A coincident pair with one velocity, and the i = j term, contribute exactly 0: the sums of a body are the
    bits of the system without its twin.  A pair further apart than 2^-18 / 2^-124 differs from the UNFLOORED long double term by no
    more than one ulp of s^2 does (3/2 of it in s^-3, 5/2 in the jerk's s^-5); a pair at 2^-29 / 2^-149 is the formula WITH the floor."""
    name, u = np.dtype(dtype).name, UNIT_ROUNDOFF[dtype]
    pos, vel = cloud(3, dtype, 5, "equal")
    pos[:, 3] = 1.0
    pos[1], vel[1] = pos[0], vel[0]
    twin = [evaluate_4(gpu, pos, vel, dtype(0)), evaluate_4(gpu, pos[[0, 2]], vel[[0, 2]], dtype(0))]
    for q in range(2):
        assert twin[0][q][0].tobytes() == twin[1][q][0].tobytes() and twin[0][q][1].tobytes() == twin[1][q][0].tobytes()
        assert twin[0][q][2, :3].any() and np.isfinite(twin[0][q]).all()
    acc_in = acc_in_for(pos)
    acc_in[1] = acc_in[0]
    six = [evaluate6(gpu, pos, vel, acc_in, dtype(0)), evaluate6(gpu, pos[[0, 2]], vel[[0, 2]], acc_in[[0, 2]], dtype(0))]
    for q in range(3):
        assert six[0][q][0].tobytes() == six[1][q][0].tobytes() and six[0][q][1].tobytes() == six[1][q][0].tobytes() and np.isfinite(six[0][q]).all()

    apart = 2.0 ** (-18 if dtype == np.float32 else -124)
    close = 2.0 ** (-29 if dtype == np.float32 else -149)
    d = np.array([close * 1.3, apart * 1.01, apart * 1.7, apart * 64 * 1.1])  # (|r| = d sqrt(1.25))
    pos_p, vel_p, acc_p = probes(dtype, 1.25 * d * d)
    floored, sizes, _ = one_term(dtype, pos_p, vel_p, acc_p, 0.0)
    r, w = -pos_p[:, :3].astype(LD), -vel_p[:, :3].astype(LD)
    s2 = (r * r).sum(axis=1)
    k = LD(NEAR_MASS) / (s2 * np.sqrt(s2))
    unfloored = dict(acc=k[:, None] * r, jerk=k[:, None] * (w - 3 * ((r * w).sum(axis=1) / s2)[:, None] * r))
    unfloored_sizes = dict(acc=norm(unfloored["acc"]), jerk=k * (norm(w) + 3 * np.abs((r * w).sum(axis=1)) / s2 * norm(r)))
    for layout in ("unit", "mixed"):
        system = one_sided_system(dtype, layout, pos_p, vel_p, acc_p)
        for got in hermite_results(gpu, *system, dtype(0)):
            err = term_errors(dtype, got, floored, sizes)
            assert (err["acc"] <= bar("hermite_eval", name, "acc")).all() and (err["jerk"] <= bar("hermite_eval", name, "jerk")).all(), layout
            far = term_errors(dtype, got, unfloored, unfloored_sizes)
            shift = LD(FLOOR[dtype]) / s2  # what the floor adds to s^2, relative: at most an ulp of s^2 (2u) beyond 2^-18 / 2^-124
            assert (shift[1:] <= 2 * u).all()
            assert (far["acc"][1:] <= bar("hermite_eval", name, "acc") + 1.5 * shift[1:]).all(), (layout, far["acc"])
            assert (far["jerk"][1:] <= bar("hermite_eval", name, "jerk") + 2.5 * shift[1:]).all(), (layout, far["jerk"])
            assert far["acc"][0] > 0.1  # (at 2^-29 / 2^-149 the floor is a tenth of s^2: the unfloored term is 15 % off)


def evaluate_4(gpu, pos, vel, eps2):
    d = Device(gpu, np.ascontiguousarray(pos), np.ascontiguousarray(vel), eps2)
    d.eval()
    out = d.get("acc"), d.get("jerk")
    d.free()
    return out


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_coincident_pair_under_softening_on_and_beyond_the_range(gpu, dtype):
    """softening^2 > 0: a coincident pair contributes a = 0 and jerk = m w / eps^3 -- at the lower and the upper edge of the range
    of s^2, one binade beyond (fp32: s^-3 is 2^127.5 below and subnormal above) and two binades beyond, as the header says: fp32 two binades below, s^-3 is infinite and so are the sums (0 * inf: NaN); two
    binades above, s^-3 is subnormal and the jerk is off by up to two units of 2^-149 in it; fp64 has room on either side."""
    win, name = WINDOW[dtype], np.dtype(dtype).name
    pos, vel = np.zeros((2, 4), dtype), np.zeros((2, 4), dtype)
    pos[:, :3], pos[:, 3] = (0.75, -0.5, 0.25), (1.0, 0.75)
    vel[1, :3] = (0.5, -0.25, 0.125)
    for e in (-win["s2"], win["s2"], -win["s2"] - 1, win["s2"] + 1, -win["s2"] - 2, win["s2"] + 2):
        eps2 = dtype(2.0 ** e)
        acc, jerk = evaluate_4(gpu, pos, vel, eps2)
        inv3 = LD(eps2) ** LD(-1.5)
        want = LD(0.75) * vel[1, :3].astype(LD) * inv3
        if dtype == np.float32 and e < -win["s2"] - 1:  # (one binade below, s^-3 = 2^127.5 is still finite: the header's limit is 2^-85.4)
            assert not np.isfinite(acc[:, :3]).any() and not np.isfinite(jerk[:, :3]).any(), e
            continue
        allowed = bar("hermite_eval", name, "jerk") + (2 * LD(2.0) ** -149 / inv3 if dtype == np.float32 and e > win["s2"] else 0)
        assert not acc[:, :3].any() and not acc[:, 3].any() and not jerk[:, 3].any(), e
        assert norm(jerk[0, :3].astype(LD) - want) <= allowed * norm(want), (e, jerk[0], want)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_field_potential_of_a_coincident_pair(gpu, dtype):
    """The potential uses the same s^2: at softening 0 a coincident pair that is not excluded contributes -m 2^30 / -m 2^150 exactly,
    an excluded one 0."""
    src = np.array([[0.75, -0.5, 0.25, 1.5]], dtype)
    out = field_run(gpu, src, src, None, None, None, dtype(0), ("acc", "pot"))
    assert out["pot"][0] == dtype(-1.5 * 2.0 ** (-WINDOW[dtype]["floor"] // 2)) and not out["acc"].any()
    out = field_run(gpu, src, src, None, None, np.zeros(1, np.uint32), dtype(0), ("acc", "pot"))
    assert out["pot"][0] == 0 and not out["acc"].any()  # (-0.0: the potential is minus the sum)


# ---------------------------------------------------------------------------------------------- 5. non-finite inputs
PLACES = {"unit chunk": 5, "mixed chunk": 400, "ragged tail": N - 1, "body 0": 0}


def poisoned_system(dtype):
    """unit mass 1; chunk 3 (bodies 384 .. 511) of other masses; the last chunk ragged (its last body after the last whole group)"""
    pos, vel = cloud(N, dtype, 83, "equal")
    pos[:, 3] = 1.0
    pos[384:512, 3] = np.linspace(0.5, 2.0, 128)
    return pos, vel, acc_in_for(pos)


def formula_rows(pos, vel, acc_in, eps2, rows):
    """a, jerk, snap of bodies `rows` by the headers' formulas as they stand, in long double (no guard: non-finite operands are data)"""
    p, v, c = pos.astype(LD), vel.astype(LD), acc_in.astype(LD)
    r, w, b = p[None, :, :3] - p[rows, None, :3], v[None, :, :3] - v[rows, None, :3], c[None, :, :3] - c[rows, None, :3]
    with np.errstate(all="ignore"):
        s2 = (r * r).sum(axis=2) + LD(eps2)
        k = (p[None, :, 3] / (s2 * np.sqrt(s2)))[:, :, None]
        alpha = ((r * w).sum(axis=2) / s2)[:, :, None]
        beta = (((w * w).sum(axis=2) + (r * b).sum(axis=2)) / s2)[:, :, None] + alpha * alpha
        jp = w - 3 * alpha * r
        return (k * r).sum(axis=1), (k * jp).sum(axis=1), (k * (b - 6 * alpha * jp - 3 * beta * r)).sum(axis=1)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("poison", ["NaN coordinate", "inf mass", "NaN mass", "NaN velocity", "NaN acc_in"])
def test_nonfinite_inputs_reach_what_the_formulas_say(gpu, dtype, place, poison):
    """The long double formulas are the rule.  A NaN coordinate, or an infinite / NaN mass, of ONE body reaches the acceleration, the
    jerk and the snap of every body (the body's own term is m 0 s^-3: inf * 0); a NaN velocity every jerk and snap and no
    acceleration; a NaN acc_in every snap and nothing else.  Nothing else becomes non-finite, .w of the outputs stays 0, and a step
    leaves the masses and velocity .w bit for bit."""
    k = PLACES[place]
    pos, vel, acc_in = poisoned_system(dtype)
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
    reached = {"acc": poison in ("NaN coordinate", "inf mass", "NaN mass"), "jerk": poison != "NaN acc_in", "snap": True}
    eps2 = dtype(0.01)
    a, j, s = formula_rows(pos, vel, acc_in, eps2, np.array(sorted({0, 1, 5, 130, 400, 777, N - 1, k})))
    for q, name in ((a, "acc"), (j, "jerk"), (s, "snap")):  # (the rule, from the formulas, on a sample of the bodies)
        assert (~np.isfinite(q)).all() if reached[name] else np.isfinite(q).all(), name
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    got4 = dict(acc=d.get("acc"), jerk=d.get("jerk"))
    d.step(dtype(1.0 / 128), new="pos2", old="pos")
    new_pos, new_vel = d.get("pos2"), d.get("vel")
    d.free()
    assert new_pos[:, 3].tobytes() == pos[:, 3].tobytes() and new_vel[:, 3].tobytes() == vel[:, 3].tobytes()
    got6 = dict(zip(("acc", "jerk", "snap"), evaluate6(gpu, pos, vel, acc_in, eps2)))
    for got in (got4, got6):
        for name, q in got.items():
            bad = ~np.isfinite(q[:, :3])
            assert bad.all() if reached[name] else not bad.any(), (name, int(bad.sum()))
            assert q[:, 3].tobytes() == np.zeros(N, dtype).tobytes(), name


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_poisoned_source_that_every_target_excludes(gpu, dtype):
    """nb_field_eval_*: exclusion is "mass 0".  A source of infinite or NaN mass that every target excludes by index reaches nothing:
    the outputs are the bits of the call with that mass 0.  One with a NaN coordinate reaches every target (0 * NaN), as the
    formulas say."""
    src, src_vel = cloud(N_SMALL, dtype, 89, "random")
    tgt, tgt_vel = cloud(300, dtype, 97, "equal")
    k = 133  # (in the ragged second chunk of 200 sources)
    self_index = np.full(300, k, np.uint32)
    outputs = ("acc", "jerk", "pot")
    clean = src.copy()
    clean[k, 3] = 0
    want = field_run(gpu, clean, tgt, src_vel, tgt_vel, None, dtype(0.01), outputs)
    assert all(np.isfinite(want[o]).all() for o in outputs)
    for mass in (np.inf, -np.inf, np.nan):
        src[k, 3] = mass
        out = field_run(gpu, src, tgt, src_vel, tgt_vel, self_index, dtype(0.01), outputs)
        for o in outputs:
            assert out[o].tobytes() == want[o].tobytes(), (mass, o)
    src[k, 3], src[k, 0] = 1.0, np.nan
    out = field_run(gpu, src, tgt, src_vel, tgt_vel, self_index, dtype(0.01), outputs)
    assert np.isnan(out["acc"][:, :3]).all() and np.isnan(out["jerk"][:, :3]).all() and np.isnan(out["pot"]).all()


# ---------------------------------------------------------------------------------------------- 6. the time-step rules
def timestep_arrays(dtype, e, low):
    """300 hand-made accelerations and jerks whose magnitudes are 2^-e, 1 and 2^e, mixed; bodies 5 and 9 are left out (|jerk| = 0, a
    NaN).  low: some bodies have |a| ~ 2^-e against |jerk| ~ 1, so the minimum is ~2^-e; else |a| and |jerk| of a body are of one
    size and the minimum, ~1/64, sits at a body of 2^-e (the next at one of 2^e)."""
    rng = np.random.default_rng(101 + e)
    n = 300
    acc, jerk = np.zeros((n, 4), np.float64), np.zeros((n, 4), np.float64)
    acc[:, :3], jerk[:, :3] = rng.standard_normal((n, 3)) + 3, rng.standard_normal((n, 3)) * 0.25 + 1
    pairs = [(-e, -e), (e, e), (0, 0), (e, 0), (0, -e)] + ([(-e, 0)] if low else [])
    ea, ej = np.array([pairs[i % len(pairs)] for i in range(n)]).T
    acc[:, :3] *= 2.0 ** ea[:, None]
    jerk[:, :3] *= 2.0 ** ej[:, None]
    acc[10, :3] /= 64   # (-e, -e)
    acc[16, :3] /= 32   # (e, e)
    jerk[11 if len(pairs) == 5 else 13, 1] = 0  # (a zero component among huge ones)
    jerk[5, :3] = 0
    jerk[9, 0] = np.nan
    return acc.astype(dtype), jerk.astype(dtype)


def timestep_rule(acc, jerk, eta):
    """the header's rule in long double: eta min |a| / |jerk| over the bodies with |jerk| > 0 and a finite ratio"""
    a, j = norm(acc[:, :3].astype(LD)), norm(jerk[:, :3].astype(LD))
    with np.errstate(all="ignore"):
        ratio = a / j
    keep = (j > 0) & np.isfinite(ratio)
    return LD(eta) * ratio[keep].min(), int(np.flatnonzero(keep)[np.argmin(ratio[keep])])


TIMESTEP_CASES = [(np.float32, 100, False), (np.float32, 100, True)] + [(np.float64, e, low) for e in (300, 520, 900) for low in (False, True)]


@gpu_only
@pytest.mark.parametrize("dtype,e,low", TIMESTEP_CASES)
def test_shared_time_step_at_extreme_magnitudes(gpu, dtype, e, low):
    """nb_hermite_timestep_* and nb_hermite_ensemble_timestep_* on accelerations and jerks of 2^+-e: the header's rule to 2u wherever
    the exact ratio is representable.  In plain fp64 |jerk|^2 underflowed from 2^-538 (the body was left out, or the result was 0
    where |a|^2 did) and overflowed from 2^512 (inf / inf: left out); the norms are scaled by a power of two each now."""
    acc, jerk = timestep_arrays(dtype, e, low)
    eta, u = dtype(0.02), UNIT_ROUNDOFF[dtype]
    want, body = timestep_rule(acc, jerk, eta)
    assert normal_in(dtype, want) and (abs(np.log2(norm(acc[body, :3].astype(LD)))) > e - 8)  # (the minimum sits at an extreme body)
    n = acc.shape[0]
    zeros = np.zeros((n, 4), dtype)
    d = Device(gpu, zeros, zeros, dtype(0.01))
    d.put("acc", acc), d.put("jerk", jerk)
    got = solo_timestep(gpu, d, eta)
    d.free()
    print(f"2^+-{e} {'low' if low else 'level'}: dt {got}, rule {float(want):.17g} at body {body}")
    assert np.isfinite(got) and got > 0
    assert abs(LD(got) - want) <= 2 * u * want, (got, want)
    others = [timestep_arrays(dtype, e2, not low) for e2 in ((50, 100) if dtype == np.float32 else (520, 900))]
    ens = Ensemble(gpu, np.zeros((3, n, 4), dtype), np.zeros((3, n, 4), dtype), dtype(0.01))
    ens.put("acc", np.stack([others[0][0], acc, others[1][0]])), ens.put("jerk", np.stack([others[0][1], jerk, others[1][1]]))
    dts = ens.timestep(eta)
    ens.free()
    assert dts[1].tobytes() == got.tobytes()
    for s, (a, j) in zip((0, 2), others):
        rule = timestep_rule(a, j, eta)[0]
        assert abs(LD(dts[s]) - rule) <= 2 * u * rule, (s, dts[s], rule)


def timestep6_arrays(dtype, e):
    """300 hand-made accelerations, jerks, snaps and crackles whose norms are 2^e, 2^-e and 1 in turn; beyond the range (e > 250) body 2
    has |a|^2 and |c|^2 underflow to 0 beside products that do not -- it gives the step the surviving products give"""
    rng = np.random.default_rng(103 + e)
    n = 300
    arrays = [rng.standard_normal((n, 4)) + 2 for _ in range(4)]
    scale = np.where(np.arange(n) % 3 == 0, 2.0 ** e, np.where(np.arange(n) % 3 == 1, 2.0 ** -e, 1.0))[:, None]
    arrays = [(q * scale).astype(dtype) for q in arrays]
    if e > 250:
        for q, p2 in zip(arrays, (-600, -100, 400, -600)):
            q[2] *= 2.0 ** p2
    for q in arrays:
        q[:, 3] = 0
    return arrays


def timestep6_rule(arrays, e, eta):
    """(the step in long double, the rows that count): inside the header's range Aarseth's rule over all bodies; beyond it the header's
    outcome -- the expression in plain fp64, bodies with a bad denominator or ratio left out, which are the ordinary bodies and body 2"""
    n = arrays[0].shape[0]
    a, j, s, c = (norm(q[:, :3].astype(LD)) for q in arrays)
    ratio = (a * s + j * j) / (j * c + s * s)
    ordinary = None
    if e > 250:
        ordinary = np.flatnonzero(np.arange(n) % 3 == 2)
        with np.errstate(all="ignore"):
            a2, j2, s2, c2 = ((q[:, :3].astype(np.float64) ** 2).sum(axis=1) for q in arrays)
            den = np.sqrt(j2 * c2) + s2
            plain = (np.sqrt(a2 * s2) + j2) / den
        kept = (den > 0) & np.isfinite(plain)
        assert set(np.flatnonzero(kept)) == set(ordinary) and np.argmin(np.where(kept, plain, np.inf)) == 2 and plain[2] < ratio[2] / 1.5
        ratio = plain[kept].astype(LD)
    return LD(eta) * np.sqrt(ratio.min()), ordinary


TIMESTEP6_CASES = [(np.float32, 100), (np.float64, 100), (np.float64, 245), (np.float64, 600)]


@gpu_only
@pytest.mark.parametrize("dtype,e", TIMESTEP6_CASES)
def test_hermite6_time_step_on_both_sides_of_its_range(gpu, dtype, e):
    """nb_hermite6_timestep_* forms plain fp64 products of two norms.  Inside the header's range (fp32: always; fp64: norms within
    2^+-250) it follows Aarseth's rule to the bound of tests/test_hermite6.py; beyond it (2^+-600) a body whose products overflow, or
    all underflow to 0, is left out -- the result is that of the other bodies alone, bit for bit, never NaN -- and a body of which
    only some products underflow gives the step the surviving ones give (here a smaller one than the exact rule's)."""
    f, scalar = hermite6_fns(gpu, dtype)
    n, eta = 300, dtype(0.02)
    arrays = timestep6_arrays(dtype, e)

    def timestep(rows):
        zeros = np.zeros((len(rows), 4), dtype)
        d = Device6(gpu, zeros, zeros, dtype(0.01))
        for key, q in zip(("acc", "jerk", "snap", "crackle"), arrays):
            d.put(key, q[rows])
        out, scratch = gpu.DeviceBuffer(8), gpu.DeviceBuffer(8192)
        gpu.check(f["timestep"](d.ptr("acc"), d.ptr("jerk"), d.ptr("snap"), d.ptr("crackle"), len(rows), scalar(eta), out.ptr, scratch.ptr, 8192, None), "nb_hermite6_timestep")
        dt = out.download(np.empty(1, dtype))[0]
        out.free(), scratch.free(), d.free()
        return dt

    got = timestep(np.arange(n))
    want, ordinary = timestep6_rule(arrays, e, eta)
    if ordinary is not None:
        assert got.tobytes() == timestep(ordinary).tobytes() and np.isfinite(got) and got > 0
    allowed = TIMESTEP6_ALLOWED[dtype]
    assert abs(LD(got) - want) <= allowed * want, (got, want)


TIMESTEP6_ALLOWED = {np.float32: 2 * float(np.finfo(np.float32).eps), np.float64: 1e-14}


@pytest.mark.parametrize("dtype,e,low", TIMESTEP_CASES)
def test_the_time_step_arrays_have_a_normal_rule(dtype, e, low):
    """the header's rule on the hand-made arrays is a normal T, and it sits at a body of extreme magnitude"""
    acc, jerk = timestep_arrays(dtype, e, low)
    want, body = timestep_rule(acc, jerk, dtype(0.02))
    assert normal_in(dtype, want) and abs(np.log2(norm(acc[body, :3].astype(LD)))) > e - 8


# ---------------------------------------------------------------------------------------------- 7. the block scheme
def tiny_tick(dtype):
    return 2.0 ** (-100 if dtype == np.float32 else -1000)


def block_sums(gpu, pos, vel, eps2):
    """a1, j1 of every body from ONE block step in which all bodies are due (level 0, tick 0, stored a = jerk = 0), through the partial
    planes and the finish kernel, and the predicted state they are the sums of.  The step is so short (2^-100 / 2^-1000) that the
    predictor returns the stored state wherever v dt is below half an ulp of x."""
    dtype, n = pos.dtype.type, pos.shape[0]
    d = BlockDevice(gpu, pos, vel, eps2, gpu.HermiteBlockParams(0.02, 0.01, tiny_tick(dtype), 0, 0))
    d.step()
    status = d.status()
    assert (status.last_active, status.flags) == (n, 0)
    out = d.get("acc"), d.get("jerk"), d.get("ws")
    d.free()
    return out


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_term_block(gpu, dtype):
    """hermite_block_eval and hermite_block_finish: the one-term sweep of test_one_term_across_the_exponent_range, near body in a
    unit chunk (the planes are in units of its mass) and in a mixed one."""
    name = np.dtype(dtype).name
    worst = {}
    for eps2, d2 in probe_sets(dtype):
        pos_p, vel_p, acc_p = probes(dtype, d2)
        terms, sizes, _ = one_term(dtype, pos_p, vel_p, acc_p, eps2)
        for layout in ("unit", "mixed"):
            pos, vel, _ = one_sided_system(dtype, layout, pos_p, vel_p, acc_p)
            acc, jerk, predicted = block_sums(gpu, pos, vel, dtype(eps2))
            # the sums are those of the PREDICTED state: the stored one, but for z = 0 + v_z dt of the probes (2^-100 / 2^-1000 of d)
            assert predicted[:, [0, 1, 3]].tobytes() == pos[:, [0, 1, 3]].tobytes() and predicted[:, 4:7].tobytes() == np.ascontiguousarray(vel[:, :3]).tobytes()
            assert not predicted[:128, 2].any() and (np.abs(predicted[128:, 2]) <= np.abs(pos_p[:, 0]) * tiny_tick(dtype)).all()
            terms, sizes, _ = one_term(dtype, predicted[128:, 0:4], predicted[128:, 4:8], acc_p, eps2)
            for output, err in term_errors(dtype, dict(acc=acc[128:, :3], jerk=jerk[128:, :3]), terms, sizes).items():
                assert np.isfinite(err).all(), (eps2, layout, output)
                worst[output] = max(worst.get(output, 0.0), float(err.max()))
    for output, value in worst.items():
        print(f"one term hermite_block_eval {name} {output}: max error over the term's magnitude {value:.3e} (bar {bar('hermite_block_eval', name, output):.3e})")
    for output, value in worst.items():
        assert value <= bar("hermite_block_eval", name, output), (output, value)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(7))
def test_block_stages_with_first_bodies_around_the_unit_window(gpu, dtype, index):
    """check_block_stages on the first-body systems: the planes are in units of the first body's mass on the window's edge, in plain
    units just outside it and at 0, -0.0 and a negative mass"""
    value = mass_values(dtype)[index]
    pos, vel = mass_system(dtype, N, "first", value)
    check_block_stages_of(gpu, pos, vel, dtype(0.01), 129, f"first {value}", 4e-3)


@gpu_only
@pytest.mark.parametrize("dtype,mexp", [(np.float32, 40), (np.float32, 60), (np.float64, 60), (np.float64, 100)])
def test_block_stages_with_species_at_opposite_mass_edges(gpu, dtype, mexp):
    """... and on the contiguous species; dt_max is the largest power of two up to 1/8 that keeps every PREDICTED coordinate (the oldest
    body is 600 ticks = 2.35 dt_max behind) within 2^40, as test_contiguous_species_at_opposite_mass_edges chooses its dt"""
    pos, vel = species_system(dtype, mexp)
    a, j = (float(np.abs(q).max()) for q in reference(pos, vel, dtype(0.01))[:2])
    dt_max = 0.125
    while dtype == np.float32 and 4 + 2 * (2.35 * dt_max) + a * (2.35 * dt_max) ** 2 / 2 + j * (2.35 * dt_max) ** 3 / 6 > 2.0 ** 40:
        dt_max /= 2
    assert dt_max >= 2.0 ** -20
    check_block_stages_of(gpu, pos, vel, dtype(0.01), 129, f"species 2^+-{mexp}", 4e-3, dt_max=dt_max)


@gpu_only
@pytest.mark.parametrize("name,lo", [("float32", -20), ("float64", -60)])
def test_block_sums_on_both_sides_of_their_cap(gpu, name, lo):
    """The block kernels keep their partial planes in units of the first body's mass: the header caps the sums of term magnitudes at
    2^126 |m_0| (2^1022 |m_0|).  The close-pair system with velocities 2^lo times the largest of section 3 sits on that cap and meets
    the bound; with the largest ones (J_i up to 2^126 / 2^1022) the bodies under the cap still meet it, and heavy bodies far beyond it
    have infinite or NaN jerks, as the header says."""
    dtype = np.dtype(name).type
    pos, vel, eps2, _ = close_pair_system(name, lo, 4)
    cap = LD(2.0) ** (WINDOW[dtype]["sums"] + lo)
    slow = vel.copy()
    slow[:, :3] = vel[:, :3] * dtype(2.0 ** lo)
    acc, jerk, predicted = block_sums(gpu, pos, slow, eps2)
    assert reference(predicted[:, 0:4], predicted[:, 4:8], eps2)[3].max() <= cap * (1 + 1e-6)
    check_eval(acc, jerk, predicted[:, 0:4], predicted[:, 4:8], eps2, f"block sums on their cap behind 2^{lo}")
    acc, jerk, predicted = block_sums(gpu, pos, vel, eps2)
    size = reference(predicted[:, 0:4], predicted[:, 4:8], eps2)[3].max(axis=1)
    under, beyond = np.flatnonzero(size <= cap), np.flatnonzero(size > cap * 2.0 ** 10)
    assert under.size >= 64 and beyond.size >= 64
    check_eval(acc, jerk, predicted[:, 0:4], predicted[:, 4:8], eps2, f"block sums under their cap behind 2^{lo}", rows=under)
    assert not np.isfinite(jerk[beyond, :3]).all(axis=1).any()


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_block_ensemble_systems_with_first_bodies_of_their_own(gpu, dtype):
    """nb_hermite_block_ensemble_step_*: one launch of three systems whose first bodies weigh 2^20 (2^60), 2^-21 (2^-61) and 0, with
    129, all and 1 bodies due: the unit of a system's planes is its own first body's mass, so after 1 and 3 calls every system holds
    the bits of the solo block steps."""
    e = WINDOW[dtype]["unit"]
    params, eps2 = gpu.HermiteBlockParams(0.02, 0.01, 0.125, 8, 0), dtype(0.01)
    systems = []
    for s, (value, n_act) in enumerate(((2.0 ** e, 129), (2.0 ** -(e + 1), N), (0.0, 1))):
        pos, vel = mass_system(dtype, N, "first", value)
        if s == 0:
            pos[128:256, 3] = 2.0 ** e  # (a unit chunk)
        now, max_level, active, levels, ticks = hand_made_schedule(N, n_act, 900 + s)
        assert max_level == params.max_level
        acc, jerk = solo_start(gpu, pos, vel, eps2, params)
        systems.append((pos, vel, acc, jerk, (ticks + 256 * s).astype(np.uint64), levels.astype(np.int32), now + 256 * s))
    ens = load_ensemble(gpu, params, systems, eps2)
    got = {}
    for k in (1, 2, 3):
        ens.step()
        got[k] = ens.everything()
    assert ens.canaries_intact()
    ens.free()
    for s, system in enumerate(systems):
        want = solo_bytes(gpu, params, system, eps2, (1, 3))
        for k in (1, 3):
            assert got[k][s] == want[k], (s, k)


def two_bodies(e):
    """two fp64 bodies whose accelerations are 2^e and jerks 2^(e-3): masses 2^+-100, r = 2^((+-100 - e) / 2) along x, w = r / 8 along y"""
    m = 2.0 ** (100 if e > 0 else -100)
    r = 2.0 ** (((100 if e > 0 else -100) - e) / 2)
    pos, vel = np.zeros((2, 4)), np.zeros((2, 4))
    pos[:, 3], pos[1, 0], vel[1, 1] = m, r, r / 8
    return pos, vel, np.float64(r * r * 2.0 ** -60)


@gpu_only
@pytest.mark.parametrize("e", [240, -240, 600, -600])
def test_block_levels_on_both_sides_of_the_range_of_dt_a(gpu, e):
    """init's want = eta_start |a| / |jerk| and the step's dt_A are plain fp64 expressions of squares and products of two norms.  With
    norms of 2^+-240, inside the header's range, the levels are the long double rule's; with 2^+-600 the squares overflow or
    underflow and the header's outcome holds: init takes dt_max (level 0); dt_A is what the expression gives in fp64 -- dt_max where
    it is infinite or NaN -- never a level out of range."""
    pos, vel, eps2 = two_bodies(e)
    # (accelerations of 2^600 over a step of 1/8 would throw the pair 2^593 apart, s^2 beyond fp64: that case steps by 2^-430, a h^2 < r)
    params = gpu.HermiteBlockParams(0.02, 0.01, 2.0 ** -430 if e == 600 else 0.125, 8, 0)
    d = BlockDevice(gpu, pos, vel, eps2, params)
    d.init()
    acc, jerk, levels0 = d.get("acc"), d.get("jerk"), d.get("levels").astype(np.int64)
    assert np.isfinite(acc).all() and np.isfinite(jerk).all() and abs(np.log2(norm(acc[:, :3].astype(LD))) - e).max() < 1
    inside = abs(e) <= 250
    rule = first_levels(acc[:, :3].astype(LD), jerk[:, :3].astype(LD), LD(params.eta_start), LD(params.dt_max), params.max_level)[0]
    assert (levels0 == (rule if inside else 0)).all(), (levels0, rule)
    assert (rule == (0 if e == 600 else 1)).all()  # (want = 0.08: between 1/16 and 1/8, far from either; far above 2^-430)
    d.step()
    a1, j1, levels1 = d.get("acc"), d.get("jerk"), d.get("levels").astype(np.int64)
    status = d.status()
    d.free()
    assert status.last_active == 2 and np.isfinite(a1).all() and np.isfinite(j1).all()
    kind = LD if inside else np.float64
    h = (params.dt_max * 2.0 ** -levels0).astype(kind)
    with np.errstate(all="ignore"):
        dt_a = aarseth(*(q[:, :3].astype(kind) for q in (acc, jerk, a1, j1)), h, kind(params.eta), kind(params.dt_max))
    want, rel = new_levels(levels0, dt_a, status.now_ticks, params.dt_max, params.max_level)
    print(f"norms of 2^{e}: levels {levels0} -> {levels1}, dt_A {dt_a}, rule {want} (distance from a threshold {rel})")
    if inside:
        assert (rel > 1e-6).all()
    else:
        assert (dt_a == params.dt_max).all()  # (the fp64 expression is infinite or NaN: dt_max exactly, no rounding to be near to)
    assert (levels1 == want).all() and ((0 <= levels1) & (levels1 <= params.max_level)).all()


@gpu_only
@pytest.mark.parametrize("name,lo", [("float32", -20), ("float64", -60)])
def test_the_escape_to_plain_units_in_the_step_and_the_ensemble(gpu, name, lo):
    """The heavy close pairs behind a light first body through the STEP kernel (dt = 0 predicts the stored state) and as one system of
    an ensemble launch beside an ordinary one: the bound, and the bits of the solo call."""
    dtype = np.dtype(name).type
    pos, vel, eps2, _ = close_pair_system(name, lo, 4)
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    solo = d.get("acc"), d.get("jerk")
    d.step(dtype(0), new="pos2", old="pos")
    stepped = d.get("acc"), d.get("jerk")
    d.free()
    check_eval(*stepped, pos, vel, eps2, f"STEP kernel, heavy close pairs behind 2^{lo}")
    other = mass_system(dtype, N, "first", 0.75)
    ens = Ensemble(gpu, np.stack([other[0], pos]), np.stack([other[1], vel]), np.array([0.01, eps2], dtype))
    ens.eval()
    acc, jerk = ens.get("acc"), ens.get("jerk")
    ens.free()
    assert acc[1].tobytes() == solo[0].tobytes() and jerk[1].tobytes() == solo[1].tobytes()
