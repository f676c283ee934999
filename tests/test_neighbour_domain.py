"""The neighbour and k-NN surveys over their operand range (the "Operand range" paragraphs of include/nbody_hip_neighbour.h and
nbody_hip_knn.h), as tests/test_fast_domain.py, test_hermite_domain.py and test_hermite6_domain.py hold the integrators to theirs.

CPU part:
  C1  no case is dropped: every lattice, probe set and density state below has a reference that is exact (lattices: integers times a
      power of two) or finite in long double, and says which outputs are normal in T and which are exactly 0, +-inf or NONE;
  C2  the two formulas that have intermediates, restated in numpy over every binade of double: the fp64 series of 1 / sqrt(s2) round a
      seed of relative error 2^-23, and the density cube with the record's rho x, rho^2, rho^2 r2.  The largest windows in which every
      intermediate is a normal double are window(T), and
  C3  window(T) is what the two headers state;
  C4  rho_ld (tests/test_knn.py), the long double density, against numpy_density on the hand-made state.
GPU part (MI355X), N = 300 and 1 025 (two and four waves per group, a ragged last tile and chunk, the lists' range split):
  G1  the exact relations on lattices times 2^e -- every d2 is exact in T, so numpy holds bit for bit -- with d2 (a) normal at the
      bottom, (b) partly subnormal, (c) the smallest attainable subnormals, (d) finite at the top, (e) partly overflowed; radii on an
      attained d2 (the strict `<`), its successor, +inf, and per body a mix of subnormal, huge, +inf, NaN and negative ones;
  G2  bodies at +-inf, two at one infinity, -0.0 beside +0.0, a NaN or +inf mass, in both libraries;
  G3  ONE potential term over the whole normal range of T against -m / sqrt(d2 + eps2) in long double (POTENTIAL_MEASURED); subnormal
      s2, and fp64 s2 from 2^1021, as launches of their own;
  G4  densities and the record: fp32 from the smallest subnormal d_K^2 to 2^127 with masses over 2^+-100; fp64 on both edges of both
      windows of C2 and beyond them.
The references and device wrappers are those of the sister modules."""
import functools
import os

import numpy as np
import pytest

from conftest import ROOT
from test_fast_domain import CAP, TOL, UNIT_ROUNDOFF
from test_hermite import LD
from test_knn import DEGENERATE, KS, NO_DENSITY, NONE, SPHERE, numpy_density, numpy_knn, numpy_structure, rho_ld
from test_knn_gpu import KnnDevice, check_lists, check_sums
from test_neighbour import NeighbourDevice, check_exact, lattice, numpy_status, numpy_survey, run_both

gpu_only = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
SIZES = (300, 1025)
REACHES = (2, 64)
F64 = np.finfo(np.float64)


def normal_in(dtype, x):
    """x (long double), rounded to T, is finite and normal -- or exactly 0 where x is"""
    x = np.asarray(x, LD)
    with np.errstate(all="ignore"):
        t = x.astype(dtype)
    return np.isfinite(t) & (((t == 0) & (x == 0)) | (np.abs(t) >= np.finfo(dtype).tiny))


def normal64(x):
    """a double that is finite, nonzero and not subnormal"""
    return np.isfinite(x) & (np.abs(x) >= F64.tiny)


# ---------------------------------------------------------------------------------------------- C2. the windows, from the arithmetic
MANTISSAS = np.array([1.0, 1.0 + 2.0 ** -52, 1.25, 1.5, 1.75, 2.0 - 2.0 ** -52])
BINADES = np.arange(F64.minexp - F64.nmant, F64.maxexp)  # -1074 .. 1023: every binade of double, the subnormal ones included


def run_round(ok, at=0):
    """the largest run of binades round `at` in which `ok` holds throughout: (lo, hi), the operands of [2^lo, 2^hi)"""
    k = int(np.flatnonzero(BINADES == at)[0])
    assert ok[k]
    lo = hi = k
    while lo > 0 and ok[lo - 1]:
        lo -= 1
    while hi + 1 < len(ok) and ok[hi + 1]:
        hi += 1
    return int(BINADES[lo]), int(BINADES[hi]) + 1


def every_binade():
    """(len(BINADES), len(MANTISSAS)) doubles; in a subnormal binade the mantissa loses its low bits, the value stays in the binade"""
    with np.errstate(under="ignore"):
        return np.ldexp(MANTISSAS[None, :], BINADES[:, None])


@functools.lru_cache(maxsize=None)
def series_window():
    """inv_sqrt(double) of csrc/neighbour.hip in numpy: y0 = the exact 1 / sqrt(s2) times (1 +- 2^-23), r = fma(-s2, y0 y0, 1),
    y = fma(y0 r, fma(r, 3/8, 1/2), y0).  The intermediates are s2, y0, y0 y0, y0 r and y (r may be 0; the product inside an fma is
    not rounded).  -> (lo, hi, the largest relative error of y inside the window)"""
    s2 = every_binade()[:, :, None]
    seed = np.array([-2.0 ** -23, -2.0 ** -24, 0.0, 2.0 ** -24, 2.0 ** -23])[None, None, :]
    with np.errstate(all="ignore"):
        exact = 1 / np.sqrt(s2.astype(LD))
        y0 = (exact * (1 + seed.astype(LD))).astype(np.float64)
        square = y0 * y0
        r = (1 - s2.astype(LD) * square.astype(LD)).astype(np.float64)  # (the fused operation: one rounding)
        y0r = y0 * r
        y = (y0r.astype(LD) * (r * 0.375 + 0.5).astype(LD) + y0.astype(LD)).astype(np.float64)
        fine = normal64(s2) & normal64(y0) & normal64(square) & np.isfinite(r) & (normal64(y0r) | (r == 0)) & normal64(y)
        err = np.abs(y.astype(LD) - exact) / exact
    ok = fine.all(axis=(1, 2))
    lo, hi = run_round(ok)
    inside = (BINADES >= lo) & (BINADES < hi)
    return lo, hi, float(err[inside].max())


@functools.lru_cache(maxsize=None)
def density_windows():
    """The density and the record's terms in double, of a body with M_i = 1 at a distance of the order of d_K from the density centre:
    cube = d_K^2 sqrt(d_K^2), c cube, rho = 1 / (c cube); rho x and rho |x - x_d| with x = |x - x_d| = sqrt(d_K^2); rho^2; rho^2 |x - x_d|^2.
    -> ((lo, hi) where the cube is a normal double and c cube finite: the density is given by the formula, (lo, hi) where every one of them
    is normal)"""
    dk = every_binade()
    with np.errstate(all="ignore"):
        root = np.sqrt(dk)
        cube = dk * root
        volume = SPHERE * cube
        rho = 1.0 / volume
        terms = (rho * root, rho * rho, (rho * rho) * dk)
    defined = (normal64(cube) & np.isfinite(volume) & (dk > 0)).all(axis=1)
    everything = defined & normal64(volume).all(axis=1) & normal64(rho).all(axis=1)
    for t in terms:
        everything &= normal64(t).all(axis=1)
    return run_round(defined), run_round(everything)


def window(dtype):
    """the "Operand range" of the two headers as exponents of two, every pair the operands of [2^lo, 2^hi)"""
    fi = np.finfo(dtype)
    cube, record = density_windows()
    s2 = (int(fi.minexp), int(fi.maxexp)) if dtype == np.float32 else series_window()[:2]  # fp32: one v_rsq_f32, no intermediate
    return dict(s2=s2, cube=cube, record=record)


def test_the_windows_come_out_of_the_arithmetic():
    """C2.  fp64 potential: the square of a seed that is 2^-23 low is subnormal from s2 = 2^1022 (1 - 2^-22), in the binade of 2^1021
    (and infinite below 2^-1024, where s2 is no normal double anyway); inside the window the series is within 2^-53 of the exact value.  Density: the cube is a normal double and c
    times it finite for d_K^2 in [2^-681, 2^681), every term of the record for unit masses in [2^-342, 2^339): rho^2 is what leaves first."""
    lo, hi, err = series_window()
    assert (lo, hi) == (-1022, 1021) and err < 2.0 ** -53, (lo, hi, err)
    cube, record = density_windows()
    assert cube == (-681, 681) and record == (-342, 339), (cube, record)
    # outside: the old rule `0 < d_K^2 < inf` gave +inf, or 0 for a body it counted as defined (already where only c cube overflows)
    with np.errstate(all="ignore"):
        for dk, bad in ((2.0 ** -720, np.inf), (2.0 ** 684, 0.0), (2.0 ** 682, 0.0)):
            assert 0 < dk < np.inf and 1.0 / (SPHERE * (dk * np.sqrt(dk))) == bad


def test_fp32_densities_need_no_window():
    """C2, fp32: d_K^2 is a float widened to double, from the smallest subnormal to the largest finite one; with masses of 2^+-100 (M_i:
    one to fifteen of them) and |x|, |x - x_d| from the smallest subnormal float to 2^65, nothing in double leaves its range: the
    whole of T is the window."""
    fi = np.finfo(np.float32)
    dk = np.ldexp(1.0, np.arange(fi.minexp - fi.nmant, fi.maxexp))[:, None, None]
    mass = np.array([2.0 ** -100, 1.0, 15 * 2.0 ** 100])[None, :, None]
    x = np.array([2.0 ** -149, 1.0, 2.0 ** 65])[None, None, :]
    with np.errstate(all="raise"):
        cube = dk * np.sqrt(dk)
        rho = mass / (SPHERE * cube)
        for q in (cube, rho, rho * x, rho * rho, (rho * rho) * (x * x), (1 << 24) * (rho * rho) * (x * x)):
            assert normal64(q).all()
    assert window(np.float32)["s2"] == (-126, 128)


# ---------------------------------------------------------------------------------------------- C3. the headers
def header_text(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return " ".join(text.replace("\n *", " ").split())


def test_the_window_is_the_one_the_headers_state():
    f32, f64 = window(np.float32), window(np.float64)
    text = header_text("nbody_hip_neighbour.h")
    paragraph = text[text.index("Operand range."):]
    assert f"[2^{f32['s2'][0]}, 2^{f32['s2'][1]}) (fp32) / [2^{f64['s2'][0]}, 2^{f64['s2'][1]}) (fp64)" in paragraph
    assert f"{CAP['float32']:.0e} (fp32) / {CAP['float64']:.0e} (fp64)".replace("e-0", "e-") in paragraph
    for phrase in ("a subnormal d2 is not 0", "a d2 that overflows is +inf and nobody's neighbour, even at a radius of +inf"):
        assert phrase in paragraph, phrase
    text = header_text("nbody_hip_knn.h")
    paragraph = text[text.index("Operand range."):]
    assert f"d_K^2 in [2^{f64['cube'][0]}, 2^{f64['cube'][1]})" in paragraph
    assert f"d_K^2 in [2^{f64['record'][0]}, 2^{f64['record'][1]})" in paragraph
    assert "[2^-511, 2^511]" in paragraph and '"Operand range" of nbody_hip_neighbour.h' in paragraph
    assert "or when the cube d_K^2 * sqrt(d_K^2) is not a positive normal double or c times it is not finite" in text
    source = open(os.path.join(ROOT, "cuda-nbody_amd", "csrc", "knn.hip")).read()
    assert "cube >= 0x1p-1022 && volume < infinity<double>()" in source and "volume = NB_KNN_SPHERE * cube" in source
    assert CAP == {"float32": 1e-6, "float64": 1e-14}


# ---------------------------------------------------------------------------------------------- C4. the long double density
def test_rho_ld_agrees_with_numpy_density_on_the_hand_made_state():
    """tests/test_knn.py's five bodies on a line: the two agree to 2 u wherever the density is defined, and define the same bodies"""
    for kind in DTYPES:
        pos = np.zeros((5, 4), kind)
        pos[:, 0] = [0, 1, 1, 3, 5]
        pos[:, 3] = [1, 2, 4, 8, 16]
        index, dist = numpy_knn(pos, 6)
        for k in (1, 2, 3, 4, 5):
            rho, good = numpy_density(pos, index, dist, k)
            ld, good_ld = rho_ld(pos, index, dist, k)
            assert np.array_equal(good, good_ld) and ld.dtype == LD
            assert (np.abs(rho.astype(LD) - ld) <= 2 * UNIT_ROUNDOFF[np.float64] * ld).all(), k
            assert k == 1 or np.array_equal(ld == 0, ~good)
        assert rho_ld(pos, index, dist, 2)[0][3] == LD(2) / (LD(SPHERE) * 8)
    # x87 range through the cube: a d_K^2 of 2^-681 is defined, and its density of 2^1021.5 M / c is a finite double because M is small
    pos = np.zeros((3, 4), np.float64)
    pos[1:, 0], pos[:, 3] = (2.0 ** -341, 2.0 ** -340.5), 2.0 ** -10
    index, dist = numpy_knn(pos, 2)
    ld, good = rho_ld(pos, index, dist, 2)
    assert good[0] and normal_in(np.float64, ld)[0] and abs(ld[0] / (LD(2.0) ** 1011.5 / LD(SPHERE)) - 1) < 1e-15


# ---------------------------------------------------------------------------------------------- G1. lattices times 2^e
CASES = ("a", "b", "c", "d", "e")


def lattice_exponent(dtype, reach, case):
    """e of the factor 2^e.  The lattice's d2 are the integers k < 2^top (reach 64: 3 * 128^2 < 2^16; reach 2: 48 < 2^6) times 2^(2e):
    (a) 2e = the exponent of the smallest normal T: every nonzero d2 is normal;
    (b) k < 4 is ... k < 2^(top - 2) is subnormal, the rest normal;
    (c) 2e = the exponent of the smallest subnormal, which is even in fp64 (-1074: the unit d2 IS the smallest subnormal) and odd in fp32
        (-149: a square of a float is 2^even times a square integer, and 2^-150 (1 + 1) has no exact terms, so 2^-148 -- two units of the
        subnormal grid, the successor of an attained d2 one unit further -- is the smallest d2 a lattice attains exactly);
    (d) the largest even 2e at which every d2 is finite;
    (e) reach 64: k < 256 finite, the rest +inf; reach 2, where every body has more than 16 neighbours at any k: only k = 0, the
        duplicates, finite."""
    fi = np.finfo(dtype)
    top = 16 if reach == 64 else 6
    twice = dict(a=fi.minexp, b=fi.minexp - (top - 2), c=fi.minexp - fi.nmant + (fi.minexp - fi.nmant) % 2, d=(fi.maxexp - top) // 2 * 2,
                 e=fi.maxexp - (8 if reach == 64 else 0))[case]
    assert twice % 2 == 0
    return twice // 2


def scaled(pos, e):
    out = pos.copy()
    out[:, :3] = np.ldexp(pos[:, :3], e)
    return out


@functools.lru_cache(maxsize=None)
def lattice_state(name, n, reach, e):
    """(positions, the lists for K = 16, the integer d2 of every pair as int64 with the diagonal -1): computed once, left unchanged"""
    dtype = np.dtype(name).type
    base = lattice(n, dtype, 100 * n + reach, reach)
    pos = scaled(base, e)
    with np.errstate(over="ignore", under="ignore"):
        index, dist = numpy_knn(pos, 16)
    whole = base[:, :3].astype(np.int64)
    k = ((whole[None, :, :] - whole[:, None, :]) ** 2).sum(axis=2)
    k[np.arange(n), np.arange(n)] = -1
    for a in (pos, index, dist, k):
        a.setflags(write=False)
    return pos, index, dist, k


def exact_d2(dtype, k, e):
    """the integers k times 2^(2e) in T, +inf where that overflows: exact wherever C1 says the state is"""
    with np.errstate(over="ignore"):
        return np.ldexp(k.astype(LD), 2 * e).astype(dtype)


def radii_of_state(dtype, k, e):
    """the smallest positive attained d2 (with its strict `<` only duplicates count), its successor, the median finite attained d2 and
    its successor, +inf.  (Where no positive d2 is finite: 0, which counts nobody, and its successor, which counts the duplicates.)"""
    kind = np.dtype(dtype).type
    d2 = exact_d2(dtype, k[k > 0], e)
    finite = np.sort(d2[np.isfinite(d2)])
    if finite.size == 0:
        finite = np.zeros(1, dtype)
    low, mid = finite[0], finite[len(finite) // 2]
    return [low, np.nextafter(low, kind(np.inf)), mid, np.nextafter(mid, kind(np.inf)), kind(np.inf)]


def mixed_radii(dtype, n, k, e):
    """per body: the smallest subnormal, an attained d2, a huge finite value, +inf, NaN, -1, -0.0"""
    fi, kind = np.finfo(dtype), np.dtype(dtype).type
    low, _, mid, _, _ = radii_of_state(dtype, k, e)
    values = np.array([fi.smallest_subnormal, low, mid, fi.max, np.inf, np.nan, -1.0, -0.0], dtype)
    return values[np.random.default_rng(n).integers(0, len(values), n)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_lattice_is_exact_and_where_its_case_says(dtype):
    """C1 for G1 and G4: in every state numpy's T arithmetic gives the integer d2 times 2^(2e) bit for bit (+inf where that overflows),
    so the kernel's fused form has nothing to round either; and the d2 lie where the case wants them."""
    fi = np.finfo(dtype)
    count = 0
    for n in SIZES:
        for reach in REACHES:
            for case in CASES:
                e = lattice_exponent(dtype, reach, case)
                pos, index, dist, k = lattice_state(np.dtype(dtype).name, n, reach, e)
                assert np.ldexp(np.ldexp(pos[:, :3], -e), e).tobytes() == pos[:, :3].tobytes() and (np.ldexp(pos[:, :3], -e) % 1 == 0).all()
                want = exact_d2(dtype, np.where(k < 0, 0, k), e)
                with np.errstate(over="ignore", under="ignore"):
                    d = pos[None, :, :3] - pos[:, None, :3]
                    d2 = d[:, :, 0] * d[:, :, 0] + (d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2])
                assert d2.dtype == dtype and d2.tobytes() == want.tobytes(), (n, reach, case)
                finite = np.isfinite(want)
                assert (np.ldexp(want[finite].astype(LD), -2 * e) == np.where(k < 0, 0, k)[finite]).all(), "no rounding anywhere"
                positive = want[k > 0]
                subnormal = positive < fi.tiny
                if case == "a":
                    assert not subnormal.any() and positive.min() < 4096 * fi.tiny and (reach == 64 or positive.min() == fi.tiny)
                elif case == "b":
                    assert subnormal.any() and (~subnormal).any() and np.isfinite(positive).all()
                elif case == "c":
                    unit = exact_d2(dtype, np.array([1]), e)[0]
                    assert unit == (fi.smallest_subnormal if dtype == np.float64 else 2 * fi.smallest_subnormal)
                    assert positive.min() == unit * k[k > 0].min() and (reach == 64 or k[k > 0].min() == 1)
                    assert subnormal.all() or reach == 64 and dtype == np.float64 or subnormal.mean() > 0.5
                elif case == "d":
                    assert np.isfinite(positive).all() and positive.max() > fi.max / (4 if reach == 64 else 2)
                else:
                    assert np.isinf(positive).any() and np.isfinite(want[k >= 0]).any() and np.isfinite(positive).any() == (reach == 64)
                    assert (index[:, 15] == NONE).any() and (dist[index == NONE] == np.inf).all(), "ranks past the finite candidates"
                    assert (np.isfinite(dist) == (index != NONE)).all()
                radii = radii_of_state(dtype, k, e)
                assert radii[0] < radii[1] and radii[0] <= radii[2] < radii[3] and (want == radii[0]).any() and (want == radii[2]).any()
                count += 1
    assert count == len(SIZES) * len(REACHES) * len(CASES) == 20


@gpu_only
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_relations_on_scaled_lattices(gpu, dtype, case, n):
    """G1.  The survey's nearest index, nearest d2 and counts, the CSR lists, both status records (check_exact) and the k-NN ranks for
    every K of KS, bit for bit against numpy."""
    kind = np.dtype(dtype).type
    for reach in REACHES:
        e = lattice_exponent(dtype, reach, case)
        pos, index, dist, k = lattice_state(np.dtype(dtype).name, n, reach, e)
        finite_pairs = int(np.isfinite(exact_d2(dtype, k[k >= 0], e)).sum())
        with np.errstate(over="ignore", under="ignore"):
            for radius_sq in radii_of_state(dtype, k, e):
                status = check_exact(gpu, pos, radius_sq=radius_sq)
                if radius_sq == np.inf:
                    assert status["total_neighbours"] == finite_pairs, "everybody at a finite d2, nobody at +inf"
                    assert (finite_pairs < n * (n - 1)) == (case == "e")
            low = check_exact(gpu, pos, radius_sq=kind(np.finfo(dtype).smallest_subnormal))
            assert low["total_neighbours"] == int((k == 0).sum()), "below the smallest subnormal there are only duplicates"
            check_exact(gpu, pos, radii=mixed_radii(dtype, n, k, e))
        for count in KS:
            d = KnnDevice(gpu, pos, count).survey(outputs=("index", "d2"))
            check_lists(d, index, dist, (n, reach, case, count))
            assert d.canaries_intact() and d.get("pos").tobytes() == pos.tobytes()
            d.free()


# ---------------------------------------------------------------------------------------------- G2. non-finite and signed-zero bodies
def special_state(dtype, n):
    """a reach-10 lattice with: body 5 at x = +inf; bodies 40 and 130 at y = +inf (their difference is NaN); the last body at z = -inf;
    body 7 at +0.0 and body 200 at -0.0 in every coordinate (coincident: d2 = 0)"""
    pos = lattice(n, dtype, 17 * n, 10)
    pos[5, 0] = np.inf
    pos[40, 1] = pos[130, 1] = np.inf
    pos[n - 1, 2] = -np.inf
    pos[7, :3], pos[200, :3] = 0.0, -0.0
    return pos


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_special_state_does_what_ieee_says(dtype):
    """C1 for G2, from numpy alone: the bodies at an infinity have no neighbour and are nobody's; the signed zeros are a coincident pair"""
    kind = np.dtype(dtype).type
    for n in SIZES:
        pos = special_state(dtype, n)
        with np.errstate(over="ignore", invalid="ignore"):
            nearest, d2, counts, _, indices, _ = numpy_survey(pos, kind(np.inf))
            index, dist = numpy_knn(pos, 16)
        away = [5, 40, 130, n - 1]
        assert (nearest[away] == NONE).all() and (d2[away] == np.inf).all() and (counts[away] == 0).all() and not np.isin(away, indices).any()
        assert not np.isin(away, index).any() and (index[away] == NONE).all()
        assert counts[0] == n - 1 - len(away) and d2[7] == 0 and d2[200] == 0 and nearest[200] <= 7 and np.signbit(pos[200, 0])
        here = np.flatnonzero((pos[:, :3] == 0).all(axis=1))
        assert nearest[7] == here[here != 7][0] and nearest[200] == here[0], "the lowest j of the coincident bodies"
        assert numpy_status(nearest, d2, counts)["closest_dist_sq"] == 0
        for k in KS[1:]:  # (body 133 of test_a_nonfinite_mass_changes_no_list: among the inner neighbours of some bodies, not of all)
            inner = (index[:, :k - 1] == 133).any(axis=1) & numpy_density(pos, index, dist, k)[1]
            assert inner.any() and not inner.all(), k


@gpu_only
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_and_signed_zero_bodies(gpu, dtype, n):
    """G2, positions: every exact output of both libraries against numpy, at a radius on an attained d2 and at +inf"""
    kind = np.dtype(dtype).type
    pos = special_state(dtype, n)
    with np.errstate(over="ignore", invalid="ignore"):
        for radius_sq in (kind(0), kind(9), kind(np.inf)):
            check_exact(gpu, pos, radius_sq=radius_sq)
        index, dist = numpy_knn(pos, 16)
    for count in KS:
        d = KnnDevice(gpu, pos, count).survey()
        check_lists(d, index, dist, (n, count))
        if count >= 2:
            check_density_outputs(d, pos, index, dist, (n, count), sums=True)
        d.free()


def formula_potentials(pos, eps2):
    """-sum_{j != i} m_j / sqrt(d2 + eps2) and sum |m_j| / sqrt(d2 + eps2) in long double, as the formula stands: non-finite operands are
    data.  The body's own slot adds m_i * 0, as the header says: 0 unless its own mass is not finite."""
    p = pos.astype(LD)
    n = pos.shape[0]
    with np.errstate(all="ignore"):
        d = p[None, :, :3] - p[:, None, :3]
        terms = p[None, :, 3] / np.sqrt((d * d).sum(axis=2) + LD(eps2))
        terms[np.arange(n), np.arange(n)] = p[:, 3] * 0
        return -terms.sum(axis=1), np.abs(terms).sum(axis=1)


@gpu_only
@pytest.mark.parametrize("mass", [np.nan, np.inf])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nonfinite_mass_changes_no_list(gpu, dtype, n, mass):
    """G2, masses.  Body 133 weighs NaN or +inf: every exact output of both libraries has the bits of the state in which it weighs 1;
    the potentials are NaN or -inf exactly where the long double formula is -- every potential: the body's own slot adds m_i * 0 -- and
    with softening and the mass of 1 they are finite and within TOL; the densities of the bodies that have it among their K - 1 inner neighbours, and no others."""
    kind, bad = np.dtype(dtype).type, 133
    clean = special_state(dtype, n)
    clean[bad, 3] = 1
    pos = clean.copy()
    pos[bad, 3] = mass
    r2, eps2 = kind(9), kind(0.25)
    want, size = formula_potentials(pos, eps2)
    assert not np.isfinite(want).any() and np.isnan(want[bad])
    clean_want, clean_size = formula_potentials(clean, eps2)
    finite = np.isfinite(clean_want)
    assert finite.sum() == n - 2, "the two bodies at one infinity are a NaN d2 apart"
    runs = []
    for state in (clean, pos):
        d, survey_status = run_both(gpu, state, None, r2, eps2, capacity=n * n)
        runs.append((b"".join(d.get(name).tobytes() for name in ("nearest", "d2", "counts", "offsets", "indices", "status")), survey_status, d.get("pot")))
        assert d.canaries_intact()
        d.free()
    assert runs[0][:2] == runs[1][:2], "no list, count, distance or status changes"
    pot = runs[1][2]
    assert np.array_equal(np.isnan(pot), np.isnan(want)) and np.array_equal(pot == -np.inf, want == -np.inf) and not (pot == np.inf).any()
    before = runs[0][2]
    assert np.array_equal(np.isnan(before), np.isnan(clean_want)) and np.array_equal(np.isfinite(before), finite)
    assert (np.abs(before[finite].astype(LD) - clean_want[finite]) <= TOL[dtype] * clean_size[finite]).all()
    with np.errstate(over="ignore", invalid="ignore"):
        index, dist = numpy_knn(pos, 16)
    for count in KS[1:]:
        outs = []
        for state in (clean, pos):
            d = KnnDevice(gpu, state, count).survey()
            check_lists(d, index, dist, (n, count))
            outs.append((d.rho64(), d.record()))
            d.free()
        reached = (index[:, :count - 1] == bad).any(axis=1) & numpy_density(clean, index, dist, count)[1]
        assert reached.any() and not reached.all()
        rho = outs[1][0]
        assert (np.isnan(rho) if np.isnan(mass) else rho == np.inf)[reached].all() and rho[~reached].tobytes() == outs[0][0][~reached].tobytes()
        for name in ("defined", "degenerate", "min_kth_dist_sq", "max_kth_dist_sq"):
            assert outs[1][1][name] == outs[0][1][name], name


# ---------------------------------------------------------------------------------------------- G3. one potential term
# Measured maxima (MI355X) of the relative error of ONE term -m / sqrt(d2 + eps2) against the long double term rounded to T, over every
# launch of potential_sets at N = 300 and 1 025; the bar is twice this and never looser than CAP.
POTENTIAL_MEASURED = {"float32": 1.485e-7, "float64": 2.962e-16}  # (fp64, s2 in [2^1021, 2^1024): 2.093e-16)
NEAR_MASS = 1.5
BOTTOM = 8  # binades at the bottom of the normal range that the eps = 0 launch leaves to eps-dominated ones (below)


def potential_sets(dtype, n):
    """[(eps^2, d2 of the n - 1 probes)], the pattern of tests/test_fast_domain.py's sweep_probes over the whole normal range of T:
    eps = 0 with d2 from 2^(lo + BOTTOM) to the top, mantissas off the powers of two; eps-dominated launches (d2 from eps^2 2^-24 to
    eps^2 2^-1/2) at eps^2 = 2^lo ... 2^(lo + BOTTOM - 1) -- s2 in every one of the bottom binades, where with eps = 0 two probes would
    be a subnormal d2 apart --, in the middle, and at 2^(hi - 1): s2 in the top binade of the window [2^lo, 2^hi)."""
    lo, top = window(dtype)["s2"]
    rng = np.random.default_rng(47 + n)
    count = n - 1
    step = (top - 0.05 - (lo + BOTTOM)) / count
    whole = 2.0 ** (lo + BOTTOM + step * np.arange(count, dtype=np.float64).astype(LD)) * rng.uniform(1.0, 2.0 ** min(step, 1.0), count)
    out = [(0.0, whole)]
    middle = (-40, 0, 40) if dtype == np.float32 else (-600, -200, 0, 200, 600)
    for e in (*range(lo, lo + BOTTOM), *middle, top - 1):
        near = 2.0 ** (e + np.linspace(-24, -0.5, count).astype(LD)) * rng.uniform(1.0, 1.25, count)
        out.append((2.0 ** e, near))
    return out


def potential_system(dtype, d2):
    """body 0 of mass 1.5 at the origin; the probes, mass 0, at (+-d, +-d/2, 0) with |r|^2 = d2, the signs taking turns so that probes at
    similar distances are not close to each other"""
    d = np.sqrt(d2 / LD(1.25))
    pos = np.zeros((d.size + 1, 4), dtype)
    turn = np.arange(d.size) % 4
    pos[1:, 0] = (d * np.where(turn & 1, -1, 1)).astype(dtype)
    pos[1:, 1] = (d * LD(0.5) * np.where(turn & 2, -1, 1)).astype(dtype)
    pos[0, 3] = NEAR_MASS
    return pos


def one_term(pos, eps2):
    """-m_0 / sqrt(d2 + eps2) of every probe in long double from the T-typed inputs, d2 by the header's expression; s2 with it"""
    p = pos.astype(LD)
    dx, dy, dz = (p[0, c] - p[1:, c] for c in range(3))
    s2 = dx * dx + (dy * dy + dz * dz) + LD(pos.dtype.type(eps2))
    return -p[0, 3] / np.sqrt(s2), s2


def pairs_in_t(pos, eps2):
    """s2 of every pair of probes in T arithmetic (as numpy_survey forms d2)"""
    with np.errstate(over="ignore", under="ignore"):
        d = pos[None, 1:, :3] - pos[1:, None, :3]
        return d[:, :, 0] * d[:, :, 0] + (d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2]) + pos.dtype.type(eps2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_probe_has_one_finite_normal_term(dtype):
    """C1 for G3.  No probe is dropped: every probe's s2 is a normal T inside the window and its term normal in T; s2 of every pair of
    PROBES (mass 0) is a normal T or +inf, so 1 / s is finite and the pair adds exactly 0 whatever the reciprocal square root does with
    subnormals; together the launches reach every binade of the window."""
    lo, hi = window(dtype)["s2"]
    fi = np.finfo(dtype)
    for n in SIZES:
        count, seen = 0, set()
        for eps2, d2 in potential_sets(dtype, n):
            assert d2.size == n - 1
            pos = potential_system(dtype, d2)
            want, s2 = one_term(pos, eps2)
            assert normal_in(dtype, want).all() and normal_in(dtype, s2).all() and (want != 0).all()
            assert (s2 >= LD(2.0) ** lo).all() and (s2 < LD(2.0) ** hi).all()
            between = pairs_in_t(pos, eps2)
            own = np.eye(n - 1, dtype=bool)
            assert ((between >= fi.tiny) | own).all(), (eps2, float(between[~own].min()))
            if eps2 == 0:
                assert (between[~own] > 0).all(), "no two probes coincide"
            seen |= set(np.floor(np.log2(s2)).astype(int).tolist())
            count += d2.size
        assert count == (n - 1) * len(potential_sets(dtype, n)) and len(potential_sets(dtype, n)) == (13 if dtype == np.float32 else 15)
        assert {lo + b for b in range(BOTTOM)} <= seen and hi - 1 in seen and seen <= set(range(lo, hi))
        if dtype == np.float32 and n == 1025:  # (four probes per binade; fp64 has 2 046 binades for at most 1 024 probes of the eps = 0 launch)
            assert seen == set(range(lo, hi))
        assert len(seen) >= min(hi - lo, (n - 1) // 2)


def probe_errors(d, pos, eps2):
    d.put("pos", pos)
    d.survey(0.0, pos.dtype.type(eps2), outputs=("pot",))
    got = d.get("pot")
    want, _ = one_term(pos, eps2)
    rounded = want.astype(pos.dtype).astype(LD)
    return got, np.abs(got[1:].astype(LD) - rounded) / np.abs(want)


@gpu_only
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_potential_term_across_the_exponent_range(gpu, dtype, n):
    """G3.  Every probe's potential is a single nonzero term -- mass 0 times a finite 1 / s is 0 --, so no summation rounding is left."""
    name = np.dtype(dtype).name
    bar = min(2 * POTENTIAL_MEASURED.get(name, np.inf), CAP[name])
    worst = 0.0
    d = NeighbourDevice(gpu, np.zeros((n, 4), dtype))
    for eps2, d2 in potential_sets(dtype, n):
        pos = potential_system(dtype, d2)
        got, err = probe_errors(d, pos, eps2)
        print(f"one potential term {name} n {n} eps2 {eps2:.3g}: max relative error {float(err.max()):.3e}")
        assert np.isfinite(got).all() and got[0] == 0, eps2
        worst = max(worst, float(err.max()))
    assert d.canaries_intact()
    d.free()
    print(f"one potential term {name} n {n}: max relative error {worst:.3e} (bar {bar:.3e})")
    assert worst <= bar, worst


def edge_values(dtype, low):
    """s2 outside the window: subnormal (the smallest, and mantissas through the subnormal binades), or fp64 from 2^1021 to the top"""
    fi = np.finfo(dtype)
    if low:
        e = np.array([fi.minexp - fi.nmant, fi.minexp - fi.nmant + 1, fi.minexp - 12, fi.minexp - 3, fi.minexp - 1], np.float64)
        return np.ldexp(np.array([1.0, 1.0, 1.3, 1.7, 1.9]), e.astype(int)).astype(dtype)
    return np.ldexp(np.array([1.0, 1.5, 1.99, 1.0, 1.1, 1.5, 1.9, 1.0, 1.1, 1.5, 1.99]), np.array([1021] * 3 + [1022] * 4 + [1023] * 4)).astype(dtype)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_subnormal_s2_is_the_edge_the_header_states(gpu, dtype):
    """G3, below the window, launches of their own: two bodies a normal distance apart whose d2 is 0 or subnormal, and softening_sq
    subnormal, so that s2 is.  As observed on the MI355X and as the header says: fp32, v_rsq_f32 takes a subnormal s2 as 0: the term is
    -m * inf -- -inf for the probe, NaN (0 * inf) for the body that sees the probe's mass of 0; fp64, the series' square of the seed is
    infinite below s2 = 2^-1024: the same -inf and NaN; from there to 2^-1022 the seed and the series hold as they do inside the window."""
    name = np.dtype(dtype).name
    for s2 in edge_values(dtype, low=True):
        pos = np.zeros((2, 4), dtype)
        pos[0, 3] = NEAR_MASS
        d = NeighbourDevice(gpu, pos)
        d.survey(0.0, s2, outputs=("pot", "nearest", "d2"))
        pot, nearest, d2 = d.get("pot"), d.get("nearest"), d.get("d2")
        d.free()
        print(f"subnormal s2 {name} {float(s2):.4g}: potentials {pot[0]!r} (sees mass 0), {pot[1]!r} (sees mass 1.5); exact {float(-LD(NEAR_MASS) / np.sqrt(LD(s2))):.6g}")
        assert nearest.tolist() == [1, 0] and not d2.any(), "the exact outputs do not depend on the softening"
        if dtype == np.float64 and s2 > 2.0 ** -1024 * (1 + 2.0 ** -20):
            want = (-LD(NEAR_MASS) / np.sqrt(LD(s2))).astype(dtype)
            assert pot[0] == 0 and abs(LD(pot[1]) - LD(want)) <= CAP[name] * abs(LD(want)), (float(s2), pot)
        else:
            assert pot[1] == -np.inf and np.isnan(pot[0]), (float(s2), pot)


@gpu_only
def test_the_top_binades_of_fp64_are_beyond_the_window(gpu):
    """G3, above the fp64 window, a launch of its own: s2 in [2^1021, 2^1024), where the square of the seed can be subnormal and r
    loses up to two bits.  Reported; held to CAP, which the header states for it too."""
    dtype = np.float64
    d2 = edge_values(dtype, low=False).astype(LD)
    pos = potential_system(dtype, d2)
    _, s2 = one_term(pos, 0.0)
    assert (s2 >= LD(2.0) ** window(dtype)["s2"][1]).all() and normal_in(dtype, s2).all()
    between = pairs_in_t(pos, 0.0)
    assert ((between >= np.finfo(dtype).tiny) | np.eye(d2.size, dtype=bool)).all()
    d = NeighbourDevice(gpu, pos)
    got, err = probe_errors(d, pos, 0.0)
    d.free()
    print(f"fp64 s2 in [2^1021, 2^1024): max relative error {float(err.max()):.3e} over {err.size} probes")
    assert np.isfinite(got).all() and err.max() <= CAP["float64"]


# ---------------------------------------------------------------------------------------------- G4. densities and the record
# (what, e per reach or a G1 case, m: masses times 2^m, sums: every term of the record is a normal double, so check_sums applies)
DENSITY_CASES = {
    np.float32: [("the smallest subnormals, heavy", "c", 100, True), ("partly subnormal", "b", 0, True), ("the bottom of the normal range, light", "a", -100, True),
                 ("the top, light", "d", -100, True), ("the top, heavy", "d", 100, True), ("partly overflowed", "e", 0, True)],
    np.float64: [("astride the lower edge of the cube", {2: -341, 64: -346}, -10, False), ("astride the upper edge of the cube", {2: 340, 64: 336}, 10, False),
                 ("inside the lower edge of the record", {2: -166, 64: -166}, 0, True), ("inside the upper edge of the record", {2: 160, 64: 160}, 0, True),
                 ("beyond the lower edge of the record", {2: -172, 64: -178}, 0, False), ("beyond the upper edge of the record", {2: 173, 64: 170}, 0, False),
                 ("the smallest subnormals: no cube", "c", 0, False), ("partly overflowed: no cube", "e", 0, False)],
}


def density_state(dtype, n, reach, case):
    what, where, m, sums = case
    e = lattice_exponent(dtype, reach, where) if isinstance(where, str) else where[reach]
    base, index, dist, k = lattice_state(np.dtype(dtype).name, n, reach, e)
    pos = base.copy()
    pos[:, 3] = np.ldexp(pos[:, 3], m)
    pos[::5, 3] = 0  # one species of mass 0
    return pos, index, dist, e


def record_terms(pos, rho):
    """in long double, from the long double densities: rho, rho x, rho |x - x_d|, rho^2, rho^2 |x - x_d|^2 of the bodies with a density"""
    has = rho != 0
    if not has.any():
        return ()
    r, x = rho[has], pos[has, :3].astype(LD)
    centre = (r[:, None] * x).sum(axis=0) / r.sum()
    off = ((x - centre) ** 2).sum(axis=1)
    terms = (r, r[:, None] * x, r * np.sqrt(off), r * r, r * r * off)
    return tuple(np.append(np.abs(t).ravel(), np.abs(t).sum()) for t in terms)  # (and the sum of each: the terms have one sign, or bound it)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_density_state_has_a_finite_reference(dtype):
    """C1 for G4: in every state every defined density is finite and normal in double (or exactly 0: every inner neighbour of the species
    of mass 0); the states astride an edge have bodies on both sides of it; where the sums are checked every term of the record is a
    normal double, and beyond the record's edges rho^2 is not."""
    count = 0
    for case in DENSITY_CASES[dtype]:
        what, where, m, sums = case
        astride = beyond = overflowed = some = False  # (over the sizes, the reaches and K)
        for n in SIZES:
            for reach in REACHES:
                pos, index, dist, e = density_state(dtype, n, reach, case)
                for k in KS[1:]:
                    rho, good = rho_ld(pos, index, dist, k)
                    assert normal_in(np.float64, rho).all() and np.array_equal(good, numpy_density(pos, index, dist, k)[1]), (what, n, reach, k)
                    some |= bool((rho[good] > 0).any())
                    dk = dist[:, k - 1].astype(np.float64)
                    plain = (dk > 0) & (dk < np.inf)
                    astride |= bool((plain & ~good).any() and good.any())  # (the old rule and the new one differ here)
                    if "no cube" in what:
                        assert not good.any()
                    if dtype == np.float32:
                        assert np.array_equal(plain, good), "fp32: the cube of a float is always a normal double"
                    overflowed |= bool((dk == np.inf).any())
                    terms = record_terms(pos, rho)
                    normal = all(normal_in(np.float64, np.where(t == 0, 1, t)).all() for t in terms)
                    if sums:
                        assert normal, (what, n, reach, k)
                    beyond |= not normal
                count += 1
        assert astride == ("astride" in what) and ("beyond" not in what or beyond) and overflowed == ("overflowed" in what), what
        assert some != ("no cube" in what), what
    assert count == len(SIZES) * len(REACHES) * len(DENSITY_CASES[dtype])


def check_density_outputs(d, pos, index, dist, what, sums):
    """rho against rho_ld within (K + 8) 2^-53; `densities` as that double rounded once; the counts, the flags, the extremes and the densest
    body exactly; the sums by check_sums, with its reference in long double"""
    n, k = d.n, d.k
    want, good = rho_ld(pos, index, dist, k)
    got = d.rho64()
    assert np.isfinite(got).all(), what
    assert (np.abs(got.astype(LD) - want) <= (k + 8) * 2.0 ** -53 * want).all(), what
    assert np.array_equal(got != 0, good & (want != 0)), what
    with np.errstate(over="ignore", under="ignore"):
        once = got.astype(d.dtype)
    assert d.get("rho").tobytes() == once.tobytes(), (what, "the double rounded once")
    with np.errstate(all="ignore"):
        ref, record = numpy_structure(pos, got, good, dist[:, k - 1], LD), d.record()
    for name in ("defined", "degenerate", "flags", "max_density", "max_density_body", "min_kth_dist_sq", "max_kth_dist_sq"):
        assert record[name] == ref[name], (what, name, record[name], ref[name])
    assert record["defined"] + record["degenerate"] == n and record["defined"] == int(good.sum())
    assert bool(record["flags"] & DEGENERATE) == bool((~good).any()) and bool(record["flags"] & NO_DENSITY) == (not (got > 0).any())
    if sums:
        check_sums(record, ref, pos, got, n, k, what)


@gpu_only
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_densities_and_the_record_across_the_range(gpu, dtype, n):
    """G4.  fp32: by C2 nothing in double leaves its range, the whole of T is the window.  fp64: astride both edges of the range in which
    the cube is a normal double (a body outside it is `degenerate`, its density 0: never +inf, and never 0 for a body counted `defined`),
    inside both edges of the range in which the record's terms are, and beyond them, where the record is what IEEE gives."""
    for reach in REACHES:
        for case in DENSITY_CASES[dtype]:
            pos, index, dist, e = density_state(dtype, n, reach, case)
            for k in KS[1:]:
                d = KnnDevice(gpu, pos, k).survey()
                what = (case[0], n, reach, k, np.dtype(dtype).name)
                check_lists(d, index, dist, what)
                check_density_outputs(d, pos, index, dist, what, sums=case[3])
                assert d.canaries_intact() and d.get("pos").tobytes() == pos.tobytes()
                d.free()
