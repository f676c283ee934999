"""The K nearest neighbours of every body, local densities and the density centre (nb_knn_*, include/nbody_hip_knn.h; libnbody_hip_knn.so
from csrc/knn*.hip).  The CPU part; the GPU part is tests/test_knn_gpu.py, which imports the helpers below.

The definitions, restated in numpy below.  With d2(i, j) = dx dx + (dy dy + dz dz) of the differences x_j - x_i in T (numpy_knn):

    the list of body i = the first K of all (d2(i, j), j), j != i by index, sorted by d2 and then by j; a NaN d2 is never a neighbour;
                         missing ranks hold NONE and +inf

and in double (numpy_density, numpy_structure), with d_K^2 the K-th d2 and M_i the masses of the K - 1 inner neighbours added in rank order:

    rho_i = M_i / (c (d_K^2 sqrt(d_K^2))),  c = 4.188790204786391;   rho_i = 0 when d_K^2 is 0, +inf or missing, or when the cube is not a
    positive normal double or c times it is not finite (`degenerate`)
    sum_density = sum rho,  centre = sum rho x / sum rho,  density_radius = sum rho |x - centre| / sum rho,
    core_radius = sqrt(sum rho^2 |x - centre|^2 / sum rho^2),  the largest rho and its lowest body,  the smallest and largest finite d_K^2

CPU tests: the boundary (declared, exported, mirrored; the other seven libraries unchanged), d2 through the one macro, the plan and the
workspace as functions of (N, K, precision), host-side argument checks, the numpy scheme on a hand-made state, the registry of knn.s (every
kernel of the listing is named once, with the cases that reach it; none has a private segment), the shape of the streaming loop."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from kernel_matrix import F32, F64, LANE_WIDTH, TYPE_NAME, kernel_name, listed_kernels
from test_capi_symbols import declared_symbols, exported_symbols
from test_hermite import CSRC
from test_neighbour import struct_fields, suffix

ERR = 10001
MAX_N = 1 << 24
MAX_K = 16
NONE = 0xFFFFFFFF
SPHERE = 4.188790204786391
DEGENERATE, NO_DENSITY = 1, 2
SYMBOLS = ["nb_knn_plan_f32", "nb_knn_plan_f64", "nb_knn_survey_f32", "nb_knn_survey_f64", "nb_knn_workspace_bytes"]
KS = (1, 2, 6, 8, 16)


# ---------------------------------------------------------------------------------------------------------------- the definitions in numpy


def numpy_knn(pos, k, block=256):
    """The lists in T arithmetic (no FMA: exact wherever the test needs bits).  pos (N, 4) of T -> index (N, k) uint32, dist_sq (N, k) T.
    The list for a smaller K is the first K columns."""
    n, kind = pos.shape[0], pos.dtype.type
    index, dist = np.full((n, k), NONE, np.uint32), np.full((n, k), np.inf, pos.dtype)
    m = min(k, n)
    with np.errstate(invalid="ignore"):
        for s in range(0, n, block):
            i = np.arange(s, min(n, s + block))
            d = pos[None, :, :3] - pos[i, None, :3]
            d2 = d[:, :, 0] * d[:, :, 0] + (d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2])
            assert d2.dtype == pos.dtype
            own = i[:, None] == np.arange(n)[None, :]
            candidate = np.where(own | np.isnan(d2), kind(np.inf), d2)
            order = np.argsort(candidate, axis=1, kind="stable")[:, :m]  # (stable: the lowest j first on equal bits)
            values = np.take_along_axis(candidate, order, axis=1)
            index[i, :m] = np.where(values < np.inf, order, NONE)
            dist[i, :m] = values
    return index, dist


def numpy_density(pos, index, dist, k):
    """-> rho (N,) float64, defined (N,) bool, from the first k columns of the lists"""
    n = pos.shape[0]
    dk = dist[:, k - 1].astype(np.float64)
    with np.errstate(over="ignore", under="ignore"):
        cube = dk * np.sqrt(dk)
        volume = SPHERE * cube
    good = (cube >= np.finfo(np.float64).tiny) & (volume < np.inf)  # a positive normal cube, a finite volume: never for d_K^2 of 0, +inf or missing
    mass = np.zeros(n)
    with np.errstate(invalid="ignore"):
        for rank in range(k - 1):  # (rank order)
            j = np.minimum(index[:, rank], n - 1)
            mass = mass + np.where(good, pos[j, 3].astype(np.float64), 0.0)
    with np.errstate(all="ignore"):
        rho = np.where(good, mass / volume, 0.0)
    return rho, good


def rho_ld(pos, index, dist, k):
    """-> rho (N,) long double, defined (N,) bool: numpy_density with x87 range and precision through the mass sum, the cube and the
    quotient.  Which bodies are `defined` is the header's rule, stated on the DOUBLE cube; where it holds the long double cube is normal too."""
    n = pos.shape[0]
    good = numpy_density(pos, index, dist, k)[1]
    dk = np.where(good, dist[:, k - 1], 1).astype(np.longdouble)
    mass = np.zeros(n, np.longdouble)
    with np.errstate(invalid="ignore"):
        for rank in range(k - 1):
            j = np.minimum(index[:, rank], n - 1)
            mass = mass + np.where(good, pos[j, 3].astype(np.longdouble), 0)
        return np.where(good, mass / (np.longdouble(SPHERE) * (dk * np.sqrt(dk))), 0), good


def numpy_structure(pos, rho, good, dk, kind=np.float64):
    """The record from the densities; the sums in `kind` (float64, or long double for the GPU tests' reference)."""
    x = pos[:, :3].astype(kind)
    r = rho.astype(kind)
    has = rho != 0  # (a density defined as 0 adds nothing, wherever the body is)
    total = r[has].sum()
    finite = dk[dk < np.inf].astype(np.float64)
    out = dict(sum_density=total, max_density=float(rho.max()), max_density_body=int(rho.argmax()), defined=int(good.sum()), degenerate=int((~good).sum()),
               min_kth_dist_sq=float(finite.min()) if len(finite) else float("inf"), max_kth_dist_sq=float(finite.max()) if len(finite) else float("-inf"))
    out["flags"] = (DEGENERATE if out["degenerate"] else 0) | (0 if total > 0 else NO_DENSITY)
    if total > 0:
        centre = (r[has, None] * x[has]).sum(axis=0) / total
        out["centre"] = tuple(centre)
        out.update(numpy_radii(pos, rho, centre, kind))
    else:
        out.update(centre=(np.nan,) * 3, density_radius=np.nan, core_radius=np.nan)
    return out


def numpy_radii(pos, rho, centre, kind=np.float64):
    has = rho != 0
    r, d = rho[has].astype(kind), pos[has, :3].astype(kind) - np.asarray(centre, dtype=kind)
    r2 = (d * d).sum(axis=1)
    return dict(density_radius=(r * np.sqrt(r2)).sum() / r.sum(), core_radius=np.sqrt((r * r * r2).sum() / (r * r).sum()))


def test_the_numpy_scheme_on_a_hand_made_state():
    """Five bodies on a line at x = 0, 1, 1, 3, 5 with masses 1, 2, 4, 8, 16; bodies 1 and 2 at one place."""
    for kind in (np.float32, np.float64):
        pos = np.zeros((5, 4), kind)
        pos[:, 0] = [0, 1, 1, 3, 5]
        pos[:, 3] = [1, 2, 4, 8, 16]
        index, dist = numpy_knn(pos, 6)
        # body 0: bodies 1 and 2 tie at d2 = 1 -> the lower index first.  bodies 1, 2: the twin is a neighbour at 0 (j != i by index); body 1 then
        # has 0 (d2 = 1) before 3 (d2 = 4).  body 3: bodies 1, 2 and 4 tie at 4 -> ascending j.  Four candidates only: ranks 4, 5 are NONE / +inf.
        assert index.tolist() == [[1, 2, 3, 4, NONE, NONE], [2, 0, 3, 4, NONE, NONE], [1, 0, 3, 4, NONE, NONE], [1, 2, 4, 0, NONE, NONE], [3, 1, 2, 0, NONE, NONE]]
        assert dist.tolist() == [[1, 1, 9, 25, np.inf, np.inf], [0, 1, 4, 16, np.inf, np.inf], [0, 1, 4, 16, np.inf, np.inf], [4, 4, 4, 9, np.inf, np.inf],
                                 [4, 16, 16, 25, np.inf, np.inf]]
        assert dist.dtype == kind and np.array_equal(numpy_knn(pos, 2)[0], index[:, :2]), "a smaller K is a prefix"
        # K = 2: M_i = the nearest's mass, d_K^2 = the second d2: rho = m / (c d^3)
        rho, good = numpy_density(pos, index, dist, 2)
        assert good.all()
        want = np.array([2 / 1, 4 / 1, 2 / 1, 2 / 8, 8 / 64]) / SPHERE  # d_K = 1, 1, 1, 2, 4
        assert np.allclose(rho, want, rtol=4e-16, atol=0)
        # the twins' first d2 is 0: with it as d_K^2 (the scheme at K = 1, which the library refuses) the formula is not evaluated: rho = 0, `degenerate`
        rho1, good1 = numpy_density(pos, index, dist, 1)
        assert good1.tolist() == [True, False, False, True, True] and rho1[1] == 0 and rho1[2] == 0
        # K = 3: M_i = the two nearest masses in rank order
        rho3, _ = numpy_density(pos, index, dist, 3)
        assert np.allclose(rho3, np.array([(2 + 4) / 27, (4 + 1) / 8, (2 + 1) / 8, (2 + 4) / 8, (8 + 2) / 64]) / SPHERE, rtol=4e-16, atol=0)
        # K = 5: nobody has five neighbours -> every density is defined as 0, the record says so
        rho5, good5 = numpy_density(pos, index, dist, 5)
        assert not good5.any() and not rho5.any()
        record = numpy_structure(pos, rho5, good5, dist[:, 4])
        assert record["flags"] == DEGENERATE | NO_DENSITY and record["degenerate"] == 5 and record["defined"] == 0 and np.isnan(record["core_radius"])
        assert record["min_kth_dist_sq"] == np.inf and record["max_kth_dist_sq"] == -np.inf and record["max_density"] == 0 and record["max_density_body"] == 0
        record = numpy_structure(pos, rho, good, dist[:, 1])
        assert record["flags"] == 0 and (record["defined"], record["degenerate"]) == (5, 0) and record["max_density_body"] == 1
        assert (record["min_kth_dist_sq"], record["max_kth_dist_sq"]) == (1.0, 16.0)
        total = want.sum()
        centre = (want * pos[:, 0]).sum() / total
        assert np.isclose(record["sum_density"], total, rtol=1e-15) and np.allclose(record["centre"], (centre, 0, 0), rtol=1e-15, atol=0)
        assert np.isclose(record["density_radius"], (want * abs(pos[:, 0] - centre)).sum() / total, rtol=1e-15)
        assert np.isclose(record["core_radius"], np.sqrt((want ** 2 * (pos[:, 0] - centre) ** 2).sum() / (want ** 2).sum()), rtol=1e-15)
        # a NaN body is nobody's neighbour and has none
        pos[4, 1] = np.nan
        index, dist = numpy_knn(pos, 4)
        assert index[4].tolist() == [NONE] * 4 and 4 not in index and index[0].tolist() == [1, 2, 3, NONE]


# ---------------------------------------------------------------------------------------------------------------- the boundary


def test_knn_header_library_and_binding_agree(pkg):
    declared = declared_symbols("nbody_hip_knn.h")
    assert declared == SYMBOLS
    assert exported_symbols(pkg.KNN_LIB_PATH) == declared
    assert sorted(pkg.KNN_SIGNATURES) == declared
    # the other seven libraries export what they did, none of it ours
    others = {pkg.LIB_PATH: 96, pkg.ENSEMBLE_LIB_PATH: 4, pkg.HERMITE_LIB_PATH: 9, pkg.HERMITE_BLOCK_LIB_PATH: 9, pkg.NEIGHBOUR_LIB_PATH: 7, pkg.FIELD_LIB_PATH: 5}
    for path, count in others.items():
        assert len(exported_symbols(path)) == count, path
        assert not set(declared) & set(exported_symbols(path)), path
    assert not set(declared) & set(exported_symbols(pkg.LAB_LIB_PATH))
    assert set(exported_symbols(pkg.LIB_PATH)) <= set(exported_symbols(pkg.LAB_LIB_PATH))
    needed = subprocess.run(["readelf", "-d", pkg.KNN_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnbody_hip" not in needed
    assert os.path.basename(pkg.KNN_LIB_PATH) == "libnbody_hip_knn.so" or "NBODY_HIP_KNN_LIB" in os.environ


def test_knn_mirrors_and_constants_match_the_header(pkg):
    text = open(os.path.join(ROOT, "include", "nbody_hip_knn.h")).read()
    ctype = {"unsigned long long": ctypes.c_ulonglong, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double, "int": ctypes.c_int,
             "unsigned": ctypes.c_uint}
    for name, mirror, size in (("nb_knn_structure", pkg.KnnStructure, 128), ("nb_knn_plan", pkg.KnnPlan, 64)):
        fields = struct_fields(text, name)
        assert [f for _, f, _ in fields] == [f for f, _ in mirror._fields_], name
        for (kind, field, count), (_, mirrored) in zip(fields, mirror._fields_):
            assert mirrored == (ctype[kind] * int(count) if count else ctype[kind]), (name, field)
        assert ctypes.sizeof(mirror) == size
    assert re.search(r"#define NB_KNN_MAX_K 16u", text) and pkg.KNN_MAX_K == MAX_K
    assert re.search(r"#define NB_KNN_SPHERE 4\.188790204786391 ", text) and pkg.KNN_SPHERE == SPHERE
    assert re.search(r"#define NB_KNN_DEGENERATE 1u", text) and pkg.KNN_DEGENERATE == DEGENERATE
    assert re.search(r"#define NB_KNN_NO_DENSITY 2u", text) and pkg.KNN_NO_DENSITY == NO_DENSITY
    # the double nearest 4 pi / 3: pi = 0x1.921fb54442d18p+1 + 0x1.1a62633145c07p-53 (the next 53 bits of pi), in exact rational arithmetic
    from fractions import Fraction
    pi = Fraction(float.fromhex("0x1.921fb54442d18p+1")) + Fraction(float.fromhex("0x1.1a62633145c07p-53"))
    exact = 4 * pi / 3
    here, up, down = Fraction(SPHERE), Fraction(np.nextafter(SPHERE, np.inf)), Fraction(np.nextafter(SPHERE, -np.inf))
    assert abs(here - exact) < abs(up - exact) and abs(here - exact) < abs(down - exact)
    for phrase in ("first K entries of all pairs (d2(i, j), j) with j != i BY INDEX", "d2 ascending, the lowest j first on equal bits", "A NaN d2 is never a neighbour",
                   "rho_i = M_i / (c * (d_K^2 * sqrt(d_K^2)))", "DEFINED AS 0 when d_K^2 is 0, +inf or missing", "sum rho_i |x_i - x_d| / sum rho_i",
                   "sqrt(sum rho_i^2 |x_i - x_d|^2 / sum rho_i^2)", "with K = 1 they are refused", '#include "nbody_hip_neighbour.h"'):
        assert phrase in text, phrase


def test_knn_computes_d2_through_the_one_macro():
    source = open(os.path.join(CSRC, "knn.hip")).read()
    code = "\n".join(line.split("//")[0] for line in source.split("\n"))
    assert code.count("NB_NEIGHBOUR_DIST_SQ(") == 1 and "dx * dx" not in code and "dx, dx" not in code
    assert '#include "../../include/nbody_hip_knn.h"' in source and '#include "nbody_lane.h"' in source
    header = open(os.path.join(ROOT, "include", "nbody_hip_knn.h")).read()
    assert "#define NB_NEIGHBOUR_DIST_SQ" not in header, "there is one expression of d2 in the project: the neighbour header's"
    for name in ("knn.hip", "knn_capi.hip", "knn_kernels.h"):
        text = "\n".join(line.split("//")[0] for line in open(os.path.join(CSRC, name)).read().split("\n"))
        assert "atomic" not in text.lower() and "hipMalloc" not in text and "Synchronize" not in text and "static " not in text.replace("static_assert", "").replace("static_cast", "")


# ---------------------------------------------------------------------------------------------------------------- plan and workspace


def expected_plan(n, k, dtype):
    """the geometry rule of the header, restated"""
    W, size = LANE_WIDTH[dtype], np.dtype(dtype).itemsize
    S = 1
    while S < 4 and 2 * S * 128 <= n:
        S *= 2
    cap = 4 if k <= 4 else 8 if k <= 8 else 16
    return dict(bodies_per_lane=W, waves_per_group=S, unroll=4 if W == 2 else 2, capacity=cap, ranges=1, tiles=-(-n // (64 * W)), block_threads=64 * S,
                lds_bytes=(S // 2) * cap * 64 * W * (size + 4), chunks=-(-n // 128), blocks=-(-n // 256), search_launches=1, structure_launches=3 if k >= 2 else 0,
                density_offset=0, density_bytes=8 * n)


def expected_workspace(n, k, dtype):
    up = lambda b: (b + 255) & ~255  # noqa: E731
    p = expected_plan(n, k, dtype)
    return up(8 * n) + up(p["tiles"] * 72) + up(p["blocks"] * 24) + up(128)


def plan_dict(pkg, n, k, dtype):
    p = pkg.knn_plan(n, k, dtype)
    return {name: getattr(p, name) for name, _ in pkg.KnnPlan._fields_}


def test_knn_plan_and_workspace_are_functions_of_n_k_and_precision(pkg):
    sizes = sorted({1, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 65536, MAX_N})
    lib = pkg.knn_lib()
    for dtype in (F32, F64):
        for n in sizes:
            for k in KS:
                plans = {tuple(plan_dict(pkg, n, k, dtype).items()) for _ in range(2)}
                assert len(plans) == 1
                got = dict(plans.pop())
                assert got == expected_plan(n, k, dtype), (n, k, dtype)
                assert got["lds_bytes"] <= 64 * 1024 and got["capacity"] >= k and got["waves_per_group"] <= got["chunks"], "every wave has a chunk"
                assert pkg.knn_workspace_bytes(n, k, dtype) == expected_workspace(n, k, dtype), (n, k, dtype)
        p = pkg.KnnPlan()
        fn = getattr(lib, "nb_knn_plan_" + suffix(dtype))
        for n, k in ((0, 1), (MAX_N + 1, 1), (100, 0), (100, MAX_K + 1)):
            assert fn(n, k, ctypes.byref(p)) == ERR, (n, k)
        assert fn(16, 2, None) == ERR
    out = ctypes.c_size_t(0)
    for bad in ((0, 2, 4), (MAX_N + 1, 2, 4), (1000, 0, 4), (1000, 17, 8), (1000, 2, 2), (1000, 2, 16)):
        assert lib.nb_knn_workspace_bytes(*bad, ctypes.byref(out)) == ERR, bad
    assert lib.nb_knn_workspace_bytes(1000, 2, 4, None) == ERR


# ---------------------------------------------------------------------------------------------------------------- argument errors


def test_knn_argument_errors_are_caught_on_the_host(pkg):
    """Everything refused here is refused before a HIP call: the made-up addresses are never dereferenced."""
    lib = pkg.knn_lib()
    count = ctypes.c_int(0)
    no_gpu = pkg.lib().nb_device_count(ctypes.byref(count)) != 0 or count.value == 0
    for dtype in (F32, F64):
        size, n, k = np.dtype(dtype).itemsize, 1024, 6
        ws_bytes = pkg.knn_workspace_bytes(n, k, dtype)
        ok = dict(pos=0x100000000, index=0x200000000, d2=0x300000000, rho=0x400000000, record=0x500000000, ws=0x600000000, ws_bytes=ws_bytes, n=n, k=k)
        length = dict(pos=4 * n * size, index=4 * n * k, d2=size * n * k, rho=n * size, record=128, ws=ws_bytes)
        align = dict(pos=4 * size, index=4, d2=size, rho=size, record=8, ws=32)
        names = ("pos", "index", "d2", "rho", "record", "ws")

        def call(**kw):
            a = {**ok, **kw}
            return getattr(lib, "nb_knn_survey_" + suffix(dtype))(a["pos"], a["n"], a["k"], a["index"], a["d2"], a["rho"], a["record"], a["ws"], a["ws_bytes"], None)

        for null in ("pos", "ws"):
            assert call(**{null: None}) == ERR, null
        for bad in (dict(n=0), dict(n=MAX_N + 1), dict(k=0), dict(k=MAX_K + 1), dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0)):
            assert call(**bad) == ERR, bad
        for name in names:
            assert call(**{name: ok[name] + align[name] // 2}) == ERR, f"{name} misaligned"
        for x in names:  # every pair of arrays: the same start, x on the last bytes of y, x running into y (32 is a multiple of every alignment)
            for y in names:
                if x == y:
                    continue
                assert call(**{x: ok[y]}) == ERR, (x, "==", y)
                assert call(**{x: ok[y] + (length[y] - 1) // 32 * 32}) == ERR, (x, "on the end of", y)
                assert call(**{x: ok[y] - (length[x] - 1) // 32 * 32}) == ERR, (x, "running into", y)
        assert call(index=None, d2=None, rho=None, record=None) == ERR, "no output and no record"
        assert call(k=1) == ERR and call(k=1, rho=None) == ERR and call(k=1, record=None) == ERR, "densities and the record need K >= 2"
        if no_gpu:  # (with a GPU the made-up addresses would be used) past the argument check: a HIP error
            assert call(k=1, rho=None, record=None) not in (0, ERR)
            assert call(index=None, d2=None, rho=None) not in (0, ERR) and call(d2=None, rho=None, record=None) not in (0, ERR), "one output, or the record alone, is enough"


# ---------------------------------------------------------------------------------------------------------------- the listing and its registry
# Every kernel of knn.s, once: knn_search<T, CAP, S> with the (N, K) that reach it -- S follows N (1 below 256 bodies, 2 from 256, 4 from 512), CAP
# follows K (4 up to 4, 8 up to 8, 16 above) --, and the record's three kernels, which run whenever the record is asked for.  A case names what
# the plan query must report for it; tests/test_knn_gpu.py asserts that on the device, then runs it.
N_BY_WAVES = {1: (1, 2, 3, 127, 128, 129, 255), 2: (256, 300, 511), 4: (512, 700, 1025, 5000)}
K_BY_CAPACITY = {4: (1, 2), 8: (6, 8), 16: (16,)}
RECORD_KERNELS = {("knn_centre", ()), ("knn_record", ()), ("knn_rings", ("float",)), ("knn_rings", ("double",))}


def knn_cases():
    """(dtype, CAP, S, n, k)"""
    return [(dtype, cap, s, n, k) for dtype in (F32, F64) for cap, ks in K_BY_CAPACITY.items() for s, sizes in N_BY_WAVES.items() for n in sizes for k in ks]


def knn_registry():
    """kernel -> the cases that reach it"""
    out = {kernel: [(300, 6)] for kernel in RECORD_KERNELS}
    for dtype, cap, s, n, k in knn_cases():
        out.setdefault(("knn_search", (TYPE_NAME[dtype], cap, s)), []).append((n, k))
    return out


def knn_listing():
    subprocess.run(["make", "-s", "-C", CSRC, "knn.s"], check=True, capture_output=True)
    return open(os.path.join(CSRC, "knn.s")).read()


def test_every_kernel_of_the_listing_is_in_the_registry(pkg):
    text = knn_listing()
    listed = listed_kernels(text)
    assert len(listed) == len(set(listed)) == 22  # 3 capacities x 3 wave counts x two precisions, knn_rings x two, knn_centre, knn_record
    registry = knn_registry()
    missing = sorted(kernel_name(k) for k in set(listed) - set(registry))
    stale = sorted(kernel_name(k) for k in set(registry) - set(listed))
    assert not missing, f"kernels of knn.s no case reaches: {missing}"
    assert not stale, f"cases that name no kernel of knn.s: {stale}"
    for dtype, cap, s, n, k in knn_cases():
        plan = plan_dict(pkg, n, k, dtype)
        assert (plan["capacity"], plan["waves_per_group"]) == (cap, s), (n, k)
    # no private segment anywhere; LDS as the plan says, and within what a static declaration compiles to
    sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(sizes) == 22 and max(sizes) == 0, sizes
    assert "scratch_" not in text and "buffer_store" not in text
    blocks = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n", text)
    lds = {}
    for size, symbol in blocks:
        if symbol.startswith("_ZN2nb"):
            lds[listed_kernels(".amdhsa_kernel " + symbol)[0]] = int(size)
    assert len(lds) == 22 and max(lds.values()) <= 64 * 1024
    for dtype, cap, s, n, k in knn_cases():
        assert lds[("knn_search", (TYPE_NAME[dtype], cap, s))] == plan_dict(pkg, n, k, dtype)["lds_bytes"], (dtype, cap, s)


def kernels_of(text):
    lines = text.split("\n")
    for i, line in enumerate(lines):
        m = re.match(r"^(_ZN2nb12_GLOBAL__N_1\d+knn_search\w+):", line)
        if m:
            end = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            yield m.group(1), lines[i:end]


# What the compiler delivers for the no-insertion path of the fp32 streaming loop, per group of 4 bodies j against a packed pair of bodies i: 24
# packed operations (6 per body j: the survey's d2), and at most 12 other vector operations in the unmasked form (the two bodies' least d2:
# v_min / v_min3, two compares) before the branch that leaves the group.
PK_GROUP, OTHER_GROUP = 24, 12


def test_knn_streaming_loop_leaves_a_group_after_one_branch():
    """Every fp32 knn_search kernel has streaming loops whose first branch comes after the group's d2 (24 packed operations), the two minima and the
    two compares, with no LDS, scratch, barrier or vector memory instruction before it: that is the no-insertion path."""
    text = knn_listing()
    seen = 0
    for name, lines in kernels_of(text):
        if "knn_searchIf" not in name:
            continue
        seen += 1
        heads = []
        for i, line in enumerate(lines):
            if "Inner Loop Header" not in line:
                continue
            stop = next((k for k in range(i, len(lines)) if lines[k].strip().startswith("s_cbranch")), None)
            head = [l.strip() for l in lines[i + 1:stop]]
            count = lambda prefix: sum(1 for l in head if l.startswith(prefix))  # noqa: E731
            if count("v_pk_fma_f32") < 8:
                continue  # (the merge loop, the one-body loop of the ragged end)
            assert count("v_pk_") == PK_GROUP, (name, count("v_pk_"))
            assert count("ds_") == 0 and count("scratch_") == 0 and count("s_barrier") == 0 and count("global_") == 0 and count("buffer_") == 0 and count("flat_") == 0, name
            assert count("v_cmp_lt_f32") == 2 and count("v_min") >= 4, (name, head)
            heads.append(count("v_") - count("v_pk_"))
        assert len(heads) == 2, (name, heads)  # the plain and the masked form
        assert min(heads) <= OTHER_GROUP, (name, heads)
    assert seen == 9
    assert "s_load_dwordx" in text


# ---------------------------------------------------------------------------------------------------------------- the cost model
# The survey's fp32 loop costs 6 packed + 7 other vector operations per body j and packed pair of bodies i (tests/test_neighbour.py).
# The search's, from the loop as compiled and the rates at which a randomly ordered cloud enters the insertion path:
#   every group        6 packed per body j, and OTHER_GROUP / 4 = 3 others (the minima, the compares)
#   a group that has a candidate in some lane (rate G): per candidate a compare, a ballot's s_cmp and a branch, counted as 3 -> 6 per body j
#   a candidate some lane wants (rate C): per slot a compare and four selects, per slot one select of the K-th entry's chain, 2 to set up
# A wave sees T = N / S candidates per body, in random order the t-th enters a body's list with probability min(1, K / t), so some lane of 64 wants it
# with probability about min(1, 64 K / t) and a group of U = 4 bodies j against W = 2 bodies i has one with about min(1, 512 K / t):
# the mean of min(1, a / t) over t <= T is a (1 + ln(T / a)) / T.  That the others cost what a packed operation does is an ASSUMPTION (as in 5.8).
SURVEY_OPS = 6 + 7


def entering_rate(a, t):
    return 1.0 if a >= t else a * (1 + np.log(t / a)) / t


def knn_model(n, k):
    """(the search's vector operations per body j and packed pair over the survey's, the share of groups on the insertion path, of candidates inserted)"""
    s, cap = expected_plan(n, k, F32)["waves_per_group"], expected_plan(n, k, F32)["capacity"]
    t = n / s
    groups, candidates = entering_rate(512 * k, t), entering_rate(64 * k, t)
    ops = 6 + OTHER_GROUP / 4 + groups * 6 + candidates * 2 * (5 * cap + cap + 2)
    return ops / SURVEY_OPS, groups, candidates


def test_the_cost_model_of_the_speed_test():
    ratio, groups, candidates = knn_model(65536, 8)
    assert 0.55 < groups < 0.65 and 0.13 < candidates < 0.15 and 1.9 < ratio < 2.2, (ratio, groups, candidates)


# ---------------------------------------------------------------------------------------------------------------- CLI
CLI = os.path.join(ROOT, "cuda-nbody_amd", "nbody")


def test_cli_refuses_knn_where_it_refuses_neighbours():
    """--knn is single-device, not for --compare / --qatest / --systems (the refusals of --neighbours, in their wording), and wants 2 <= K <= 16"""
    base = ["--numbodies=1024", "--steps=1", "--knn=6"]
    for extra in (base + ["--numdevices=2"], base + ["--devices=0,1"], ["--numdevices=2"] + base, base + ["--compare"], base + ["--qatest"], base + ["--systems=3"],
                  base + ["--integrator=hermite", "--numdevices=2"], base + ["--integrator=hermite-block", "--devices=0,1"], base + ["--integrator=hermite", "--compare"],
                  ["-numbodies=1024", "-steps=1", "-knn=6", "-compare"]):
        r = subprocess.run([CLI, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr, (extra, r.returncode, r.stderr[:300])
        twin = ["--neighbours=0.5" if a.lstrip("-").startswith("knn=") else a for a in extra]
        e = subprocess.run([CLI, *twin], capture_output=True, text=True, timeout=60)
        assert e.returncode == 1 and "CRITICAL ERROR" in e.stderr, ("--neighbours is refused there too", twin)
    for extra, message in ((["--numdevices=2"], "--knn is single-device: it cannot be combined with --numdevices or --devices naming more than one GPU"),
                           (["--compare"], "--knn cannot be combined with --compare or --qatest (those runs step two systems)"),
                           (["--systems=3"], "--systems cannot be combined with"), (["--numbodies=16777217"], "--knn: --numbodies must be at most 16777216")):
        r = subprocess.run([CLI, *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and message in r.stderr, (extra, r.stderr[:300])
    for bad in ("--knn=0", "--knn=1", "--knn=17", "--knn=-3", "--knn=six", "--knn=", "--knn", "--knn=2.5"):
        r = subprocess.run([CLI, "--numbodies=1024", "--steps=1", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr, (bad, r.returncode, r.stderr[:300])
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--knn UINT" in r.stdout
