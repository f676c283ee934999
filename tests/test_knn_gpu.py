"""nb_knn_* on the device (include/nbody_hip_knn.h); the definitions, the numpy restatement and the registry are in tests/test_knn.py.

1  exact: integer lattices (every d2 is exact in T, so the numpy lists hold bit for bit), every index and every d2 bit; one place, a NaN body,
   a line ascending and descending; every instantiation of the registry, after the plan query selected it
2  exact at size against nb_neighbour_survey_*: rank 0, the counts within the K-th distance, order, no self, no repeats, the same bits twice
3  random clouds against long double: each d2 within gamma = 6u of its pair's, nobody outside a row closer than (1 - 2 gamma) its last, order
4  densities and the record: on the lattices against numpy ((K + 8) u; fp32 = the double rounded once), counts and flags exact; on the clouds the
   sums within (N + K + 64) 2^-53 of their terms' magnitudes against long double, the radii within twice that about the DEVICE's centre
5  the Python class gives the C calls' bits; `nbody --knn=6 --numbodies=4096 --steps=1` prints the Python record of the dumped state; a graph
   capture of two calls (one linear stream) replays to the same bits
6  speed: 65 536 bodies fp32, K = 8, against nb_neighbour_survey_f32 in the same process, no more than 2 x the cost model of tests/test_knn.py
Every buffer has canaries round it; inputs stay bit-untouched."""
import ctypes
import functools

import numpy as np
import pytest

from kernel_matrix import TYPE_NAME
from test_fast_domain import UNIT_ROUNDOFF
from test_hermite import LD, hip_runtime
from test_knn import (DEGENERATE, K_BY_CAPACITY, KS, N_BY_WAVES, NO_DENSITY, NONE, knn_model, knn_registry, numpy_density, numpy_knn, numpy_radii, numpy_structure,
                      plan_dict)
from test_neighbour import GAMMA, NeighbourDevice, lattice, normal_cloud, suffix

gpu_only = pytest.mark.gpu
OUTPUTS = ("index", "d2", "rho", "record")
DTYPES = [np.float32, np.float64]


class KnnDevice:
    """the arrays of one state and one K on the device, through the C calls; PAD canary bytes round every array; outputs start as 0xC3 bytes"""
    PAD = 256

    def __init__(self, gpu, pos, k, ws_fill=None):
        self.gpu, self.dtype, self.n, self.k = gpu, pos.dtype, pos.shape[0], int(k)
        self.lib = gpu.knn_lib()
        n = self.n
        self.ws_bytes = gpu.knn_workspace_bytes(n, self.k, self.dtype)
        self.kinds = dict(pos=(self.dtype, 4 * n), index=(np.dtype(np.uint32), n * self.k), d2=(self.dtype, n * self.k), rho=(self.dtype, n), record=(np.dtype(np.uint8), 128),
                          ws=(np.dtype(np.uint8), self.ws_bytes))
        self.bufs = {}
        for name, (kind, count) in self.kinds.items():
            nbytes = count * kind.itemsize
            host = np.full(nbytes + 2 * self.PAD, 0xA5, np.uint8)
            host[self.PAD:self.PAD + nbytes] = 0xC3 if name in OUTPUTS else 0
            if name == "ws" and ws_fill is not None:
                host[self.PAD:self.PAD + nbytes] = ws_fill
            buf = gpu.DeviceBuffer(host.nbytes)
            buf.upload(host)
            self.bufs[name] = buf
        self.put("pos", pos)

    def ptr(self, name):
        return self.bufs[name].ptr.value + self.PAD

    def put(self, name, data):
        kind, count = self.kinds[name]
        data = np.ascontiguousarray(data, dtype=kind).reshape(-1)
        assert data.size == count
        self.gpu.check(self.gpu.lib().nb_h2d(self.ptr(name), data.ctypes.data, data.nbytes, None), "nb_h2d")

    def get(self, name):
        kind, count = self.kinds[name]
        out = np.empty(count, kind)
        self.gpu.check(self.gpu.lib().nb_d2h(out.ctypes.data, self.ptr(name), out.nbytes, None), "nb_d2h")
        return out.reshape(self.n, self.k) if name in ("index", "d2") else out

    def record(self):
        s = self.gpu.KnnStructure.from_buffer_copy(self.get("record").tobytes())
        assert not any(s.reserved)
        return self.gpu.knn_structure_dict(s)

    def rho64(self):
        """the double rho[N] of the workspace, where the plan says it is"""
        p = self.gpu.knn_plan(self.n, self.k, self.dtype)
        assert p.density_bytes == 8 * self.n
        return self.get("ws")[p.density_offset:p.density_offset + p.density_bytes].view(np.float64).copy()

    def canaries_intact(self):
        for buf in self.bufs.values():
            host = buf.download(np.empty(buf.nbytes, np.uint8))
            if not ((host[:self.PAD] == 0xA5).all() and (host[-self.PAD:] == 0xA5).all()):
                return False
        return True

    def untouched(self, name):
        return bool((self.get(name).view(np.uint8) == 0xC3).all())

    def survey(self, outputs=None, stream=None):
        outputs = (OUTPUTS if self.k >= 2 else ("index", "d2")) if outputs is None else outputs
        fn = getattr(self.lib, "nb_knn_survey_" + suffix(self.dtype))
        out = [self.ptr(name) if name in outputs else None for name in OUTPUTS]
        self.gpu.check(fn(self.ptr("pos"), self.n, self.k, *out, self.ptr("ws"), self.ws_bytes, stream), "nb_knn_survey")
        return self

    def everything(self):
        return b"".join(self.get(name).tobytes() for name in OUTPUTS)

    def free(self):
        for buf in self.bufs.values():
            buf.free()


@functools.lru_cache(maxsize=None)
def lattice_reference(n, reach, type_name):
    """(pos, the lists for K = 16: a smaller K is their first columns), computed once and left unchanged"""
    dtype = np.float32 if type_name == "float" else np.float64
    pos = lattice(n, dtype, 100 * n + reach, reach)
    index, dist = numpy_knn(pos, 16)
    for a in (pos, index, dist):
        a.setflags(write=False)
    return pos, index, dist


def check_lists(d, index, dist, what):
    assert np.array_equal(d.get("index"), index[:, :d.k]), what
    assert d.get("d2").tobytes() == np.ascontiguousarray(dist[:, :d.k]).tobytes(), what


def check_densities(d, pos, index, dist, what):
    """4, given the exact lists: rho against numpy, the counts, the extremes and the flags exactly, the sums to the bound of their length"""
    n, k, u = d.n, d.k, 2.0 ** -53
    rho, good = numpy_density(pos, index, dist, k)
    got = d.rho64()
    assert (np.abs(got - rho) <= (k + 8) * u * rho).all(), what
    assert np.array_equal(got == 0, ~good), what
    out = d.get("rho")
    if d.dtype == np.float64:
        assert out.tobytes() == got.tobytes(), what
    else:
        assert out.tobytes() == got.astype(np.float32).tobytes(), (what, "the double rounded once")
        assert (np.abs(out.astype(np.float64) - rho) <= 2 * UNIT_ROUNDOFF[np.float32] * rho).all(), what
    want, record = numpy_structure(pos, got, good, dist[:, k - 1], LD), d.record()
    for name in ("defined", "degenerate", "flags", "max_density", "max_density_body", "min_kth_dist_sq", "max_kth_dist_sq"):
        assert record[name] == want[name], (what, name, record[name], want[name])
    assert record["defined"] + record["degenerate"] == n
    check_sums(record, want, pos, got, n, k, what)


def check_sums(record, want, pos, rho, n, k, what):
    """sum rho and sum rho x within (N + K + 64) 2^-53 of the sums of their terms' magnitudes, the radii within twice that about the device's centre;
    `want` in long double from the device's own rho"""
    bound = (n + k + 64) * 2.0 ** -53
    if want["flags"] & NO_DENSITY:
        assert not record["sum_density"] > 0 and all(np.isnan(record[name]) for name in ("density_radius", "core_radius")) and np.isnan(record["centre"]).all(), what
        return
    total = want["sum_density"]
    assert abs(LD(record["sum_density"]) - total) <= bound * total, (what, record["sum_density"], total)
    has = rho != 0
    for axis in range(3):
        terms = rho[has].astype(LD) * pos[has, axis].astype(LD)
        # centre = sum rho x / sum rho: the numerator's error, the denominator's relative error on the quotient's magnitude bound, one division
        allowed = (bound * np.abs(terms).sum() + bound * np.abs(terms).sum() + 2.0 ** -53 * abs(terms.sum())) / total
        assert abs(LD(record["centre"][axis]) - terms.sum() / total) <= allowed, (what, axis, record["centre"][axis], terms.sum() / total)
    about = numpy_radii(pos, rho, record["centre"], LD)
    for name in ("density_radius", "core_radius"):
        assert abs(LD(record[name]) - about[name]) <= 2 * bound * about[name], (what, name, record[name], about[name])


SMALL = sorted({1, 2, 3, *KS, *(k + 1 for k in KS), 127, 128, 129, 255, 256, 300, 1025} | {n for sizes in N_BY_WAVES.values() for n in sizes if n <= 1025})


@gpu_only
@pytest.mark.parametrize("sizes", [tuple(SMALL), (5000,)], ids=["to1025", "5000"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_lattices(gpu, dtype, sizes):
    """1 and 4.  Reach 2 (125 places: ties and duplicates everywhere) and reach 64; N across the chunk and tile edges, N = K and K + 1 (ranks of NONE),
    every S and every capacity: each case runs after the plan query named its instantiation, and together they are the registry's."""
    reached = set()
    for n in sizes:
        for reach in (2, 64):
            pos, index, dist = lattice_reference(n, reach, TYPE_NAME[dtype])
            for k in KS:
                plan = plan_dict(gpu, n, k, dtype)
                reached.add(("knn_search", (TYPE_NAME[dtype], plan["capacity"], plan["waves_per_group"])))
                d = KnnDevice(gpu, pos, k).survey()
                what = (n, reach, k, np.dtype(dtype).name)
                check_lists(d, index, dist, what)
                if k >= 2:
                    check_densities(d, pos, index, dist, what)
                    if n <= k:
                        assert d.record()["flags"] == DEGENERATE | NO_DENSITY and d.record()["degenerate"] == n, what
                else:
                    assert d.untouched("rho") and d.untouched("record"), what
                assert d.canaries_intact() and d.get("pos").tobytes() == pos.tobytes(), (what, "canaries, inputs bit-untouched")
                d.free()
    if len(sizes) > 1:
        want = {kernel for kernel in knn_registry() if kernel[0] == "knn_search" and kernel[1][0] == TYPE_NAME[dtype]}
        assert reached == want, (sorted(want - reached), sorted(reached - want))
        assert {n for ns in N_BY_WAVES.values() for n in ns} <= set(SMALL) | {5000} and {k for ks in K_BY_CAPACITY.values() for k in ks} == set(KS)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_special_states(gpu, dtype):
    """1, further: 130 bodies at one place; one NaN body; 1 000 bodies on a line with integer x, ascending (every later body j of a wave is farther from
    the low bodies and closer to the high ones) and descending"""
    same = np.zeros((130, 4), dtype)
    same[:, 3] = 1
    nan = lattice(300, dtype, 900, 10).copy()
    nan[130, 1] = np.nan
    up = np.zeros((1000, 4), dtype)
    up[:, 0], up[:, 3] = np.arange(1000), 1
    down = up[::-1].copy()
    for name, pos in (("one place", same), ("a NaN body", nan), ("ascending", up), ("descending", down)):
        index, dist = numpy_knn(pos, 16)
        if name == "one place":
            assert index[0].tolist() == list(range(1, 17)) and index[129].tolist() == list(range(16)) and not dist.any(), "every d2 is 0: the lowest other indices"
        if name == "a NaN body":
            assert (index[130] == NONE).all() and 130 not in index
        for k in KS:
            d = KnnDevice(gpu, pos, k).survey()
            check_lists(d, index, dist, (name, k))
            if k >= 2:
                check_densities(d, pos, index, dist, (name, k))
                if name == "one place":
                    assert d.record()["degenerate"] == 130 and d.record()["flags"] == DEGENERATE | NO_DENSITY and d.record()["max_kth_dist_sq"] == 0.0
            assert d.canaries_intact() and d.get("pos").tobytes() == pos.tobytes()
            d.free()


@gpu_only
@pytest.mark.parametrize("n", [70000, 262144])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_at_size_against_the_neighbour_library(gpu, dtype, n):
    """2.  A random normal cloud, K = 8; no O(N^2) host work"""
    k = 8
    pos = normal_cloud(n, dtype)
    d = KnnDevice(gpu, pos, k).survey()
    index, dist, first = d.get("index"), d.get("d2"), d.everything()
    assert d.canaries_intact() and d.get("pos").tobytes() == pos.tobytes()
    d.free()
    again = KnnDevice(gpu, pos, k, ws_fill=0xFF).survey()
    assert again.everything() == first, "the same bits from a second call, the record included, on a workspace of 0xFF bytes"
    again.free()
    s = NeighbourDevice(gpu, pos, radii=dist[:, k - 1])
    s.survey(0.0)
    nearest, nearest_d2, counts = s.get("nearest"), s.get("d2"), s.get("counts")
    s.free()
    assert np.array_equal(index[:, 0], nearest) and dist[:, 0].tobytes() == nearest_d2.tobytes(), "rank 0 is the survey's nearest, bit for bit"
    assert np.array_equal(counts, (dist < dist[:, k - 1:k]).sum(axis=1)), "the bodies strictly within the K-th distance are the row's entries below it"
    step_d, step_j = np.diff(dist, axis=1), np.diff(index.astype(np.int64), axis=1)
    assert (step_d >= 0).all() and (step_j[step_d == 0] > 0).all(), "rows are non-decreasing, ascending j on equal bits"
    assert (index != np.arange(n, dtype=np.uint32)[:, None]).all() and (index < n).all(), "no row holds its own body"
    ordered = np.sort(index, axis=1)
    assert (np.diff(ordered.astype(np.int64), axis=1) > 0).all(), "no row holds a body twice"


def long_double_rows(pos, rows):
    """d2 of the bodies `rows` to every body in long double, from the T-typed positions; the own body +inf"""
    p = pos[:, :3].astype(LD)
    d = p[None, :, :] - p[rows, None, :]
    d2 = (d * d).sum(axis=2)
    d2[np.arange(len(rows)), rows] = np.inf
    return d2


def check_cloud(gpu, dtype, n, k, rows=None):
    """3 and 4 on a random cloud of random masses"""
    pos, gamma = normal_cloud(n, dtype, "random"), LD(GAMMA[dtype])
    d = KnnDevice(gpu, pos, k).survey()
    index, dist, rho, record = d.get("index"), d.get("d2"), d.rho64(), d.record()
    assert d.canaries_intact() and d.get("pos").tobytes() == pos.tobytes()
    d.free()
    rows = np.arange(n) if rows is None else rows
    for s in range(0, len(rows), 256):
        i = rows[s:s + 256]
        exact = long_double_rows(pos, i)
        named = np.take_along_axis(exact, index[i].astype(np.int64), axis=1)
        got = dist[i].astype(LD)
        assert (np.abs(got - named) <= gamma * named).all(), "each reported d2 is its pair's to gamma"
        np.put_along_axis(exact, index[i].astype(np.int64), np.inf, axis=1)
        assert (exact.min(axis=1) >= (1 - 2 * gamma) * got[:, -1]).all(), "nobody outside a row is closer than (1 - 2 gamma) its last"
    step_d, step_j = np.diff(dist, axis=1), np.diff(index.astype(np.int64), axis=1)
    assert (step_d >= 0).all() and (step_j[step_d == 0] > 0).all() and (index < n).all()
    good = rho != 0
    assert record["defined"] == n and record["degenerate"] == 0 and record["flags"] == 0 and good.all()
    # rho itself from the device's own lists, in numpy's double: the same operations
    mine, _ = numpy_density(pos, index, dist, k)
    assert (np.abs(rho - mine) <= (k + 8) * 2.0 ** -53 * mine).all()
    want = numpy_structure(pos, rho, good, dist[:, k - 1], LD)
    for name in ("max_density", "max_density_body", "min_kth_dist_sq", "max_kth_dist_sq"):
        assert record[name] == want[name], name
    check_sums(record, want, pos, rho, n, k, (n, k, np.dtype(dtype).name))
    return record


@gpu_only
@pytest.mark.parametrize("k", [6, 16])
@pytest.mark.parametrize("n", [300, 5000])
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_clouds_against_long_double(gpu, dtype, n, k):
    check_cloud(gpu, dtype, n, k)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_sampled_bodies_of_a_large_cloud_against_long_double(gpu, dtype):
    rows = np.sort(np.random.default_rng(11).choice(65536, 256, replace=False))
    check_cloud(gpu, dtype, 65536, 6, rows)


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_density_centre_of_a_shifted_plummer_cloud(gpu, dtype):
    """A Plummer-like cloud (radii of the Plummer mass profile, scale 1, isotropic directions) shifted by (3, -2, 1): the density centre lies within the
    cloud's own core radius of the shift, and both radii are of the order of the scale"""
    n, k = 4096, 6
    rng = np.random.default_rng(3)
    r = (rng.uniform(0.001, 0.99, n) ** (-2 / 3) - 1) ** -0.5
    direction = rng.standard_normal((n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    pos = np.zeros((n, 4), dtype)
    pos[:, :3] = r[:, None] * direction + np.array([3.0, -2.0, 1.0])
    pos[:, 3] = 1.0 / n
    s = gpu.KnnSurvey(n, dtype)
    out = s.survey(pos, k)
    record = out["structure"]
    off = np.linalg.norm(np.array(record["centre"]) - np.array([3.0, -2.0, 1.0]))
    print(f"centre off by {off:.4f}; density radius {record['density_radius']:.4f}, core radius {record['core_radius']:.4f}")
    assert off < record["core_radius"] and 0.1 < record["core_radius"] < 1.0 and 0.1 < record["density_radius"] < 1.5
    radii = s.lagrangian_radii([0.1, 0.5, 0.9])
    assert (np.diff(radii) > 0).all() and 0.5 < radii[1] < 2.0, radii  # (the Plummer half-mass radius is 1.30 scales; the sample stops at 99 % of the mass)
    assert np.array_equal(radii, gpu.lagrangian_radii(pos, record["centre"], [0.1, 0.5, 0.9]))
    s.free()


@gpu_only
@pytest.mark.parametrize("dtype", DTYPES)
def test_python_class_graph_capture_and_null_outputs(gpu, dtype):
    """5.  The class gives the C calls' bits (a host array, a device address); two calls recorded in one linear stream capture replay to the same bits;
    an output that is not asked for stays untouched and changes no bit of the others"""
    n, k = 3000, 6
    pos = normal_cloud(n, dtype, "species")
    base = KnnDevice(gpu, pos, k).survey()
    want = base.everything()
    s = gpu.KnnSurvey(n, dtype)
    for positions in (pos, base.ptr("pos")):
        out = s.survey(positions, k)
        assert out["knn_index"].tobytes() == base.get("index").tobytes() and out["knn_dist_sq"].tobytes() == base.get("d2").tobytes()
        assert out["densities"].tobytes() == base.get("rho").tobytes() and out["structure"] == base.record()
        assert len(s.lagrangian_radii([0.5])) == 1
    lone = s.survey(pos, 1)
    assert lone["densities"] is None and lone["structure"] is None and np.array_equal(lone["knn_index"][:, 0], base.get("index")[:, 0])
    with pytest.raises(ValueError):
        s.survey(pos, 17)
    with pytest.raises(ValueError):
        s.survey(pos[:-1], k)
    with pytest.raises(gpu.NBodyHipError):
        s.survey(pos, 1, densities=True)
    s.free()

    lib, hip = gpu.lib(), hip_runtime()
    stream = ctypes.c_void_p()
    gpu.check(lib.nb_stream_create(ctypes.byref(stream)), "nb_stream_create")
    first, second = KnnDevice(gpu, pos, k, ws_fill=0xFF), KnnDevice(gpu, pos, 16, ws_fill=0xFF)
    sixteen = KnnDevice(gpu, pos, 16).survey().everything()
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    graph, graph_exec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0
    first.survey(stream=stream)
    second.survey(stream=stream)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
    assert first.untouched("index") and second.untouched("record"), "recorded, not run"
    assert hip.hipGraphInstantiate(ctypes.byref(graph_exec), graph, None, None, 0) == 0
    for _ in range(2):
        assert hip.hipGraphLaunch(graph_exec, stream) == 0
        gpu.check(lib.nb_stream_synchronize(stream), "nb_stream_synchronize")
        assert first.everything() == want and second.everything() == sixteen, "captured and replayed"
    assert first.canaries_intact() and second.canaries_intact()
    assert hip.hipGraphExecDestroy(graph_exec) == 0 and hip.hipGraphDestroy(graph) == 0
    first.free(), second.free()
    gpu.check(lib.nb_stream_destroy(stream), "nb_stream_destroy")

    for mask in range(1, 15):
        asked = tuple(name for bit, name in enumerate(OUTPUTS) if mask >> bit & 1)
        some = KnnDevice(gpu, pos, k).survey(outputs=asked)
        for name in OUTPUTS:
            if name in asked:
                assert some.get(name).tobytes() == base.get(name).tobytes(), (asked, name)
            else:
                assert some.untouched(name), (asked, name)
        assert some.canaries_intact(), asked
        some.free()
    base.free()


def cli_knn_lines(stdout):
    """the five lines of `nbody --knn` as a dict of floats and ints"""
    import re
    number = r"([-+0-9.eE]+|nan|inf|-inf)"
    out = {}
    m = re.search(rf"^density centre: {number} {number} {number} \(K = (\d+), (\d+) bodies defined, (\d+) degenerate\)$", stdout, re.M)
    out.update(centre=tuple(float(v) for v in m.groups()[:3]), k=int(m.group(4)), defined=int(m.group(5)), degenerate=int(m.group(6)))
    m = re.search(rf"^density radius: {number}, core radius: {number}$", stdout, re.M)
    out.update(density_radius=float(m.group(1)), core_radius=float(m.group(2)))
    m = re.search(rf"^densest body: (\d+), density {number}$", stdout, re.M)
    out.update(max_density_body=int(m.group(1)), max_density=float(m.group(2)))
    m = re.search(rf"^K-th neighbour distance: smallest {number}, largest {number}$", stdout, re.M)
    out.update(smallest=float(m.group(1)), largest=float(m.group(2)))
    m = re.search(rf"^Lagrangian radii \(10%, 50%, 90%\): {number} {number} {number}$", stdout, re.M)
    out.update(lagrangian=tuple(float(v) for v in m.groups()))
    return out


@gpu_only
@pytest.mark.parametrize("flags", [(), ("--fp64",), ("--integrator=hermite-block",)], ids=["fp32", "fp64", "hermite-block"])
def test_cli_prints_the_record_of_the_dumped_state(gpu, tmp_path, flags):
    """5.  `nbody --knn=6 --numbodies=4096 --steps=1 --dump`: the record it prints is the Python one for the dumped state, digit for digit (17
    significant digits), after the run's own lines and --neighbours' three"""
    import subprocess
    from test_knn import CLI
    n, k = 4096, 6
    dump = tmp_path / "state.bin"
    r = subprocess.run([CLI, f"--numbodies={n}", "--steps=1", f"--knn={k}", "--neighbours=0.5", f"--dump={dump}", *flags], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    dtype = np.float64 if "--fp64" in flags else np.float32
    pos = np.fromfile(dump, dtype=dtype)[:4 * n].reshape(n, 4)
    s = gpu.KnnSurvey(n, dtype)
    want = s.survey(pos, k)["structure"]
    radii = s.lagrangian_radii([0.1, 0.5, 0.9])
    s.free()
    got = cli_knn_lines(r.stdout)
    assert r.stdout.index("deepest potential:") < r.stdout.index("density centre:")
    assert got["centre"] == want["centre"] and (got["k"], got["defined"], got["degenerate"]) == (k, want["defined"], want["degenerate"])
    assert (got["density_radius"], got["core_radius"], got["max_density"], got["max_density_body"]) == (want["density_radius"], want["core_radius"], want["max_density"],
                                                                                                       want["max_density_body"])
    assert (got["smallest"], got["largest"]) == (np.sqrt(want["min_kth_dist_sq"]), np.sqrt(want["max_kth_dist_sq"]))
    assert np.allclose(got["lagrangian"], radii, rtol=1e-13, atol=0), (got["lagrangian"], radii)


@gpu_only
def test_knn_speed_sanity(gpu):
    """6.  65 536 bodies fp32, K = 8, a random cloud; device events, the median of 5 single calls after warm-up, against nb_neighbour_survey_f32 without
    potentials in the same process: no more than 2 x the cost model of tests/test_knn.py (the house margin)."""
    n, k, dtype = 65536, 8, np.float32
    pos = normal_cloud(n, dtype)
    model, groups, candidates = knn_model(n, k)

    def median_ms(fn):
        fn(), fn()
        times = []
        for _ in range(5):
            start, stop = gpu.Event(), gpu.Event()
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_ms(stop))
        return sorted(times)[2]

    s = NeighbourDevice(gpu, pos)
    t_survey = median_ms(lambda: s.survey(0.01, 0.0, outputs=("nearest", "d2", "counts")))
    s.free()
    d = KnnDevice(gpu, pos, k)
    t_lists = median_ms(lambda: d.survey(outputs=("index", "d2")))
    t_all = median_ms(lambda: d.survey())
    d.free()
    print(f"survey {t_survey:.3f} ms; knn lists {t_lists:.3f} ms = {t_lists / t_survey:.2f}x, with densities and the record {t_all:.3f} ms = {t_all / t_survey:.2f}x "
          f"(model {model:.2f}x from {groups:.2f} of the groups and {candidates:.3f} of the candidates on the insertion path; ratio / model {t_all / t_survey / model:.2f})")
    assert t_all <= 2 * model * t_survey, (t_all, t_survey, model)
