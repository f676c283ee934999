"""The energy diagnostics pair by pair and body by body: nb_energy_* (csrc/nbody_energy.hip) and nb_energy_ensemble_*
(csrc/energy_ensemble.hip) reduce a system to thirteen doubles, and a sum over random cubes cannot see one pair among millions.

1. Probe pairs.  A system of n bodies on a fixed cloud in which only bodies i < j have a mass (1.5 and 0.75): its potential must be,
   BIT FOR BIT, what the same entry point gives for those two bodies alone -- every other term is m_j * inv with a zero factor and a
   finite inv, and the fp64 fold adds exact zeros -- so a dropped pair shows as 0 and a doubled one as twice the value.  The two-body
   value is held to the long double -m_i m_j / sqrt(d^2 + eps^2) within min(2 x measured, CAP) of tests/test_fast_domain.py.  Up to
   130 bodies every pair is probed; above that every pair among the edge indices of the geometry (edge_indices below).  The sizes come
   from the plan query: every (R, S) nb_energy_ensemble_plan_* can select, the largest shape with 1 .. 6 blocks, sizes one body past a
   block boundary; the solo call at block counts of both parities and at its first size with two splits.
2. Probe bodies.  The same with ONE body of mass 1.5 and random positions and velocities everywhere: all thirteen doubles must be, bit
   for bit, those of that body alone, which are held to long double formulas within 8 x 2^-53 of each term's magnitude.
3. Non-finite inputs.  A NaN coordinate, an infinite mass, a NaN velocity and a zero-mass body ON another body with eps^2 == 0 poison
   their own system's fields as the definition says, evaluated in numpy in the kernel's order, and no other system's bytes.
4. The "Operand range" paragraph of include/nbody_hip.h and include/nbody_hip_energy_ensemble.h states what 1 - 3 and
   tests/test_fast_domain.py::test_energy_pair_potential_across_the_exponent_range hold.

The CPU tests need no device: the probe builder against the fp64 numpy sum of tests/test_energy.py, the coverage of the sizes against
the plan query, the header paragraph."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, entry
from test_energy import FIELDS, Softening, gpu_energy, random_state, ref_energy
from test_energy_ensemble import geometry, measure, record_bytes, upload
from test_fast_domain import CAP, ENERGY_MEASURED, sweep_probes

gpu_only = pytest.mark.gpu
LD = np.longdouble
F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
LANE_WIDTH = {F32: 2, F64: 1}
M_I, M_J = 1.5, 0.75       # the two masses of a probe pair; M_I is the mass of a probe body
EPS2 = (0.01, 0.0)         # softened, and not: the bystanders coincide with nothing, so eps 0 stays finite
ALL_PAIRS_UP_TO = 130      # n(n-1)/2 systems in one launch: 8 385 at the most
LARGEST = 2600             # no size of the ensemble's list is above it
SOLO_BLOCK = {F32: 512, F64: 256}  # nbody_energy.hip: 64 lanes x 4 vectors of W bodies i, whatever N
# 2, 3, 5 and 9 / 17 blocks, the last of one body, and 4097 with two workgroups per block; 1537 / 769: four blocks, where the antipodal
# pairs are (0, 2), taken whole, and (1, 3), against a block of one body
SOLO_SIZES = {F32: (513, 1025, 1537, 2049, 4097), F64: (257, 513, 769, 1025, 4097)}
TERM_TOL = 8 * 2.0 ** -53  # an O(N) term of one body: six fp64 roundings with margin


# ---------------------------------------------------------------------------------------------------------------- geometry
def ensemble_shape(pkg, n, dtype):
    """(R, S, B, NB, splits) of the plan query: vectors per lane, waves, bodies of a block, blocks, workgroups that share a block"""
    (lane, waves, groups, _, _), _ = geometry(pkg, n, 1, dtype)
    block = 64 * lane
    blocks = -(-n // block)
    assert groups % blocks == 0, (n, groups, blocks)
    return lane // LANE_WIDTH[dtype], waves, block, blocks, groups // blocks


def solo_shape(pkg, n, dtype):
    """(B, NB) of nb_energy_*; the workspace query (one 128-byte record per workgroup, the larger of the two precisions) must hold them"""
    block = SOLO_BLOCK[dtype]
    blocks = -(-n // block)
    assert pkg.energy_workspace_bytes(n) % 128 == 0 and pkg.energy_workspace_bytes(n) // 128 >= blocks
    return block, blocks


def windows(pkg, dtype, last):
    """[((R, S), first n, last n)] of the plan query over 1 .. last"""
    out = []
    for n in range(1, last + 1):
        shape = ensemble_shape(pkg, n, dtype)[:2]
        if out and out[-1][0] == shape:
            out[-1][2] = n
        else:
            out.append([shape, n, n])
    return [tuple(w) for w in out]


def ensemble_sizes(pkg, dtype):
    """The sizes of parts 1 and 2, read off the plan query: the first (from 3 bodies: a pair and a bystander) and the last n of every
    window of (R, S) up to LARGEST; B + 1 wherever a shape has it (two blocks, the second of one body); for the largest shape
    (NB - 1) B + 1 for NB = 2 .. 6, one block where the shape has it, and four whole blocks."""
    found = windows(pkg, dtype, LARGEST)
    out = set()
    for k, (shape, first, last) in enumerate(found):
        out.add(max(first, 3))
        if k + 1 < len(found):
            out.add(last)
        block = ensemble_shape(pkg, first, dtype)[2]
        if first <= block + 1 <= last:
            out.add(block + 1)
    shape, first, last = found[-1]
    block = ensemble_shape(pkg, first, dtype)[2]
    out |= {n for n in [(nb - 1) * block + 1 for nb in range(2, 7)] + [block, 4 * block] if first <= n <= last}
    return sorted(out)


def edge_indices(n, block, blocks):
    """the bodies at which the geometry changes: the ends of a wave's slots, of chunks, of blocks, of the antipodal block, of the system"""
    h = blocks // 2
    raw = (0, 1, 63, 64, 65, 127, 128, block - 1, block, block + 1, 2 * block - 1, 2 * block, h * block - 1, h * block, h * block + 64,
           n - 65, n - 64, n - 2, n - 1)
    return sorted({i for i in raw if 0 <= i < n})


def probe_pairs(n, block, blocks):
    """(K, 2) index pairs i < j: all of them up to ALL_PAIRS_UP_TO bodies, else all among the edge indices"""
    idx = np.arange(n) if n <= ALL_PAIRS_UP_TO else np.array(edge_indices(n, block, blocks))
    i, j = np.triu_indices(len(idx), 1)
    pairs = np.stack([idx[i], idx[j]], axis=1)
    assert n <= ALL_PAIRS_UP_TO or len(pairs) >= 15, (n, len(pairs))
    return pairs


def probe_bodies(n, block, blocks):
    return np.arange(n) if n <= ALL_PAIRS_UP_TO else np.array(edge_indices(n, block, blocks))


# ---------------------------------------------------------------------------------------------------------------- probe systems
_CLOUD = {}


def cloud(n, dtype):
    """the first n points of ONE seeded cloud in [-1, 1]^3, rounded to T: distinct, every d^2 normal in T"""
    if dtype not in _CLOUD:
        _CLOUD[dtype] = np.random.default_rng(20261021).uniform(-1, 1, (65536, 3)).astype(dtype)
    return _CLOUD[dtype][:n]


def probe_pair_systems(n, pairs, dtype):
    """(K, n, 4) systems in which only bodies i, j of pair k have a mass, and the (K, 2, 4) two-body systems of those bodies alone"""
    k = np.arange(len(pairs))
    pos = np.zeros((len(pairs), n, 4), dtype)
    pos[:, :, :3] = cloud(n, dtype)
    pos[k, pairs[:, 0], 3], pos[k, pairs[:, 1], 3] = M_I, M_J
    two = np.stack([pos[k, pairs[:, 0]], pos[k, pairs[:, 1]]], axis=1)
    return pos, two


def pair_potentials(two, eps2):
    """long double -m_i m_j / sqrt(d^2 + eps^2) of (K, 2, 4) two-body systems, eps^2 as T holds it"""
    p = two.astype(LD)
    d = p[:, 1, :3] - p[:, 0, :3]
    return -p[:, 0, 3] * p[:, 1, 3] / np.sqrt((d * d).sum(axis=1) + LD(two.dtype.type(eps2)))


def probe_body_systems(n, bodies, dtype, seed):
    """(K, n, 4) positions and velocities, all random, in which only body bodies[k] of system k has a mass; and the one-body systems"""
    pos, vel = (np.array(a, dtype).reshape(n, 4) for a in random_state(n, seed))
    pos[:, 3] = 0
    k = np.arange(len(bodies))
    many_pos, many_vel = np.repeat(pos[None], len(bodies), axis=0), np.repeat(vel[None], len(bodies), axis=0)
    many_pos[k, bodies, 3] = M_I
    return many_pos, many_vel, many_pos[k, bodies][:, None, :].copy(), many_vel[k, bodies][:, None, :].copy()


def one_body_terms(pos, vel):
    """{field: (long double value, magnitude)} of ONE body {x, y, z, m}, {vx, vy, vz, -}; 13 values in the order of nb_energy_t"""
    (x, y, z, m), (vx, vy, vz) = pos.astype(LD), vel.astype(LD)[:3]
    kin = m * (vx * vx + vy * vy + vz * vz) / 2
    value = [kin, LD(0), kin, m, m * vx, m * vy, m * vz, m * (y * vz - z * vy), m * (z * vx - x * vz), m * (x * vy - y * vx), x, y, z]
    size = [kin, LD(0), kin, m, abs(m * vx), abs(m * vy), abs(m * vz), m * (abs(y * vz) + abs(z * vy)), m * (abs(z * vx) + abs(x * vz)),
            m * (abs(x * vy) + abs(y * vx)), abs(x), abs(y), abs(z)]
    return np.array(value, LD), np.array(size, LD)


def record(result):
    """the 13 doubles of a result dict in the order of nb_energy_t"""
    return np.frombuffer(record_bytes(result), np.float64)


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- checks
def pair_bound(dtype):
    name = np.dtype(dtype).name
    return min(2 * ENERGY_MEASURED[name], CAP[name])


def check_probe_pairs(got, ref, pairs, two, eps2, what):
    """got: the potentials and masses of the probe systems; ref: the potentials of the two-body systems from the same entry point.
    Returns the worst relative error of the two-body values against long double."""
    pot, mass, alone = np.array(got[0], np.float64), np.array(got[1], np.float64), np.array(ref, np.float64)
    want = pair_potentials(two, eps2)
    broken = np.flatnonzero(~(np.isfinite(alone) & (alone < 0)))
    assert not len(broken), f"{what} eps^2 = {eps2}: the two-body potential is not a finite negative number: " + "; ".join(
        f"pair ({pairs[k][0]}, {pairs[k][1]}) alone gives {alone[k]!r}, in the probe system {pot[k]!r}" for k in broken[:6])
    err = np.abs((alone.astype(LD) - want) / want).astype(np.float64)
    worst = float(err.max()) if len(err) else 0.0
    print(f"{what} eps^2 = {eps2}: {len(pairs)} probe pairs, two-body potentials within {worst:.3e} of long double (bound {pair_bound(two.dtype.type):.3e})")
    bad = np.flatnonzero(bits(pot) != bits(alone))
    assert not len(bad), f"{what} eps^2 = {eps2}: {len(bad)} of {len(pairs)} probe pairs are not counted exactly once: " + "; ".join(
        f"pair ({pairs[k][0]}, {pairs[k][1]}) gives {pot[k]!r}, {pot[k] / alone[k]:.6g} x the two-body {alone[k]!r}" for k in bad[:6])
    off = np.flatnonzero(mass != M_I + M_J)
    assert not len(off), f"{what} eps^2 = {eps2}: mass != 2.25 in the systems of pairs {[tuple(pairs[k]) for k in off[:6]]}: {mass[off[:6]]}"
    k = int(err.argmax()) if len(err) else 0
    assert worst <= pair_bound(two.dtype.type), f"{what} eps^2 = {eps2}: pair ({pairs[k][0]}, {pairs[k][1]}): {alone[k]!r} is {worst:.3e} off {want[k]!r}"
    return worst


def ensemble_probe_pairs(gpu, dtype, n, what):
    """part 1 through nb_energy_ensemble_*: all probe systems of the size in ONE call per eps^2, their two-body systems in another"""
    _, _, block, blocks, _ = ensemble_shape(gpu, n, dtype)
    pairs = probe_pairs(n, block, blocks)
    if not len(pairs):
        return 0.0
    pos, two = probe_pair_systems(n, pairs, dtype)
    still, still2 = np.zeros_like(pos), np.zeros_like(two)
    worst = 0.0
    for eps2 in EPS2:
        got = measure(gpu, pos, still, dtype, eps2)
        ref = measure(gpu, two, still2, dtype, eps2)
        worst = max(worst, check_probe_pairs(([e["potential"] for e in got], [e["mass"] for e in got]), [e["potential"] for e in ref], pairs, two, eps2, what))
    return worst


def check_probe_bodies(got, ref, bodies, one_pos, one_vel, what):
    """got: (K, 13) records of the probe systems; ref: (K, 13) of the one-body systems from the same entry point"""
    got, ref = np.asarray(got), np.asarray(ref)
    bad = np.flatnonzero((bits(got) != bits(ref)).any(axis=1))
    names = [f if k is None else f"{f}[{k}]" for f in FIELDS for k in ((None,) if f in FIELDS[:4] else range(3))]
    assert not len(bad), f"{what}: {len(bad)} of {len(bodies)} probe bodies are not counted exactly once: " + "; ".join(
        f"body {bodies[k]}: " + ", ".join(f"{names[f]} {got[k, f]!r} for {ref[k, f]!r}" for f in np.flatnonzero(bits(got[k]) != bits(ref[k]))) for k in bad[:4])
    assert (got[:, 1] == 0).all(), f"{what}: a potential is not exactly 0"
    worst = 0.0
    for k in range(len(bodies)):
        value, size = one_body_terms(one_pos[k, 0], one_vel[k, 0])
        err = np.abs(ref[k].astype(LD) - value)
        assert (err <= TERM_TOL * size).all(), f"{what}: body {bodies[k]} alone: {dict(zip(names, ref[k]))} against {dict(zip(names, value))}"
        worst = max(worst, float((err[size > 0] / size[size > 0]).max()))
    return worst


def ensemble_probe_bodies(gpu, dtype, n, what):
    """part 2 through nb_energy_ensemble_*: one launch per size and eps^2, and one of the one-body systems"""
    _, _, block, blocks, _ = ensemble_shape(gpu, n, dtype)
    bodies = probe_bodies(n, block, blocks)
    pos, vel, one_pos, one_vel = probe_body_systems(n, bodies, dtype, 7000 + n)
    worst = 0.0
    for eps2 in EPS2:
        got = [record(e) for e in measure(gpu, pos, vel, dtype, eps2)]
        ref = [record(e) for e in measure(gpu, one_pos, one_vel, dtype, eps2)]
        worst = max(worst, check_probe_bodies(got, ref, bodies, one_pos, one_vel, f"{what} eps^2 = {eps2}"))
    print(f"{what}: {len(bodies)} probe bodies, one-body terms within {worst:.3e} of long double (bound {TERM_TOL:.3e})")
    return worst


class SoloSystem:
    """one uploaded system of n bodies of mass 0 for nb_energy_*; set() changes single masses between calls"""

    def __init__(self, gpu, pos, vel, dtype):
        self.gpu, self.dtype, self.n = gpu, dtype, len(pos)
        self.pos, self.vel = upload(gpu, np.ascontiguousarray(pos, dtype)), upload(gpu, np.ascontiguousarray(vel, dtype))
        self.small = gpu.DeviceBuffer(8 * np.dtype(dtype).itemsize), gpu.DeviceBuffer(8 * np.dtype(dtype).itemsize)
        self.work = gpu.DeviceBuffer(gpu.energy_workspace_bytes(self.n))

    def set(self, body, mass):
        size = np.dtype(self.dtype).itemsize
        value = np.array([mass], self.dtype)
        self.gpu.check(self.gpu.lib().nb_h2d(ctypes.c_void_p(self.pos.ptr.value + (4 * int(body) + 3) * size), value.ctypes.data_as(ctypes.c_void_p), size, None), "nb_h2d")

    def energy(self):
        return self.gpu.energy(self.pos.ptr, self.vel.ptr, self.n, self.dtype, workspace=self.work)

    def alone(self, pos, vel):
        """the same entry point on the few bodies of (k, 4) arrays"""
        self.small[0].upload(np.ascontiguousarray(pos, self.dtype)), self.small[1].upload(np.ascontiguousarray(vel, self.dtype))
        return self.gpu.energy(self.small[0].ptr, self.small[1].ptr, len(pos), self.dtype, workspace=self.work)

    def free(self):
        for buf in (self.pos, self.vel, self.work, *self.small):
            buf.free()


# ---------------------------------------------------------------------------------------------------------------- CPU
# The windows of (R, S) over 1 <= n <= 65 536, as plan_energy_ensemble gives them.  fp64 never reaches four vectors and four waves with
# one block (256 bodies are (4, 2)), and never has more than one workgroup per block.
WINDOWS = {F32: (((1, 1), 1, 128), ((1, 2), 129, 255), ((2, 2), 256, 256), ((2, 4), 257, 511), ((4, 4), 512, 65536)),
           F64: (((1, 1), 1, 127), ((2, 1), 128, 128), ((2, 2), 129, 255), ((4, 2), 256, 256), ((4, 4), 257, 65536))}


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_sizes_cover_every_shape_the_plan_can_select(pkg, dtype):
    assert tuple(windows(pkg, dtype, 65536)) == WINDOWS[dtype]
    sizes = ensemble_sizes(pkg, dtype)
    shapes = {n: ensemble_shape(pkg, n, dtype) for n in sizes}
    assert sizes[-1] <= LARGEST and sizes[0] >= 3 and 8 <= len(sizes) <= 16, sizes
    assert {s[:2] for s in shapes.values()} == {w[0] for w in WINDOWS[dtype]}
    for shape, first, last in WINDOWS[dtype]:
        assert max(first, 3) in sizes and (last in sizes or last == 65536), (shape, sizes)  # the single-size windows among them
    largest = [s for s in shapes.values() if s[:2] == (4, 4)]
    every = {ensemble_shape(pkg, n, dtype)[4] for n in range(1, 65537, 61)}
    if dtype == F32:
        assert {s[3] for s in largest} >= {1, 2, 3, 4, 5, 6} and every == {1, 2}
    else:  # (one block of 256 is (4, 2); no fp64 plan shares a block)
        assert {s[3] for s in largest} >= {2, 3, 4, 5, 6} and every == {1} and shapes[256][:4] == (4, 2, 256, 1)
    assert {s[4] for s in largest} == every
    # one body past a block boundary: in every shape that has two blocks, and in the largest at every block count from 2 to 6
    one_past = {(s[:2], s[3]) for n, s in shapes.items() if n == (s[3] - 1) * s[2] + 1 and s[3] >= 2}
    assert one_past >= {((4, 4), nb) for nb in range(2, 7)}
    for shape, first, last in WINDOWS[dtype]:
        block = ensemble_shape(pkg, first, dtype)[2]
        assert (shape, 2) in one_past or not first <= block + 1 <= last, shape
    # a whole last block at an even block count, where the antipodal pair of blocks is full on both sides
    assert any(s[:2] == (4, 4) and s[3] % 2 == 0 and n == s[3] * s[2] for n, s in shapes.items())
    # the probes: every pair up to 130 bodies, at least 15 pairs above, all inside the system
    for n, (_, _, block, blocks, _) in shapes.items():
        pairs = probe_pairs(n, block, blocks)
        assert len(pairs) == (n * (n - 1) // 2 if n <= ALL_PAIRS_UP_TO else len(edge_indices(n, block, blocks)) * (len(edge_indices(n, block, blocks)) - 1) // 2)
        assert (pairs[:, 0] < pairs[:, 1]).all() and pairs.min() == 0 and pairs.max() == n - 1 and len({tuple(p) for p in pairs}) == len(pairs)
    for n in SOLO_SIZES[dtype]:
        block, blocks = solo_shape(pkg, n, dtype)
        assert len(probe_pairs(n, block, blocks)) >= 15
    assert {solo_shape(pkg, n, dtype)[1] % 2 for n in SOLO_SIZES[dtype]} == {0, 1}
    # the solo call's size with two workgroups per block: the query answers for the larger of the two precisions, fp64's 5, 9 and 17 blocks
    assert [pkg.energy_workspace_bytes(n) // 128 for n in (1025, 2049, 4097)] == [5, 9, 2 * 17]


def test_edge_indices_are_the_ones_listed():
    assert edge_indices(2049, 512, 5) == [0, 1, 63, 64, 65, 127, 128, 511, 512, 513, 1023, 1024, 1088, 1984, 1985, 2047, 2048]
    assert edge_indices(257, 256, 2) == [0, 1, 63, 64, 65, 127, 128, 192, 193, 255, 256]
    assert edge_indices(131, 128, 2) == [0, 1, 63, 64, 65, 66, 67, 127, 128, 129, 130]


@pytest.mark.parametrize("dtype", DTYPES)
def test_probe_systems_hold_a_single_term(dtype):
    """the builders against the fp64 numpy sum: every probe pair system's potential is finite, nonzero and the single term; every probe
    body system's record is the body's own"""
    for n, block in ((7, 64), (130, 64), (513, 256), (1100, 512)):
        points = cloud(n, dtype).astype(np.float64)
        assert len(np.unique(points, axis=0)) == n and (np.abs(points) <= 1).all()
        d2 = ((points[:, None, :] - points[None, :, :]) ** 2).sum(axis=2)[np.triu_indices(n, 1)]
        assert (d2.astype(dtype) >= np.finfo(dtype).tiny).all()
        pairs = probe_pairs(n, block, -(-n // block))
        pairs = pairs[:: max(1, len(pairs) // 40)]  # (the numpy sum is O(n^2) per system)
        pos, two = probe_pair_systems(n, pairs, dtype)
        assert ((pos[:, :, 3] != 0).sum(axis=1) == 2).all() and not (pos[:, :, :3] != cloud(n, dtype)).any()
        for eps2 in EPS2:
            want = pair_potentials(two, eps2)
            for k, (i, j) in enumerate(pairs):
                ref = ref_energy(pos[k], np.zeros_like(pos[k]), float(dtype(eps2)))
                assert np.isfinite(ref["potential"]) and ref["potential"] < 0 and ref["mass"] == M_I + M_J, (n, i, j)
                assert abs(ref["potential"] - float(want[k])) <= 4 * 2.0 ** -53 * abs(float(want[k])), (n, i, j, ref["potential"], want[k])
                assert ref["potential"] == ref_energy(two[k], np.zeros_like(two[k]), float(dtype(eps2)))["potential"], (n, i, j)
        bodies = probe_bodies(n, block, -(-n // block))[::7]
        many_pos, many_vel, one_pos, one_vel = probe_body_systems(n, bodies, dtype, 7000 + n)
        assert ((many_pos[:, :, 3] != 0).sum(axis=1) == 1).all() and (many_vel[:, :, :3] != 0).all()
        for k, i in enumerate(bodies):
            ref = ref_energy(many_pos[k], many_vel[k], 0.01)
            value, size = one_body_terms(one_pos[k, 0], one_vel[k, 0])
            assert ref["potential"] == 0 and (np.abs(record(ref).astype(LD) - value) <= TERM_TOL * size).all(), (n, i)
            assert one_pos[k, 0].tobytes() == many_pos[k, i].tobytes() and one_vel[k, 0].tobytes() == many_vel[k, i].tobytes()


HEADERS = ("nbody_hip.h", "nbody_hip_energy_ensemble.h")


def test_the_operand_range_is_the_one_the_headers_state():
    """the paragraph of both headers against the probes, the bounds and the constants it speaks of"""
    window = {}
    for dtype in DTYPES:  # the whole powers of two between the smallest and the largest d^2 + eps^2 of the probes
        s2 = np.concatenate([d2 + eps2 for eps2, d2 in sweep_probes(dtype)])
        assert (s2.astype(dtype) >= np.finfo(dtype).tiny).all() and np.isfinite(s2.astype(dtype)).all()
        window[dtype] = f"[2^{int(np.ceil(np.log2(s2.min())))}, 2^{int(np.floor(np.log2(s2.max())))}]"
    assert window == {F32: "[2^-83, 2^84]", F64: "[2^-599, 2^601]"}
    csrc = os.path.join(ROOT, "cuda-nbody_amd", "csrc")
    solo, ensemble = open(os.path.join(csrc, "nbody_energy.hip")).read(), open(os.path.join(csrc, "energy_ensemble.hip")).read()
    chunk, unit = int(re.search(r"constexpr unsigned kChunk\s*=\s*(\d+);", solo).group(1)), int(re.search(r"constexpr unsigned kUnit\s*=\s*(\d+);", ensemble).group(1))
    assert CAP == {"float32": 1e-6, "float64": 1e-14}
    for name in HEADERS:
        text = open(os.path.join(ROOT, "include", name)).read()
        text = re.sub(r"\s*\n \*\s*", " ", text)
        paragraph = text[text.index("Operand range."):]
        paragraph = paragraph[:paragraph.index("*/")]
        assert f"d^2 + eps^2 in {window[F32]} (fp32) / {window[F64]} (fp64)" in paragraph, name
        assert "1e-6 (fp32) / 1e-14 (fp64)" in paragraph and "tests/test_energy_domain.py" in paragraph, name
        assert f"at most {chunk} (nb_energy_f32) / {unit} (nb_energy_ensemble_f32) bodies j" in paragraph, name
        for rule in ("A NaN coordinate", "An infinite mass", "A NaN velocity", "0 * inf = NaN", "no other system"):
            assert rule in paragraph, (name, rule)
        assert "contribute nothing when eps^2 > 0 or when they coincide with no body" in text, name
        assert "Zero-mass padding bodies contribute nothing." not in text, name
    assert "never run over more than 128" not in open(os.path.join(ROOT, "include", HEADERS[1])).read()


# ---------------------------------------------------------------------------------------------------------------- GPU: 1. probe pairs
def _sizes(dtype):
    return ensemble_sizes(entry.load_package(), dtype)


ENSEMBLE_CASES = [(dtype, n) for dtype in DTYPES for n in _sizes(dtype)]
SOLO_CASES = [(dtype, n) for dtype in DTYPES for n in SOLO_SIZES[dtype]]
case_id = lambda case: f"{np.dtype(case[0]).name}-{case[1]}"  # noqa: E731


@gpu_only
@pytest.mark.parametrize("case", ENSEMBLE_CASES, ids=case_id)
def test_ensemble_counts_every_probe_pair_once(gpu, case):
    """every probe system of the size in one launch per eps^2.  Measured (MI355X): the two-body potentials of the cloud are within
    1.675e-7 (fp32) / 3.359e-16 (fp64) of long double (ENERGY_PROBE_MEASURED of tests/test_fast_domain.py), inside the asserted
    min(2 x ENERGY_MEASURED, CAP) = 2.244e-7 / 4.764e-16."""
    dtype, n = case
    ensemble_probe_pairs(gpu, dtype, n, f"nb_energy_ensemble {np.dtype(dtype).name} n = {n} {ensemble_shape(gpu, n, dtype)}")


@gpu_only
@pytest.mark.parametrize("case", SOLO_CASES, ids=case_id)
def test_solo_counts_every_probe_pair_once(gpu, case):
    """nb_energy_*: the pairs among the edge indices, one call per pair on one uploaded array where only the two masses change"""
    dtype, n = case
    block, blocks = solo_shape(gpu, n, dtype)
    pairs = probe_pairs(n, block, blocks)
    pos = np.zeros((n, 4), dtype)
    pos[:, :3] = cloud(n, dtype)
    system = SoloSystem(gpu, pos, np.zeros_like(pos), dtype)
    try:
        for eps2 in EPS2:
            got, ref, twos = ([], []), [], []
            with Softening(gpu, dtype, eps2):
                for i, j in pairs:
                    system.set(i, M_I), system.set(j, M_J)
                    e = system.energy()
                    system.set(i, 0), system.set(j, 0)
                    two = np.array([[*pos[i, :3], M_I], [*pos[j, :3], M_J]], dtype)
                    got[0].append(e["potential"]), got[1].append(e["mass"]), twos.append(two)
                    ref.append(system.alone(two, np.zeros_like(two))["potential"])
            check_probe_pairs(got, ref, pairs, np.stack(twos), eps2, f"nb_energy {np.dtype(dtype).name} n = {n} ({blocks} blocks of {block})")
    finally:
        system.free()


# ---------------------------------------------------------------------------------------------------------------- GPU: 2. probe bodies
@gpu_only
@pytest.mark.parametrize("case", ENSEMBLE_CASES, ids=case_id)
def test_ensemble_counts_every_probe_body_once(gpu, case):
    dtype, n = case
    ensemble_probe_bodies(gpu, dtype, n, f"nb_energy_ensemble {np.dtype(dtype).name} n = {n} {ensemble_shape(gpu, n, dtype)}")


@gpu_only
@pytest.mark.parametrize("case", SOLO_CASES, ids=case_id)
def test_solo_counts_every_probe_body_once(gpu, case):
    dtype, n = case
    block, blocks = solo_shape(gpu, n, dtype)
    bodies = probe_bodies(n, block, blocks)
    many_pos, many_vel, one_pos, one_vel = probe_body_systems(n, bodies, dtype, 7000 + n)
    pos = many_pos[0].copy()
    pos[:, 3] = 0
    system = SoloSystem(gpu, pos, many_vel[0], dtype)
    what = f"nb_energy {np.dtype(dtype).name} n = {n} ({blocks} blocks of {block})"
    try:
        for eps2 in EPS2:
            got, ref = [], []
            with Softening(gpu, dtype, eps2):
                for k, i in enumerate(bodies):
                    system.set(i, M_I)
                    got.append(record(system.energy()))
                    system.set(i, 0)
                    ref.append(record(system.alone(one_pos[k], one_vel[k])))
            worst = check_probe_bodies(got, ref, bodies, one_pos, one_vel, f"{what} eps^2 = {eps2}")
        print(f"{what}: {len(bodies)} probe bodies, one-body terms within {worst:.3e} of long double (bound {TERM_TOL:.3e})")
    finally:
        system.free()


# ---------------------------------------------------------------------------------------------------------------- GPU: 3. non-finite inputs
POISONS = ("a NaN coordinate", "clean", "an infinite mass", "a NaN velocity", "clean", "a zero-mass body on another")  # four poisoned systems, two clean


def poisoned_batch(n, dtype, seed):
    """six systems of n bodies (POISONS) and the same six untouched; the poisoned bodies sit in different chunks and blocks"""
    clean_pos = np.stack([np.array(random_state(n, seed + s)[0], dtype).reshape(n, 4) for s in range(len(POISONS))])
    clean_vel = np.stack([np.array(random_state(n, seed + s)[1], dtype).reshape(n, 4) for s in range(len(POISONS))])
    pos, vel = clean_pos.copy(), clean_vel.copy()
    pos[0, 70, 1] = np.nan
    pos[2, n - 3, 3] = np.inf
    vel[3, 129, 0] = np.nan
    pos[5, n - 40] = [*pos[5, 10, :3], 0]  # (a later body j of mass 0 on body 10: the kernels reach it as m_j * inf)
    return pos, vel, clean_pos, clean_vel


def definition(pos, vel, eps2):
    """nb_energy_t in fp64 numpy in the kernels' order of operations: d^2 = dz^2 + (dy^2 + (dx^2 + eps^2)), the masked terms j <= i as
    m_j * 0, a body's sum times m_i, the O(N) terms as the kernels write them; 13 values"""
    with np.errstate(all="ignore"):
        p, m, v = pos[:, :3].astype(np.float64), pos[:, 3].astype(np.float64), vel[:, :3].astype(np.float64)
        d = p[None, :, :] - p[:, None, :]
        d2 = d[:, :, 2] ** 2 + (d[:, :, 1] ** 2 + (d[:, :, 0] ** 2 + float(pos.dtype.type(eps2))))
        n = len(m)
        inv = np.where(np.arange(n)[None, :] > np.arange(n)[:, None], 1.0 / np.sqrt(d2), 0.0)
        pot = -(m * (m[None, :] * inv).sum(axis=1)).sum()
        kin = 0.5 * (m * (v[:, 0] ** 2 + v[:, 1] ** 2 + v[:, 2] ** 2)).sum()
        mass = m.sum()
        return np.array([kin, pot, kin + pot, mass, *(m[:, None] * v).sum(axis=0), *(m[:, None] * np.cross(p, v)).sum(axis=0),
                         *((m[:, None] * p).sum(axis=0) / mass)])


def kinds(values):
    return ["NaN" if np.isnan(x) else "+inf" if x == np.inf else "-inf" if x == -np.inf else "finite" for x in values]


def check_poisoned(got, clean, pos, vel, eps2, what):
    """got, clean: the records of the six systems with and without the poison"""
    for s, poison in enumerate(POISONS):
        want = kinds(definition(pos[s], vel[s], eps2))
        assert kinds(got[s]) == want, f"{what}, {poison}: {dict(zip(range(13), kinds(got[s])))} for {want}"
        if poison == "clean":
            assert got[s].tobytes() == clean[s].tobytes() and np.isfinite(got[s]).all(), f"{what}: a clean system's bytes changed beside poisoned ones"
        elif poison == "a NaN velocity":  # the potential, the mass and the centre of mass never read a velocity
            for f in (1, 3, 10, 11, 12):
                assert np.isfinite(got[s][f]) and bits(got[s][f]) == bits(clean[s][f]), (what, poison, f)
        elif poison == "a zero-mass body on another":
            # today's behaviour, pinned: 0 * inf = NaN with eps^2 == 0; softened, the body contributes nothing
            assert want[1] == ("NaN" if eps2 == 0 else "finite"), (what, want)
            if eps2 != 0:
                assert np.isfinite(got[s]).all(), (what, poison)


@gpu_only
@pytest.mark.parametrize("dtype,n", [(F32, 300), (F32, 1100), (F64, 300), (F64, 600)])
def test_nonfinite_inputs_stay_in_their_system_and_their_fields(gpu, dtype, n):
    pos, vel, clean_pos, clean_vel = poisoned_batch(n, dtype, 900 + n)
    name = np.dtype(dtype).name
    for eps2 in (0.0, 0.01):
        clean = [record(e) for e in measure(gpu, clean_pos, clean_vel, dtype, eps2)]
        got = [record(e) for e in measure(gpu, pos, vel, dtype, eps2)]
        check_poisoned(got, clean, pos, vel, eps2, f"nb_energy_ensemble {name} n = {n} eps^2 = {eps2}")
        solo_clean = [record(gpu_energy(gpu, clean_pos[s], clean_vel[s], dtype, eps2)) for s in range(len(POISONS))]
        solo = [record(gpu_energy(gpu, pos[s], vel[s], dtype, eps2)) for s in range(len(POISONS))]
        check_poisoned(solo, solo_clean, pos, vel, eps2, f"nb_energy {name} n = {n} eps^2 = {eps2}")
