"""Nearest neighbours, potentials and neighbour lists (nb_neighbour_*, include/nbody_hip_neighbour.h; libnbody_hip_neighbour.so from
csrc/neighbour*.hip).

The scheme, restated in numpy below (numpy_survey): with d2(i, j) = dx dx + dy dy + dz dz of the differences x_j - x_i in T,

    nearest_index[i]   = the lowest j != i of smallest d2 (NONE when no d2 compares less than +inf),   nearest_dist_sq[i] = that d2
    counts[i]          = #{j != i : d2(i, j) < r2_i},          lists: those j ascending, offsets = the exclusive prefix of the counts
    potentials[i]      = -sum_{j != i} m_j / sqrt(d2 + eps2)
    status             = the total of the counts; the closest pair (the lowest i of smallest nearest_dist_sq and its nearest); the largest
                         count and the lowest body that has it; OVERFLOW when the total exceeds the capacity of a lists call

CPU tests: the boundary (declared, exported, mirrored; the other five libraries unchanged), the plan and the workspace as functions of
(N, precision), host-side argument checks, the instruction mix of the fp32 streaming loops.  GPU tests: exact cases (integer lattices:
every d2 is exact in T, so the numpy result holds bit for bit whatever the kernel fuses) E1 - E4; random clouds against long double
numpy from the same T-typed inputs with gamma = 6u on distances (a difference carries one rounding, 2u on its square; the squares and the
two additions add at most one each: 5u to first order, 6u covers the second), nearest indices within (1 + 2 gamma) of the minimum and at
most 1e-4 N of them off the long double argmin, pairs within gamma r2 of the radius free and at most 1e-4 of the entries, potentials per
body within TOL of tests/test_fast_domain.py; (1/2) sum m phi against nb_energy_*; invariants (bits, streams, NaN workspace, canaries,
inputs, capture, null outputs); a block-step run end to end; the Python class; a speed sanity bound."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_capi_symbols import declared_symbols, exported_symbols
from test_fast_domain import TOL, UNIT_ROUNDOFF
from test_hermite import CSRC, LD, hip_runtime

ERR = 10001
MAX_N = 1 << 24
NONE = 0xFFFFFFFF
OVERFLOW = 1
SYMBOLS = ["nb_neighbour_lists_f32", "nb_neighbour_lists_f64", "nb_neighbour_plan_f32", "nb_neighbour_plan_f64", "nb_neighbour_survey_f32", "nb_neighbour_survey_f64",
           "nb_neighbour_workspace_bytes"]
GAMMA = {kind: 6 * u for kind, u in UNIT_ROUNDOFF.items()}
# what the compiler delivers for the fp32 streaming loops of the survey, per packed pair of bodies i and body j: packed
# operations without / with potentials, v_rsq_f32 with potentials, other vector operations (unmasked loop; the masked loop runs once per wave)
PK_PLAIN, PK_POT, RSQ, OTHER, OTHER_MASKED = 6, 8, 2, 7, 12
# issue cycles (docs/history.md: packed fp32 op 4.08, v_rsq_f32 8.3; the one-sided step: 11 packed + 2 v_rsq_f32).  That one of the other
# vector operations costs what a packed one does is an ASSUMPTION, not a measurement.
PK_CYCLES, RSQ_CYCLES = 4.08, 8.3
ONE_SIDED = 11 * PK_CYCLES + 2 * RSQ_CYCLES
MODEL_PLAIN = (PK_PLAIN + OTHER) * PK_CYCLES / ONE_SIDED
MODEL_POT = ((PK_POT + OTHER) * PK_CYCLES + RSQ * RSQ_CYCLES) / ONE_SIDED


def suffix(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def scalar_of(dtype):
    return np.float32 if np.dtype(dtype) == np.float32 else float


# ---------------------------------------------------------------------------------------------------------------- the scheme in numpy


def numpy_survey(pos, r2, block=512):
    """The scheme in T arithmetic (no FMA: exact wherever the test needs bits).  pos (N, 4) of T; r2 a scalar or (N,) of T.
    -> nearest (uint32), nearest_d2 (T), counts (uint32), offsets (uint64, N + 1), indices (uint32), status dict (capacity = enough)"""
    n, kind = pos.shape[0], pos.dtype.type
    r2 = np.broadcast_to(np.asarray(r2, dtype=pos.dtype), (n,))
    nearest, nearest_d2, counts, lists = np.full(n, NONE, np.uint32), np.full(n, np.inf, pos.dtype), np.zeros(n, np.uint32), []
    with np.errstate(invalid="ignore"):
        for s in range(0, n, block):
            i = np.arange(s, min(n, s + block))
            d = pos[None, :, :3] - pos[i, None, :3]
            d2 = d[:, :, 0] * d[:, :, 0] + (d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2])
            assert d2.dtype == pos.dtype
            own = i[:, None] == np.arange(n)[None, :]
            candidate = np.where(own | np.isnan(d2), kind(np.inf), d2)
            k = candidate.argmin(axis=1)  # (the first of equal values: the lowest j)
            least = candidate[np.arange(len(i)), k]
            found = least < np.inf
            nearest[i], nearest_d2[i] = np.where(found, k, NONE), least
            inside = (d2 < r2[i, None]) & ~own
            counts[i] = inside.sum(axis=1)
            lists.extend(np.nonzero(row)[0].astype(np.uint32) for row in inside)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(counts, dtype=np.uint64)
    indices = np.concatenate(lists) if lists else np.zeros(0, np.uint32)
    return nearest, nearest_d2, counts, offsets, indices, numpy_status(nearest, nearest_d2, counts)


def numpy_status(nearest, nearest_d2, counts, lists_call=False, capacity=None):
    status = dict(total_neighbours=int(counts.sum(dtype=np.uint64)), closest_dist_sq=float("inf"), closest_i=NONE, closest_j=NONE,
                  max_count=int(counts.max()), max_count_body=int(counts.argmax()), flags=0)
    if not lists_call and (nearest != NONE).any():
        i = int(nearest_d2.argmin())  # (the lowest i of equal values)
        status.update(closest_dist_sq=float(nearest_d2[i]), closest_i=i, closest_j=int(nearest[i]))
    if capacity is not None and status["total_neighbours"] > capacity:
        status["flags"] = OVERFLOW
    return status


def test_the_numpy_scheme_on_a_hand_made_state():
    """five bodies on a line, two of them at one place: the tie rule, j != i by index, the strict radius, the status record"""
    pos = np.zeros((5, 4), np.float32)
    pos[:, 0] = [0, 1, 1, 3, 5]
    pos[:, 3] = 1
    nearest, d2, counts, offsets, indices, status = numpy_survey(pos, np.float32(4))
    assert nearest.tolist() == [1, 2, 1, 1, 3] and d2.tolist() == [1, 0, 0, 4, 4]
    assert counts.tolist() == [2, 2, 2, 0, 0], "d2 = 4 is not < 4"
    assert offsets.tolist() == [0, 2, 4, 6, 6, 6] and indices.tolist() == [1, 2, 0, 2, 0, 1]
    assert status == dict(total_neighbours=6, closest_dist_sq=0.0, closest_i=1, closest_j=2, max_count=2, max_count_body=0, flags=0)
    nearest, d2, counts, _, _, status = numpy_survey(pos[:1], np.float32(4))
    assert nearest.tolist() == [NONE] and d2.tolist() == [np.inf] and counts.tolist() == [0]
    assert status == dict(total_neighbours=0, closest_dist_sq=float("inf"), closest_i=NONE, closest_j=NONE, max_count=0, max_count_body=0, flags=0)


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_neighbour_header_library_and_binding_agree(pkg):
    declared = declared_symbols("nbody_hip_neighbour.h")
    assert declared == SYMBOLS
    assert exported_symbols(pkg.NEIGHBOUR_LIB_PATH) == declared
    assert sorted(pkg.NEIGHBOUR_SIGNATURES) == declared
    # the other five libraries export what they did, none of it ours
    others = {pkg.LIB_PATH: 96, pkg.ENSEMBLE_LIB_PATH: 4, pkg.HERMITE_LIB_PATH: 9, pkg.HERMITE_BLOCK_LIB_PATH: 9}
    for path, count in others.items():
        assert len(exported_symbols(path)) == count, path
        assert not set(declared) & set(exported_symbols(path)), path
    assert not set(declared) & set(exported_symbols(pkg.LAB_LIB_PATH))
    assert set(exported_symbols(pkg.LIB_PATH)) <= set(exported_symbols(pkg.LAB_LIB_PATH))
    needed = subprocess.run(["readelf", "-d", pkg.NEIGHBOUR_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnbody_hip" not in needed


def struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(unsigned long long|uint64_t|uint32_t|double|int|unsigned)\s+(\w+)(?:\[(\d+)\])?;", body)


def test_neighbour_mirrors_and_constants_match_the_header(pkg):
    text = open(os.path.join(ROOT, "include", "nbody_hip_neighbour.h")).read()
    ctype = {"unsigned long long": ctypes.c_ulonglong, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double, "int": ctypes.c_int,
             "unsigned": ctypes.c_uint}
    for name, mirror, size in (("nb_neighbour_status", pkg.NeighbourStatus, 64), ("nb_neighbour_plan", pkg.NeighbourPlan, 64)):
        fields = struct_fields(text, name)
        assert [f for _, f, _ in fields] == [f for f, _ in mirror._fields_], name
        for (kind, field, count), (_, mirrored) in zip(fields, mirror._fields_):
            assert mirrored == (ctype[kind] * int(count) if count else ctype[kind]), (name, field)
        assert ctypes.sizeof(mirror) == size
    assert re.search(r"#define NB_NEIGHBOUR_MAX_BODIES \(1u << 24\)", text) and pkg.NEIGHBOUR_MAX_BODIES == MAX_N
    assert re.search(r"#define NB_NEIGHBOUR_NONE 0xFFFFFFFFu", text) and pkg.NEIGHBOUR_NONE == NONE
    assert re.search(r"#define NB_NEIGHBOUR_OVERFLOW 1u", text) and pkg.NEIGHBOUR_OVERFLOW == OVERFLOW
    assert "FMA((dx), (dx), FMA((dy), (dy), (dz) * (dz)))" in text, "the one expression of d2"
    source = open(os.path.join(CSRC, "neighbour.hip")).read()
    assert source.count("NB_NEIGHBOUR_DIST_SQ(") == 2 and "dx * dx" not in source, "every kernel computes d2 by the header's expression (packed and scalar form)"


def expected_plan(n, dtype):
    W = 2 if np.dtype(dtype) == np.float32 else 1
    size = np.dtype(dtype).itemsize
    S = 1
    while S < 8 and 2 * S * 128 <= n:
        S *= 2
    tiles, chunks = -(-n // (64 * W)), -(-n // 128)
    need, J = -(-2048 // tiles), 1
    while J < need and 2 * J <= chunks:
        J *= 2
    return dict(bodies_per_lane=W, waves_per_group=S, unroll=4 if W == 2 else 2, tiles=tiles, block_threads=64 * S, lds_bytes=(S - 1) * 2 * 64 * W * (size + 4),
                chunks=chunks, list_ranges=J, list_groups=tiles * J, survey_launches=2, list_launches=5, reserved=0, planes_offset=0, planes_bytes=J * n * 4)


def expected_workspace(n, dtype):
    up = lambda b: (b + 255) & ~255  # noqa: E731
    p = expected_plan(n, dtype)
    return up(p["planes_bytes"]) + up(-(-n // 256) * 8) + up(p["tiles"] * 32) + up(64)


def test_neighbour_plan_and_workspace_are_functions_of_n_and_precision(pkg):
    sizes = sorted({1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 1000, 1023, 1024, 1025, 2085, 4096, 5000, 16384, 16385, 65536, 70000, 262144, MAX_N})
    lib = pkg.neighbour_lib()
    for dtype in (np.float32, np.float64):
        for n in sizes:
            plans = set()
            for _ in range(3):
                p = pkg.neighbour_plan(n, dtype)
                plans.add(tuple(getattr(p, name) for name, _ in pkg.NeighbourPlan._fields_))
            assert len(plans) == 1
            got = dict(zip((name for name, _ in pkg.NeighbourPlan._fields_), plans.pop()))
            assert got == expected_plan(n, dtype), (n, dtype)
            assert got["lds_bytes"] <= 64 * 1024 and got["list_ranges"] <= got["chunks"], "every range of the lists has a chunk"
            assert got["list_groups"] >= min(2048, got["tiles"] * got["chunks"]) // 2 or got["list_ranges"] == 1
            assert pkg.neighbour_workspace_bytes(n, dtype) == expected_workspace(n, dtype), (n, dtype)
        p = pkg.NeighbourPlan()
        fn = getattr(lib, "nb_neighbour_plan_" + suffix(dtype))
        for n in (0, MAX_N + 1):
            assert fn(n, ctypes.byref(p)) == ERR, n
        assert fn(16, None) == ERR
    out = ctypes.c_size_t(0)
    for bad in ((0, 4), (MAX_N + 1, 4), (1000, 2), (1000, 16)):
        assert lib.nb_neighbour_workspace_bytes(*bad, ctypes.byref(out)) == ERR, bad
    assert lib.nb_neighbour_workspace_bytes(1000, 4, None) == ERR


def test_neighbour_argument_errors_are_caught_on_the_host(pkg):
    """Everything refused here is refused before a HIP call: the made-up addresses are never dereferenced."""
    lib = pkg.neighbour_lib()
    for dtype in (np.float32, np.float64):
        scalar, size, n = scalar_of(dtype), np.dtype(dtype).itemsize, 1024
        ws_bytes = pkg.neighbour_workspace_bytes(n, dtype)
        ok = dict(pos=0x100000000, radii=0x200000000, nearest=0x300000000, d2=0x400000000, counts=0x500000000, pot=0x600000000, status=0x700000000, ws=0x800000000,
                  offsets=0x900000000, indices=0xA00000000, ws_bytes=ws_bytes, n=n, radius=0.5, eps2=0.01, capacity=4096)
        length = dict(pos=4 * n * size, radii=n * size, nearest=4 * n, d2=n * size, counts=4 * n, pot=n * size, status=64, ws=ws_bytes, offsets=8 * (n + 1), indices=4 * 4096)
        align = dict(pos=4 * size, radii=size, nearest=4, d2=size, counts=4, pot=size, status=8, ws=32, offsets=8, indices=4)

        def survey(**kw):
            a = {**ok, **kw}
            return getattr(lib, "nb_neighbour_survey_" + suffix(dtype))(a["pos"], a["n"], scalar(a["radius"]), a["radii"], scalar(a["eps2"]), a["nearest"], a["d2"], a["counts"],
                                                                        a["pot"], a["status"], a["ws"], a["ws_bytes"], None)

        def lists(**kw):
            a = {**ok, **kw}
            return getattr(lib, "nb_neighbour_lists_" + suffix(dtype))(a["pos"], a["n"], scalar(a["radius"]), a["radii"], a["offsets"], a["indices"], a["capacity"], a["status"],
                                                                       a["ws"], a["ws_bytes"], None)

        for call, names, required in ((survey, ("pos", "radii", "nearest", "d2", "counts", "pot", "status", "ws"), ("pos", "status", "ws")),
                                      (lists, ("pos", "radii", "offsets", "indices", "status", "ws"), ("pos", "offsets", "indices", "status", "ws"))):
            for null in required:
                assert call(**{null: None}) == ERR, null
            for bad in (dict(n=0), dict(n=MAX_N + 1), dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0), dict(radii=None, radius=-1.0), dict(radii=None, radius=float("nan")),
                        dict(radii=None, radius=-0.5)):
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
        assert survey(eps2=-0.01) == ERR and survey(eps2=float("nan")) == ERR
        assert survey(nearest=None, d2=None, counts=None, pot=None) == ERR, "no output at all"
        assert lists(capacity=1 << 62) == ERR
        count = ctypes.c_int(0)
        if pkg.lib().nb_device_count(ctypes.byref(count)) != 0 or count.value == 0:  # (with a GPU the made-up addresses would be used)
            assert lists(indices=None, capacity=0) not in (0, ERR), "a call that only sizes the lists passes the argument check: a HIP error"


def kernels_of(text):
    lines = text.split("\n")
    for i, line in enumerate(lines):
        m = re.match(r"^(_ZN2nb12_GLOBAL__N_1\d+(?:neighbour|list)_\w+):", line)
        if m:
            end = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            yield m.group(1), lines[i:end]


def test_neighbour_streaming_loops_keep_their_mix():
    """Every streaming loop of the fp32 neighbour_survey kernels (8 packed pairs per trip: two groups of 4 bodies j against a packed
    pair of bodies i): 6 v_pk_* per packed pair without potentials, 8 v_pk_* + 2 v_rsq_f32 with; at most 7 other vector operations in
    the unmasked loop (minimum, group select, count) and 12 in the masked one; bodies j by s_load; no LDS, scratch or barrier
    instruction; no kernel of the file uses scratch or more than 128 VGPRs."""
    subprocess.run(["make", "-s", "-C", CSRC, "neighbour.s"], check=True, capture_output=True)
    text = open(os.path.join(CSRC, "neighbour.s")).read()
    seen = 0
    for name, lines in kernels_of(text):
        if "neighbour_surveyIf" not in name:
            continue
        seen += 1
        with_pot = "ELb1E" in name
        others = []
        for i, line in enumerate(lines):
            if "Inner Loop Header" not in line:
                continue
            label = lines[i - 1].split(":")[0].strip()
            stop = next((k for k in range(i, len(lines)) if ("s_cbranch" in lines[k] or "s_branch" in lines[k]) and label in lines[k]), None)
            if stop is None:
                continue
            body = [l.strip() for l in lines[i + 1:stop]]
            count = lambda prefix: sum(1 for l in body if l.startswith(prefix))  # noqa: E731
            if count("v_pk_fma_f32") < 8:
                continue  # (the one-body loop of the ragged end, the fold, the index search)
            pairs = 8
            assert count("v_pk_") == (PK_POT if with_pot else PK_PLAIN) * pairs, (name, label, count("v_pk_") / pairs)
            assert count("v_rsq_f32") == (RSQ * pairs if with_pot else 0), (name, label)
            assert count("ds_") == 0 and count("scratch_") == 0 and count("s_barrier") == 0, (name, label)
            assert count("s_load") >= 2 and count("global_load") == 0 and count("buffer_load") == 0 and count("global_store") == 0, (name, label)
            assert count("v_mov") <= 2, (name, label, "one per group: the group's first index for the select")
            others.append(count("v_") - count("v_pk_") - count("v_rsq_f32"))
        assert len(others) == 2, (name, others)
        assert min(others) <= OTHER * 8 and max(others) <= OTHER_MASKED * 8, (name, others)
    assert seen == 8  # S = 1, 2, 4, 8 x (without, with potentials): the compiled forms do not multiply per requested output
    assert len(re.findall(r"^_ZN2nb12_GLOBAL__N_1\d+neighbour_survey\w+:", text, re.M)) == 16
    sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    vgprs = [int(m) for m in re.findall(r"\.vgpr_count:\s+(\d+)", text)]
    assert len(sizes) == 24 and max(sizes) == 0, sizes
    assert len(vgprs) == 24 and max(vgprs) <= 128, vgprs


def test_neighbour_sources_keep_the_scalar_unit_to_loads():
    for name in ("neighbour.hip", "neighbour_capi.hip", "neighbour_kernels.h"):
        src = open(os.path.join(CSRC, name)).read().lower()
        for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_dcache_" + "wb", "s_dcache_" + "discard", "atomicadd"):
            assert word not in src, (name, word)
    text = open(os.path.join(CSRC, "neighbour.s")).read() if os.path.exists(os.path.join(CSRC, "neighbour.s")) else ""
    assert "s_" + "store" not in text and "_atomic" not in text


# ---------------------------------------------------------------------------------------------------------------- GPU
gpu_only = pytest.mark.gpu
OUTPUTS = ("nearest", "d2", "counts", "pot", "offsets", "indices", "status")


class NeighbourDevice:
    """the arrays of one state on the device, through the C calls; PAD canary bytes round every array; outputs start as 0xC3 bytes"""
    PAD = 256

    def __init__(self, gpu, pos, radii=None, capacity=0, ws_fill=None):
        self.gpu, self.dtype, self.n, self.capacity = gpu, pos.dtype, pos.shape[0], int(capacity)
        self.scalar, self.lib = scalar_of(self.dtype), gpu.neighbour_lib()
        n, size = self.n, self.dtype.itemsize
        self.ws_bytes = gpu.neighbour_workspace_bytes(n, self.dtype)
        self.kinds = dict(pos=(self.dtype, 4 * n), radii=(self.dtype, n), nearest=(np.dtype(np.uint32), n), d2=(self.dtype, n), counts=(np.dtype(np.uint32), n),
                          pot=(self.dtype, n), offsets=(np.dtype(np.uint64), n + 1), indices=(np.dtype(np.uint32), max(1, self.capacity)), status=(np.dtype(np.uint8), 64),
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
        self.has_radii = radii is not None
        if self.has_radii:
            self.put("radii", radii)

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
        return out

    def status(self):
        s = self.gpu.NeighbourStatus.from_buffer_copy(self.get("status").tobytes())
        assert not any(s.reserved)
        return self.gpu.neighbour_status_dict(s)

    def canaries_intact(self):
        for name, buf in self.bufs.items():
            host = buf.download(np.empty(buf.nbytes, np.uint8))
            if not ((host[:self.PAD] == 0xA5).all() and (host[-self.PAD:] == 0xA5).all()):
                return False
        return True

    def untouched(self, name):
        return bool((self.get(name).view(np.uint8) == 0xC3).all())

    def survey(self, radius_sq=0.0, eps2=0.0, outputs=("nearest", "d2", "counts"), stream=None):
        fn = getattr(self.lib, "nb_neighbour_survey_" + suffix(self.dtype))
        out = [self.ptr(name) if name in outputs else None for name in ("nearest", "d2", "counts", "pot")]
        self.gpu.check(fn(self.ptr("pos"), self.n, self.scalar(radius_sq), self.ptr("radii") if self.has_radii else None, self.scalar(eps2), *out, self.ptr("status"),
                          self.ptr("ws"), self.ws_bytes, stream), "nb_neighbour_survey")

    def lists(self, radius_sq=0.0, capacity=None, stream=None):
        fn = getattr(self.lib, "nb_neighbour_lists_" + suffix(self.dtype))
        capacity = self.capacity if capacity is None else capacity
        assert capacity <= self.capacity
        self.gpu.check(fn(self.ptr("pos"), self.n, self.scalar(radius_sq), self.ptr("radii") if self.has_radii else None, self.ptr("offsets"), self.ptr("indices"), capacity,
                          self.ptr("status"), self.ptr("ws"), self.ws_bytes, stream), "nb_neighbour_lists")

    def everything(self):
        return b"".join(self.get(name).tobytes() for name in OUTPUTS)

    def free(self):
        for buf in self.bufs.values():
            buf.free()


def lattice(n, dtype, seed, reach):
    """integer coordinates of magnitude <= reach <= 64 (every d2 <= 3 * 128^2 is exact in T), masses 2^-3 .. 2^3"""
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 4), dtype)
    pos[:, :3] = rng.integers(-reach, reach + 1, (n, 3))
    pos[:, 3] = 2.0 ** rng.integers(-3, 4, n)
    return pos


def check_exact(gpu, pos, radius_sq=None, radii=None, outputs=("nearest", "d2", "counts")):
    """E1: a survey and a lists call of one state against numpy_survey, every output and every field of both status records"""
    n = pos.shape[0]
    nearest, d2, counts, offsets, indices, status = numpy_survey(pos, radius_sq if radii is None else radii)
    d = NeighbourDevice(gpu, pos, radii, capacity=len(indices))
    d.survey(0.0 if radius_sq is None else radius_sq, 0.25, outputs)
    what = (n, pos.dtype, radius_sq, radii is not None)
    if "nearest" in outputs:
        assert np.array_equal(d.get("nearest"), nearest), what
    if "d2" in outputs:
        assert d.get("d2").tobytes() == d2.tobytes(), what
    if "counts" in outputs:
        assert np.array_equal(d.get("counts"), counts), what
    assert d.status() == status, (what, d.status(), status)
    d.lists(0.0 if radius_sq is None else radius_sq)
    assert np.array_equal(d.get("offsets"), offsets), what
    assert np.array_equal(d.get("indices")[:len(indices)], indices), what
    assert d.status() == numpy_status(nearest, d2, counts, lists_call=True), (what, d.status())
    assert d.canaries_intact(), what
    assert d.get("pos").tobytes() == pos.tobytes(), "inputs bit-untouched"
    d.free()
    return status


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_lattices(gpu, dtype):
    """E1.  Integer lattices: duplicated points (reach 2: 125 places), exact ties everywhere; N across the chunk and tile edges; a scalar
    radius (0; one that ties exactly with many d2, so the strict comparison shows; larger than the system) and per-body radii"""
    kind = np.dtype(dtype).type
    for n in (1, 2, 3, 127, 128, 129, 300, 5000):
        for reach in ((2, 64) if n <= 300 else (20,)):
            pos = lattice(n, dtype, 100 * n + reach, reach)
            for radius_sq in (0.0, 9.0 if reach < 64 else 2500.0, 1e9):
                status = check_exact(gpu, pos, radius_sq=kind(radius_sq), outputs=("nearest", "d2", "counts", "pot") if radius_sq == 9.0 else ("nearest", "d2", "counts"))
                if radius_sq == 0.0:
                    assert status["total_neighbours"] == 0, "nothing is closer than 0, a duplicate included"
                if radius_sq == 1e9:
                    assert status["total_neighbours"] == n * (n - 1) and status["max_count_body"] == 0
            if n >= 127 and reach == 2:
                assert status["closest_dist_sq"] == 0.0, "a duplicate IS a neighbour at 0"
            rng = np.random.default_rng(n)
            radii = rng.choice(np.array([0, 1, 4, 9, 100, 1e9], dtype), n)
            check_exact(gpu, pos, radii=radii)
    same = np.zeros((130, 4), dtype)  # every body at one place: every d2 is 0, every nearest is the lowest other index
    same[:, 3] = 1
    nearest = numpy_survey(same, kind(1))[0]
    assert nearest[0] == 1 and (nearest[1:] == 0).all()
    check_exact(gpu, same, radius_sq=kind(1))


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_overflow_leaves_offsets_complete_and_indices_untouched(gpu, dtype):
    """E2"""
    kind = np.dtype(dtype).type
    for n, reach, radius_sq in ((300, 6, 20.0), (5000, 20, 60.0)):
        pos = lattice(n, dtype, 7 * n, reach)
        nearest, d2, counts, offsets, indices, _ = numpy_survey(pos, kind(radius_sq))
        total = len(indices)
        assert total > n
        d = NeighbourDevice(gpu, pos, capacity=total)
        d.lists(kind(radius_sq), capacity=total - 1)
        assert np.array_equal(d.get("offsets"), offsets), "offsets complete and right"
        assert d.untouched("indices"), "indices bit-untouched"
        assert d.status() == numpy_status(nearest, d2, counts, lists_call=True, capacity=total - 1) and d.status()["flags"] == OVERFLOW
        assert d.status()["total_neighbours"] == total, "the needed total"
        d.lists(kind(radius_sq), capacity=0)
        assert d.untouched("indices") and d.status()["flags"] == OVERFLOW and d.status()["total_neighbours"] == total
        d.lists(kind(radius_sq), capacity=total)
        assert d.status()["flags"] == 0 and np.array_equal(d.get("indices"), indices)
        assert d.canaries_intact()
        d.free()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_nan_body_is_nobodys_neighbour(gpu, dtype):
    """E3"""
    kind = np.dtype(dtype).type
    for n, bad in ((2, 1), (300, 130), (5000, 4999)):
        pos = lattice(n, dtype, 3 * n, 10)
        pos[bad, 1] = np.nan
        nearest, d2, counts, offsets, indices, status = numpy_survey(pos, kind(30))
        assert nearest[bad] == NONE and d2[bad] == np.inf and counts[bad] == 0 and bad not in nearest and bad not in indices
        d = NeighbourDevice(gpu, pos, capacity=len(indices))
        d.survey(kind(30))
        assert np.array_equal(d.get("nearest"), nearest) and d.get("d2").tobytes() == d2.tobytes() and np.array_equal(d.get("counts"), counts)
        assert d.status() == status
        d.lists(kind(30))
        assert np.array_equal(d.get("offsets"), offsets) and np.array_equal(d.get("indices")[:len(indices)], indices)
        d.free()


def normal_cloud(n, dtype, mass="equal"):
    """the positions of the issue: default_rng(7).standard_normal((N, 3)) cast to T; masses as tests/test_hermite.py's cloud()"""
    rng = np.random.default_rng(7)
    pos = np.zeros((n, 4), dtype)
    pos[:, :3] = rng.standard_normal((n, 3))
    if mass == "equal":
        pos[:, 3] = 1.0 / n
    elif mass == "species":
        pos[:, 3] = np.where(np.arange(n) < (2 * n) // 3, 0.5, 3.0)
    else:
        pos[:, 3] = 2.0 ** np.random.default_rng(8).uniform(-10, 10, n)
    return pos


def cloud_radius_sq(n, dtype):
    return np.dtype(dtype).type((0.35 * (5000 / n) ** (1 / 3)) ** 2)


@gpu_only
@pytest.mark.parametrize("n", [70000, 262144])
def test_exact_invariants_on_large_clouds(gpu, n):
    """E4: invariants of the device's own outputs, fp32, a shared radius; no O(N^2) host work"""
    dtype = np.float32
    pos, r2 = normal_cloud(n, dtype), cloud_radius_sq(n, dtype)
    d = NeighbourDevice(gpu, pos, capacity=40 * n)
    d.survey(r2)
    nearest, d2, counts, status = d.get("nearest").astype(np.int64), d.get("d2"), d.get("counts"), d.status()
    d.lists(r2)
    offsets, lists_status = d.get("offsets"), d.status()
    total = int(offsets[-1])
    indices = d.get("indices")[:total].astype(np.int64)
    assert d.canaries_intact()
    d.free()
    assert lists_status["flags"] == 0 and lists_status["total_neighbours"] == total == status["total_neighbours"]
    assert (nearest != NONE).all() and (d2[nearest] <= d2).all(), "my nearest neighbour has a neighbour at least as close: me"
    assert np.array_equal(counts, np.diff(offsets).astype(np.uint32)), "counts == diff(offsets)"
    owner = np.repeat(np.arange(n, dtype=np.int64), counts)
    forward, backward = owner * n + indices, indices * n + owner
    assert (np.diff(forward) > 0).all(), "each list is ascending (and the lists follow each other)"
    assert np.array_equal(forward, np.sort(backward)), "the relation is symmetric: d2(i, j) and d2(j, i) are the same bits"
    listed = d2 < r2
    assert np.array_equal(listed, counts > 0)
    assert np.isin(np.arange(n, dtype=np.int64)[listed] * n + nearest[listed], forward).all(), "the nearest is in the list whenever it is within the radius"
    i = int(d2.argmin())
    assert (status["closest_dist_sq"], status["closest_i"], status["closest_j"]) == (float(d2[i]), i, int(nearest[i])) and i < nearest[i]
    assert (status["max_count"], status["max_count_body"]) == (int(counts.max()), int(counts.argmax())) == (lists_status["max_count"], lists_status["max_count_body"])
    print(f"N = {n}: {total / n:.1f} entries per list, the longest {counts.max()}; closest pair ({i}, {nearest[i]}) at {float(d2[i]) ** 0.5:.3g}")


def long_double_reference(pos, r2, gamma, eps2s, masses, rows=None):
    """From the T-typed pos, in long double, for the bodies `rows` (default: all): the smallest d2 over j != i and its (lowest) j; the pairs
    (as i * N + j, ascending) with d2 < r2 and those within gamma r2 of r2; per (eps2, mass vector) the sums of m_j / sqrt(d2 + eps2)"""
    n = pos.shape[0]
    p = pos[:, :3].astype(LD)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    least, arg, inside, undecided = np.zeros(len(rows), LD), np.zeros(len(rows), np.int64), [], []
    sums = {(e, k): np.zeros(len(rows), LD) for e in eps2s for k in range(len(masses))}
    r2, band = LD(r2), LD(gamma) * LD(r2)
    block = max(1, min(512, (1 << 21) // n))
    columns = np.arange(n)
    for s in range(0, len(rows), block):
        i = rows[s:s + block]
        d = p[None, :, :] - p[i, None, :]
        d2 = (d * d).sum(axis=2)
        own = i[:, None] == columns[None, :]
        others = np.where(own, LD(np.inf), d2)
        k = others.argmin(axis=1)
        arg[s:s + len(i)], least[s:s + len(i)] = k, others[np.arange(len(i)), k]
        code = i[:, None].astype(np.int64) * n + columns[None, :]
        inside.append(code[(d2 < r2) & ~own])
        undecided.append(code[(np.abs(d2 - r2) <= band) & ~own])
        for e in eps2s:
            with np.errstate(divide="ignore"):
                inv = np.where(own, LD(0), 1 / np.sqrt(d2 + LD(e)))
            for which, m in enumerate(masses):
                sums[(e, which)][s:s + len(i)] = (inv * m.astype(LD)[None, :]).sum(axis=1)
    return least, arg, np.concatenate(inside), np.concatenate(undecided), sums


def exact_d2(pos, i, j):
    d = pos[j, :3].astype(LD) - pos[i, :3].astype(LD)
    return (d * d).sum(axis=1)


def check_cloud(gpu, dtype, n, mass_kinds, eps2s, rows=None):
    """a random cloud against long double: distances, nearest indices, counts and lists, potentials (for the bodies `rows`)"""
    kind, gamma, tol = np.dtype(dtype).type, GAMMA[dtype], TOL[dtype]
    clouds = [normal_cloud(n, dtype, mass) for mass in mass_kinds]
    pos, r2 = clouds[0], cloud_radius_sq(n, dtype)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    least, arg, inside, undecided, sums = long_double_reference(pos, r2, gamma, eps2s, [c[:, 3] for c in clouds], rows)
    d = NeighbourDevice(gpu, pos, capacity=60 * n)
    d.survey(r2)
    nearest, d2, counts = d.get("nearest").astype(np.int64), d.get("d2"), d.get("counts")
    d.lists(r2)
    offsets = d.get("offsets")
    indices = d.get("indices")[:int(offsets[-1])].astype(np.int64)
    assert d.status()["flags"] == 0 and np.array_equal(counts, np.diff(offsets).astype(np.uint32))
    # distances: the stored d2 against the long double d2 of the pair the kernel named
    assert (nearest[rows] != NONE).all()
    exact = exact_d2(pos, rows, nearest[rows])
    err = np.abs(d2[rows].astype(LD) - exact) / exact
    assert (err <= gamma).all(), (n, dtype, float(err.max() / UNIT_ROUNDOFF[dtype]))
    # nearest index: within (1 + 2 gamma) of the minimum for every body; off the long double argmin for at most 1e-4 N
    assert (exact <= (1 + 2 * LD(gamma)) * least).all(), (n, dtype)
    off = int((nearest[rows] != arg).sum())
    assert off <= 1e-4 * len(rows), (n, dtype, off)
    # counts and lists: a pair within gamma r2 of the radius may be in or out, every other pair is exactly right
    owner = np.repeat(np.arange(n, dtype=np.int64), counts)
    listed = owner * n + indices
    listed = listed[np.isin(owner, rows)] if len(rows) < n else listed
    assert (np.diff(listed) > 0).all()
    wrong = np.setxor1d(listed, inside, assume_unique=True)
    assert np.isin(wrong, undecided).all(), (n, dtype, len(wrong))
    assert len(undecided) <= 1e-4 * max(1, len(listed)), (n, dtype, len(undecided), len(listed))
    print(f"N = {n} {suffix(dtype)}: d2 within {float(err.max() / UNIT_ROUNDOFF[dtype]):.2f} u; {off} nearest indices off the long double argmin; "
          f"{len(undecided)} undecided pairs ({len(wrong)} decided the other way) of {len(listed)} entries, the longest list {counts[rows].max()}")
    # potentials, per body, relative to |phi| (all terms have one sign)
    for which, cloud in enumerate(clouds):
        d.put("pos", cloud)
        for e in eps2s:
            d.survey(r2, kind(e), outputs=("pot",))
            want = -sums[(e, which)]
            got = d.get("pot")[rows].astype(LD)
            worst = float((np.abs(got - want) / np.abs(want)).max())
            assert np.isfinite(d.get("pot")[rows]).all() and worst <= tol, (n, dtype, mass_kinds[which], e, worst)
            print(f"    potentials, masses {mass_kinds[which]}, eps2 {e}: within {worst / tol:.3f} of the tolerance")
    assert d.canaries_intact()
    d.free()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [300, 5000])
def test_random_clouds_against_long_double(gpu, dtype, n):
    check_cloud(gpu, dtype, n, ("equal", "species", "random"), (0.01, 1e-6, 0.0))


@gpu_only
def test_a_random_cloud_of_20000_against_long_double(gpu):
    check_cloud(gpu, np.float32, 20000, ("equal", "random"), (0.01,))


@gpu_only
@pytest.mark.parametrize("n", [65536, 262144])
def test_sampled_bodies_of_large_clouds_against_long_double(gpu, n):
    rows = np.sort(np.random.default_rng(n).choice(n, 64, replace=False))
    check_cloud(gpu, np.float32, n, ("equal", "species", "random"), (0.01, 0.0), rows)


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_coincident_pair_at_no_softening(gpu, dtype):
    """-inf for the two bodies of the pair, finite (and right) for the rest; with softening everything is finite"""
    n = 1000
    pos = normal_cloud(n, dtype, "random")
    pos[700, :3] = pos[3, :3]
    d = NeighbourDevice(gpu, pos)
    d.survey(0.0, 0.0, outputs=("nearest", "pot"))
    pot, nearest = d.get("pot"), d.get("nearest")
    assert pot[3] == -np.inf and pot[700] == -np.inf and (nearest[3], nearest[700]) == (700, 3)
    rest = np.setdiff1d(np.arange(n), [3, 700])
    sums = long_double_reference(pos, 0.0, 0.0, (0.0,), [pos[:, 3]], rest)[4][(0.0, 0)]
    assert np.isfinite(pot[rest]).all() and (np.abs(pot[rest].astype(LD) + sums) <= TOL[dtype] * sums).all()
    d.survey(0.0, 1e-4, outputs=("pot",))
    assert np.isfinite(d.get("pot")).all()
    d.free()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_potentials_against_nb_energy(gpu, dtype):
    """(1/2) sum m_i phi_i, summed in fp64 on the host, against nb_energy_*'s potential of the same state at 65 536 bodies: 1e-5 relative in
    fp32 (the per-body 5e-6 plus the 5e-6 DESIGN.md 5.4 states for nb_energy_f32), 2e-12 in fp64"""
    n, kind = 65536, np.dtype(dtype).type
    pos, eps2 = normal_cloud(n, dtype, "species"), kind(0.01)
    d = NeighbourDevice(gpu, pos)
    d.survey(0.0, eps2, outputs=("pot",))
    mine = 0.5 * float((pos[:, 3].astype(np.float64) * d.get("pot").astype(np.float64)).sum())
    gpu.set_softening_squared(eps2 if dtype == np.float32 else float(eps2))
    zeros = gpu.DeviceBuffer(pos.nbytes)
    theirs = gpu.energy(d.ptr("pos"), zeros.ptr, n, dtype)["potential"]
    zeros.free(), d.free()
    print(f"{suffix(dtype)}: (1/2) sum m phi = {mine!r}, nb_energy potential = {theirs!r}: {abs(mine - theirs) / abs(theirs):.3g} relative")
    assert abs(mine - theirs) <= (1e-5 if dtype == np.float32 else 2e-12) * abs(theirs)


def run_both(gpu, pos, radii, r2, eps2, capacity, stream=None, ws_fill=None):
    d = NeighbourDevice(gpu, pos, radii, capacity=capacity, ws_fill=ws_fill)
    d.survey(r2, eps2, outputs=("nearest", "d2", "counts", "pot"), stream=stream)
    if stream is not None:
        gpu.check(gpu.lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
    survey_status = d.get("status").tobytes()
    d.lists(r2, stream=stream)
    if stream is not None:
        gpu.check(gpu.lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
    return d, survey_status


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_neighbour_bits_and_invariants(gpu, dtype):
    """the same bits from two calls, on another stream, with a NaN-filled workspace, from a captured graph replayed twice; canaries;
    inputs untouched; null outputs leave their arrays untouched and do not change the bits of the others"""
    n, kind = 2085, np.dtype(dtype).type
    pos = normal_cloud(n, dtype, "random")
    radii = (np.random.default_rng(5).uniform(0.05, 0.6, n) ** 2).astype(dtype)
    lib = gpu.lib()
    for with_radii in (False, True):
        r2, eps2, capacity = kind(0.09), kind(1e-3), 200 * n
        given = radii if with_radii else None
        base, base_survey_status = run_both(gpu, pos, given, r2, eps2, capacity)
        want = base.everything()
        total = base.status()["total_neighbours"]
        assert n < total <= capacity and base.canaries_intact()
        assert base.get("pos").tobytes() == pos.tobytes() and (not with_radii or base.get("radii").tobytes() == radii.tobytes()), "inputs bit-untouched"
        base.survey(r2, eps2, outputs=("nearest", "d2", "counts", "pot"))
        assert base.get("status").tobytes() == base_survey_status
        base.lists(r2)
        assert base.everything() == want, "again, on the workspace the first calls left"
        again, status = run_both(gpu, pos, given, r2, eps2, capacity, ws_fill=0xFF)
        assert again.everything() == want and status == base_survey_status, "NaN workspace (0xFF bytes: NaN in both precisions, ~0 as integers)"
        again.free()
        stream = ctypes.c_void_p()
        gpu.check(lib.nb_stream_create(ctypes.byref(stream)), "nb_stream_create")
        other, status = run_both(gpu, pos, given, r2, eps2, capacity, stream=stream, ws_fill=0xFF)
        assert other.everything() == want and status == base_survey_status, "another stream"
        other.free()

        # a survey + lists pair recorded in a stream capture and replayed twice
        hip = hip_runtime()
        captured = NeighbourDevice(gpu, pos, given, capacity=capacity, ws_fill=0xFF)
        gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
        graph, graph_exec = ctypes.c_void_p(), ctypes.c_void_p()
        assert hip.hipStreamBeginCapture(stream, 0) == 0
        captured.survey(r2, eps2, outputs=("nearest", "d2", "counts", "pot"), stream=stream)
        captured.lists(r2, stream=stream)
        assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
        assert captured.untouched("nearest") and captured.untouched("offsets"), "recorded, not run"
        assert hip.hipGraphInstantiate(ctypes.byref(graph_exec), graph, None, None, 0) == 0
        for _ in range(2):
            assert hip.hipGraphLaunch(graph_exec, stream) == 0
            gpu.check(lib.nb_stream_synchronize(stream), "nb_stream_synchronize")
            assert captured.everything() == want, "captured and replayed"
        assert captured.canaries_intact()
        assert hip.hipGraphExecDestroy(graph_exec) == 0 and hip.hipGraphDestroy(graph) == 0
        captured.free()
        gpu.check(lib.nb_stream_destroy(stream), "nb_stream_destroy")

        # every subset of the outputs: what is asked for has the bits of the full call, what is not stays untouched
        names = ("nearest", "d2", "counts", "pot")
        for mask in range(1, 15):
            asked = tuple(name for k, name in enumerate(names) if mask >> k & 1)
            some = NeighbourDevice(gpu, pos, given)
            some.survey(r2, eps2, outputs=asked)
            for name in names:
                if name in asked:
                    assert some.get(name).tobytes() == base.get(name).tobytes(), (asked, name)
                else:
                    assert some.untouched(name), (asked, name)
            assert some.get("status").tobytes() == base_survey_status and some.canaries_intact(), asked
            some.free()
        base.free()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_python_class_gives_the_c_calls_bits(gpu, dtype):
    n, kind = 3000, np.dtype(dtype).type
    pos = normal_cloud(n, dtype, "species")
    r2, eps2 = kind(0.04), kind(1e-3)
    d = NeighbourDevice(gpu, pos, capacity=100 * n)
    d.survey(r2, eps2, outputs=("nearest", "d2", "counts", "pot"))
    survey_status = d.status()
    d.lists(r2)
    total = d.status()["total_neighbours"]
    s = gpu.NeighbourSurvey(n, dtype, softening_sq=eps2)
    for positions in (pos, d.ptr("pos")):  # a host array, a device address
        out = s.survey(positions, radius_sq=r2, potentials=True)
        assert out["status"] == survey_status
        for key, name in (("nearest_index", "nearest"), ("nearest_dist_sq", "d2"), ("counts", "counts"), ("potentials", "pot")):
            assert out[key].tobytes() == d.get(name).tobytes(), key
    assert s.survey(pos, radius_sq=r2)["potentials"] is None
    sized = s.lists(pos, radius_sq=r2)
    assert sized["indices"] is None and sized["status"]["flags"] == OVERFLOW and sized["status"]["total_neighbours"] == total
    out = s.lists(pos, radius_sq=r2, capacity=total)
    assert out["status"] == d.status() and np.array_equal(out["offsets"], d.get("offsets")) and np.array_equal(out["indices"], d.get("indices")[:total])
    radii = np.full(n, r2, dtype)
    assert np.array_equal(s.lists(pos, radii_sq=radii, capacity=total)["indices"], out["indices"])
    with pytest.raises(ValueError):
        s.survey(pos)
    with pytest.raises(ValueError):
        s.survey(pos[:-1], radius_sq=r2)
    s.free(), d.free()


@gpu_only
def test_the_binary_of_a_block_step_run_is_the_closest_pair(gpu):
    """DESIGN.md 5.7's 256-body cloud with the circular binary (bodies 0 and 1, separation 0.01), stepped by HermiteBlockSystem to t = 1/8: the
    survey of the synchronised snapshot names (0, 1), and its separation agrees with the positions read back to gamma"""
    from test_hermite_block import BINARY_DT_MAX, BINARY_EPS2, BINARY_ETA_START, BINARY_LEVELS, binary_cloud
    pos, vel = binary_cloud()
    n = pos.shape[0]
    system = gpu.HermiteBlockSystem(n, np.float64, softening_sq=BINARY_EPS2, eta=0.02, eta_start=BINARY_ETA_START, dt_max=BINARY_DT_MAX, max_level=BINARY_LEVELS)
    system.set_state(pos, vel)
    system.init()
    status = system.advance(0.125)
    assert status.now_ticks == 1 << BINARY_LEVELS and status.block_steps > 100
    system.sync()
    s = gpu.NeighbourSurvey(n, np.float64, softening_sq=BINARY_EPS2)
    out = s.survey(system.snapshot_ptrs()[0], radius_sq=0.05 ** 2, potentials=True)
    x = system.snapshot()[0]
    system.free(), s.free()
    record = out["status"]
    assert (record["closest_i"], record["closest_j"]) == (0, 1) and out["nearest_index"][0] == 1 and out["nearest_index"][1] == 0
    exact = float(exact_d2(x, np.array([0]), np.array([1]))[0])
    assert abs(record["closest_dist_sq"] - exact) <= GAMMA[np.float64] * exact and record["closest_dist_sq"] == out["nearest_dist_sq"][0]
    assert abs(np.sqrt(exact) - 0.01) < 1e-4, "the binary is still circular"
    assert out["counts"][0] >= 1 and out["counts"][1] >= 1 and out["potentials"].argmin() in (0, 1), "the deepest potential is in the binary"


@gpu_only
def test_neighbour_survey_speed_sanity(gpu):
    """65 536 bodies fp32, device events, median of 5 single calls after warm-up: a survey takes no more than 2 x the issue-cost model of
    its loop AS COMPILED relative to the one-sided FAST step (nb_integrate_f32 without a workspace, 11 packed + 2 v_rsq_f32): without
    potentials (6 packed + 7 other vector operations) 0.86, with (8 + 7 and 2 v_rsq_f32) 1.27."""
    from test_hermite import Device, cloud
    n, dtype = 65536, np.float32
    pos, vel = cloud(n, dtype, 1, "equal", 1.0)
    eps2, dt = dtype(0.01), dtype(1e-3)
    gpu.set_softening_squared(eps2)
    d = Device(gpu, pos, vel, eps2)
    lib = gpu.lib()
    state = {"read": "pos"}

    def euler():
        write = "pos2" if state["read"] == "pos" else "pos"
        gpu.check(lib.nb_integrate_f32(d.ptr(write), d.ptr(state["read"]), d.ptr("vel"), dt, np.float32(1.0), n, 256, gpu.NB_MODE_FAST, None), "nb_integrate_f32")
        state["read"] = write

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

    t_euler = median_ms(euler)
    d.free()
    s = NeighbourDevice(gpu, pos)
    r2 = cloud_radius_sq(n, dtype)
    t_plain = median_ms(lambda: s.survey(r2, eps2, outputs=("nearest", "d2", "counts")))
    t_pot = median_ms(lambda: s.survey(r2, eps2, outputs=("nearest", "d2", "counts", "pot")))
    s.free()
    print(f"one-sided FAST step {t_euler:.3f} ms; survey {t_plain:.3f} ms = {t_plain / t_euler:.2f}x (model {MODEL_PLAIN:.2f}x, ratio / model {t_plain / t_euler / MODEL_PLAIN:.2f}); "
          f"with potentials {t_pot:.3f} ms = {t_pot / t_euler:.2f}x (model {MODEL_POT:.2f}x, ratio / model {t_pot / t_euler / MODEL_POT:.2f})")
    assert t_plain <= 2 * MODEL_PLAIN * t_euler, (t_plain, t_euler, MODEL_PLAIN)
    assert t_pot <= 2 * MODEL_POT * t_euler, (t_pot, t_euler, MODEL_POT)


# ---------------------------------------------------------------------------------------------------------------- CLI
CLI = os.path.join(ROOT, "cuda-nbody_amd", "nbody")


def test_cli_refuses_neighbours_where_it_refuses_energy():
    """--neighbours is single-device, not for --compare / --qatest / --systems (the refusals of --energy), and wants a radius"""
    base = ["--numbodies=1024", "--steps=1", "--neighbours=0.5"]
    for extra in (base + ["--numdevices=2"], base + ["--devices=0,1"], ["--numdevices=2"] + base, base + ["--compare"], base + ["--qatest"], base + ["--systems=3"],
                  base + ["--integrator=hermite", "--numdevices=2"], base + ["--integrator=hermite-block", "--devices=0,1"], base + ["--integrator=hermite", "--compare"],
                  ["--numbodies=1024", "--steps=1", "--neighbours=-0.5"], ["--numbodies=1024", "--steps=1", "--neighbours=nan"], ["--numbodies=1024", "--steps=1", "--neighbours=inf"],
                  ["--numbodies=1024", "--steps=1", "--neighbours=x"], ["--numbodies=1024", "--steps=1", "--neighbours="], ["--numbodies=1024", "--steps=1", "--neighbours"],
                  ["--numbodies=16777217", "--steps=1", "--neighbours=0.5"], ["-numbodies=1024", "-steps=1", "-neighbours=0.5", "-compare"]):
        r = subprocess.run([CLI, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr, (extra, r.returncode, r.stderr[:300])
        with_energy = [a.replace("neighbours=0.5", "energy") for a in extra]
        if with_energy != extra and "--numbodies=16777217" not in extra:
            e = subprocess.run([CLI, *with_energy], capture_output=True, text=True, timeout=60)
            assert e.returncode == 1 and "CRITICAL ERROR" in e.stderr, ("--energy is refused there too", with_energy)
    r = subprocess.run([CLI, "--numbodies=1024", "--steps=1", "--neighbours=0.5", "--numdevices=2"], capture_output=True, text=True, timeout=60)
    assert "--neighbours is single-device" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--neighbours FLOAT" in r.stdout


def cli_neighbour_lines(stdout):
    pair = re.search(r"^closest pair: bodies (\d+) and (\d+), separation (\S+)$", stdout, re.M)
    counts = re.search(r"^neighbours within (\S+): mean (\S+), largest (\d+) at body (\d+)$", stdout, re.M)
    deepest = re.search(r"^deepest potential: (\S+) at body (\d+)$", stdout, re.M)
    assert pair and counts and deepest, stdout[-800:]
    return ((int(pair[1]), int(pair[2]), float(pair[3])), (float(counts[1]), float(counts[2]), int(counts[3]), int(counts[4])), (float(deepest[1]), int(deepest[2])))


@gpu_only
def test_cli_prints_the_survey_of_the_final_state(gpu, tmp_path):
    """nbody --neighbours with the three integrators: the lines describe the state the run dumps (surveyed here through the Python
    class), and come after the run's own lines and --energy's"""
    n, steps, radius = 4096, 3, 0.75
    for integrator, extra in (("hermite-block", ["--eta=0.05", "--levels=12"]), ("hermite", []), ("euler", []), ("euler", ["--fp64"])):
        dtype = np.float64 if "--fp64" in extra else np.float32
        out = tmp_path / "state.bin"
        r = subprocess.run([CLI, f"--integrator={integrator}", f"--numbodies={n}", f"--steps={steps}", f"--dump={out}", "--energy", f"--neighbours={radius}", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        pos = np.fromfile(out, dtype=dtype)[:4 * n].reshape(n, 4)
        softening = dtype(np.float32(0.1))
        s = gpu.NeighbourSurvey(n, dtype, softening_sq=softening * softening)
        want = s.survey(pos, radius_sq=dtype(radius) * dtype(radius), potentials=True)
        s.free()
        pair, counts, deepest = cli_neighbour_lines(r.stdout)
        status = want["status"]
        assert pair[:2] == (status["closest_i"], status["closest_j"]) and abs(pair[2] - np.sqrt(status["closest_dist_sq"])) <= 1e-8 * pair[2], (integrator, pair, status)
        assert counts[0] == radius and abs(counts[1] - status["total_neighbours"] / n) <= 1e-8 * counts[1] and counts[2:] == (status["max_count"], status["max_count_body"])
        body = int(want["potentials"].argmin())
        assert deepest[1] == body and abs(deepest[0] - float(want["potentials"][body])) <= 1e-8 * abs(deepest[0])
        assert r.stdout.index("energy end") < r.stdout.index("closest pair:"), "after --energy's lines"
    r = subprocess.run([CLI, f"--numbodies={n}", "--benchmark", "-i=2", f"--neighbours={radius}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    cli_neighbour_lines(r.stdout)
    bench = r.stdout.index("billion interactions per second")
    assert bench < r.stdout.index("closest pair:"), "the reference's benchmark lines stay first"
