"""Energies of every system of an ensemble in one call (nb_energy_ensemble_*, include/nbody_hip_energy_ensemble.h;
csrc/energy_ensemble.hip) and `nbody --systems=B --energies`.

CPU tests: the boundary (declared, exported, mirrored, nowhere else), host-side argument checks, the plan and the workspace query, the
compiled kernels (no scratch, <= 128 VGPRs in fp32, the solo pair loop's instruction mix), the shared text, the command line's
rejections.  GPU tests: exactness against the fp64 numpy sum of tests/test_energy.py on the same inputs at every size where the
geometry changes, 65 536 bodies against the solo call, two-body systems bit for bit against the solo call, independence of the batch,
the softening array, zero-mass padding, the drift summary, the state of a Hermite ensemble, the command line with all five ensemble
runs, and the cost against one ensemble step and against B solo calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, entry
from test_capi_symbols import declared_symbols, exported_symbols
from test_energy import FIELDS, Softening, assert_matches, random_state, ref_energy

PKG = os.path.join(ROOT, "cuda-nbody_amd")
CSRC = os.path.join(PKG, "csrc")
CLI = os.path.join(PKG, "nbody")
HEADER = "nbody_hip_energy_ensemble.h"
ERR = 10001
gpu_only = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_exports_exactly_its_header_and_nobody_else_does(pkg):
    names = declared_symbols(HEADER)
    assert names == sorted(["nb_energy_ensemble_plan_f32", "nb_energy_ensemble_plan_f64", "nb_energy_ensemble_workspace_bytes", "nb_energy_ensemble_f32",
                            "nb_energy_ensemble_f64", "nb_energy_ensemble_drift"])
    assert exported_symbols(pkg.ENERGY_ENSEMBLE_LIB_PATH) == names == sorted(pkg.ENERGY_ENSEMBLE_SIGNATURES)
    lib = pkg.energy_ensemble_lib()
    assert not [n for n in names if not hasattr(lib, n)]
    others = {k: getattr(pkg, k) for k in dir(pkg) if k.endswith("LIB_PATH") and k != "ENERGY_ENSEMBLE_LIB_PATH"}
    assert len(others) >= 14, sorted(others)
    for key, path in others.items():
        assert not set(exported_symbols(path)) & set(names), key
    # what the other libraries export is what it was
    assert len(exported_symbols(pkg.LIB_PATH)) == 96 and len(exported_symbols(pkg.ENSEMBLE_LIB_PATH)) == 4
    needed = subprocess.run(["readelf", "-d", pkg.ENERGY_ENSEMBLE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnbody_hip" not in needed  # it links none of the others


def struct_fields(text, tag, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (tag, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t.strip(), f, int(k) if k else 1) for t, f, k in re.findall(r"([\w ]+?)\s+(\w+)(?:\[(\d+)\])?;", body)]


def test_ctypes_mirrors_match_the_header(pkg):
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    sizes = {"int": 4, "unsigned": 4, "double": 8, "unsigned long long": 8}
    for tag, name, mirror, total in (("nb_energy_ensemble_plan", "nb_energy_ensemble_plan_t", pkg.EnergyEnsemblePlan, 32),
                                     ("nb_energy_ensemble_drift_record", "nb_energy_ensemble_drift_t", pkg.EnergyDrift, 64)):
        fields = struct_fields(text, tag, name)
        assert [f for _, f, _ in fields] == [f for f, _ in mirror._fields_], name
        offset = 0
        for (ctype, field, count), (_, mirrored) in zip(fields, mirror._fields_):
            assert ctypes.sizeof(mirrored) == sizes[ctype] * count, field
            assert getattr(mirror, field).offset == offset, field  # (no padding: every field sits where the C compiler puts it)
            offset += sizes[ctype] * count
        assert ctypes.sizeof(mirror) == offset == total, name
    assert "no softening floor" in text.lower()


def test_argument_errors_are_caught_on_the_host(pkg):
    """Nothing here reaches HIP: every call is refused before a launch (the addresses are never dereferenced)."""
    lib = pkg.energy_ensemble_lib()
    n, b = 1024, 7
    need = ctypes.c_size_t(0)
    assert lib.nb_energy_ensemble_workspace_bytes(n, b, ctypes.byref(need)) == 0 and need.value > 0
    pos, vel, ws, res, eps = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    for fn, size in ((lib.nb_energy_ensemble_f32, 4), (lib.nb_energy_ensemble_f64, 8)):
        ok = dict(p=pos, v=vel, n=n, b=b, e=eps, s=1, w=ws, wb=need.value, r=res)
        call = lambda **kw: fn(kw["p"], kw["v"], kw["n"], kw["b"], 0.01, kw["e"], kw["s"], kw["w"], kw["wb"], kw["r"], None)  # noqa: E731
        bodies = 4 * n * b * size
        for null in ("p", "v", "w", "r"):
            assert call(**{**ok, null: None}) == ERR, null
        assert call(**{**ok, "n": 0}) == ERR and call(**{**ok, "b": 0}) == ERR
        assert call(**{**ok, "n": 65537, "b": 1}) == ERR
        assert call(**{**ok, "n": 65536, "b": 32769}) == ERR          # N * B above 2^31
        assert call(**{**ok, "s": 0}) == ERR                            # softening_stride == 0
        assert call(**{**ok, "wb": need.value - 1}) == ERR
        assert call(**{**ok, "p": pos + size}) == ERR                   # bodies not vec4-aligned
        assert call(**{**ok, "v": vel + 2 * size}) == ERR
        assert call(**{**ok, "w": ws + 4}) == ERR and call(**{**ok, "r": res + 4}) == ERR  # workspace, results: 8 bytes
        assert call(**{**ok, "e": eps + size // 2}) == ERR              # the softening array: sizeof(T)
        assert call(**{**ok, "w": pos}) == ERR                          # workspace on top of the positions
        assert call(**{**ok, "w": pos + bodies - 8}) == ERR             # ... or on their last body
        assert call(**{**ok, "r": vel + 64}) == ERR                     # results inside the velocities
        assert call(**{**ok, "r": ws + 8}) == ERR                       # results overlapping the workspace
        assert call(**{**ok, "r": ws + need.value - 8}) == ERR
        assert call(**{**ok, "e": pos + 16}) == ERR                     # softening array inside the positions
        assert call(**{**ok, "e": res + 104 * b - size}) == ERR         # ... on the last result
        assert call(**{**ok, "e": ws, "s": 4}) == ERR
        assert call(**{**ok, "e": res - (4 * (b - 1) + 1) * size + size, "s": 4}) == ERR  # stride 4: its last element is the results' first bytes
    plan = pkg.EnergyEnsemblePlan()
    for fn in (lib.nb_energy_ensemble_plan_f32, lib.nb_energy_ensemble_plan_f64):
        assert fn(n, b, None) == ERR and fn(0, b, ctypes.byref(plan)) == ERR and fn(n, 0, ctypes.byref(plan)) == ERR and fn(65537, 1, ctypes.byref(plan)) == ERR
        assert fn(65536, 32768, ctypes.byref(plan)) == 0 and fn(65536, 32769, ctypes.byref(plan)) == ERR
    assert lib.nb_energy_ensemble_workspace_bytes(n, b, None) == ERR and lib.nb_energy_ensemble_workspace_bytes(0, b, ctypes.byref(need)) == ERR
    assert lib.nb_energy_ensemble_workspace_bytes(65537, 1, ctypes.byref(need)) == ERR
    start, end, out = 0x10000000, 0x20000000, 0x30000000
    drift = lib.nb_energy_ensemble_drift
    assert drift(None, end, b, out, None) == ERR and drift(start, None, b, out, None) == ERR and drift(start, end, b, None, None) == ERR
    assert drift(start, end, 0, out, None) == ERR
    assert drift(start + 4, end, b, out, None) == ERR and drift(start, end, b, out + 4, None) == ERR
    assert drift(start, end, b, start + 104, None) == ERR and drift(start, end, b, end + 104 * b - 8, None) == ERR


PLAN_FIELDS = ("bodies_per_lane", "waves_per_group", "groups_per_system", "block_threads", "lds_bytes")
SWEEP = sorted(set(list(range(1, 700)) + list(range(700, 4300, 7)) + [1 << k for k in range(10, 17)] + [(1 << k) + 1 for k in range(10, 16)] + [65535]))


def geometry(pkg, n, b, dtype):
    p = pkg.energy_ensemble_plan(n, b, dtype)
    return tuple(getattr(p, f) for f in PLAN_FIELDS), p.grid_blocks


def test_plan_is_a_function_of_n_and_precision_alone(pkg):
    for dtype in (np.float32, np.float64):
        w = 2 if dtype is np.float32 else 1
        for n in SWEEP:
            one, grid = geometry(pkg, n, 1, dtype)
            assert grid == one[2]
            for b in (7, 256):
                other, grid = geometry(pkg, n, b, dtype)
                assert other == one and grid == one[2] * b, (n, b)
            lane, waves, groups, threads, lds = one
            assert lane in (w, 2, 4, 4 * w) and waves in (1, 2, 4) and threads == 64 * waves and lds == 12 * 8 * threads and lane % waves == 0, (n, one)
            assert n < 128 or 64 * lane <= n, (n, one)                       # no empty slot from 128 bodies (fp32: a packed pair at least)
            assert groups * 128 * 7 <= pkg.energy_ensemble_workspace_bytes(n, 7)  # one 128-byte record per workgroup fits the workspace
    # a 256-body system: one block of four bodies per lane, two waves; 1 024 bodies in fp32: a batch of 256 puts four waves on every SIMD
    assert geometry(pkg, 256, 1, np.float32)[0][:4] == (4, 2, 1, 128) and geometry(pkg, 256, 1, np.float64)[0][:4] == (4, 2, 1, 128)
    assert geometry(pkg, 1024, 256, np.float32) == ((8, 4, 4, 256, 24576), 1024)


def test_workspace_query_is_monotone_and_a_few_bytes_per_body(pkg):
    for b in (1, 7, 256):
        got = [pkg.energy_ensemble_workspace_bytes(n, b) for n in SWEEP]
        assert all(x > 0 and x % 128 == 0 for x in got)
        assert all(x <= y for x, y in zip(got, got[1:])), b
        for n, x in zip(SWEEP, got):
            assert x <= (2 * n + 1152) * b, (n, b, x)  # 2 bytes per body and nine records per system
            assert x == pkg.energy_ensemble_workspace_bytes(n, 1) * b
    assert pkg.energy_ensemble_workspace_bytes(65536, 32768) <= 2 * (1 << 31) + 1152 * 32768


def kernels_of(lines):
    """(name, start, end) of every kernel of a listing"""
    out = []
    for i, line in enumerate(lines):
        m = re.match(r"(_ZN2nb\S+):", line)
        if m:
            out.append((m.group(1), i, next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))))
    return out


def test_compiled_kernels_keep_the_solo_pair_loop_and_use_no_scratch():
    subprocess.run(["make", "-s", "-C", CSRC, "asm"], check=True, capture_output=True)
    text = open(os.path.join(CSRC, "energy_ensemble.s")).read()
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(sizes) == 14 and set(sizes) == {"0"} and "scratch_" not in text
    lines = text.split("\n")
    kernels = kernels_of(lines)
    names = [k[0] for k in kernels]
    assert any("energy_ensemble_finish" in n for n in names) and any("energy_ensemble_drift_summary" in n for n in names)
    fp32 = [k for k in kernels if "energy_ensemble_pairsIf" in k[0]]
    assert len(fp32) == 7 and len([k for k in kernels if "energy_ensemble_pairsId" in k[0]]) == 5
    for name, start, end in fp32:
        tail = "\n".join(lines[end:end + 60])
        assert int(re.search(r"; NumVgprs: (\d+)", tail).group(1)) <= 128, name
        loops = []
        for i in range(start, end):
            if "Inner Loop Header" not in lines[i]:
                continue
            label = lines[i - 1].split(":")[0].strip()
            stop = next((k for k in range(i, end) if "s_cbranch" in lines[k] and label in lines[k]), None)
            if stop is None:
                continue
            body = [l.strip().split()[0] for l in lines[i + 1:stop] if l.strip() and not l.strip().startswith(";")]
            if "v_rsq_f32_e32" in body:
                loops.append(body)
        assert len(loops) >= 4, name  # unmasked and masked, each unrolled and its remainder
        for body in loops:
            # per packed pair of bodies i and body j: 3 v_pk_add, 4 v_pk_fma, 2 v_rsq -- the solo kernel's mix -- and no fp64 inside
            assert body.count("v_pk_add_f32") * 2 == body.count("v_rsq_f32_e32") * 3 and body.count("v_pk_fma_f32") == body.count("v_rsq_f32_e32") * 2, name
            assert not [op for op in body if op.startswith("v_") and "f64" in op], name
            assert any(op.startswith("s_load") for op in body) and not any(op.startswith(("ds_", "global_load", "buffer_load")) for op in body), name


def test_sources_share_the_pair_arithmetic_and_hold_no_state():
    read = lambda name: open(os.path.join(CSRC, name)).read()  # noqa: E731
    for name in ("energy_ensemble.hip", "energy_ensemble_api.hip", "energy_ensemble_kernels.h", "energy_pair.inc"):
        code = re.sub(r"//.*", "", read(name))
        for word in ("atomic", "hipMalloc", "Synchronize", "mutex"):
            assert word not in code, (name, word)
    for unit in ("nbody_energy.hip", "energy_ensemble.hip"):
        assert '#include "energy_pair.inc"' in read(unit), unit
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".h", ".inc")) and name != "energy_pair.inc":
            # (neighbour.hip has an untemplated inv_sqrt of its own squared distances: another function)
            assert not re.search(r"inv_sqrt<\w+>\([^;{]*\)\s*\{", read(name)) and not re.search(r"\bsweep\s*\([^;{]*\)\s*\{", read(name)), name
    shared = read("energy_pair.inc")
    assert re.search(r"void sweep\(", shared) and len(re.findall(r"inv_sqrt<\w+>\(\w+ d2\) \{", shared)) == 2 and "void tree_sum(" in shared
    api = read("energy_ensemble_api.hip")
    assert '#include "capi_check.h"' in api and re.search(r"\bspans_ok\(\{", api)
    mk = read("Makefile")
    assert "$(eval $(call small_library,energy_ensemble,energy_ensemble.o energy_ensemble_api.o))" in mk and re.search(r"^ASM :=.*\benergy_ensemble\.s\b", mk, re.M)


def test_cli_energies_flag_and_its_rejections():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--energies" in r.stdout
    base = ["--systems=3", "--numbodies=256", "--steps=2", "--energies"]
    for args in (["--energies", "--steps=2"], ["--energies", "--benchmark"], ["--energies=1"] + base[:3], base + ["--numdevices=2"], ["--energies", "--numdevices=2", "--benchmark"],
                 base + ["--compare"], ["--energies", "--compare"], base + ["--hostmem"], ["--energies", "--hostmem", "--benchmark"], base + ["--energy"]):
        r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr, (args, r.stdout[-300:], r.stderr[-300:])
    r = subprocess.run([CLI, "--energies", "--steps=2"], capture_output=True, text=True, timeout=60)
    assert "--systems" in r.stderr and "--energy)" in r.stderr  # the message names the flag for one system


# ---------------------------------------------------------------------------------------------------------------- GPU

BASE_SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1024, 4097]


def plan_change_sizes(limit=4200, most=24):
    """n - 1, n, n + 1 at every n <= limit where a field of the plan but the grid changes in either precision: the changes of the bodies per lane
    and the waves first, then those of the groups alone, smallest first; at most `most` sizes beyond BASE_SIZES"""
    pkg = entry.load_package()
    shape, groups = [], []
    for dtype in (np.float32, np.float64):
        before = geometry(pkg, 1, 1, dtype)[0]
        for n in range(2, limit + 1):
            now = geometry(pkg, n, 1, dtype)[0]
            if now != before:
                (shape if (now[0], now[1]) != (before[0], before[1]) else groups).append(n)
            before = now
    out = []
    for n in sorted(set(shape)) + sorted(set(groups)):
        for m in (n - 1, n, n + 1):
            if m not in BASE_SIZES and m not in out and len(out) < most:
                out.append(m)
    return sorted(out)


def upload(pkg, array):
    array = np.ascontiguousarray(array)
    buf = pkg.DeviceBuffer(max(array.nbytes, 8))
    buf.upload(array)
    return buf


def measure(pkg, pos, vel, dtype, eps2=0.0, system_eps2=None, stride=1, stream=None):
    """energy_ensemble of host arrays (B, N, 4): a list of B dicts"""
    pos, vel = np.ascontiguousarray(pos, dtype=dtype), np.ascontiguousarray(vel, dtype=dtype)
    b, n = pos.shape[0], pos.shape[1]
    bufs = [upload(pkg, pos), upload(pkg, vel)]
    table = None
    if system_eps2 is not None:
        bufs.append(upload(pkg, np.ascontiguousarray(system_eps2, dtype=dtype)))
        table = bufs[-1].ptr
    try:
        return pkg.energy_ensemble(bufs[0].ptr, bufs[1].ptr, n, b, dtype, softening_sq=eps2, system_softening_sq=table, softening_stride=stride, stream=stream)
    finally:
        for buf in bufs:
            buf.free()


def three_systems(n, seed):
    states = [random_state(n, seed + 1000 * s) for s in range(3)]
    return np.stack([p.reshape(n, 4) for p, _ in states]), np.stack([v.reshape(n, 4) for _, v in states])


@gpu_only
@pytest.mark.parametrize("eps2", [0.01, 0.0])
@pytest.mark.parametrize("n", BASE_SIZES + plan_change_sizes())
def test_every_system_matches_fp64_numpy(gpu, n, eps2):
    pos, vel = three_systems(n, 100 + n)
    # fp32: the inputs rounded to fp32 and widened back, so that numpy sees exactly what the GPU sees
    pos32, vel32 = pos.astype(np.float32), vel.astype(np.float32)
    got32 = measure(gpu, pos32, vel32, np.float32, eps2)
    got64 = measure(gpu, pos, vel, np.float64, eps2)
    assert len(got32) == len(got64) == 3
    for s in range(3):
        want32 = ref_energy(pos32[s], vel32[s], float(np.float32(eps2)))
        assert_matches(got32[s], want32, 5e-6 if eps2 else 2e-5, 1e-6)
        want64 = ref_energy(pos[s], vel[s], eps2)
        assert_matches(got64[s], want64, 1e-12, 1e-13)
        if n == 1:
            assert got32[s]["potential"] == 0 and got64[s]["potential"] == 0


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_65536_bodies_agree_with_the_solo_call(gpu, dtype):
    n, b, eps2 = 65536, 2, 0.01
    tol = 1e-5 if dtype == np.float32 else 2e-12  # one solo tolerance from each side
    rng = np.random.default_rng(65536)
    pos = np.empty((b, n, 4), dtype)
    pos[:, :, :3], pos[:, :, 3] = rng.uniform(-1, 1, (b, n, 3)), rng.uniform(0.5, 1.5, (b, n))
    vel = np.zeros((b, n, 4), dtype)
    vel[:, :, :3] = rng.normal(0, 1, (b, n, 3))
    d_pos, d_vel = upload(gpu, pos), upload(gpu, vel)
    try:
        got = gpu.energy_ensemble(d_pos.ptr, d_vel.ptr, n, b, dtype, softening_sq=eps2)
        with Softening(gpu, dtype, eps2):
            solo = [gpu.energy(ctypes.c_void_p(d_pos.ptr.value + s * pos[0].nbytes), ctypes.c_void_p(d_vel.ptr.value + s * vel[0].nbytes), n, dtype) for s in range(b)]
    finally:
        d_pos.free(), d_vel.free()
    for s in range(b):
        m, p, v = pos[s, :, 3].astype(np.float64), pos[s, :, :3].astype(np.float64), vel[s, :, :3].astype(np.float64)
        scales = {"momentum": np.abs(m[:, None] * v).sum(axis=0), "angular_momentum": np.abs(m[:, None] * np.cross(p, v)).sum(axis=0),
                  "center_of_mass": np.abs(m[:, None] * p).sum(axis=0) / m.sum()}
        for f in ("kinetic", "potential", "total", "mass"):
            assert abs(got[s][f] - solo[s][f]) <= tol * abs(solo[s][f]), (s, f, got[s][f], solo[s][f])
        for f, scale in scales.items():
            assert (np.abs(np.array(got[s][f]) - np.array(solo[s][f])) <= tol * scale).all(), (s, f, got[s][f], solo[s][f])
    assert got[0]["total"] != got[1]["total"]


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_body_potentials_are_the_solo_calls_bit_for_bit(gpu, dtype):
    """The states of tests/test_fast_domain.py::test_energy_pair_potential_across_the_exponent_range, one system per state with its
    own softening^2: one pair, the shared arithmetic, an exact fp64 fold."""
    from test_fast_domain import sweep_probes

    states, eps = [], []
    for eps2, d2 in sweep_probes(dtype):
        for dd in d2[:: 4 if dtype == np.float32 else 2]:
            x = dtype(np.sqrt(dd / 1.25))
            states.append([0, 0, 0, 1.5, x, x * dtype(0.5), 0, 0.75])
            eps.append(eps2)
    pos, eps = np.array(states, dtype).reshape(-1, 2, 4), np.array(eps, dtype)
    b = len(pos)
    assert b >= 200
    got = measure(gpu, pos, np.zeros_like(pos), dtype, eps2=123.0, system_eps2=eps)
    work = gpu.DeviceBuffer(gpu.energy_workspace_bytes(2))
    d_pos, d_vel = upload(gpu, pos), upload(gpu, np.zeros(8, dtype))
    try:
        for s in range(b):
            gpu.set_softening_squared(dtype(eps[s]))
            solo = gpu.energy(ctypes.c_void_p(d_pos.ptr.value + s * pos[0].nbytes), d_vel.ptr, 2, dtype, workspace=work)
            assert np.float64(got[s]["potential"]).tobytes() == np.float64(solo["potential"]).tobytes(), (s, eps[s], got[s]["potential"], solo["potential"])
            assert np.isfinite(got[s]["potential"]) and got[s]["potential"] < 0
    finally:
        work.free(), d_pos.free(), d_vel.free()
        gpu.set_softening_squared(dtype(np.float32(0.1)) * dtype(np.float32(0.1)))


def record_bytes(result):
    return np.concatenate([np.atleast_1d(np.array(result[f], np.float64)) for f in FIELDS]).tobytes()


@gpu_only
@pytest.mark.parametrize("dtype,n", [(np.float32, 300), (np.float32, 1100), (np.float64, 300)])
def test_a_system_does_not_depend_on_the_batch_and_only_its_own_bytes_are_written(gpu, dtype, n):
    lib, elib = gpu.lib(), gpu.energy_ensemble_lib()
    fn = elib.nb_energy_ensemble_f32 if dtype == np.float32 else elib.nb_energy_ensemble_f64
    eps2 = dtype(0.01)
    rng = np.random.default_rng(n)
    mine = [np.array(a, dtype).reshape(n, 4) for a in random_state(n, 5)]
    guard = 256
    stream = ctypes.c_void_p()
    gpu.check(lib.nb_stream_create(ctypes.byref(stream)))
    seen = set()
    try:
        for b, places in ((1, (0,)), (7, (0, 3, 6))):
            pos = np.stack([np.array(random_state(n, 50 + s)[0], dtype).reshape(n, 4) for s in range(b)])
            vel = np.stack([np.array(random_state(n, 50 + s)[1], dtype).reshape(n, 4) for s in range(b)]) * dtype(rng.uniform(0.5, 2))
            for s in places:
                pos[s], vel[s] = mine
            need = gpu.energy_ensemble_workspace_bytes(n, b)
            d_pos, d_vel = upload(gpu, pos), upload(gpu, vel)
            ws, res = gpu.DeviceBuffer(need + guard), gpu.DeviceBuffer(guard + 104 * b + guard)
            res_ptr = ctypes.c_void_p(res.ptr.value + guard)
            try:
                for on, fill in ((None, 0), (stream, 0), (None, 0xFF), (stream, 0xFF)):
                    gpu.check(lib.nb_memset(ws.ptr, fill, need, None))
                    gpu.check(lib.nb_memset(ctypes.c_void_p(ws.ptr.value + need), 0xA5, guard, None))
                    gpu.check(lib.nb_memset(res.ptr, 0x5A, res.nbytes, None))
                    gpu.check(lib.nb_device_synchronize())
                    gpu.check(fn(d_pos.ptr, d_vel.ptr, n, b, eps2 if dtype == np.float32 else float(eps2), None, 1, ws.ptr, need, res_ptr, on))
                    gpu.check(lib.nb_stream_synchronize(on))
                    gpu.check(lib.nb_device_synchronize())
                    out, tail = res.download(np.zeros(res.nbytes, np.uint8)), ws.download(np.zeros(need + guard, np.uint8))
                    assert (out[:guard] == 0x5A).all() and (out[guard + 104 * b:] == 0x5A).all(), "bytes around the results were written"
                    assert (tail[need:] == 0xA5).all(), "bytes past the workspace were written"
                    for s in places:
                        seen.add(out[guard + 104 * s:guard + 104 * (s + 1)].tobytes())
                    others = {out[guard + 104 * s:guard + 104 * (s + 1)].tobytes() for s in range(b) if s not in places}
                    assert len(others) == b - len(places) and not others & seen
                assert d_pos.download(np.zeros_like(pos)).tobytes() == pos.tobytes() and d_vel.download(np.zeros_like(vel)).tobytes() == vel.tobytes()
            finally:
                for buf in (d_pos, d_vel, ws, res):
                    buf.free()
    finally:
        lib.nb_stream_destroy(stream)
    assert len(seen) == 1, "the same system gave different bytes in another batch, place, stream or workspace"
    total = np.frombuffer(next(iter(seen)), np.float64)[2]
    want = ref_energy(mine[0], mine[1], float(eps2))["total"]
    assert abs(total - want) <= (5e-6 if dtype == np.float32 else 1e-12) * abs(want)


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_softening_array_equals_scalar_calls(gpu, dtype):
    n, b = 257, 5
    pos = np.stack([np.array(random_state(n, 70 + s)[0], dtype).reshape(n, 4) for s in range(b)])
    vel = np.stack([np.array(random_state(n, 70 + s)[1], dtype).reshape(n, 4) for s in range(b)])
    eps = np.array([0.0, 0.01, 1e-4, 0.25, 2.0], dtype)
    scalar = [record_bytes(measure(gpu, pos[s:s + 1], vel[s:s + 1], dtype, eps2=eps[s])[0]) for s in range(b)]
    assert len(set(scalar)) == b
    assert [record_bytes(r) for r in measure(gpu, pos, vel, dtype, eps2=7.0, system_eps2=eps, stride=1)] == scalar
    # the plain ensemble's {dt, damping, eps^2, -} table, the pointer at its third column
    table = np.full((b, 4), 99, dtype)
    table[:, 2] = eps
    d_pos, d_vel, d_table = upload(gpu, pos), upload(gpu, vel), upload(gpu, table)
    try:
        got = gpu.energy_ensemble(d_pos.ptr, d_vel.ptr, n, b, dtype, softening_sq=7.0, system_softening_sq=ctypes.c_void_p(d_table.ptr.value + 2 * table.itemsize),
                                  softening_stride=4)
    finally:
        d_pos.free(), d_vel.free(), d_table.free()
    assert [record_bytes(r) for r in got] == scalar


@gpu_only
def test_zero_mass_padding_changes_nothing(gpu):
    """300 bodies padded to 512 with zero-mass bodies at the origin (as tipsy.cpp pads), softened; a second system keeps it company"""
    pos, vel = (np.array(a, np.float32).reshape(300, 4) for a in random_state(300, 11))
    pad = np.zeros((2, 512, 4), np.float32), np.zeros((2, 512, 4), np.float32)
    pad[0][0, :300], pad[1][0, :300] = pos, vel
    pad[0][1], pad[1][1] = (np.array(a, np.float32).reshape(512, 4) for a in random_state(512, 12))
    got = measure(gpu, pad[0], pad[1], np.float32, 0.01)
    assert_matches(got[0], ref_energy(pos, vel, float(np.float32(0.01))), 5e-6, 1e-6)
    assert_matches(got[1], ref_energy(pad[0][1], pad[1][1], float(np.float32(0.01))), 5e-6, 1e-6)
    got64 = measure(gpu, pad[0].astype(np.float64), pad[1].astype(np.float64), np.float64, 0.01)
    assert_matches(got64[0], ref_energy(pos, vel, 0.01), 1e-12, 1e-13)


def drift_reference(start, end):
    """the 64-byte record from the same B records, in numpy"""
    e0, e1 = start[:, 2], end[:, 2]
    with np.errstate(all="ignore"):
        rel = np.abs(e1 - e0) / np.abs(e0)
    finite = np.isfinite(rel)
    key = np.where(finite, rel, np.inf)
    with np.errstate(all="ignore"):
        mom = np.nanmax(np.where(np.isnan(end[:, 4:7] - start[:, 4:7]), -1.0, np.abs(end[:, 4:7] - start[:, 4:7])), axis=1)
    return {"systems": len(e0), "worst_system": int(np.argmax(key)), "worst_relative_drift": float(key.max()),
            "rms_relative_drift": float(np.sqrt((rel[finite] ** 2).sum() / finite.sum())) if finite.any() else 0.0,
            "worst_momentum_drift": float(max(mom.max(), 0.0)), "worst_momentum_system": int(np.argmax(mom)) if mom.max() >= 0 else 0, "not_finite": int((~finite).sum())}


@gpu_only
@pytest.mark.parametrize("case", ["finite", "a NaN total", "an infinite total", "a zero start", "two not finite", "one system", "300 systems"])
def test_drift_summary_agrees_with_numpy(gpu, case):
    b = {"one system": 1, "300 systems": 300}.get(case, 16)
    rng = np.random.default_rng(len(case))
    start = rng.normal(0, 1, (b, 13))
    start[:, 2] = -np.abs(start[:, 2]) - 0.1
    end = start * (1 + rng.normal(0, 1e-6, (b, 13)))
    if b == 16:
        end[11, 2] = start[11, 2] * (1 + 3e-4)       # the worst of the finite ones
        end[5, 2] = start[5, 2] * (1 - 3e-4 * (1 - 1e-9))
        end[9, 4:7] = start[9, 4:7] + (1e-3, -2e-3, 5e-4)
    if case == "a NaN total":
        end[13, 2] = np.nan
    elif case == "an infinite total":
        end[7, 2] = -np.inf
    elif case == "a zero start":
        start[12, 2] = 0.0
    elif case == "two not finite":
        end[14, 2], start[3, 2], end[3, 5] = np.inf, np.nan, np.nan
    want = drift_reference(start, end)
    d_start, d_end = upload(gpu, start), upload(gpu, end)
    guard = gpu.DeviceBuffer(64 * 3)
    try:
        gpu.check(gpu.lib().nb_memset(guard.ptr, 0x5A, guard.nbytes, None))
        gpu.check(gpu.lib().nb_device_synchronize())
        gpu.check(gpu.energy_ensemble_lib().nb_energy_ensemble_drift(d_start.ptr, d_end.ptr, b, ctypes.c_void_p(guard.ptr.value + 64), None))
        gpu.check(gpu.lib().nb_device_synchronize())
        around = guard.download(np.zeros(guard.nbytes, np.uint8))
        got = gpu.energy_ensemble_drift(d_start, d_end, b)
    finally:
        d_start.free(), d_end.free(), guard.free()
    assert (around[:64] == 0x5A).all() and (around[128:] == 0x5A).all() and (around[64 + 40:128] == 0).all()
    mirror = gpu.EnergyDrift.from_buffer_copy(around[64:128].tobytes())
    assert {k: getattr(mirror, k) for k in got} == got  # the same bytes on every call
    for key in ("systems", "worst_system", "worst_momentum_system", "not_finite"):
        assert got[key] == want[key], (key, got, want)
    for key in ("worst_relative_drift", "rms_relative_drift", "worst_momentum_drift"):
        if np.isinf(want[key]):
            assert got[key] == want[key], (key, got, want)
        else:
            assert abs(got[key] - want[key]) <= 1e-14 * abs(want[key]), (key, got[key], want[key])
    if b == 16 and case == "finite":
        assert got["worst_system"] == 11 and got["worst_momentum_system"] == 9 and got["not_finite"] == 0
    if case == "two not finite":
        assert got["worst_system"] == 3 and got["not_finite"] == 2 and got["worst_relative_drift"] == np.inf


@gpu_only
def test_state_of_a_hermite_ensemble_is_measured_in_place(gpu):
    n, b, eps2 = 256, 8, 0.01
    pos = np.stack([np.array(random_state(n, 300 + s)[0]).reshape(n, 4) for s in range(b)])
    vel = np.stack([np.array(random_state(n, 300 + s)[1]).reshape(n, 4) for s in range(b)]) * 0.3
    ensemble = gpu.HermiteEnsemble(n, b, np.float64, softening_sq=eps2)
    try:
        ensemble.set_state(pos, vel)
        ensemble.eval()
        for _ in range(8):
            ensemble.step(1.0 / 1024)
        got = gpu.energy_ensemble(ensemble._pos.ptr, ensemble._vel.ptr, n, b, np.float64, softening_sq=eps2)
        now_pos, now_vel = ensemble.get_positions(), ensemble.get_velocities()
    finally:
        ensemble.free()
    assert now_pos.tobytes() != pos.tobytes()
    for s in range(b):
        assert_matches(got[s], ref_energy(now_pos[s], now_vel[s], eps2), 1e-12, 1e-13)


CLI_RUNS = {"plain": [], "hermite-ensemble": ["--integrator=hermite-ensemble"], "hermite6-ensemble": ["--integrator=hermite6-ensemble"],
            "hermite-block-ensemble": ["--integrator=hermite-block-ensemble", "--levels=12"], "hermite6-block-ensemble": ["--integrator=hermite6-block-ensemble", "--levels=12"]}
_CLI_START = {}


def cli_start_state(gpu, oracle, n, b):
    """the start state of `nbody --systems` as tests/test_ensemble.py re-creates it, and its energies: computed once"""
    if (n, b) not in _CLI_START:
        from oracle import scales_for

        pos, vel = np.empty((b, n, 4), np.float32), np.empty((b, n, 4), np.float32)
        p0, v0 = oracle.startup_state(n, np.float32)
        pos[0], vel[0] = p0.reshape(n, 4), v0.reshape(n, 4)
        c, v = scales_for(n)
        for s in range(1, b):
            ps, vs = oracle.randomise(1, n, c, v, np.float32)
            pos[s], vel[s] = ps.reshape(n, 4), vs.reshape(n, 4)
        eps2 = np.float32(0.1) * np.float32(0.1)
        _CLI_START[(n, b)] = (pos, vel, measure(gpu, pos, vel, np.float32, eps2), [ref_energy(pos[s], vel[s], float(eps2)) for s in range(b)])
    return _CLI_START[(n, b)]


@gpu_only
@pytest.mark.parametrize("run", list(CLI_RUNS))
def test_cli_prints_the_energies_of_every_ensemble_run(gpu, oracle, tmp_path, run):
    n, b, steps = 256, 3, 4
    out = tmp_path / "state.bin"
    r = subprocess.run([CLI, f"--systems={b}", f"--numbodies={n}", f"--steps={steps}", "--energies", f"--dump={out}", *CLI_RUNS[run]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    number = r"([-+.\deinfa]+)"
    start = re.search(r"^energies start: systems=(\d+) total_min=%s total_median=%s total_max=%s$" % (number, number, number), r.stdout, re.M)
    end = re.search(r"^energies end \((\d+ steps|t = \S+)\): worst_system=(\d+) relative_drift_max=%s relative_drift_rms=%s momentum_drift_max=%s not_finite=(\d+)$"
                    % (number, number, number), r.stdout, re.M)
    assert start and end, r.stdout[-1500:]
    assert r.stdout.index("energies start") < r.stdout.index("energies end")
    assert end.group(1) == (f"t = {steps * 0.016:g}" if "block" in run else f"{steps} steps")
    pos0, vel0, gpu0, ref0 = cli_start_state(gpu, oracle, n, b)
    close = lambda a, w, tol=1e-7: abs(a - w) <= tol * abs(w)  # noqa: E731
    totals = sorted(e["total"] for e in gpu0)
    assert int(start.group(1)) == b
    for text, want in zip(start.groups()[1:], (totals[0], totals[b // 2], totals[-1])):
        assert close(float(text), want), (text, want)
    for text, want in zip(start.groups()[1:], (lambda t: (t[0], t[b // 2], t[-1]))(sorted(e["total"] for e in ref0))):
        assert close(float(text), want, 5e-6), (text, want)
    # the dumped state, measured here
    data = np.fromfile(out, dtype=np.float32)
    assert data.size == 2 * 4 * n * b
    pos1, vel1 = data[:4 * n * b].reshape(b, n, 4), data[4 * n * b:].reshape(b, n, 4)
    eps2 = np.float32(0.1) * np.float32(0.1)
    gpu1 = measure(gpu, pos1, vel1, np.float32, eps2)
    for s in range(b):
        assert close(gpu1[s]["total"], ref_energy(pos1[s], vel1[s], float(eps2))["total"], 5e-6), s
    drifts = np.array([abs(e1["total"] - e0["total"]) / abs(e0["total"]) for e0, e1 in zip(gpu0, gpu1)])
    momenta = np.array([np.abs(np.array(e1["momentum"]) - np.array(e0["momentum"])).max() for e0, e1 in zip(gpu0, gpu1)])
    assert int(end.group(2)) == int(np.argmax(drifts)) and int(end.group(6)) == 0
    assert close(float(end.group(3)), drifts.max(), 1e-6) and close(float(end.group(4)), np.sqrt((drifts ** 2).mean()), 1e-6)
    assert close(float(end.group(5)), momenta.max(), 1e-6)
    assert drifts.max() > 0
    if run == "plain":  # --benchmark measures outside the timed region and still prints both lines
        r = subprocess.run([CLI, f"--systems={b}", f"--numbodies={n}", "--benchmark", "-i=3", "--energies"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and re.search(r"^energies end \(4 steps\): worst_system=\d+ ", r.stdout, re.M) and "energies start: systems=3" in r.stdout, r.stdout[-800:]


@gpu_only
def test_costs_no_more_than_an_ensemble_step_and_less_than_solo_calls(gpu):
    """1 024 bodies x 256 systems, fp32: one nb_energy_ensemble_f32 call against one FAST nb_ensemble_integrate_f32 step of the same batch
    and against 256 nb_energy_f32 calls back to back; medians of 5 event-timed calls after a warm-up"""
    lib, elib = gpu.lib(), gpu.energy_ensemble_lib()
    n, b = 1024, 256
    rng = np.random.default_rng(1024)
    pos = np.empty((b, n, 4), np.float32)
    pos[:, :, :3], pos[:, :, 3] = rng.uniform(-1, 1, (b, n, 3)), rng.uniform(0.5, 1.5, (b, n))
    vel = np.zeros((b, n, 4), np.float32)
    vel[:, :, :3] = rng.normal(0, 1, (b, n, 3))
    ensemble = gpu.BodyEnsembleHIP(n, b, np.float32, gpu.NB_MODE_FAST)
    ensemble.set_positions(pos), ensemble.set_velocities(vel)
    ws = gpu.DeviceBuffer(max(gpu.energy_ensemble_workspace_bytes(n, b), gpu.energy_workspace_bytes(n)))
    res = gpu.DeviceBuffer(104 * b)
    start, stop = gpu.Event(), gpu.Event()
    eps2 = np.float32(0.01)
    p, q, v = ensemble._pos[0].ptr, ensemble._pos[1].ptr, ensemble._vel.ptr

    def timed(call):
        call()  # warm-up
        gpu.check(lib.nb_device_synchronize())
        times = []
        for _ in range(5):
            start.record()
            call()
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_ms(stop))
        return float(np.median(times))

    def solo_calls():
        for s in range(b):
            off = s * 16 * n
            gpu.check(lib.nb_energy_f32(ctypes.c_void_p(p.value + off), ctypes.c_void_p(v.value + off), n, ws.ptr, ws.nbytes, ctypes.c_void_p(res.ptr.value + 104 * s), None))

    try:
        energy_ms = timed(lambda: gpu.check(elib.nb_energy_ensemble_f32(p, v, n, b, eps2, None, 1, ws.ptr, ws.nbytes, res.ptr, None)))
        batch = res.download(np.zeros(13 * b))
        step_ms = timed(lambda: gpu.check(gpu.ensemble_lib().nb_ensemble_integrate_f32(q, p, v, n, b, np.float32(0), np.float32(1), eps2, None, gpu.NB_MODE_FAST, None)))
        with Softening(gpu, np.float32, eps2):
            solo_ms = timed(solo_calls)
        solo = res.download(np.zeros(13 * b))
    finally:
        ensemble.free(), ws.free(), res.free()
    print(f"nb_energy_ensemble_f32 {energy_ms:.4f} ms, FAST ensemble step {step_ms:.4f} ms, ratio {energy_ms / step_ms:.3f}; "
          f"{b} nb_energy_f32 calls {solo_ms:.4f} ms, ratio {energy_ms / solo_ms:.4f}")
    assert np.abs(batch.reshape(b, 13)[:, 2] - solo.reshape(b, 13)[:, 2]).max() <= 1e-5 * np.abs(solo.reshape(b, 13)[:, 2]).min()
    assert energy_ms <= step_ms, (energy_ms, step_ms)
    assert energy_ms < solo_ms, (energy_ms, solo_ms)
