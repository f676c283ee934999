"""Ensembles: many independent systems of one size stepped in one launch (nb_ensemble_*, include/nbody_hip_ensemble.h;
libnbody_hip_ensemble.so from csrc/ensemble_*.hip).

CPU tests: the boundary (declared, exported, mirrored; the product library unchanged), host-side argument checks, the plan as a
function of N alone, and the FAST loop's instruction mix.  GPU tests: STRICT bit for bit against the CPU oracle, FAST against the
long double yardstick of tests/test_fast_domain.py, invariance of a system's bits under the batch, isolation of non-finite systems,
canaries, zero-mass padding, a batch past 4 GiB, the throughput against back-to-back single-system calls, and the Python class."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_capi_symbols import declared_symbols, exported_symbols
from test_fast_domain import check_step

ERR = 10001
MAX_N, MAX_TOTAL = 65536, 1 << 31
CSRC = os.path.join(ROOT, "cuda-nbody_amd", "csrc")


def fns(pkg, dtype):
    lib = pkg.ensemble_lib()
    if np.dtype(dtype) == np.float32:
        return lib.nb_ensemble_integrate_f32, lib.nb_ensemble_plan_f32, np.float32
    return lib.nb_ensemble_integrate_f64, lib.nb_ensemble_plan_f64, float


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_ensemble_header_library_and_binding_agree(pkg):
    declared = declared_symbols("nbody_hip_ensemble.h")
    assert declared == ["nb_ensemble_integrate_f32", "nb_ensemble_integrate_f64", "nb_ensemble_plan_f32", "nb_ensemble_plan_f64"]
    assert exported_symbols(pkg.ENSEMBLE_LIB_PATH) == declared
    assert sorted(pkg.ENSEMBLE_SIGNATURES) == declared
    # the product library is untouched: still exactly its two headers, 96 symbols, none of the ensemble's
    assert len(exported_symbols(pkg.LIB_PATH)) == 96
    assert not set(declared) & set(exported_symbols(pkg.LIB_PATH))
    # and the ensemble library does not link it
    needed = subprocess.run(["readelf", "-d", pkg.ENSEMBLE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnbody_hip" not in needed


def test_ensemble_plan_mirror_matches_the_header(pkg):
    text = open(os.path.join(ROOT, "include", "nbody_hip_ensemble.h")).read()
    body = re.search(r"typedef struct nb_ensemble_plan \{.*?\*/(.*?)\} nb_ensemble_plan_t;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int|unsigned long long|unsigned)\s+(\w+);", body)
    assert [f for _, f in fields] == [f for f, _ in pkg.EnsemblePlan._fields_]
    sizes = {"int": 4, "unsigned": 4, "unsigned long long": 8}
    for (ctype, name), (_, pytype) in zip(fields, pkg.EnsemblePlan._fields_):
        assert ctypes.sizeof(pytype) == sizes[ctype], name
    assert ctypes.sizeof(pkg.EnsemblePlan) == 32


def test_ensemble_argument_errors_are_caught_on_the_host(pkg):
    """Nothing here reaches HIP: every call is refused before a launch (the addresses are never dereferenced)."""
    for dtype in (np.float32, np.float64):
        fn, _, scalar = fns(pkg, dtype)
        size = np.dtype(dtype).itemsize
        n, b = 1024, 8
        span = 4 * n * b * size
        new, old, vel, par = 0x100000000, 0x200000000, 0x300000000, 0x400000000
        ok = dict(new=new, old=old, vel=vel, n=n, b=b, par=par, mode=1)

        def call(**kw):
            a = {**ok, **kw}
            return fn(a["new"], a["old"], a["vel"], a["n"], a["b"], scalar(0.01), scalar(1.0), scalar(0.01), a["par"], a["mode"], None)

        for null in ("new", "old", "vel"):
            assert call(**{null: None}) == ERR, null
        for bad in (dict(n=0), dict(n=MAX_N + 1), dict(b=0), dict(n=MAX_N, b=MAX_TOTAL // MAX_N + 1), dict(n=3, b=MAX_TOTAL // 3 + 1)):
            assert call(**bad) == ERR, bad
        for mode in (-1, 2, 7):
            assert call(mode=mode) == ERR, mode
        for name in ("new", "old", "vel", "par"):
            assert call(**{name: ok[name] + 4 * size // 2}) == ERR, f"{name} misaligned"
        assert call(new=old) == ERR
        assert call(new=old + span - 4 * size) == ERR           # new on the last body of old
        assert call(new=vel + 4 * size) == ERR                  # new inside the velocities
        assert call(vel=old - span + 4 * size) == ERR           # velocities running into old
        for name in ("new", "old", "vel"):
            assert call(par=ok[name] + span - 4 * size) == ERR, f"params inside {name}"
            assert call(par=ok[name] - 4 * b * size + 4 * size) == ERR, f"params running into {name}"


def test_ensemble_plan_is_a_function_of_n_alone(pkg):
    """Across N = 1 .. 65 536 every plan field but grid_blocks is the same for every B that keeps N*B <= 2^31; the query refuses
    what the step refuses."""
    sizes = sorted({1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 1000, 1023, 1024, 1025, 2085, 4096, 16384, 16385, 32768, 65535, 65536})
    for dtype in (np.float32, np.float64):
        _, plan_fn, _ = fns(pkg, dtype)
        for n in sizes:
            plans = []
            for b in (1, 2, 7, 1000, 1 << 20):
                if n * b > MAX_TOTAL:
                    p = pkg.EnsemblePlan()
                    assert plan_fn(n, b, ctypes.byref(p)) == ERR, (n, b)
                    continue
                p = pkg.ensemble_plan(n, b, dtype)
                assert p.grid_blocks == p.groups_per_system * b
                plans.append(tuple(getattr(p, f) for f, _ in pkg.EnsemblePlan._fields_ if f != "grid_blocks"))
            assert len(set(plans)) == 1, (n, plans)
            I, S, groups, threads, lds, _ = (*plans[0], None)
            assert threads == 64 * S and groups == -(-n // (64 * I)) and lds <= 64 * 1024
            assert I <= 4 and (dtype == np.float64 or I % 2 == 0)
            if n >= 128:
                assert n // S >= 128, (n, S)  # every wave streams at least one chunk of 128 bodies j
            if 256 <= n <= 16384:
                assert S >= I, (n, S, I)       # 262 144 bodies in all: 4 096 S / I >= 4 096 waves, 4 per SIMD
        p = pkg.EnsemblePlan()
        for n, b in ((0, 1), (MAX_N + 1, 1), (1, 0), (MAX_N, MAX_TOTAL // MAX_N + 1)):
            assert plan_fn(n, b, ctypes.byref(p)) == ERR, (n, b)
        assert plan_fn(16, 1, None) == ERR


def test_ensemble_fast_loops_keep_the_one_sided_mix():
    """fp32 unit-mass loops of every FAST ensemble kernel: 11 v_pk_* and 2 v_rsq_f32 per packed pair, no LDS instruction and no
    barrier in the loop; no ensemble kernel uses scratch or more than 128 VGPRs."""
    subprocess.run(["make", "-s", "-C", CSRC, "ensemble_fast.s", "ensemble_strict.s"], check=True, capture_output=True)
    text = open(os.path.join(CSRC, "ensemble_fast.s")).read()
    lines = text.split("\n")
    kernels = re.findall(r"^(_ZN2nb12_GLOBAL__N_113ensemble_fastIfLi\d+ELi\d+EEEvNS_12EnsembleArgsIT_EE):", text, re.M)
    assert len(kernels) == 4, kernels
    for kernel in kernels:
        start = next(i for i, l in enumerate(lines) if l.startswith(kernel + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        unit = []
        for i in range(start, end):
            if "Inner Loop Header" not in lines[i]:
                continue
            label = lines[i - 1].split(":")[0].strip()
            stop = next((k for k in range(i, end) if ("s_cbranch" in lines[k] or "s_branch" in lines[k]) and label in lines[k]), None)
            if stop is None:
                continue
            body = [l.strip() for l in lines[i + 1:stop]]
            count = lambda prefix: sum(1 for l in body if l.startswith(prefix))  # noqa: E731
            if count("v_rsq_f32") == 32 and count("v_pk_") == 11 * 16:  # a streaming loop of 16 packed pairs, no mass multiply
                unit.append((count("ds_"), count("s_barrier"), count("scratch_"), count("s_load")))
        assert unit, kernel
        for lds, barriers, scratch, loads in unit:
            assert lds == 0 and barriers == 0 and scratch == 0 and loads >= 2, (kernel, unit)
        # ... and the only v_pk_* counts of its streaming loops are 11 (unit / species) and 12 (mixed) per packed pair
    for name in ("ensemble_fast.s", "ensemble_strict.s"):
        t = open(os.path.join(CSRC, name)).read()
        sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", t)]
        vgprs = [int(m) for m in re.findall(r"\.vgpr_count:\s+(\d+)", t)]
        assert sizes and max(sizes) == 0, (name, sizes)
        assert vgprs and max(vgprs) <= 128, (name, vgprs)


# ---------------------------------------------------------------------------------------------------------------- GPU
gpu_only = pytest.mark.gpu


def T(dtype, x):
    return np.dtype(dtype).type(np.float32(x))


def eps2_of(dtype, softening):
    s = T(dtype, softening)
    return s * s


def step(pkg, pos, vel, mode, dt=0.016, damping=1.0, softening=0.1, params=None, steps=1):
    """`steps` ensemble steps of the (B, N, 4) arrays through the C calls; returns the (B, N, 4) results"""
    dtype = pos.dtype
    B, N, _ = pos.shape
    fn, _, scalar = fns(pkg, dtype)
    bufs = [pkg.DeviceBuffer(pos.nbytes) for _ in range(3)]
    bufs[0].upload(np.ascontiguousarray(pos))
    bufs[2].upload(np.ascontiguousarray(vel))
    pbuf = None
    if params is not None:
        params = np.ascontiguousarray(params, dtype=dtype)
        pbuf = pkg.DeviceBuffer(params.nbytes)
        pbuf.upload(params)
    read = 0
    for _ in range(steps):
        rc = fn(bufs[1 - read].ptr, bufs[read].ptr, bufs[2].ptr, N, B, scalar(T(dtype, dt)), scalar(T(dtype, damping)),
                scalar(eps2_of(dtype, softening)), pbuf.ptr if pbuf else None, mode, None)
        pkg.check(rc, "nb_ensemble_integrate")
        read = 1 - read
    out = bufs[read].download(np.empty_like(pos)), bufs[2].download(np.empty_like(vel))
    for b in bufs + ([pbuf] if pbuf else []):
        b.free()
    return out


def systems(oracle, dtype, n, count, seed0=11):
    """`count` systems of n bodies from different seeds and the three configurations, as (B, N, 4) arrays"""
    pos, vel = np.empty((count, n, 4), dtype), np.empty((count, n, 4), dtype)
    for s in range(count):
        oracle.srand(seed0 + 17 * s)
        p, v = oracle.randomise(s % 3, n, 1.54 if s % 2 else 0.68, 8.0 if s % 2 else 20.0, dtype)
        pos[s], vel[s] = p.reshape(n, 4), v.reshape(n, 4)
    return pos, vel


def oracle_steps(oracle, pos, vel, steps, dt=0.016, damping=1.0, softening=0.1):
    p, v = pos.reshape(-1).copy(), vel.reshape(-1).copy()
    oracle.update(p, v, dt, steps=steps, softening=softening, damping=damping)
    return p.reshape(pos.shape), v.reshape(vel.shape)


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,b", [(1, 7), (63, 7), (1024, 1), (1024, 7), (2085, 7)])
def test_strict_every_system_matches_the_oracle(gpu, oracle, dtype, n, b):
    pos, vel = systems(oracle, dtype, n, b)
    for steps in (1, 10):
        got_pos, got_vel = step(gpu, pos, vel, gpu.NB_MODE_STRICT, steps=steps)
        for s in range(b):
            want_pos, want_vel = oracle_steps(oracle, pos[s], vel[s], steps)
            assert got_pos[s].tobytes() == want_pos.tobytes(), (steps, s)
            assert got_vel[s].tobytes() == want_vel.tobytes(), (steps, s)


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_strict_demo_rows_through_system_params(gpu, oracle, dtype):
    n = 1024
    pos, vel = np.empty((7, n, 4), dtype), np.empty((7, n, 4), dtype)
    table = np.zeros((7, 4), dtype)
    for row, prm in enumerate(gpu.DEMO_PARAMS):
        oracle.srand(100 + row)
        p, v = oracle.randomise(row % 3, n, prm.cluster_scale, prm.velocity_scale, dtype)
        pos[row], vel[row] = p.reshape(n, 4), v.reshape(n, 4)
        table[row] = (T(dtype, prm.time_step), T(dtype, prm.damping), eps2_of(dtype, prm.softening), 0)
    got_pos, got_vel = step(gpu, pos, vel, gpu.NB_MODE_STRICT, dt=1.0, damping=0.5, softening=3.0, params=table, steps=3)
    for row, prm in enumerate(gpu.DEMO_PARAMS):
        want_pos, want_vel = oracle_steps(oracle, pos[row], vel[row], 3, dt=prm.time_step, damping=prm.damping, softening=prm.softening)
        assert got_pos[row].tobytes() == want_pos.tobytes(), row
        assert got_vel[row].tobytes() == want_vel.tobytes(), row


def reference_mass_systems(oracle, dtype, n=1024):
    exps = (20, -20, 21, -21, 40, -40) if dtype == np.float32 else (60, -60, 61, -61)
    pos, vel = systems(oracle, dtype, n, len(exps), seed0=5)
    pos[..., 3] = np.linspace(0.5, 2.0, n).astype(dtype)
    for s, e in enumerate(exps):
        pos[s, 0, 3] = dtype(2.0 ** e)
    return pos, vel


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,b", [(1, 7), (63, 7), (1024, 7), (2085, 7), ("mass", None)])
def test_fast_every_system_within_the_yardstick(gpu, oracle, dtype, n, b):
    if n == "mass":
        pos, vel = reference_mass_systems(oracle, dtype)
    else:
        pos, vel = systems(oracle, dtype, n, b)
    dt, damping = 0.016, 0.995
    got_pos, got_vel = step(gpu, pos, vel, gpu.NB_MODE_FAST, dt=dt, damping=damping)
    for s in range(pos.shape[0]):
        check_step(got_pos[s].reshape(-1), got_vel[s].reshape(-1), pos[s].reshape(-1), vel[s].reshape(-1), T(dtype, dt), T(dtype, damping),
                   eps2_of(dtype, 0.1), f"system {s}")


@gpu_only
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_systems_bits_do_not_depend_on_the_batch(gpu, oracle, dtype, mode):
    for n in (63, 1024):
        pos, vel = systems(oracle, dtype, n, 7, seed0=3)
        alone = step(gpu, pos[3:4], vel[3:4], mode)
        batch = step(gpu, pos, vel, mode)
        again = step(gpu, pos, vel, mode)
        assert batch[0].tobytes() == again[0].tobytes() and batch[1].tobytes() == again[1].tobytes()
        moved_pos, moved_vel = pos[::-1].copy(), vel[::-1].copy()  # the system at another index, other neighbours
        moved_pos[0], moved_vel[0] = pos[6] * 2, vel[6]
        moved = step(gpu, moved_pos, moved_vel, mode)
        big_pos, big_vel = np.tile(pos[:1], (1000, 1, 1)), np.tile(vel[:1], (1000, 1, 1))
        big_pos[999], big_vel[999] = pos[3], vel[3]
        big = step(gpu, big_pos, big_vel, mode)
        for where, got in (("in the batch", (batch[0][3:4], batch[1][3:4])), ("moved", (moved[0][3:4], moved[1][3:4])), ("B = 1 000", (big[0][999:], big[1][999:]))):
            assert got[0].tobytes() == alone[0].tobytes() and got[1].tobytes() == alone[1].tobytes(), (n, where)
        assert big[0][0].tobytes() == batch[0][0].tobytes()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nonfinite_system_leaves_the_others_alone(gpu, oracle, dtype):
    n = 1024
    pos, vel = systems(oracle, dtype, n, 5, seed0=29)
    clean = {m: step(gpu, pos, vel, m) for m in (0, 1)}
    bad_pos, bad_vel = pos.copy(), vel.copy()
    bad_pos[1, 10, 0] = np.nan
    bad_pos[3, 0, 3] = np.inf
    bad_vel[4, 7, 2] = np.nan
    with np.errstate(all="ignore"):
        got = {m: step(gpu, bad_pos, bad_vel, m) for m in (0, 1)}
    for m in (0, 1):
        for s in (0, 2):
            assert got[m][0][s].tobytes() == clean[m][0][s].tobytes() and got[m][1][s].tobytes() == clean[m][1][s].tobytes(), (m, s)
    nonfinite = {m: ~(np.isfinite(got[m][0][..., :3]).all(-1) & np.isfinite(got[m][1][..., :3]).all(-1)) for m in (0, 1)}
    assert np.array_equal(nonfinite[0], nonfinite[1])
    assert nonfinite[0][1].all() and nonfinite[0][3].all() and nonfinite[0][4].sum() == 1


@gpu_only
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ensemble_writes_only_its_own_bytes(gpu, oracle, dtype, mode):
    n, b, pad = 63, 7, 64  # (pad bodies of canary before and after every array)
    fn, _, scalar = fns(gpu, dtype)
    pos, vel = systems(oracle, dtype, n, b, seed0=41)
    vel[..., 3] = np.arange(n * b, dtype=dtype).reshape(b, n) + dtype(0.25)
    table = np.tile(np.array([T(dtype, 0.0), T(dtype, 1.0), eps2_of(dtype, 0.1), 0], dtype), (b, 1))
    table[::2, 0] = T(dtype, 0.016)
    canary = np.full(4 * pad, 1234.5, dtype)
    arrays = [pos, np.zeros_like(pos), vel, table]
    bufs = []
    for a in arrays:
        host = np.concatenate([canary, a.reshape(-1), canary])
        buf = gpu.DeviceBuffer(host.nbytes)
        buf.upload(host)
        bufs.append((buf, host))
    ptr = lambda k: bufs[k][0].ptr.value + 4 * pad * np.dtype(dtype).itemsize  # noqa: E731
    gpu.check(fn(ptr(1), ptr(0), ptr(2), n, b, scalar(0), scalar(0), scalar(0), ptr(3), mode, None), "nb_ensemble_integrate")
    out = [buf.download(np.empty_like(host)) for buf, host in bufs]
    for k, (o, (_, host)) in enumerate(zip(out, bufs)):
        assert o[:4 * pad].tobytes() == canary.tobytes() and o[-4 * pad:].tobytes() == canary.tobytes(), k
    assert out[0].tobytes() == bufs[0][1].tobytes()  # old positions unchanged
    assert out[3].tobytes() == bufs[3][1].tobytes()  # the parameters too
    new_pos = out[1][4 * pad:-4 * pad].reshape(b, n, 4)
    new_vel = out[2][4 * pad:-4 * pad].reshape(b, n, 4)
    assert new_vel[..., 3].tobytes() == vel[..., 3].tobytes()
    assert new_pos[..., 3].tobytes() == pos[..., 3].tobytes()
    assert np.isfinite(new_pos).all() and np.isfinite(new_vel).all()
    assert new_pos[1::2].tobytes() == pos[1::2].tobytes()  # dt = 0: positions stay where they are
    for buf, _ in bufs:
        buf.free()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_mass_padding_leaves_the_real_bodies_bit_identical(gpu, oracle, dtype):
    real, padded = 1000, 1024
    pos, vel = systems(oracle, dtype, real, 3, seed0=61)
    ppos, pvel = np.zeros((3, padded, 4), dtype), np.zeros((3, padded, 4), dtype)
    ppos[:, :real], pvel[:, :real] = pos, vel
    ppos[:, real:, 0] = np.linspace(50, 60, padded - real).astype(dtype)
    ppos[:, real:, 3] = 0
    for steps in (1, 5):
        a = step(gpu, pos, vel, gpu.NB_MODE_STRICT, steps=steps)
        b = step(gpu, ppos, pvel, gpu.NB_MODE_STRICT, steps=steps)
        assert b[0][:, :real].tobytes() == a[0].tobytes() and b[1][:, :real].tobytes() == a[1].tobytes(), steps


@gpu_only
def test_strict_batch_past_4_gib(gpu, oracle):
    """N = 1 024, B = 262 145 fp32: 4 GiB + 16 KiB per array; the first and the last system both equal the oracle."""
    n, b = 1024, 262145
    itemsize = 4
    span = 4 * n * b * itemsize
    assert span > 1 << 32
    pos, vel = systems(oracle, np.float32, n, 2, seed0=71)
    bufs = [gpu.DeviceBuffer(span) for _ in range(3)]  # (cleared: the systems in between are all bodies at the origin)
    try:
        last = 4 * n * (b - 1) * itemsize
        lib = gpu.lib()
        for s, off in ((0, 0), (1, last)):
            gpu.check(lib.nb_h2d(bufs[0].ptr.value + off, pos[s].ctypes.data, pos[s].nbytes, None), "nb_h2d")
            gpu.check(lib.nb_h2d(bufs[2].ptr.value + off, vel[s].ctypes.data, vel[s].nbytes, None), "nb_h2d")
        gpu.check(gpu.ensemble_lib().nb_ensemble_integrate_f32(bufs[1].ptr, bufs[0].ptr, bufs[2].ptr, n, b, np.float32(0.016), np.float32(1.0),
                                                               eps2_of(np.float32, 0.1), None, gpu.NB_MODE_STRICT, None), "nb_ensemble_integrate")
        for s, off in ((0, 0), (1, last)):
            got_pos, got_vel = np.empty_like(pos[s]), np.empty_like(vel[s])
            gpu.check(lib.nb_d2h(got_pos.ctypes.data, bufs[1].ptr.value + off, got_pos.nbytes, None), "nb_d2h")
            gpu.check(lib.nb_d2h(got_vel.ctypes.data, bufs[2].ptr.value + off, got_vel.nbytes, None), "nb_d2h")
            want_pos, want_vel = oracle_steps(oracle, pos[s], vel[s], 1)
            assert got_pos.tobytes() == want_pos.tobytes() and got_vel.tobytes() == want_vel.tobytes(), s
    finally:
        for buf in bufs:
            buf.free()


@gpu_only
def test_one_ensemble_step_beats_back_to_back_single_steps(gpu, oracle):
    """B = 256, N = 1 024, fp32 FAST: one ensemble step at least 5x faster than 256 nb_integrate_f32 calls on one stream."""
    n, b = 1024, 256
    pos, vel = systems(oracle, np.float32, n, 4, seed0=83)
    pos, vel = np.tile(pos, (b // 4, 1, 1)), np.tile(vel, (b // 4, 1, 1))
    bufs = [gpu.DeviceBuffer(pos.nbytes) for _ in range(3)]
    bufs[0].upload(pos)
    bufs[2].upload(vel)
    lib, ens = gpu.lib(), gpu.ensemble_lib()
    gpu.check(lib.nb_set_softening_sq_f32(eps2_of(np.float32, 0.1)), "nb_set_softening_sq_f32")
    stride = 4 * n * 4
    eps2 = eps2_of(np.float32, 0.1)

    def ensemble():
        gpu.check(ens.nb_ensemble_integrate_f32(bufs[1].ptr, bufs[0].ptr, bufs[2].ptr, n, b, np.float32(0.016), np.float32(1.0), eps2, None, 1, None), "ens")

    def singles():
        for s in range(b):
            gpu.check(lib.nb_integrate_f32(bufs[1].ptr.value + s * stride, bufs[0].ptr.value + s * stride, bufs[2].ptr.value + s * stride,
                                           np.float32(0.016), np.float32(1.0), n, 256, 1, None), "single")

    def timed(fn, reps):
        fn()
        start, stop = gpu.Event(), gpu.Event()
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_ms(stop) / reps

    t_single = min(timed(singles, 5) for _ in range(2))
    t_ens = min(timed(ensemble, 50) for _ in range(2))
    print(f"ensemble step {t_ens * 1e3:.1f} us, 256 single steps {t_single * 1e3:.1f} us: {t_single / t_ens:.1f}x")
    for buf in bufs:
        buf.free()
    assert t_single >= 5 * t_ens, (t_ens, t_single)


@gpu_only
@pytest.mark.parametrize("mode", [0, 1])
def test_python_class_gives_the_c_calls_bits(gpu, oracle, mode):
    for dtype in (np.float32, np.float64):
        n, b = 300, 5
        pos, vel = systems(oracle, dtype, n, b, seed0=91)
        table = np.tile(np.array([T(dtype, 0.01), T(dtype, 0.99), eps2_of(dtype, 0.2), 0], dtype), (b, 1))
        want = step(gpu, pos, vel, mode, steps=3, params=table)
        ens = gpu.BodyEnsembleHIP(n, b, dtype, mode)
        ens.set_positions(pos)
        ens.set_velocities(vel)
        for _ in range(3):
            ens.update(0.5, 0.5, 1.0, params=table)
        got = ens.get_positions(), ens.get_velocities()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        want = step(gpu, pos, vel, mode, dt=0.016, damping=1.0, softening=0.1, steps=2)
        ens.set_positions(pos)
        ens.set_velocities(vel)
        for _ in range(2):
            ens.update(T(dtype, 0.016), T(dtype, 1.0), eps2_of(dtype, 0.1))
        got = ens.get_positions(), ens.get_velocities()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        ens.free()


# ---------------------------------------------------------------------------------------------------------------- CLI
CLI = os.path.join(ROOT, "cuda-nbody_amd", "nbody")


def test_cli_rejects_what_an_ensemble_cannot_do(tmp_path):
    tipsy = tmp_path / "model.tipsy"
    tipsy.write_bytes(b"\0" * 64)
    base = ["--systems=3", "--numbodies=1024", "--steps=1"]
    for extra in (["--systems=0", "--numbodies=1024", "--steps=1"], ["--systems=3", "--steps=1"], ["--systems=3", "--numbodies=65537", "--steps=1"],
                  base + ["--numdevices=2"], base + ["--devices=0,1"], base + ["--hostmem"], base + [f"--tipsy={tipsy}"], base + ["--compare"],
                  base + ["--qatest"], base + ["--graph"], base + ["--energy"], base + ["--no-workspace"], base + ["--workspace-mib=64"]):
        r = subprocess.run([CLI, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr, (extra, r.returncode, r.stderr[:300])
    r = subprocess.run([CLI, "--systems=3", "--steps=1"], capture_output=True, text=True, timeout=60)
    assert "--numbodies" in r.stderr and "65536" in r.stderr


@gpu_only
def test_cli_systems_dump_and_benchmark(gpu, oracle, tmp_path):
    n, b, steps = 1024, 3, 10
    ens, one = tmp_path / "ens.bin", tmp_path / "one.bin"
    r = subprocess.run([CLI, f"--systems={b}", f"--numbodies={n}", "--mode=strict", f"--steps={steps}", f"--dump={ens}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([CLI, f"--numbodies={n}", "--mode=strict", f"--steps={steps}", f"--dump={one}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    data = np.fromfile(ens, dtype=np.float32)
    assert data.size == 2 * 4 * n * b
    pos, vel = data[:4 * n * b].reshape(b, n, 4), data[4 * n * b:].reshape(b, n, 4)
    single = np.fromfile(one, dtype=np.float32)
    assert pos[0].tobytes() == single[:4 * n].tobytes() and vel[0].tobytes() == single[4 * n:].tobytes()
    # systems 1 and 2: the next two draws after the start-up state, stepped by the oracle
    oracle.startup_state(n, np.float32)
    from oracle import scales_for
    c, v = scales_for(n)
    for s in (1, 2):
        p0, v0 = oracle.randomise(1, n, c, v, np.float32)
        oracle.update(p0, v0, 0.016, steps=steps)
        assert pos[s].tobytes() == p0.tobytes() and vel[s].tobytes() == v0.tobytes(), s
    r = subprocess.run([CLI, f"--systems={b}", f"--numbodies={n}", "--benchmark", "-i=20"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"^(\d+) bodies x (\d+) systems, total time for (\d+) iterations: ([\d.]+) ms\n= ([\d.]+) billion interactions per second\n= ([\d.]+) single-precision GFLOP/s at 20 flops", r.stdout, re.M)
    assert m, r.stdout[-600:]
    got_n, got_b, iters, ms, ips, gflops = int(m[1]), int(m[2]), int(m[3]), float(m[4]), float(m[5]), float(m[6])
    assert (got_n, got_b, iters) == (n, b, 20)
    want = b * n * n * iters / (ms * 1e-3) * 1e-9
    assert abs(ips - want) <= 0.01 * want + 0.002, (ips, want)
    assert abs(gflops - 20 * ips) <= 0.01 * gflops + 0.02
