"""4th-order Hermite steps (nb_hermite_*, include/nbody_hip_hermite.h; libnbody_hip_hermite.so from csrc/hermite_*.hip).

CPU tests: the boundary (declared, exported, mirrored; the other libraries unchanged), host-side argument checks, the plan as a
function of N alone, the instruction mix of the fp32 streaming loops.  GPU tests: accelerations and jerks against long double sums

    a_i    = sum_j m_j s^-3 r,   jerk_i = sum_j m_j s^-3 (w - 3 (r.w) s^-2 r),   r = x_j - x_i, w = v_j - v_i, s^2 = r.r + eps^2

per body and component to tol A_i / tol J_i, A = sum m s^-3 |r_k|, J = sum m s^-3 (|w_k| + 3 (sum_c |r_c w_c|) s^-2 |r_k|), tol the
FAST force tolerance of tests/test_fast_domain.py (5e-6 fp32, 1e-14 fp64); one step against the long double P(EC)^1 step from the same
inputs; the order of the scheme on a two-body orbit and a 256-body cloud; energy through nb_energy_f64 against the first-order
step; invariants (bits, in place, dt = 0, canaries, capture); the shared time step; the Python class; a speed sanity bound."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_capi_symbols import declared_symbols, exported_symbols
from test_fast_domain import TOL, UNIT_ROUNDOFF

ERR = 10001
MAX_N = 1 << 26
CSRC = os.path.join(ROOT, "cuda-nbody_amd", "csrc")
SYMBOLS = ["nb_hermite_eval_f32", "nb_hermite_eval_f64", "nb_hermite_plan_f32", "nb_hermite_plan_f64", "nb_hermite_step_f32", "nb_hermite_step_f64",
           "nb_hermite_timestep_f32", "nb_hermite_timestep_f64", "nb_hermite_workspace_bytes"]
# what the compiler delivers for the fp32 streaming loops, per packed pair of interactions
PK_UNIT, PK_MIXED, RSQ = 25, 26, 2
# issue cycles with 3-4 runnable waves per SIMD (docs/history.md: packed fp32 op 4.08, v_rsq_f32 8.3; the one-sided step: 11 + 2 = 61.5)
PK_CYCLES, RSQ_CYCLES = 4.08, 8.3
ISSUE_MODEL = (PK_UNIT * PK_CYCLES + RSQ * RSQ_CYCLES) / (11 * PK_CYCLES + 2 * RSQ_CYCLES)


def fns(pkg, dtype):
    lib = pkg.hermite_lib()
    sfx = "f32" if np.dtype(dtype) == np.float32 else "f64"
    scalar = np.float32 if sfx == "f32" else float
    return {name: getattr(lib, f"nb_hermite_{name}_{sfx}") for name in ("eval", "step", "timestep", "plan")}, scalar


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_hermite_header_library_and_binding_agree(pkg):
    declared = declared_symbols("nbody_hip_hermite.h")
    assert declared == SYMBOLS
    assert exported_symbols(pkg.HERMITE_LIB_PATH) == declared
    assert sorted(pkg.HERMITE_SIGNATURES) == declared
    # the other libraries are untouched: the product still exports its 96 symbols, the ensemble library its 4, none of them ours
    assert len(exported_symbols(pkg.LIB_PATH)) == 96
    assert len(exported_symbols(pkg.ENSEMBLE_LIB_PATH)) == 4
    assert not set(declared) & (set(exported_symbols(pkg.LIB_PATH)) | set(exported_symbols(pkg.ENSEMBLE_LIB_PATH)))
    needed = subprocess.run(["readelf", "-d", pkg.HERMITE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnbody_hip" not in needed


def test_hermite_plan_mirror_and_constants_match_the_header(pkg):
    text = open(os.path.join(ROOT, "include", "nbody_hip_hermite.h")).read()
    body = re.search(r"typedef struct nb_hermite_plan \{.*?\*/(.*?)\} nb_hermite_plan_t;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int|unsigned)\s+(\w+);", body)
    assert [f for _, f in fields] == [f for f, _ in pkg.HermitePlan._fields_]
    assert ctypes.sizeof(pkg.HermitePlan) == 24
    assert re.search(r"#define NB_HERMITE_MAX_BODIES \(1u << 26\)", text) and pkg.HERMITE_MAX_BODIES == MAX_N
    assert int(re.search(r"#define NB_HERMITE_TIMESTEP_SCRATCH_BYTES (\d+)", text).group(1)) == pkg.HERMITE_TIMESTEP_SCRATCH_BYTES


def test_hermite_argument_errors_are_caught_on_the_host(pkg):
    """Everything refused here is refused before a HIP call (the addresses are never dereferenced); new == old is NOT refused by
    the argument check -- without a GPU that call then answers a HIP error, with one it would run, so it is only made without."""
    lib = pkg.hermite_lib()
    out = ctypes.c_size_t(0)
    assert lib.nb_hermite_workspace_bytes(1000, 4, ctypes.byref(out)) == 0 and out.value == 32000
    assert lib.nb_hermite_workspace_bytes(1000, 8, ctypes.byref(out)) == 0 and out.value == 64000
    for bad in ((0, 4), (MAX_N + 1, 4), (1000, 2), (1000, 16)):
        assert lib.nb_hermite_workspace_bytes(*bad, ctypes.byref(out)) == ERR, bad
    assert lib.nb_hermite_workspace_bytes(1000, 4, None) == ERR
    count = ctypes.c_int(0)
    no_gpu = pkg.lib().nb_device_count(ctypes.byref(count)) != 0 or count.value == 0
    for dtype in (np.float32, np.float64):
        f, scalar = fns(pkg, dtype)
        size = np.dtype(dtype).itemsize
        n = 1024
        span = 4 * n * size
        ok = dict(new=0x100000000, old=0x200000000, vel=0x300000000, acc=0x400000000, jerk=0x500000000, ws=0x600000000, ws_bytes=2 * span, n=n)
        names = ("new", "old", "vel", "acc", "jerk", "ws")

        def step(**kw):
            a = {**ok, **kw}
            return f["step"](a["new"], a["old"], a["vel"], a["acc"], a["jerk"], a["ws"], a["ws_bytes"], a["n"], scalar(0.01), scalar(0.01), None)

        for null in names:
            assert step(**{null: None}) == ERR, null
        assert step(new=None, old=None) == ERR
        for bad in (dict(n=0), dict(n=MAX_N + 1), dict(ws_bytes=2 * span - 1), dict(ws_bytes=0)):
            assert step(**bad) == ERR, bad
        for name in names:
            assert step(**{name: ok[name] + 2 * size}) == ERR, f"{name} misaligned"
        for x in names:  # every pair of arrays, overlapping by one body at either end
            for y in names:
                if x == y:
                    continue
                len_y = 2 * span if y == "ws" else span
                len_x = 2 * span if x == "ws" else span
                assert step(**{x: ok[y] + len_y - 4 * size}) == ERR, (x, "on the last body of", y)
                assert step(**{x: ok[y] - len_x + 4 * size}) == ERR, (x, "running into", y)
                if {x, y} != {"new", "old"}:
                    assert step(**{x: ok[y]}) == ERR, (x, "==", y)
        assert step(new=ok["old"] + 4 * size) == ERR  # new and old may be the SAME array, not shifted ones
        if no_gpu:
            assert step(new=ok["old"]) not in (0, ERR)  # past the argument check: a HIP error

        def evaluate(**kw):
            a = {**ok, **kw}
            return f["eval"](a["acc"], a["jerk"], a["old"], a["vel"], a["n"], scalar(0.01), None)

        for null in ("acc", "jerk", "old", "vel"):
            assert evaluate(**{null: None}) == ERR, null
            assert evaluate(**{null: ok[null] + 2 * size}) == ERR, null
        for bad in (dict(n=0), dict(n=MAX_N + 1), dict(acc=ok["old"]), dict(jerk=ok["vel"] + span - 4 * size), dict(acc=ok["jerk"]), dict(old=ok["vel"])):
            assert evaluate(**bad) == ERR, bad

        def timestep(**kw):
            a = {"dt": 0x700000000, "scratch": 0x800000000, "bytes": 8192, **ok, **kw}
            return f["timestep"](a["acc"], a["jerk"], a["n"], scalar(0.02), a["dt"], a["scratch"], a["bytes"], None)

        for bad in (dict(acc=None), dict(jerk=None), dict(dt=None), dict(scratch=None), dict(n=0), dict(n=MAX_N + 1), dict(bytes=8191), dict(dt=0x700000000 + size // 2),
                    dict(scratch=0x800000004), dict(acc=ok["acc"] + 2 * size), dict(dt=ok["acc"] + 4 * size), dict(scratch=ok["jerk"]), dict(acc=ok["jerk"])):
            assert timestep(**bad) == ERR, bad


def test_hermite_plan_is_a_function_of_n_alone(pkg):
    sizes = sorted({1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 1000, 1023, 1024, 1025, 2085, 4096, 16384, 16385, 32768, 65535, 65536})
    for dtype in (np.float32, np.float64):
        f, _ = fns(pkg, dtype)
        W = 2 if dtype == np.float32 else 1
        for n in sizes + [262144, MAX_N]:
            plans = set()
            for _ in range(3):
                p = pkg.hermite_plan(n, dtype)
                plans.add(tuple(getattr(p, name) for name, _ in pkg.HermitePlan._fields_))
            assert len(plans) == 1
            I, S, U, groups, threads, lds = plans.pop()
            assert I == W and U == (4 if dtype == np.float32 else 2) and S in (1, 2, 4, 8)
            assert threads == 64 * S and groups == -(-n // (64 * I)) and lds <= 64 * 1024
            assert S == 8 or 2 * S * 128 > n
            if n >= 128:
                assert n // S >= 128, (n, S)  # every wave streams at least one chunk of 128 bodies j
        p = pkg.HermitePlan()
        for n in (0, MAX_N + 1):
            assert f["plan"](n, ctypes.byref(p)) == ERR, n
        assert f["plan"](16, None) == ERR


def kernels_of(text):
    lines = text.split("\n")
    for i, line in enumerate(lines):
        m = re.match(r"^(_ZN2nb12_GLOBAL__N_1\d+hermite_\w+):", line)
        if m:
            end = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            yield m.group(1), lines[i:end]


def test_hermite_streaming_loops_keep_their_mix():
    """Every streaming loop of the fp32 hermite_eval kernels (8 packed pairs of interactions per trip: two groups of 4 bodies j):
    2 v_rsq_f32 and 25 (no mass multiply) or 26 v_pk_* per packed pair, bodies j by s_load, no LDS, scratch or barrier instruction
    and no v_mov; no kernel of the file uses scratch or more than 128 VGPRs."""
    subprocess.run(["make", "-s", "-C", CSRC, "hermite_eval.s"], check=True, capture_output=True)
    text = open(os.path.join(CSRC, "hermite_eval.s")).read()
    seen = 0
    for name, lines in kernels_of(text):
        if "hermite_evalIf" not in name:
            continue
        seen += 1
        mixes = []
        for i, line in enumerate(lines):
            if "Inner Loop Header" not in line:
                continue
            label = lines[i - 1].split(":")[0].strip()
            stop = next((k for k in range(i, len(lines)) if ("s_cbranch" in lines[k] or "s_branch" in lines[k]) and label in lines[k]), None)
            if stop is None:
                continue
            body = [l.strip() for l in lines[i + 1:stop]]
            count = lambda prefix: sum(1 for l in body if l.startswith(prefix))  # noqa: E731
            if count("v_rsq_f32") < 4:
                continue  # (the one-body loop of the ragged end, the fold)
            pairs = count("v_rsq_f32") // RSQ
            assert count("v_rsq_f32") == RSQ * pairs and pairs == 8, (name, label)
            assert count("v_pk_") in (PK_UNIT * pairs, PK_MIXED * pairs), (name, label, count("v_pk_") / pairs)
            assert count("ds_") == 0 and count("scratch_") == 0 and count("s_barrier") == 0 and count("v_mov") == 0, (name, label)
            assert count("s_load") >= 2 and count("global_load") == 0 and count("buffer_load") == 0, (name, label)
            mixes.append(count("v_pk_") // pairs)
        assert sorted(mixes) == [PK_UNIT, PK_MIXED], (name, mixes)
    assert seen == 8  # S = 1, 2, 4, 8 x (eval, step)
    sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    vgprs = [int(m) for m in re.findall(r"\.vgpr_count:\s+(\d+)", text)]
    assert len(sizes) == 22 and max(sizes) == 0, sizes
    assert len(vgprs) == 22 and max(vgprs) <= 128, vgprs
    assert PK_MIXED <= 28


def test_hermite_sources_keep_the_scalar_unit_to_loads():
    for name in ("hermite_eval.hip", "hermite_capi.hip", "hermite_boundary.h", "hermite_kernels.h"):
        src = open(os.path.join(CSRC, name)).read().lower()
        for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_dcache_" + "wb", "s_dcache_" + "discard", "atomicadd"):
            assert word not in src, (name, word)
    text = open(os.path.join(CSRC, "hermite_eval.s")).read() if os.path.exists(os.path.join(CSRC, "hermite_eval.s")) else ""
    assert "s_" + "store" not in text and "_atomic" not in text


# ---------------------------------------------------------------------------------------------------------------- GPU
gpu_only = pytest.mark.gpu
LD = np.longdouble


_REFERENCES = {}


def reference(pos, vel, eps2, rows=None):
    """(a, jerk, A, J) of bodies `rows` (default: all) as (len(rows), 3) arrays, from the T-typed (n, 4) pos and vel: a and jerk summed
    in long double; A and J (the sums of term magnitudes the allowances scale with) in float64, which is plenty for a bound"""
    p, v = pos.astype(LD), vel.astype(LD)
    p64, v64 = pos.astype(np.float64), vel.astype(np.float64)
    key = (hashlib.sha1(p64.tobytes() + v64.tobytes()).hexdigest(), float(eps2), None if rows is None else tuple(rows))  # (the values, whatever T held them)
    if key in _REFERENCES:
        return _REFERENCES[key]
    n = p.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = [np.zeros((len(rows), 3), LD) for _ in range(4)]
    block = max(1, min(256, (1 << 21) // n))
    for s in range(0, len(rows), block):
        i = rows[s:s + block]
        r = p[None, :, :3] - p[i, None, :3]
        w = v[None, :, :3] - v[i, None, :3]
        s2 = (r * r).sum(axis=2) + LD(eps2)
        with np.errstate(all="ignore"):
            k = np.where(s2 > 0, p[None, :, 3] / (s2 * np.sqrt(s2)), 0)   # (eps^2 = 0: a coincident pair contributes 0)
            t = np.where(s2 > 0, 3 * (r * w).sum(axis=2) / s2, 0)
        out[0][s:s + len(i)] = (k[:, :, None] * r).sum(axis=1)
        out[1][s:s + len(i)] = (k[:, :, None] * (w - t[:, :, None] * r)).sum(axis=1)
        r64 = np.abs(p64[None, :, :3] - p64[i, None, :3])
        w64 = np.abs(v64[None, :, :3] - v64[i, None, :3])
        s64 = s2.astype(np.float64)
        with np.errstate(all="ignore"):
            k64 = np.abs(k.astype(np.float64))
            t64 = np.where(s64 > 0, 3 * (r64 * w64).sum(axis=2) / s64, 0)
        out[2][s:s + len(i)] = (k64[:, :, None] * r64).sum(axis=1)
        out[3][s:s + len(i)] = (k64[:, :, None] * (w64 + t64[:, :, None] * r64)).sum(axis=1)
    if len(_REFERENCES) < 8 and n >= 4096:
        _REFERENCES[key] = out
    return out


class Device:
    """the arrays of one system on the device, through the C calls"""

    def __init__(self, gpu, pos, vel, eps2, pad=0, ws_fill=None):
        self.gpu, self.dtype, self.n = gpu, pos.dtype, pos.shape[0]
        self.f, self.scalar = fns(gpu, self.dtype)
        self.eps2, self.pad = eps2, pad
        size = self.dtype.itemsize
        self.canary = np.full(4 * pad, 1234.5, self.dtype)
        self.bufs = {}
        for name, count in (("pos", 4), ("pos2", 4), ("vel", 4), ("acc", 4), ("jerk", 4), ("ws", 8)):
            host = np.concatenate([self.canary, np.zeros(count * self.n, self.dtype), self.canary])
            if name == "ws" and ws_fill is not None:
                host[4 * pad:4 * pad + 8 * self.n] = ws_fill
            buf = gpu.DeviceBuffer(host.nbytes)
            buf.upload(host)
            self.bufs[name] = buf
        self.ws_bytes = 8 * self.n * size
        self.put("pos", pos), self.put("vel", vel)

    def ptr(self, name):
        return self.bufs[name].ptr.value + 4 * self.pad * self.dtype.itemsize

    def put(self, name, data):
        data = np.ascontiguousarray(data, dtype=self.dtype)
        self.gpu.check(self.gpu.lib().nb_h2d(self.ptr(name), data.ctypes.data, data.nbytes, None), "nb_h2d")

    def get(self, name):
        out = np.empty((self.n, 8 if name == "ws" else 4), self.dtype)
        self.gpu.check(self.gpu.lib().nb_d2h(out.ctypes.data, self.ptr(name), out.nbytes, None), "nb_d2h")
        return out

    def canaries_intact(self):
        for name, buf in self.bufs.items():
            host = buf.download(np.empty(buf.nbytes // self.dtype.itemsize, self.dtype))
            if self.pad and not (host[:4 * self.pad].tobytes() == self.canary.tobytes() and host[-4 * self.pad:].tobytes() == self.canary.tobytes()):
                return False
        return True

    def eval(self, pos="pos", stream=None):
        self.gpu.check(self.f["eval"](self.ptr("acc"), self.ptr("jerk"), self.ptr(pos), self.ptr("vel"), self.n, self.scalar(self.eps2), stream), "nb_hermite_eval")

    def step(self, dt, new="pos", old="pos", stream=None):
        self.gpu.check(self.f["step"](self.ptr(new), self.ptr(old), self.ptr("vel"), self.ptr("acc"), self.ptr("jerk"), self.ptr("ws"), self.ws_bytes, self.n,
                                      self.scalar(dt), self.scalar(self.eps2), stream), "nb_hermite_step")

    def state(self, pos="pos"):
        return tuple(self.get(k) for k in (pos, "vel", "acc", "jerk"))

    def free(self):
        for buf in self.bufs.values():
            buf.free()


def evaluate(gpu, pos, vel, eps2):
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    out = d.get("acc"), d.get("jerk")
    d.free()
    return out


def check_eval(acc, jerk, pos, vel, eps2, what, rows=None):
    dtype = pos.dtype.type
    a, j, A, J = reference(pos, vel, eps2, rows)
    rows = np.arange(pos.shape[0]) if rows is None else rows
    assert np.isfinite(a).all() and np.isfinite(j).all(), f"{what}: the yardstick itself is not finite"
    tol = LD(TOL[dtype])
    err_a, err_j = np.abs(acc[rows, :3].astype(LD) - a), np.abs(jerk[rows, :3].astype(LD) - j)
    with np.errstate(all="ignore"):
        worst_a = float(np.nanmax(np.where(A > 0, err_a / A, np.where(err_a > 0, np.inf, 0))))
        worst_j = float(np.nanmax(np.where(J > 0, err_j / J, np.where(err_j > 0, np.inf, 0))))
    print(f"{what}: acc {worst_a:.3g}, jerk {worst_j:.3g} of their term magnitudes (tol {float(tol):.1g})")
    assert np.isfinite(acc[rows]).all() and np.isfinite(jerk[rows]).all(), what
    assert (err_a <= tol * A).all(), f"{what}: acceleration at {worst_a / float(tol):.3g} x its bound"
    assert (err_j <= tol * J).all(), f"{what}: jerk at {worst_j / float(tol):.3g} x its bound"
    assert not acc[rows, 3].any() and not jerk[rows, 3].any(), f"{what}: .w of acc / jerk is not 0"


def cloud(n, dtype, seed, mass="equal", vscale=0.3):
    rng = np.random.default_rng(seed)
    pos, vel = np.zeros((n, 4), dtype), np.zeros((n, 4), dtype)
    pos[:, :3] = rng.standard_normal((n, 3))
    vel[:, :3] = rng.standard_normal((n, 3)) * vscale
    vel[:, 3] = rng.uniform(0.01, 0.5, n)
    if mass == "equal":
        pos[:, 3] = 1.0 / n
    elif mass == "species":
        pos[:, 3] = np.where(np.arange(n) < (2 * n) // 3, 0.5, 3.0)
    elif mass == "random":
        pos[:, 3] = 2.0 ** rng.uniform(-10, 10, n)
    elif mass == "zeros":
        pos[:, 3] = np.where(rng.uniform(size=n) < 0.3, 0.0, 1.0)
    return pos, vel


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_eval_against_long_double_sizes_and_masses(gpu, dtype):
    for n in (1, 2, 63, 64, 65, 1000, 5000):
        for mass in (("equal", "species", "random", "zeros") if n in (65, 1000) else ("equal",) if n == 5000 else ("equal", "random")):
            for eps2, vscale in ((0.01, 0.3), (1e-6, 3.0)) if n <= 1000 else ((float(np.float32(0.01)), 1.0),):  # (the same eps^2 in both precisions)
                pos, vel = cloud(n, dtype, 1000 + n, mass, vscale)
                if n == 5000:  # one fp32-representable cloud for both precisions: its long double sums are formed once
                    pos, vel = (q.astype(dtype) for q in cloud(n, np.float32, 1000 + n, mass, vscale))
                acc, jerk = evaluate(gpu, pos, vel, dtype(eps2))
                check_eval(acc, jerk, pos, vel, dtype(eps2), f"n {n} {mass} eps2 {eps2}")


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_eval_unsoftened_and_coincident(gpu, dtype):
    # eps^2 = 0, no coincident bodies: the i = j term contributes 0, not NaN
    for n, mass in ((2, "equal"), (65, "random"), (1000, "equal"), (1000, "species")):
        pos, vel = cloud(n, dtype, 7 + n, mass)
        acc, jerk = evaluate(gpu, pos, vel, dtype(0))
        check_eval(acc, jerk, pos, vel, dtype(0), f"unsoftened n {n} {mass}")
    # a coincident pair with eps^2 > 0: its term is a = 0, jerk = m w / eps^3 (the formulas as they stand)
    pos, vel = cloud(300, dtype, 5, "random")
    pos[17, :3] = pos[200, :3]
    eps2 = dtype(0.01)
    acc, jerk = evaluate(gpu, pos, vel, eps2)
    check_eval(acc, jerk, pos, vel, eps2, "coincident pair")
    two_pos, two_vel = pos[[17, 200]].copy(), vel[[17, 200]].copy()
    acc, jerk = evaluate(gpu, two_pos, two_vel, eps2)
    assert not acc[:, :3].any()
    want = two_pos[1, 3].astype(LD) * (two_vel[1, :3].astype(LD) - two_vel[0, :3].astype(LD)) / (LD(eps2) * np.sqrt(LD(eps2)))
    assert np.allclose(jerk[0, :3].astype(LD), want, rtol=8 * UNIT_ROUNDOFF[dtype], atol=0)


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_eval_demo_rows(gpu, oracle, dtype):
    n = 1024
    for row, prm in enumerate(gpu.DEMO_PARAMS):
        oracle.srand(100 + row)
        p, v = oracle.randomise(row % 3, n, prm.cluster_scale, prm.velocity_scale, dtype)
        pos, vel = p.reshape(n, 4), v.reshape(n, 4)
        s = dtype(np.float32(prm.softening))
        acc, jerk = evaluate(gpu, pos, vel, s * s)
        check_eval(acc, jerk, pos, vel, s * s, f"demo row {row}")


@gpu_only
@pytest.mark.parametrize("n,dtype", [(65536, np.float32), (65536, np.float64), (262144, np.float32)])
def test_eval_large_sampled(gpu, n, dtype):
    pos, vel = cloud(n, dtype, 3, "equal", 1.0)
    pos[:, 3] = 1.0
    if dtype == np.float32:
        pos[n // 2:n // 2 + 5000, 3] = 0.75  # some chunks take the mass-multiplying loop
    eps2 = dtype(0.01)
    acc, jerk = evaluate(gpu, pos, vel, eps2)
    rows = np.random.default_rng(4).choice(n, 64, replace=False)
    check_eval(acc, jerk, pos, vel, eps2, f"n {n}", rows=rows)
    assert np.isfinite(acc).all() and np.isfinite(jerk).all()


def ld_step(pos, vel, acc, jerk, dt, eps2, predicted):
    """The P(EC)^1 step in long double from T-typed inputs, stage by stage, with the allowance of each stage.

    predict: held to the long double predictor by the roundings each term passes through in T (x: 1, v dt: 2, a dt^2/2: 3,
             j dt^3/6: 5 -- 1/3, dt/3, three FMAs).  `predicted` is the workspace the call left: the T-typed state the evaluation saw.
    evaluate: a1, j1 of THAT state in long double, allowance tol A / tol J -- the evaluation's tolerance is defined on a T-typed
             state (a tolerance on the sums cannot cover what an ulp of a predicted position does to a close pair's force).
    correct: long double from the inputs and a1, j1; allowance: the evaluation's through dt/2 and dt^2/12, plus 2u of the result's
             own rounding (the construction of step_bounds in test_fast_domain.py, extended by the two dt^2/12 terms)."""
    dtype = pos.dtype.type
    tol, u = LD(TOL[dtype]), LD(UNIT_ROUNDOFF[dtype])
    x, v, a0, j0 = (q[:, :3].astype(LD) for q in (pos, vel, acc, jerk))
    dt = LD(dt)
    adt = abs(dt)
    xp = x + v * dt + a0 * dt * dt / 2 + j0 * dt ** 3 / 6
    vp = v + a0 * dt + j0 * dt * dt / 2
    bound_xp = u * (np.abs(x) + 2 * np.abs(v) * adt + 3 * np.abs(a0) * dt * dt / 2 + 5 * np.abs(j0) * adt ** 3 / 6) * (1 + 8 * u)
    bound_vp = u * (np.abs(v) + 2 * np.abs(a0) * adt + 3 * np.abs(j0) * dt * dt / 2) * (1 + 8 * u)
    assert (np.abs(predicted[:, 0:3].astype(LD) - xp) <= bound_xp).all(), "predicted positions"
    assert (np.abs(predicted[:, 4:7].astype(LD) - vp) <= bound_vp).all(), "predicted velocities"
    assert predicted[:, 3].tobytes() == pos[:, 3].tobytes() and not predicted[:, 7].any()
    a1, j1, A, J = reference(predicted[:, 0:4], predicted[:, 4:8], eps2)
    h, d12 = adt / 2, dt * dt / 12
    v1 = v + (a0 + a1) * dt / 2 + (j0 - j1) * d12
    x1 = x + (v + v1) * dt / 2 + (a0 - a1) * d12
    bound_a, bound_j = tol * A, tol * J
    bound_v = h * bound_a + d12 * bound_j + 2 * u * (np.abs(v) + h * np.abs(a0 + a1) + d12 * np.abs(j0 - j1))
    bound_x = h * bound_v + d12 * bound_a + 2 * u * (np.abs(x) + h * np.abs(v + v1) + d12 * np.abs(a0 - a1))
    return (x1, v1, a1, j1), (bound_x, bound_v, bound_a, bound_j)


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_step_against_long_double(gpu, dtype):
    for n, mass, eps2, dt in ((1, "equal", 0.01, 0.01), (65, "random", 0.01, 0.01), (1000, "equal", 0.01, 1.0 / 64), (1000, "species", 1e-4, 1e-3), (2085, "equal", 0.01, -0.01)):
        check_one_step(gpu, dtype, n, mass, eps2, dt)


def check_one_step(gpu, dtype, n, mass, eps2, dt):
    """an evaluation and one step of cloud(n, mass) against ld_step, stage by stage; shared with tests/test_kernel_matrix.py"""
    pos, vel = cloud(n, dtype, 31 + n, mass)
    check_step_of(gpu, pos, vel, dtype(eps2), dtype(dt), f"n {n} {mass}")


def check_step_of(gpu, pos, vel, eps2, dt, what):
    """an evaluation and one step of the T-typed state (pos, vel) against ld_step, stage by stage; shared with tests/test_hermite_domain.py"""
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    acc, jerk = d.get("acc"), d.get("jerk")
    d.step(dt, new="pos2", old="pos")
    got, predicted = d.state("pos2"), d.get("ws")
    d.free()
    want, bounds = ld_step(pos, vel, acc, jerk, dt, eps2, predicted)
    for name, g, w, b in zip(("position", "velocity", "acceleration", "jerk"), got, want, bounds):
        err = np.abs(g[:, :3].astype(LD) - w)
        with np.errstate(all="ignore"):
            print(f"{what} dt {dt}: {name} at {float(np.nanmax(np.where(b > 0, err / b, 0))):.3g} of its bound")
        assert (err <= b).all(), (what, name)
    assert got[0][:, 3].tobytes() == pos[:, 3].tobytes() and got[1][:, 3].tobytes() == vel[:, 3].tobytes()
    assert not got[2][:, 3].any() and not got[3][:, 3].any()


def run(gpu, pos, vel, eps2, dt, steps):
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    for _ in range(steps):
        d.step(dt)
    out = d.get("pos"), d.get("vel")
    d.free()
    return out


def order_cloud():
    """256 bodies of mass 1/256, Gaussian positions (sigma 1) and velocities (sigma 0.3), default_rng(1992).  The order test takes the
    max norm over bodies, which one close fly-by sets (crossing time eps / |w| ~ 0.24 = 8 steps of 1/32), so whether 32 steps are
    already in the dt^4 regime depends on the draw: the numpy fp64 scheme below (numpy_hermite, not the code under test) gives
    ratios 19.05 17.68 16.92 for seed 20240, 25.07 18.06 16.49 for seed 2, and 16.31 16.00 16.03 for this one."""
    return cloud(256, np.float64, 1992, "equal", 0.3)


def numpy_hermite(pos, vel, eps2, steps, t_end=1.0):
    """the scheme in plain numpy fp64: positions after `steps` steps to t_end"""
    x, v, m = pos[:, :3].copy(), vel[:, :3].copy(), pos[:, 3]

    def evaluate(x, v):
        r, w = x[None] - x[:, None], v[None] - v[:, None]
        s2 = (r * r).sum(axis=2) + eps2
        k = m[None] / (s2 * np.sqrt(s2))
        rw = (r * w).sum(axis=2)
        return (k[:, :, None] * r).sum(axis=1), (k[:, :, None] * (w - 3 * (rw / s2)[:, :, None] * r)).sum(axis=1)

    dt = t_end / steps
    a, j = evaluate(x, v)
    for _ in range(steps):
        xp = x + v * dt + a * dt * dt / 2 + j * dt ** 3 / 6
        vp = v + a * dt + j * dt * dt / 2
        a1, j1 = evaluate(xp, vp)
        v1 = v + (a + a1) * dt / 2 + (j - j1) * dt * dt / 12
        x = x + (v + v1) * dt / 2 + (a - a1) * dt * dt / 12
        v, a, j = v1, a1, j1
    return x


@gpu_only
def test_the_scheme_is_fourth_order_on_a_circular_orbit(gpu):
    """Two bodies of mass 1/2, separation 1, eps^2 = 0, one period in n steps: the error falls by 2^4 = 16 (+- 12 %) per halving."""
    pos = np.array([[-0.5, 0, 0, 0.5], [0.5, 0, 0, 0.5]], np.float64)
    vel = np.array([[0, -0.5, 0, 0], [0, 0.5, 0, 0]], np.float64)
    errors = []
    for n in (128, 256, 512, 1024):
        dt = np.float64(2 * np.pi / n)
        p, _ = run(gpu, pos, vel, np.float64(0), dt, n)
        t = n * dt
        errors.append(np.abs((p[1, :3] - p[0, :3]) - np.array([np.cos(t), np.sin(t), 0])).max())
    ratios = [a / b for a, b in zip(errors, errors[1:])]
    print("errors", errors, "ratios", ratios)
    assert all(14 <= r <= 18 for r in ratios), (errors, ratios)
    assert errors[-1] < 1e-8


@gpu_only
def test_the_scheme_is_fourth_order_on_a_cloud(gpu):
    pos, vel = order_cloud()
    eps2 = np.float64(0.01)
    ref, _ = run(gpu, pos, vel, eps2, np.float64(1.0 / 1024), 1024)
    errors = []
    for n in (32, 64, 128, 256):
        p, _ = run(gpu, pos, vel, eps2, np.float64(1.0 / n), n)
        errors.append(np.abs(p[:, :3] - ref[:, :3]).max())
    ratios = [a / b for a, b in zip(errors, errors[1:])]
    print("errors", errors, "ratios", ratios)
    assert all(14 <= r <= 18 for r in ratios), (errors, ratios)
    # ... and the trajectory is the scheme's: the plain numpy fp64 scheme lands on the same positions to rounding (1e-12: the
    # 64-step truncation error is 7.7e-8, fp64 rounding over 64 steps of 256-term sums some 1e-14)
    p, _ = run(gpu, pos, vel, eps2, np.float64(1.0 / 64), 64)
    assert np.abs(p[:, :3] - numpy_hermite(pos, vel, eps2, 64)).max() < 1e-12


def energy_drift(gpu, dtype, hermite):
    pos, vel = order_cloud()
    pos, vel = pos.astype(dtype), vel.astype(dtype)
    n, eps2, dt, steps = pos.shape[0], dtype(0.01), dtype(1.0 / 64), 64
    gpu.set_softening_squared(eps2 if dtype == np.float32 else float(eps2))
    d = Device(gpu, pos, vel, eps2)
    e0 = gpu.energy(d.ptr("pos"), d.ptr("vel"), n, dtype)["total"]
    read = "pos"
    if hermite:
        d.eval()
        for _ in range(steps):
            d.step(dt)
    else:
        fn = gpu.lib().nb_integrate_f32 if dtype == np.float32 else gpu.lib().nb_integrate_f64
        for _ in range(steps):
            write = "pos2" if read == "pos" else "pos"
            gpu.check(fn(d.ptr(write), d.ptr(read), d.ptr("vel"), d.scalar(dt), d.scalar(1.0), n, 256, gpu.NB_MODE_FAST, None), "nb_integrate")
            read = write
    e1 = gpu.energy(d.ptr(read), d.ptr("vel"), n, dtype)["total"]
    d.free()
    return abs(e1 - e0) / abs(e0)


@gpu_only
def test_energy_through_the_projects_diagnostic(gpu):
    """the cloud of the order test, 64 steps to t = 1, nb_energy_*: fp64 Hermite below 1/1000 of the first-order step's relative energy
    error and below 1e-6; fp32 below the first-order step's"""
    h64, e64 = energy_drift(gpu, np.float64, True), energy_drift(gpu, np.float64, False)
    h32, e32 = energy_drift(gpu, np.float32, True), energy_drift(gpu, np.float32, False)
    print(f"relative energy error: fp64 hermite {h64:.3g} euler {e64:.3g}; fp32 hermite {h32:.3g} euler {e32:.3g}")
    assert h64 < e64 / 1000 and h64 < 1e-6, (h64, e64)
    assert h32 < e32, (h32, e32)


def hip_runtime():
    hip = ctypes.CDLL("libamdhip64.so")
    for name in ("hipStreamBeginCapture", "hipStreamEndCapture", "hipGraphInstantiate", "hipGraphLaunch", "hipGraphExecDestroy", "hipGraphDestroy"):
        getattr(hip, name).restype = ctypes.c_int
    hip.hipStreamBeginCapture.argtypes = [ctypes.c_void_p, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    hip.hipGraphInstantiate.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    hip.hipGraphLaunch.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipGraphExecDestroy.argtypes = [ctypes.c_void_p]
    hip.hipGraphDestroy.argtypes = [ctypes.c_void_p]
    return hip


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_step_invariants(gpu, dtype):
    n, eps2, dt = 2085, dtype(0.01), dtype(0.01)
    pos, vel = cloud(n, dtype, 77, "species")
    lib = gpu.lib()

    def fresh(**kw):
        d = Device(gpu, pos, vel, eps2, pad=64, **kw)
        d.eval()
        return d

    base = fresh()
    start = base.state()
    assert start[0].tobytes() == pos.tobytes() and start[1].tobytes() == vel.tobytes()  # eval only reads the state
    base.step(dt, new="pos2", old="pos")
    want = base.state("pos2")
    assert base.get("pos").tobytes() == pos.tobytes()  # old positions untouched by a ping-pong step
    assert base.canaries_intact()
    ws = base.get("ws")
    assert ws[:, 3].tobytes() == pos[:, 3].tobytes() and not ws[:, 7].any()
    base.free()

    def same(got, what):
        for g, w, name in zip(got, want, ("pos", "vel", "acc", "jerk")):
            assert g.tobytes() == w.tobytes(), (what, name)

    again = fresh(ws_fill=np.nan)  # call to call, garbage in the workspace
    again.step(dt, new="pos2", old="pos")
    same(again.state("pos2"), "again, NaN workspace")
    again.free()

    inplace = fresh(ws_fill=1e30)  # new == old gives the bits of ping-pong
    inplace.step(dt)
    same(inplace.state(), "in place")
    assert inplace.canaries_intact()
    inplace.free()

    stream = ctypes.c_void_p()
    gpu.check(lib.nb_stream_create(ctypes.byref(stream)), "nb_stream_create")
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    other = Device(gpu, pos, vel, eps2, pad=64)
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    other.eval(stream=stream)
    other.step(dt, new="pos2", old="pos", stream=stream)
    gpu.check(lib.nb_stream_synchronize(stream), "nb_stream_synchronize")
    same(other.state("pos2"), "another stream")
    other.free()

    # a step recorded in a stream capture and replayed
    hip = hip_runtime()
    captured = fresh()
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    graph, graph_exec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0
    captured.step(dt, new="pos2", old="pos", stream=stream)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
    assert captured.get("pos2").tobytes() == np.zeros((n, 4), dtype).tobytes()  # recorded, not run
    assert hip.hipGraphInstantiate(ctypes.byref(graph_exec), graph, None, None, 0) == 0
    assert hip.hipGraphLaunch(graph_exec, stream) == 0
    gpu.check(lib.nb_stream_synchronize(stream), "nb_stream_synchronize")
    same(captured.state("pos2"), "captured and replayed")
    assert hip.hipGraphExecDestroy(graph_exec) == 0 and hip.hipGraphDestroy(graph) == 0
    captured.free()
    gpu.check(lib.nb_stream_destroy(stream), "nb_stream_destroy")

    # dt = 0: positions and velocities stay, the stored derivatives are nb_hermite_eval of the state
    still = fresh()
    a0, j0 = still.get("acc"), still.get("jerk")
    still.put("acc", np.full((n, 4), 3.0, dtype)), still.put("jerk", np.full((n, 4), -2.0, dtype))
    still.step(dtype(0))
    got = still.state()
    assert got[0].tobytes() == pos.tobytes() and got[1].tobytes() == vel.tobytes()
    assert got[2].tobytes() == a0.tobytes() and got[3].tobytes() == j0.tobytes()
    still.free()

    # masses and velocity .w come through
    assert want[0][:, 3].tobytes() == pos[:, 3].tobytes() and want[1][:, 3].tobytes() == vel[:, 3].tobytes()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_momentum_over_100_steps(gpu, dtype):
    """Equal masses: total momentum changes by the summation error of the forces only: per step and component at most
    dt/2 tol sum_i m A_i + dt^2/12 tol sum_i m J_i (+ rounding of the velocity updates, 2u sum |m v|), 100 steps of it."""
    n, eps2, dt = 1000, dtype(0.01), dtype(0.01)
    pos, vel = cloud(n, dtype, 9, "equal")
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    _, _, A, J = reference(pos, vel, eps2)
    for _ in range(100):
        d.step(dt)
    p1, v1 = d.get("pos"), d.get("vel")
    d.free()
    m = pos[:, 3].astype(LD)
    before, after = (m[:, None] * vel[:, :3].astype(LD)).sum(axis=0), (m[:, None] * v1[:, :3].astype(LD)).sum(axis=0)
    tol, u = LD(TOL[dtype]), LD(UNIT_ROUNDOFF[dtype])
    scale = 2 * max(float((m[:, None] * np.abs(v1[:, :3])).sum(axis=0).max()), float((m[:, None] * np.abs(vel[:, :3])).sum(axis=0).max()))
    # (A and J of the start, doubled: the cloud barely moves in t = 1)
    allowed = 100 * (LD(dt) / 2 * tol * 2 * (m[:, None] * A).sum(axis=0) + LD(dt) ** 2 / 12 * tol * 2 * (m[:, None] * J).sum(axis=0) + 2 * u * scale)
    print("momentum change", np.abs(after - before), "allowed", allowed)
    assert (np.abs(after - before) <= allowed).all()
    assert p1[:, 3].tobytes() == pos[:, 3].tobytes()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_shared_time_step(gpu, dtype):
    f, scalar = fns(gpu, dtype)
    u = UNIT_ROUNDOFF[dtype]
    eta = dtype(0.02)
    for n in (1, 2, 300, 70000, 300000):
        pos, vel = cloud(n, dtype, 13 + n, "random" if n < 1000 else "equal")
        d = Device(gpu, pos, vel, dtype(0.01))
        d.eval()
        acc, jerk = d.get("acc"), d.get("jerk")
        if n >= 300:
            jerk[5] = 0          # a zero-jerk body is left out
            jerk[9, 0] = np.nan  # a non-finite ratio is left out
            if n == 300000:
                acc[7, :3] = 0   # ... a zero acceleration is the minimum
            d.put("acc", acc), d.put("jerk", jerk)
        out, scratch = gpu.DeviceBuffer(8), gpu.DeviceBuffer(8192)
        scratch.upload(np.full(1024, -1.0))
        results = []
        for _ in range(2):
            gpu.check(f["timestep"](d.ptr("acc"), d.ptr("jerk"), n, scalar(eta), out.ptr, scratch.ptr, 8192, None), "nb_hermite_timestep")
            results.append(out.download(np.empty(1, dtype))[0])
        assert results[0].tobytes() == results[1].tobytes()
        a2, j2 = (acc[:, :3].astype(LD) ** 2).sum(axis=1), (jerk[:, :3].astype(LD) ** 2).sum(axis=1)
        with np.errstate(all="ignore"):
            ratio = np.sqrt(a2 / j2)
        ratio = ratio[(j2 > 0) & np.isfinite(ratio)]
        if n == 1:
            assert ratio.size == 0 and results[0] == np.inf
        else:
            want = LD(eta) * ratio.min()
            assert abs(LD(results[0]) - want) <= 2 * u * want, (n, results[0], want)
            if n == 300000:
                assert results[0] == 0
        out.free(), scratch.free(), d.free()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_python_class_gives_the_c_calls_bits(gpu, dtype):
    n, eps2, dt = 777, dtype(0.01), dtype(0.005)
    pos, vel = cloud(n, dtype, 55, "random")
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    for _ in range(3):
        d.step(dt)
    want = d.state()
    f, scalar = fns(gpu, dtype)
    out, scratch = gpu.DeviceBuffer(8), gpu.DeviceBuffer(8192)
    gpu.check(f["timestep"](d.ptr("acc"), d.ptr("jerk"), n, scalar(dtype(0.02)), out.ptr, scratch.ptr, 8192, None), "nb_hermite_timestep")
    want_dt = out.download(np.empty(1, dtype))[0]
    out.free(), scratch.free(), d.free()
    system = gpu.HermiteSystem(n, dtype, softening_sq=eps2)
    system.set_state(pos, vel)
    system.eval()
    for _ in range(3):
        system.step(dt)
    got = system.get_positions(), system.get_velocities(), system.get_accelerations(), system.get_jerks()
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert system.suggested_dt(dtype(0.02)).tobytes() == want_dt.tobytes()
    system.free()
    with pytest.raises(gpu.NBodyHipError):
        gpu.HermiteSystem(0, dtype)


@gpu_only
def test_hermite_step_speed_sanity(gpu):
    """65 536 bodies fp32, device events, median of 5 after warm-up: a Hermite step takes no more than 2 x the issue-cost model
    (25 packed ops + 2 v_rsq_f32 against 11 + 2 per packed pair: 1.93) relative to the one-sided FAST step (nb_integrate_f32)."""
    n, dtype = 65536, np.float32
    pos, vel = cloud(n, dtype, 1, "equal", 1.0)
    pos[:, 3] = 1.0
    eps2, dt = dtype(0.01), dtype(1e-3)
    gpu.set_softening_squared(eps2)
    d = Device(gpu, pos, vel, eps2)
    d.eval()
    lib = gpu.lib()

    def hermite():
        d.step(dt)

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

    t_hermite = median_ms(hermite)
    t_euler = median_ms(euler)
    d.free()
    print(f"hermite step {t_hermite:.3f} ms, one-sided FAST step {t_euler:.3f} ms: {t_hermite / t_euler:.2f}x (model {ISSUE_MODEL:.2f}x)")
    assert t_hermite <= 2 * ISSUE_MODEL * t_euler, (t_hermite, t_euler, ISSUE_MODEL)


# ---------------------------------------------------------------------------------------------------------------- CLI
CLI = os.path.join(ROOT, "cuda-nbody_amd", "nbody")


def test_cli_rejects_what_the_hermite_integrator_cannot_do(tmp_path):
    tipsy = tmp_path / "model.tipsy"
    tipsy.write_bytes(b"\0" * 64)
    base = ["--integrator=hermite", "--numbodies=1024", "--steps=1"]
    for extra in (["--integrator=hermite", "--steps=1"], ["--integrator=leapfrog", "--numbodies=1024", "--steps=1"], ["--integrator=hermite", "--numbodies=67108865", "--steps=1"],
                  base + ["--mode=strict"], base + ["--numdevices=2"], base + ["--devices=0,1"], base + ["--hostmem"], base + ["--systems=3"], base + [f"--tipsy={tipsy}"],
                  base + ["--compare"], base + ["--qatest"], base + ["--graph"], base + ["--no-workspace"], base + ["--workspace-mib=64"],
                  ["-integrator=hermite", "-numbodies=1024", "-steps=1", "-mode=strict"], ["--integrator", "hermite", "--numbodies", "1024", "--steps", "1", "--hostmem"]):
        r = subprocess.run([CLI, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr, (extra, r.returncode, r.stderr[:300])
    r = subprocess.run([CLI, "--integrator=hermite", "--numbodies=1024", "--steps=1", "--mode=strict"], capture_output=True, text=True, timeout=60)
    assert "--integrator=hermite has no strict mode" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--integrator TEXT [euler]" in r.stdout


@gpu_only
def test_cli_hermite_dump_energy_and_benchmark(gpu, oracle, tmp_path):
    n, steps = 4096, 10
    for flag in ("--integrator=hermite", "-integrator=hermite"):
        out = tmp_path / "hermite.bin"
        r = subprocess.run([CLI, flag, f"--numbodies={n}", f"--steps={steps}", f"--dump={out}", "--energy"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        data = np.fromfile(out, dtype=np.float32)
        assert data.size == 2 * 4 * n
        pos0, vel0 = oracle.startup_state(n, np.float32)
        s = np.float32(0.1)
        want = run(gpu, pos0.reshape(n, 4), vel0.reshape(n, 4), s * s, np.float32(0.016), steps)
        assert data[:4 * n].tobytes() == want[0].tobytes() and data[4 * n:].tobytes() == want[1].tobytes(), flag
        m = re.search(r"^energy end \(10 steps\): .* relative_drift=(\S+)$", r.stdout, re.M)
        assert m and "energy start: kinetic=" in r.stdout, r.stdout[-600:]
        assert abs(float(m[1])) < 1e-3
    # --integrator=euler is a run without the flag
    a, b = tmp_path / "a.bin", tmp_path / "b.bin"
    for file, extra in ((a, ["--integrator=euler"]), (b, [])):
        r = subprocess.run([CLI, *extra, f"--numbodies={n}", f"--steps={steps}", f"--dump={file}"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    assert a.read_bytes() == b.read_bytes()
    r = subprocess.run([CLI, "--integrator=hermite", f"--numbodies={n}", "--benchmark", "-i=20", "--fp64"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"^(\d+) bodies, hermite integrator, total time for (\d+) iterations: ([\d.]+) ms\n= ([\d.]+) ms per step\n= ([\d.]+) billion interactions per second\n"
                  r"= ([\d.]+) double-precision GFLOP/s at 43 flops per acceleration \+ jerk interaction", r.stdout, re.M)
    assert m, r.stdout[-600:]
    got_n, iters, ms, per_step, ips = int(m[1]), int(m[2]), float(m[3]), float(m[4]), float(m[5])
    assert (got_n, iters) == (n, 20)
    assert abs(per_step - ms / 20) <= 0.01 * per_step + 0.002
    want = n * n * iters / (ms * 1e-3) * 1e-9
    assert abs(ips - want) <= 0.01 * want + 0.002, (ips, want)
