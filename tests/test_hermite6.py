"""6th-order Hermite steps (nb_hermite6_*, include/nbody_hip_hermite6.h; libnbody_hip_hermite6.so from csrc/hermite6_*.hip).

CPU tests: the boundary (declared, exported, mirrored), host-side argument checks, the plan as a function of N alone, the instruction
mix of the fp32 streaming loops, the command line.  GPU tests: accelerations, jerks and snaps against long double sums

    r = x_j - x_i, w = v_j - v_i, b = a_j - a_i, s^2 = r.r + eps^2, k = m_j s^-3
    alpha = (r.w) / s^2,  beta = (w.w + r.b) / s^2 + alpha^2,  J' = w - 3 alpha r,  S' = b - 6 alpha J' - 3 beta r
    a_i = sum k r,   jerk_i = sum k J',   snap_i = sum k S'

per body and component to tol x the sum of term magnitudes (the same expressions with every operand's absolute value and + for every -),
tol the FAST force tolerance of tests/test_fast_domain.py (5e-6 fp32, 1e-14 fp64); init; one step stage by stage against a long double
step; the order of the scheme on a two-body orbit and a 256-body cloud; energy through nb_energy_*; invariants (bits, in place, canaries,
capture); the time step; the Python class and the command line; a speed sanity bound against nb_hermite_step of the same session."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_capi_symbols import declared_symbols, exported_symbols
from test_fast_domain import TOL, UNIT_ROUNDOFF
from test_hermite import CLI, cloud, energy_drift, gpu_only, hip_runtime, order_cloud
from test_hermite import Device as Device4
from test_hermite import run as run4

ERR = 10001
MAX_N = 1 << 26
LD = np.longdouble
CSRC = os.path.join(ROOT, "cuda-nbody_amd", "csrc")
SYMBOLS = ["nb_hermite6_eval_f32", "nb_hermite6_eval_f64", "nb_hermite6_init_f32", "nb_hermite6_init_f64", "nb_hermite6_plan_f32", "nb_hermite6_plan_f64",
           "nb_hermite6_step_f32", "nb_hermite6_step_f64", "nb_hermite6_timestep_f32", "nb_hermite6_timestep_f64", "nb_hermite6_workspace_bytes"]
# what the compiler delivers for the fp32 streaming loops, per packed pair of interactions
PK6_UNIT, PK6_MIXED, RSQ = 47, 48, 2
DP6_UNIT, DP6_MIXED = 54, 55  # fp64: v_*_f64 per interaction, the v_rsq_f64 seed included
# nb_hermite_*'s loop (tests/test_hermite.py) and the issue cycles of docs/history.md: packed fp32 op 4.08, v_rsq_f32 8.3
PK4_UNIT, PK_CYCLES, RSQ_CYCLES = 25, 4.08, 8.3
ISSUE_MODEL = (PK6_UNIT * PK_CYCLES + RSQ * RSQ_CYCLES) / (PK4_UNIT * PK_CYCLES + RSQ * RSQ_CYCLES)


def fns(pkg, dtype):
    lib = pkg.hermite6_lib()
    sfx = "f32" if np.dtype(dtype) == np.float32 else "f64"
    scalar = np.float32 if sfx == "f32" else float
    return {name: getattr(lib, f"nb_hermite6_{name}_{sfx}") for name in ("eval", "init", "step", "timestep", "plan")}, scalar


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_hermite6_header_library_and_binding_agree(pkg):
    declared = declared_symbols("nbody_hip_hermite6.h")
    assert declared == SYMBOLS
    assert exported_symbols(pkg.HERMITE6_LIB_PATH) == declared
    assert sorted(pkg.HERMITE6_SIGNATURES) == declared
    others = set(exported_symbols(pkg.LIB_PATH)) | set(exported_symbols(pkg.HERMITE_LIB_PATH))
    assert not set(declared) & others
    needed = subprocess.run(["readelf", "-d", pkg.HERMITE6_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnbody_hip" not in needed  # links none of the other libraries


def test_hermite6_plan_mirror_and_constants_match_the_header(pkg):
    text = open(os.path.join(ROOT, "include", "nbody_hip_hermite6.h")).read()
    body = re.search(r"typedef struct nb_hermite6_plan \{.*?\*/(.*?)\} nb_hermite6_plan_t;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int|unsigned)\s+(\w+);", body)
    assert [f for _, f in fields] == [f for f, _ in pkg.Hermite6Plan._fields_]
    assert pkg.Hermite6Plan._fields_ == pkg.HermitePlan._fields_ and ctypes.sizeof(pkg.Hermite6Plan) == 24  # the fields of nb_hermite_plan_t
    assert re.search(r"#define NB_HERMITE6_MAX_BODIES \(1u << 26\)", text) and pkg.HERMITE6_MAX_BODIES == MAX_N
    assert int(re.search(r"#define NB_HERMITE6_TIMESTEP_SCRATCH_BYTES (\d+)", text).group(1)) == pkg.HERMITE6_TIMESTEP_SCRATCH_BYTES == pkg.HERMITE_TIMESTEP_SCRATCH_BYTES


def test_hermite6_argument_errors_are_caught_on_the_host(pkg):
    """The list of test_hermite_argument_errors_are_caught_on_the_host with the new arrays: everything refused here is refused before a
    HIP call (the addresses are never dereferenced); new == old and acc_out == acc_in are NOT refused by the argument check -- without a
    GPU those calls then answer a HIP error, with one they would run, so they are only made without."""
    lib = pkg.hermite6_lib()
    out = ctypes.c_size_t(0)
    assert lib.nb_hermite6_workspace_bytes(1000, 4, ctypes.byref(out)) == 0 and out.value == 48000
    assert lib.nb_hermite6_workspace_bytes(1000, 8, ctypes.byref(out)) == 0 and out.value == 96000
    for bad in ((0, 4), (MAX_N + 1, 4), (1000, 2), (1000, 16)):
        assert lib.nb_hermite6_workspace_bytes(*bad, ctypes.byref(out)) == ERR, bad
    assert lib.nb_hermite6_workspace_bytes(1000, 4, None) == ERR
    count = ctypes.c_int(0)
    no_gpu = pkg.lib().nb_device_count(ctypes.byref(count)) != 0 or count.value == 0
    for dtype in (np.float32, np.float64):
        f, scalar = fns(pkg, dtype)
        size = np.dtype(dtype).itemsize
        n = 1024
        span = 4 * n * size
        ok = dict(new=0x100000000, old=0x200000000, vel=0x300000000, acc=0x400000000, jerk=0x500000000, snap=0x600000000, crackle=0x700000000, ws=0x800000000,
                  accin=0x900000000, ws_bytes=3 * span, n=n)
        length = lambda name: 3 * span if name == "ws" else span  # noqa: E731

        def step(**kw):
            a = {**ok, **kw}
            return f["step"](a["new"], a["old"], a["vel"], a["acc"], a["jerk"], a["snap"], a["crackle"], a["ws"], a["ws_bytes"], a["n"], scalar(0.01), scalar(0.01), None)

        names = ("new", "old", "vel", "acc", "jerk", "snap", "crackle", "ws")
        for null in names:
            assert step(**{null: None}) == ERR, null
        assert step(new=None, old=None) == ERR
        for bad in (dict(n=0), dict(n=MAX_N + 1), dict(ws_bytes=3 * span - 1), dict(ws_bytes=2 * span), dict(ws_bytes=0)):
            assert step(**bad) == ERR, bad
        for name in names:
            assert step(**{name: ok[name] + 2 * size}) == ERR, f"{name} misaligned"
        for x in names:  # every pair of arrays, overlapping by one body at either end
            for y in names:
                if x == y:
                    continue
                assert step(**{x: ok[y] + length(y) - 4 * size}) == ERR, (x, "on the last body of", y)
                assert step(**{x: ok[y] - length(x) + 4 * size}) == ERR, (x, "running into", y)
                if {x, y} != {"new", "old"}:
                    assert step(**{x: ok[y]}) == ERR, (x, "==", y)
        assert step(snap=ok["crackle"]) == ERR  # snap == crackle
        assert step(new=ok["old"] + 4 * size) == ERR  # new and old may be the SAME array, not shifted ones
        if no_gpu:
            assert step(new=ok["old"]) not in (0, ERR)  # past the argument check: a HIP error

        def evaluate(**kw):
            a = {**ok, **kw}
            return f["eval"](a["acc"], a["jerk"], a["snap"], a["old"], a["vel"], a["accin"], a["ws"], a["ws_bytes"], a["n"], scalar(0.01), None)

        names = ("acc", "jerk", "snap", "old", "vel", "accin", "ws")
        for null in names:
            assert evaluate(**{null: None}) == ERR, null
            assert evaluate(**{null: ok[null] + 2 * size}) == ERR, null
        for x in names:
            for y in names:
                if x == y:
                    continue
                assert evaluate(**{x: ok[y] + length(y) - 4 * size}) == ERR, (x, "on the last body of", y)
                if {x, y} != {"acc", "accin"}:
                    assert evaluate(**{x: ok[y]}) == ERR, (x, "==", y)
        for bad in (dict(n=0), dict(n=MAX_N + 1), dict(ws_bytes=3 * span - 1), dict(acc=ok["accin"] + 4 * size)):
            assert evaluate(**bad) == ERR, bad
        if no_gpu:
            assert evaluate(acc=ok["accin"]) not in (0, ERR)  # acc_out == acc_in is accepted: past the argument check

        def init(**kw):
            a = {**ok, **kw}
            return f["init"](a["acc"], a["jerk"], a["snap"], a["crackle"], a["old"], a["vel"], a["ws"], a["ws_bytes"], a["n"], scalar(0.01), None)

        names = ("acc", "jerk", "snap", "crackle", "old", "vel", "ws")
        for null in names:
            assert init(**{null: None}) == ERR, null
            assert init(**{null: ok[null] + 2 * size}) == ERR, null
        for x in names:
            for y in names:
                if x != y:
                    assert init(**{x: ok[y]}) == ERR, (x, "==", y)
        for bad in (dict(n=0), dict(n=MAX_N + 1), dict(ws_bytes=3 * span - 1), dict(snap=ok["crackle"] + span - 4 * size)):
            assert init(**bad) == ERR, bad

        def timestep(**kw):
            a = {"dt": 0xa00000000, "scratch": 0xb00000000, "bytes": 8192, **ok, **kw}
            return f["timestep"](a["acc"], a["jerk"], a["snap"], a["crackle"], a["n"], scalar(0.02), a["dt"], a["scratch"], a["bytes"], None)

        for bad in (dict(acc=None), dict(jerk=None), dict(snap=None), dict(crackle=None), dict(dt=None), dict(scratch=None), dict(n=0), dict(n=MAX_N + 1), dict(bytes=8191),
                    dict(dt=0xa00000000 + size // 2), dict(scratch=0xb00000004), dict(acc=ok["acc"] + 2 * size), dict(dt=ok["acc"] + 4 * size), dict(scratch=ok["jerk"]),
                    dict(acc=ok["jerk"]), dict(snap=ok["crackle"]), dict(dt=ok["snap"]), dict(scratch=ok["crackle"] + span - 8)):
            assert timestep(**bad) == ERR, bad


def test_hermite6_plan_is_a_function_of_n_alone(pkg):
    sizes = sorted({1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 1000, 1023, 1024, 1025, 2085, 4096, 9001, 16384, 65536, 262144, MAX_N})
    for dtype in (np.float32, np.float64):
        f, _ = fns(pkg, dtype)
        W, size = (2, 4) if dtype == np.float32 else (1, 8)
        for n in sizes:
            plans = set()
            for _ in range(3):
                p = pkg.hermite6_plan(n, dtype)
                plans.add(tuple(getattr(p, name) for name, _ in pkg.Hermite6Plan._fields_))
            assert len(plans) == 1
            I, S, U, groups, threads, lds = plans.pop()
            assert I == W and U == (2 if dtype == np.float32 else 1) and S in (1, 2, 4, 8)
            assert threads == 64 * S and groups == -(-n // (64 * I))
            assert lds == max(S - 1, 1) * 9 * W * 64 * size <= 64 * 1024  # nine sums per body i and folded wave
            assert S == 8 or 2 * S * 128 > n
            if n >= 128:
                assert n // S >= 128, (n, S)
        assert [pkg.hermite6_plan(n, dtype).waves_per_group for n in (1, 255, 256, 511, 512, 1023, 1024)] == [1, 1, 2, 2, 4, 4, 8]
        p = pkg.Hermite6Plan()
        for n in (0, MAX_N + 1):
            assert f["plan"](n, ctypes.byref(p)) == ERR, n
        assert f["plan"](16, None) == ERR


def kernels_of(text):
    lines = text.split("\n")
    for i, line in enumerate(lines):
        m = re.match(r"^(_ZN2nb12_GLOBAL__N_1\d+hermite6_\w+):", line)
        if m:
            end = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            yield m.group(1), lines[i:end]


def test_hermite6_streaming_loops_keep_their_mix():
    """Every streaming loop of the fp32 hermite6_eval kernels (4 packed pairs of interactions per trip: two groups of 2 bodies j): 2 v_rsq_f32
    and 47 (no mass multiply) or 48 v_pk_* per packed pair (fp64: 54 or 55 v_*_f64 per interaction), bodies j by s_load, no LDS, scratch
    or barrier instruction and no v_mov; no kernel of the file uses scratch; the fp32 kernels stay within 128 VGPRs (4 waves per SIMD), the fp64 ones within 168 (3)."""
    subprocess.run(["make", "-s", "-C", CSRC, "hermite6_eval.s"], check=True, capture_output=True)
    text = open(os.path.join(CSRC, "hermite6_eval.s")).read()
    seen = 0
    for name, lines in kernels_of(text):
        if "hermite6_evalI" not in name:
            continue
        seen += 1
        fp32 = "hermite6_evalIf" in name
        rsq = "v_rsq_f32" if fp32 else "v_rsq_f64"
        per_trip = 8 if fp32 else 2  # fp32: 4 packed pairs x 2 halves; fp64: two groups of one body j
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
            if count(rsq) < per_trip:
                continue  # (the one-body loop of the ragged end, the fold)
            assert count(rsq) == per_trip, (name, label)
            assert count("ds_") == 0 and count("scratch_") == 0 and count("s_barrier") == 0 and count("v_mov") == 0, (name, label)
            assert count("s_load") >= 2 and count("global_load") == 0 and count("buffer_load") == 0, (name, label)
            if fp32:
                pairs = per_trip // RSQ
                assert count("v_pk_") in (PK6_UNIT * pairs, PK6_MIXED * pairs), (name, label, count("v_pk_") / pairs)
                mixes.append(count("v_pk_") // pairs)
            else:
                mixes.append(sum(1 for l in body if re.match(r"v_\w+_f64", l)) // 2)
        assert sorted(mixes) == ([PK6_UNIT, PK6_MIXED] if fp32 else [DP6_UNIT, DP6_MIXED]), (name, mixes)
    assert seen == 16  # (fp32, fp64) x S = 1, 2, 4, 8 x (eval, step)
    sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(sizes) == 24 and max(sizes) == 0, sizes
    for name, vgprs in re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        assert int(vgprs) <= (168 if "hermite6_evalId" in name else 128), (name, vgprs)


CLI_BASE = ["--integrator=hermite6", "--numbodies=1024", "--steps=1"]


def test_cli_rejects_what_the_hermite6_integrator_cannot_do(tmp_path):
    tipsy = tmp_path / "model.tipsy"
    tipsy.write_bytes(b"\0" * 64)
    base = CLI_BASE
    for extra in (["--integrator=hermite6", "--steps=1"], ["--integrator=hermite8", "--numbodies=1024", "--steps=1"], ["--integrator=hermite6", "--numbodies=67108865", "--steps=1"],
                  base + ["--mode=strict"], base + ["--numdevices=2"], base + ["--devices=0,1"], base + ["--hostmem"], base + ["--systems=3"], base + [f"--tipsy={tipsy}"],
                  base + ["--compare"], base + ["--qatest"], base + ["--graph"], base + ["--no-workspace"], base + ["--workspace-mib=64"], base + ["--eta=0.01"], base + ["--levels=3"],
                  ["-integrator=hermite6", "-numbodies=1024", "-steps=1", "-mode=strict"], ["--integrator", "hermite6", "--numbodies", "1024", "--steps", "1", "--hostmem"]):
        r = subprocess.run([CLI, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr, (extra, r.returncode, r.stderr[:300])
    r = subprocess.run([CLI, *base, "--mode=strict"], capture_output=True, text=True, timeout=60)
    assert "--integrator=hermite has no strict mode" in r.stderr  # --integrator=hermite's messages
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--integrator TEXT [euler]" in r.stdout and "--integrator=hermite6 " in r.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU
_REFERENCES = {}


def reference6(pos, vel, acc, eps2, rows=None):
    """(a, jerk, snap, A, J, S) of bodies `rows` (default: all) as (len(rows), 3) arrays from the T-typed (n, 4) pos, vel and acc: the sums in
    long double; A, J, S (the sums of term magnitudes: every operand's absolute value, + for every -) in float64, plenty for a bound.
    Kept by the inputs' values, whatever T held them: an fp32-representable state is summed once for both precisions."""
    p, v, b = pos.astype(LD), vel.astype(LD), acc.astype(LD)
    key = (pos.astype(np.float64).tobytes(), vel.astype(np.float64).tobytes(), acc.astype(np.float64).tobytes(), float(eps2), None if rows is None else tuple(rows))
    if key in _REFERENCES:
        return _REFERENCES[key]
    n = p.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = [np.zeros((len(rows), 3), LD) for _ in range(3)] + [np.zeros((len(rows), 3), np.float64) for _ in range(3)]
    block = max(1, min(256, (1 << 19) // n))
    for s in range(0, len(rows), block):
        i = rows[s:s + block]
        r = p[None, :, :3] - p[i, None, :3]
        w = v[None, :, :3] - v[i, None, :3]
        d = b[None, :, :3] - b[i, None, :3]
        s2 = (r * r).sum(axis=2) + LD(eps2)
        with np.errstate(all="ignore"):
            k = np.where(s2 > 0, p[None, :, 3] / (s2 * np.sqrt(s2)), 0)  # (eps^2 = 0: a coincident pair contributes 0)
            alpha = np.where(s2 > 0, (r * w).sum(axis=2) / s2, 0)
            beta = np.where(s2 > 0, ((w * w).sum(axis=2) + (r * d).sum(axis=2)) / s2, 0) + alpha * alpha
        jp = w - 3 * alpha[:, :, None] * r
        sp = d - 6 * alpha[:, :, None] * jp - 3 * beta[:, :, None] * r
        k3 = k[:, :, None]
        out[0][s:s + len(i)] = (k3 * r).sum(axis=1)
        out[1][s:s + len(i)] = (k3 * jp).sum(axis=1)
        out[2][s:s + len(i)] = (k3 * sp).sum(axis=1)
        ra, wa, da, s64 = (np.abs(q).astype(np.float64) for q in (r, w, d, s2))
        with np.errstate(all="ignore"):
            ka = np.abs(k3).astype(np.float64)
            alpha_a = np.where(s64 > 0, (ra * wa).sum(axis=2) / s64, 0)
            beta_a = np.where(s64 > 0, ((wa * wa).sum(axis=2) + (ra * da).sum(axis=2)) / s64, 0) + alpha_a * alpha_a
        jpa = wa + 3 * alpha_a[:, :, None] * ra
        spa = da + 6 * alpha_a[:, :, None] * jpa + 3 * beta_a[:, :, None] * ra
        out[3][s:s + len(i)] = (ka * ra).sum(axis=1)
        out[4][s:s + len(i)] = (ka * jpa).sum(axis=1)
        out[5][s:s + len(i)] = (ka * spa).sum(axis=1)
    if len(_REFERENCES) < 96:
        _REFERENCES[key] = out
    return out


class Device:
    """the arrays of one system on the device, through the C calls"""
    ARRAYS = (("pos", 4), ("pos2", 4), ("vel", 4), ("acc", 4), ("jerk", 4), ("snap", 4), ("crackle", 4), ("accin", 4), ("ws", 12))

    def __init__(self, gpu, pos, vel, eps2, pad=0, ws_fill=None):
        self.gpu, self.dtype, self.n = gpu, pos.dtype, pos.shape[0]
        self.f, self.scalar = fns(gpu, self.dtype)
        self.eps2, self.pad = eps2, pad
        self.canary = np.full(4 * pad, 1234.5, self.dtype)
        self.bufs = {}
        for name, count in self.ARRAYS:
            host = np.concatenate([self.canary, np.zeros(count * self.n, self.dtype), self.canary])
            if name == "ws" and ws_fill is not None:
                host[4 * pad:4 * pad + 12 * self.n] = ws_fill
            buf = gpu.DeviceBuffer(host.nbytes)
            buf.upload(host)
            self.bufs[name] = buf
        self.ws_bytes = 12 * self.n * self.dtype.itemsize
        self.put("pos", pos), self.put("vel", vel)

    def ptr(self, name):
        return self.bufs[name].ptr.value + 4 * self.pad * self.dtype.itemsize

    def put(self, name, data):
        data = np.ascontiguousarray(data, dtype=self.dtype)
        self.gpu.check(self.gpu.lib().nb_h2d(self.ptr(name), data.ctypes.data, data.nbytes, None), "nb_h2d")

    def get(self, name):
        out = np.empty((self.n, 12 if name == "ws" else 4), self.dtype)
        self.gpu.check(self.gpu.lib().nb_d2h(out.ctypes.data, self.ptr(name), out.nbytes, None), "nb_d2h")
        return out

    def canaries_intact(self):
        for buf in self.bufs.values():
            host = buf.download(np.empty(buf.nbytes // self.dtype.itemsize, self.dtype))
            if self.pad and not (host[:4 * self.pad].tobytes() == self.canary.tobytes() and host[-4 * self.pad:].tobytes() == self.canary.tobytes()):
                return False
        return True

    def eval(self, acc_in="accin", acc_out="acc", stream=None):
        self.gpu.check(self.f["eval"](self.ptr(acc_out), self.ptr("jerk"), self.ptr("snap"), self.ptr("pos"), self.ptr("vel"), self.ptr(acc_in), self.ptr("ws"), self.ws_bytes,
                                      self.n, self.scalar(self.eps2), stream), "nb_hermite6_eval")

    def init(self, stream=None):
        self.gpu.check(self.f["init"](self.ptr("acc"), self.ptr("jerk"), self.ptr("snap"), self.ptr("crackle"), self.ptr("pos"), self.ptr("vel"), self.ptr("ws"), self.ws_bytes,
                                      self.n, self.scalar(self.eps2), stream), "nb_hermite6_init")

    def step(self, dt, new="pos", old="pos", stream=None):
        self.gpu.check(self.f["step"](self.ptr(new), self.ptr(old), self.ptr("vel"), self.ptr("acc"), self.ptr("jerk"), self.ptr("snap"), self.ptr("crackle"), self.ptr("ws"),
                                      self.ws_bytes, self.n, self.scalar(dt), self.scalar(self.eps2), stream), "nb_hermite6_step")

    def state(self, pos="pos"):
        return tuple(self.get(k) for k in (pos, "vel", "acc", "jerk", "snap", "crackle"))

    def free(self):
        for buf in self.bufs.values():
            buf.free()


def evaluate(gpu, pos, vel, acc_in, eps2):
    d = Device(gpu, pos, vel, eps2)
    d.put("accin", acc_in)
    d.eval()
    out = d.get("acc"), d.get("jerk"), d.get("snap")
    d.free()
    return out


def worst_fraction(err, bound):
    with np.errstate(all="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0))))


def check_eval(got, pos, vel, acc_in, eps2, what, rows=None):
    dtype = pos.dtype.type
    ref = reference6(pos, vel, acc_in, eps2, rows)
    rows = np.arange(pos.shape[0]) if rows is None else rows
    tol = LD(TOL[dtype])
    worst = []
    for g, want, mag, name in zip(got, ref[:3], ref[3:], ("acceleration", "jerk", "snap")):
        assert np.isfinite(want).all(), f"{what}: the yardstick itself is not finite"
        err = np.abs(g[rows, :3].astype(LD) - want)
        worst.append(worst_fraction(err, tol * mag))
        assert np.isfinite(g[rows]).all(), (what, name)
        assert (err <= tol * mag).all(), f"{what}: {name} at {worst[-1]:.3g} x its bound"
        assert not g[rows, 3].any(), f"{what}: .w of {name} is not 0"
    print(f"{what}: acc {worst[0]:.3g}, jerk {worst[1]:.3g}, snap {worst[2]:.3g} of their bounds")
    return worst


def state32(n, dtype, seed, mass, vscale):
    """cloud() and a random acc_in (normal, scale 2), fp32-representable, in T: both precisions share one long double reference"""
    pos, vel = (q.astype(dtype) for q in cloud(n, np.float32, seed, mass, vscale))
    acc = np.zeros((n, 4), dtype)
    acc[:, :3] = (np.random.default_rng(seed + 1).standard_normal((n, 3)) * 2).astype(np.float32)
    acc[:, 3] = 7.0  # (.w of acc_in is not interpreted)
    return pos, vel, acc


SMALL = (1, 2, 63, 64, 65, 127, 128, 129)
MIDDLE = (255, 256, 257, 511, 512, 1023, 1025)


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", SMALL + MIDDLE + (1000,))
def test_eval_against_long_double_sums(gpu, n, dtype):
    masses = ("equal", "random") if n in SMALL else ("equal", "species") if n in MIDDLE else ("equal", "species", "random", "zeros")
    for mass in masses:
        for eps2, vscale in ((0.01, 0.3), (1e-6, 3.0)):
            pos, vel, acc = state32(n, dtype, 6000 + n, mass, vscale)
            eps2 = dtype(np.float32(eps2))  # (the same eps^2 in both precisions)
            check_eval(evaluate(gpu, pos, vel, acc, eps2), pos, vel, acc, eps2, f"n {n} {mass} eps2 {eps2}")


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mass", ["equal", "species"])
def test_eval_9001_sampled(gpu, mass, dtype):
    """S = 8, every wave streams more than kFlushEvery chunks (71 chunks / 8 waves), and the last chunk is ragged with an odd body"""
    n = 9001
    pos, vel, acc = state32(n, dtype, 9001, mass, 1.0)
    eps2 = dtype(np.float32(0.01))
    got = evaluate(gpu, pos, vel, acc, eps2)
    rows = np.sort(np.random.default_rng(4).choice(n, 64, replace=False))
    check_eval(got, pos, vel, acc, eps2, f"n {n} {mass}", rows=rows)
    assert all(np.isfinite(g).all() for g in got)


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_eval_unsoftened_and_coincident(gpu, dtype):
    # eps^2 = 0, no coincident bodies: the i = j term contributes 0, not NaN
    for n, mass in ((2, "equal"), (65, "random"), (1000, "species")):
        pos, vel, acc = state32(n, dtype, 7 + n, mass, 0.3)
        check_eval(evaluate(gpu, pos, vel, acc, dtype(0)), pos, vel, acc, dtype(0), f"unsoftened n {n} {mass}")
    # N = 1: the self term alone, exact zeros
    pos, vel, acc = state32(1, dtype, 3, "equal", 0.3)
    for g in evaluate(gpu, pos, vel, acc, dtype(0)):
        assert g.tobytes() == np.zeros((1, 4), dtype).tobytes()
    # a coincident pair (same position, velocity and acc_in) with eps^2 = 0 contributes exactly 0: the sums are those of the system
    # without body 200 as far as body 17 is concerned, and finite everywhere
    pos, vel, acc = state32(300, dtype, 5, "random", 0.3)
    pos[200, :3], vel[200, :3], acc[200, :3] = pos[17, :3], vel[17, :3], acc[17, :3]
    got = evaluate(gpu, pos, vel, acc, dtype(0))
    assert all(np.isfinite(g).all() for g in got)
    check_eval(got, pos, vel, acc, dtype(0), "coincident pair, unsoftened")
    two = [q[[17, 200]].copy() for q in (pos, vel, acc)]
    for g in evaluate(gpu, *two, dtype(0)):
        assert g.tobytes() == np.zeros((2, 4), dtype).tobytes()
    # ... and with different velocities the sums stay finite
    vel[200, :3] += dtype(0.25)
    assert all(np.isfinite(g).all() for g in evaluate(gpu, pos, vel, acc, dtype(0)))


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_init_is_two_evaluations_and_a_zero_crackle(gpu, dtype):
    for n, mass in ((65, "random"), (1000, "equal"), (2085, "species")):
        pos, vel = cloud(n, dtype, 21 + n, mass)
        eps2 = dtype(0.01)
        d = Device(gpu, pos, vel, eps2, ws_fill=np.nan)
        d.put("crackle", np.full((n, 4), 5.0, dtype))
        d.init()
        acc, jerk, snap, crackle = (d.get(k) for k in ("acc", "jerk", "snap", "crackle"))
        assert crackle.tobytes() == np.zeros((n, 4), dtype).tobytes()
        assert d.get("pos").tobytes() == pos.tobytes() and d.get("vel").tobytes() == vel.tobytes()
        d.free()
        a0, j0, _ = evaluate(gpu, pos, vel, np.zeros((n, 4), dtype), eps2)
        assert acc.tobytes() == a0.tobytes() and jerk.tobytes() == j0.tobytes()
        a1, j1, s1 = evaluate(gpu, pos, vel, a0, eps2)
        assert a1.tobytes() == a0.tobytes() and j1.tobytes() == j0.tobytes() and snap.tobytes() == s1.tobytes()
        # acc_out == acc_in gives the bits of two arrays
        d = Device(gpu, pos, vel, eps2)
        d.put("acc", a0)
        d.eval(acc_in="acc", acc_out="acc")
        assert d.get("acc").tobytes() == a0.tobytes() and d.get("snap").tobytes() == s1.tobytes()
        d.free()


def ld_step(pos, vel, acc, jerk, snap, crackle, dt, eps2, predicted):
    """The P(EC)^1 step in long double from T-typed inputs, stage by stage, with the allowance of each stage.

    predict: held to the long double predictor by the roundings each term passes through in T in a Horner form with the coefficients
             h/2, h/3 (two roundings), h/4, h/5 (two): x_p: x 1, v h 2, a h^2/2 3, j h^3/6 6, s h^4/24 7, c h^5/120 9; v_p: 1, 2, 3, 6, 6;
             a_p: 1, 2, 3, 5.  `predicted` is the workspace the call left: the T-typed state the evaluation saw.
    evaluate: a1, j1, s1 of THAT state in long double, allowance tol x their term magnitudes (test 1's bound).
    correct: long double from the inputs and a1, j1, s1; allowance: the evaluation's carried through h/2, h^2/10 and h^3/120 (for c1
             through 60/h^3, 36/h^2 and 9/h), plus 2u of the sum of the result's term magnitudes (the structure of
             test_hermite.ld_step)."""
    dtype = pos.dtype.type
    tol, u = LD(TOL[dtype]), LD(UNIT_ROUNDOFF[dtype])
    x, v, a0, j0, s0, c0 = (q[:, :3].astype(LD) for q in (pos, vel, acc, jerk, snap, crackle))
    h = LD(dt)
    xp = x + v * h + a0 * h ** 2 / 2 + j0 * h ** 3 / 6 + s0 * h ** 4 / 24 + c0 * h ** 5 / 120
    vp = v + a0 * h + j0 * h ** 2 / 2 + s0 * h ** 3 / 6 + c0 * h ** 4 / 24
    ap = a0 + j0 * h + s0 * h ** 2 / 2 + c0 * h ** 3 / 6
    A = np.abs
    slack = 1 + 32 * u
    bound_xp = u * (A(x) + 2 * A(v) * h + 3 * A(a0) * h ** 2 / 2 + 6 * A(j0) * h ** 3 / 6 + 7 * A(s0) * h ** 4 / 24 + 9 * A(c0) * h ** 5 / 120) * slack
    bound_vp = u * (A(v) + 2 * A(a0) * h + 3 * A(j0) * h ** 2 / 2 + 6 * A(s0) * h ** 3 / 6 + 6 * A(c0) * h ** 4 / 24) * slack
    bound_ap = u * (A(a0) + 2 * A(j0) * h + 3 * A(s0) * h ** 2 / 2 + 5 * A(c0) * h ** 3 / 6) * slack
    for name, got, want, bound in (("positions", predicted[:, 0:3], xp, bound_xp), ("velocities", predicted[:, 4:7], vp, bound_vp), ("accelerations", predicted[:, 8:11], ap, bound_ap)):
        err = np.abs(got.astype(LD) - want)
        print(f"predicted {name} at {worst_fraction(err, bound):.3g} of their bound")
        assert (err <= bound).all(), f"predicted {name}"
    assert predicted[:, 3].tobytes() == pos[:, 3].tobytes() and not predicted[:, 7].any() and not predicted[:, 11].any()
    a1, j1, s1, mag_a, mag_j, mag_s = reference6(predicted[:, 0:4], predicted[:, 4:8], predicted[:, 8:12], eps2)
    ba, bj, bs = tol * mag_a, tol * mag_j, tol * mag_s
    h2, t10, t120 = h / 2, h * h / 10, h ** 3 / 120
    v1 = v + (a0 + a1) * h2 - (j1 - j0) * t10 + (s0 + s1) * t120
    x1 = x + (v + v1) * h2 - (a1 - a0) * t10 + (j0 + j1) * t120
    d0, d1, d2 = a1 - a0 - j0 * h - s0 * h * h / 2, (j1 - j0 - s0 * h) * h, (s1 - s0) * h * h
    c1 = (60 * d0 - 36 * d1 + 9 * d2) / h ** 3
    bv = h2 * ba + t10 * bj + t120 * bs + 2 * u * (A(v) + h2 * A(a0 + a1) + t10 * A(j1 - j0) + t120 * A(s0 + s1))
    bx = h2 * bv + t10 * ba + t120 * bj + 2 * u * (A(x) + h2 * A(v + v1) + t10 * A(a1 - a0) + t120 * A(j0 + j1))
    mag_c = (60 * (A(a1) + A(a0) + A(j0) * h + A(s0) * h * h / 2) + 36 * (A(j1) + A(j0) + A(s0) * h) * h + 9 * (A(s1) + A(s0)) * h * h) / h ** 3
    bc = 60 / h ** 3 * ba + 36 / h ** 2 * bj + 9 / h * bs + 2 * u * mag_c
    return (x1, v1, a1, j1, s1, c1), (bx, bv, ba, bj, bs, bc)


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,mass", [(65, "equal"), (65, "random"), (1000, "equal"), (1000, "random"), (300, "equal"), (600, "equal"), (1100, "equal")])
def test_one_step_against_long_double(gpu, n, mass, dtype):
    check_one_step6(gpu, dtype, n, mass)


def check_one_step6(gpu, dtype, n, mass):
    """the second step of a run of cloud(n, mass) (so that the crackle the predictor reads is not 0) against ld_step, stage by stage; shared
    with tests/test_kernel_matrix.py"""
    pos, vel = cloud(n, dtype, 31 + n, mass)
    eps2, dt = dtype(0.01), dtype(1.0 / 64)
    d = Device(gpu, pos, vel, eps2)
    d.init()
    d.step(dt)
    before = d.state()
    assert before[5][:, :3].any()
    d.step(dt, new="pos2", old="pos")
    got, predicted = d.state("pos2"), d.get("ws")
    d.free()
    want, bounds = ld_step(*before, dt, eps2, predicted)
    for name, g, w, b in zip(("position", "velocity", "acceleration", "jerk", "snap", "crackle"), got, want, bounds):
        err = np.abs(g[:, :3].astype(LD) - w)
        print(f"n {n} {mass} dt {dt}: {name} at {worst_fraction(err, b):.3g} of its bound")
        assert (err <= b).all(), (n, mass, name)
    assert got[0][:, 3].tobytes() == pos[:, 3].tobytes() and got[1][:, 3].tobytes() == vel[:, 3].tobytes()
    assert not any(g[:, 3].any() for g in got[2:])


def run(gpu, pos, vel, eps2, dt, steps):
    d = Device(gpu, pos, vel, eps2)
    d.init()
    for _ in range(steps):
        d.step(dt)
    out = d.get("pos"), d.get("vel")
    d.free()
    return out


def numpy_hermite6(pos, vel, eps2, steps, t_end):
    """the scheme in plain numpy fp64: positions after `steps` steps to t_end"""
    x, v, m = pos[:, :3].copy(), vel[:, :3].copy(), pos[:, 3]

    def evaluate(x, v, a):
        r, w, b = x[None] - x[:, None], v[None] - v[:, None], a[None] - a[:, None]
        s2 = (r * r).sum(axis=2) + eps2
        with np.errstate(all="ignore"):
            k = np.where(s2 > 0, m[None] / (s2 * np.sqrt(s2)), 0)[:, :, None]
            alpha = np.where(s2 > 0, (r * w).sum(axis=2) / s2, 0)[:, :, None]
            beta = np.where(s2 > 0, ((w * w).sum(axis=2) + (r * b).sum(axis=2)) / s2, 0)[:, :, None] + alpha * alpha
        jp = w - 3 * alpha * r
        return (k * r).sum(axis=1), (k * jp).sum(axis=1), (k * (b - 6 * alpha * jp - 3 * beta * r)).sum(axis=1)

    h = t_end / steps
    a, j, _ = evaluate(x, v, np.zeros_like(x))
    _, _, s = evaluate(x, v, a)
    c = np.zeros_like(x)
    for _ in range(steps):
        xp = x + v * h + a * h ** 2 / 2 + j * h ** 3 / 6 + s * h ** 4 / 24 + c * h ** 5 / 120
        vp = v + a * h + j * h ** 2 / 2 + s * h ** 3 / 6 + c * h ** 4 / 24
        ap = a + j * h + s * h ** 2 / 2 + c * h ** 3 / 6
        a1, j1, s1 = evaluate(xp, vp, ap)
        v1 = v + (a + a1) * h / 2 - (j1 - j) * h ** 2 / 10 + (s + s1) * h ** 3 / 120
        x = x + (v + v1) * h / 2 - (a1 - a) * h ** 2 / 10 + (j + j1) * h ** 3 / 120
        c = (60 * (a1 - a - j * h - s * h * h / 2) - 36 * (j1 - j - s * h) * h + 9 * (s1 - s) * h * h) / h ** 3
        v, a, j, s = v1, a1, j1, s1
    return x


@gpu_only
def test_the_scheme_is_sixth_order_on_a_circular_orbit(gpu):
    """Two bodies of mass 1/2, separation 1, eps^2 = 0, one period in n steps: the position error falls by 2^6 = 64 (+- 12 %: the
    4th-order scheme gives 16, the scheme without the crackle term 31) per halving, is the plain numpy fp64 scheme's to two digits,
    and at 128 steps is below 1/100 of nb_hermite_step_f64's."""
    pos = np.array([[-0.5, 0, 0, 0.5], [0.5, 0, 0, 0.5]], np.float64)
    vel = np.array([[0, -0.5, 0, 0], [0, 0.5, 0, 0]], np.float64)

    def error(p, t):
        exact = 0.5 * np.array([[-np.cos(t), -np.sin(t), 0], [np.cos(t), np.sin(t), 0]])
        return np.abs(p[:, :3] - exact).max()

    errors, restated = [], []
    for n in (32, 64, 128, 256):
        dt = np.float64(2 * np.pi / n)
        p, _ = run(gpu, pos, vel, np.float64(0), dt, n)
        errors.append(error(p, n * dt))
        restated.append(error(numpy_hermite6(pos, vel, 0.0, n, n * dt), n * dt))
    ratios = [a / b for a, b in zip(errors, errors[1:])]
    p4, _ = run4(gpu, pos, vel, np.float64(0), np.float64(2 * np.pi / 128), 128)
    fourth = error(p4, 128 * np.float64(2 * np.pi / 128))
    print("errors", errors, "numpy", restated, "ratios", ratios, "4th order at 128 steps", fourth, "=", fourth / errors[2], "x")
    assert all(abs(e - r) <= 0.01 * r for e, r in zip(errors, restated)), (errors, restated)
    assert all(56 <= r <= 72 for r in ratios), (errors, ratios)
    assert errors[2] < fourth / 100, (errors[2], fourth)


@gpu_only
def test_the_scheme_gains_on_a_cloud(gpu):
    """the 256-body cloud of test_hermite's order test, eps^2 = 0.01, to t = 1 in 16, 32, 64 steps against 256 steps: each halving gains at
    least 32 x (the ratio wobbles far from the asymptote, hence a floor), and 32 steps beat nb_hermite_step_f64's 32 steps"""
    pos, vel = order_cloud()
    eps2 = np.float64(0.01)
    ref, _ = run(gpu, pos, vel, eps2, np.float64(1.0 / 256), 256)
    errors = []
    for n in (16, 32, 64):
        p, _ = run(gpu, pos, vel, eps2, np.float64(1.0 / n), n)
        errors.append(np.abs(p[:, :3] - ref[:, :3]).max())
    ratios = [a / b for a, b in zip(errors, errors[1:])]
    p4, _ = run4(gpu, pos, vel, eps2, np.float64(1.0 / 32), 32)
    fourth = np.abs(p4[:, :3] - ref[:, :3]).max()
    print("errors", errors, "ratios", ratios, "4th order at 32 steps", fourth)
    assert all(r >= 32 for r in ratios), (errors, ratios)
    assert errors[1] < fourth, (errors[1], fourth)


def energy_drift6(gpu, dtype):
    pos, vel = order_cloud()
    pos, vel = pos.astype(dtype), vel.astype(dtype)
    n, eps2, dt, steps = pos.shape[0], dtype(0.01), dtype(1.0 / 64), 64
    gpu.set_softening_squared(eps2 if dtype == np.float32 else float(eps2))
    d = Device(gpu, pos, vel, eps2)
    e0 = gpu.energy(d.ptr("pos"), d.ptr("vel"), n, dtype)["total"]
    d.init()
    for _ in range(steps):
        d.step(dt)
    e1 = gpu.energy(d.ptr("pos"), d.ptr("vel"), n, dtype)["total"]
    d.free()
    return abs(e1 - e0) / abs(e0)


@gpu_only
def test_energy_through_the_projects_diagnostic(gpu):
    """the cloud of the order test, 64 steps of 1/64, nb_energy_*: the fp64 relative drift is below nb_hermite_step's, measured here; fp32
    is finite and below 1e-6"""
    h64, h32 = energy_drift6(gpu, np.float64), energy_drift6(gpu, np.float32)
    fourth = energy_drift(gpu, np.float64, True)
    print(f"relative energy drift: fp64 hermite6 {h64:.3g}, hermite {fourth:.3g}; fp32 hermite6 {h32:.3g}")
    assert h64 < fourth, (h64, fourth)
    assert np.isfinite(h32) and h32 < 1e-6, h32


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_step_invariants(gpu, dtype):
    n, eps2, dt = 2085, dtype(0.01), dtype(0.01)
    pos, vel = cloud(n, dtype, 77, "species")
    lib = gpu.lib()
    names = ("pos", "vel", "acc", "jerk", "snap", "crackle")

    def fresh(**kw):
        d = Device(gpu, pos, vel, eps2, pad=64, **kw)
        d.init()
        return d

    base = fresh()
    start = base.state()
    assert start[0].tobytes() == pos.tobytes() and start[1].tobytes() == vel.tobytes()  # init only reads the state
    base.step(dt, new="pos2", old="pos")
    want = base.state("pos2")
    assert base.get("pos").tobytes() == pos.tobytes()  # old positions untouched by a ping-pong step
    assert base.canaries_intact()
    ws = base.get("ws")
    assert ws[:, 3].tobytes() == pos[:, 3].tobytes() and not ws[:, 7].any() and not ws[:, 11].any()
    for _ in range(3):
        base.step(dt, new="pos2", old="pos2")
    four = base.state("pos2")
    base.free()

    def same(got, expected, what):
        for g, w, name in zip(got, expected, names):
            assert g.tobytes() == w.tobytes(), (what, name)

    again = fresh(ws_fill=np.nan)  # call to call, garbage in the workspace
    again.step(dt, new="pos2", old="pos")
    same(again.state("pos2"), want, "again, NaN workspace")
    again.free()

    inplace = fresh(ws_fill=1e30)  # new == old gives the bits of ping-pong
    inplace.step(dt)
    same(inplace.state(), want, "in place")
    assert inplace.canaries_intact()
    inplace.free()

    stream = ctypes.c_void_p()
    gpu.check(lib.nb_stream_create(ctypes.byref(stream)), "nb_stream_create")
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    other = Device(gpu, pos, vel, eps2, pad=64)
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    other.init(stream=stream)
    other.step(dt, new="pos2", old="pos", stream=stream)
    gpu.check(lib.nb_stream_synchronize(stream), "nb_stream_synchronize")
    same(other.state("pos2"), want, "another stream")
    assert other.canaries_intact()
    other.free()

    # four steps recorded in one stream capture (a linear chain on one stream) and replayed: the bits of four plain steps
    hip = hip_runtime()
    captured = fresh()
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    graph, graph_exec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0
    captured.step(dt, new="pos2", old="pos", stream=stream)
    for _ in range(3):
        captured.step(dt, new="pos2", old="pos2", stream=stream)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
    assert captured.get("pos2").tobytes() == np.zeros((n, 4), dtype).tobytes()  # recorded, not run
    assert hip.hipGraphInstantiate(ctypes.byref(graph_exec), graph, None, None, 0) == 0
    assert hip.hipGraphLaunch(graph_exec, stream) == 0
    gpu.check(lib.nb_stream_synchronize(stream), "nb_stream_synchronize")
    same(captured.state("pos2"), four, "captured and replayed")
    assert hip.hipGraphExecDestroy(graph_exec) == 0 and hip.hipGraphDestroy(graph) == 0
    assert captured.canaries_intact()
    captured.free()
    gpu.check(lib.nb_stream_destroy(stream), "nb_stream_destroy")

    # masses and velocity .w come through; .w of the derivatives is 0
    assert four[0][:, 3].tobytes() == pos[:, 3].tobytes() and four[1][:, 3].tobytes() == vel[:, 3].tobytes()
    assert not any(q[:, 3].any() for q in four[2:])


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_time_step(gpu, dtype):
    """eta sqrt(min (|a||s| + |j|^2) / (|j||c| + |s|^2)) against long double on the stored arrays: 2 ulp of T for fp32 inputs, 1e-14 relative
    for fp64 (about ten fp64 roundings of positive terms)"""
    f, scalar = fns(gpu, dtype)
    eta = dtype(0.02)
    allowed = 2 * float(np.finfo(np.float32).eps) if dtype == np.float32 else 1e-14
    for n, steps in ((1, 0), (2, 1), (300, 0), (300, 2), (70000, 0)):
        pos, vel = cloud(n, dtype, 13 + n, "random" if n < 1000 else "equal")
        d = Device(gpu, pos, vel, dtype(0.01))
        d.init()
        for _ in range(steps):
            d.step(dtype(1.0 / 64))
        arrays = [d.get(k) for k in ("acc", "jerk", "snap", "crackle")]
        if steps == 0:
            assert not arrays[3].any()  # a zero crackle right after init is accepted
        if n == 300:
            arrays[2][5] = 0       # |s| = 0: denominator |j||c|
            arrays[1][9, 0] = np.nan  # a non-finite ratio is left out
            arrays[2][11], arrays[3][11] = 0, 0  # a denominator of 0 is left out
            for k, q in zip(("acc", "jerk", "snap", "crackle"), arrays):
                d.put(k, q)
        out, scratch = gpu.DeviceBuffer(8), gpu.DeviceBuffer(8192)
        scratch.upload(np.full(1024, -1.0))
        results = []
        for _ in range(2):
            gpu.check(f["timestep"](d.ptr("acc"), d.ptr("jerk"), d.ptr("snap"), d.ptr("crackle"), n, scalar(eta), out.ptr, scratch.ptr, 8192, None), "nb_hermite6_timestep")
            results.append(out.download(np.empty(1, dtype))[0])
        assert results[0].tobytes() == results[1].tobytes()
        a, j, s, c = (np.sqrt((q[:, :3].astype(LD) ** 2).sum(axis=1)) for q in arrays)
        with np.errstate(all="ignore"):
            den = j * c + s * s
            ratio = (a * s + j * j) / den
        ratio = ratio[(den > 0) & np.isfinite(ratio)]
        if n == 1:
            assert ratio.size == 0 and results[0] == np.inf  # every snap is 0
        else:
            want = LD(eta) * np.sqrt(ratio.min())
            print(f"n {n} after {steps} steps: dt {results[0]}, off by {float(abs(LD(results[0]) - want) / want):.3g} (allowed {allowed:.3g})")
            assert abs(LD(results[0]) - want) <= allowed * want, (n, results[0], want)
        out.free(), scratch.free(), d.free()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_python_class_gives_the_c_calls_bits(gpu, dtype):
    n, eps2, dt = 777, dtype(0.01), dtype(0.005)
    pos, vel = cloud(n, dtype, 55, "random")
    d = Device(gpu, pos, vel, eps2)
    d.init()
    for _ in range(3):
        d.step(dt)
    want = d.state()
    f, scalar = fns(gpu, dtype)
    out, scratch = gpu.DeviceBuffer(8), gpu.DeviceBuffer(8192)
    gpu.check(f["timestep"](d.ptr("acc"), d.ptr("jerk"), d.ptr("snap"), d.ptr("crackle"), n, scalar(dtype(0.02)), out.ptr, scratch.ptr, 8192, None), "nb_hermite6_timestep")
    want_dt = out.download(np.empty(1, dtype))[0]
    out.free(), scratch.free(), d.free()
    system = gpu.Hermite6System(n, dtype, softening_sq=eps2)
    system.set_state(pos, vel)
    system.eval()
    for _ in range(3):
        system.step(dt)
    got = system.get_positions(), system.get_velocities(), system.get_accelerations(), system.get_jerks(), system.get_snaps(), system.get_crackles()
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert system.suggested_dt(dtype(0.02)).tobytes() == want_dt.tobytes()
    system.free()
    with pytest.raises(gpu.NBodyHipError):
        gpu.Hermite6System(0, dtype)


@gpu_only
def test_cli_hermite6_dump_energy_and_benchmark(gpu, oracle, tmp_path):
    n, steps = 4096, 10
    out = tmp_path / "hermite6.bin"
    r = subprocess.run([CLI, "--integrator=hermite6", f"--numbodies={n}", f"--steps={steps}", f"--dump={out}", "--energy"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    data = np.fromfile(out, dtype=np.float32)
    assert data.size == 2 * 4 * n
    pos0, vel0 = oracle.startup_state(n, np.float32)
    s = np.float32(0.1)
    system = gpu.Hermite6System(n, np.float32, softening_sq=s * s)
    system.set_state(pos0.reshape(n, 4), vel0.reshape(n, 4))
    system.eval()
    for _ in range(steps):
        system.step(np.float32(0.016))
    want = system.get_positions(), system.get_velocities()
    system.free()
    assert data[:4 * n].tobytes() == want[0].tobytes() and data[4 * n:].tobytes() == want[1].tobytes()
    m = re.search(r"^energy end \(10 steps\): .* relative_drift=(\S+)$", r.stdout, re.M)
    assert m and "energy start: kinetic=" in r.stdout, r.stdout[-600:]
    assert abs(float(m[1])) < 1e-3
    r = subprocess.run([CLI, "--integrator=hermite6", f"--numbodies={n}", "--benchmark", "-i=20", "--fp64"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"^(\d+) bodies, hermite6 integrator, total time for (\d+) iterations: ([\d.]+) ms\n= ([\d.]+) ms per step\n= ([\d.]+) billion interactions per second\n"
                  r"= ([\d.]+) double-precision GFLOP/s at 80 flops per acceleration \+ jerk \+ snap interaction", r.stdout, re.M)
    assert m, r.stdout[-600:]
    got_n, iters, ms, per_step, ips, gflops = int(m[1]), int(m[2]), float(m[3]), float(m[4]), float(m[5]), float(m[6])
    assert (got_n, iters) == (n, 20)
    assert abs(per_step - ms / 20) <= 0.01 * per_step + 0.002
    want_ips = n * n * iters / (ms * 1e-3) * 1e-9
    assert abs(ips - want_ips) <= 0.02 * want_ips + 0.002
    assert abs(gflops - 80 * ips) <= 0.02 * 80 * ips + 0.2


@gpu_only
def test_hermite6_step_speed_sanity(gpu):
    """65 536 bodies fp32, device events, median of 5 after warm-up: a 6th-order step takes no more than 2 x the issue-cost model (47 packed
    ops + 2 v_rsq_f32 against 25 + 2 per packed pair: 1.76) relative to nb_hermite_step_f32 of the same session."""
    n, dtype = 65536, np.float32
    pos, vel = cloud(n, dtype, 1, "equal", 1.0)
    pos[:, 3] = 1.0
    eps2, dt = dtype(0.01), dtype(1e-3)
    d6 = Device(gpu, pos, vel, eps2)
    d6.init()
    d4 = Device4(gpu, pos, vel, eps2)
    d4.eval()

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

    t6 = median_ms(lambda: d6.step(dt))
    t4 = median_ms(lambda: d4.step(dt))
    d6.free(), d4.free()
    print(f"hermite6 step {t6:.3f} ms, hermite step {t4:.3f} ms: {t6 / t4:.2f}x (model {ISSUE_MODEL:.2f}x)")
    assert t6 <= 2 * ISSUE_MODEL * t4, (t6, t4, ISSUE_MODEL)
