"""Hermite steps of many independent systems, a time step per system (nb_hermite_ensemble_*, include/nbody_hip_hermite_ensemble.h;
libnbody_hip_hermite_ensemble.so from csrc/hermite_ensemble*.hip).

CPU tests: the boundary (declared, exported, mirrored; the other libraries unchanged), host-side argument checks, the plan against
nb_hermite_plan_*, the instruction mix of the fp32 streaming loops, the registry of hermite_ensemble.s.  GPU tests: every system's bits
against the solo calls (tests/test_hermite.py's Device on that system alone) on and around every switch of S, one system per S against
the long double bounds of tests/test_hermite.py; independence of a system from B, its index, its neighbours, the stream and the workspace;
the time step's edge cases; the adaptive form against a numpy restatement of the header's rule that drives the solo calls; graph capture;
the Python class; a speed sanity bound."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kernel_matrix import ENSEMBLE_LARGE, F32, F64, MASSES, N_BY_WAVES, kernel_name, listed_kernels
from test_capi_symbols import declared_symbols, exported_symbols
from test_fast_domain import UNIT_ROUNDOFF
from test_hermite import LD, PK_MIXED, PK_UNIT, RSQ, Device, check_eval, cloud, fns as solo_fns, hip_runtime, kernels_of, ld_step

ERR = 10001
MAX_N, MAX_TOTAL = 65536, 1 << 28
CSRC = os.path.join(ROOT, "cuda-nbody_amd", "csrc")
HEADER = "nbody_hip_hermite_ensemble.h"
SYMBOLS = sorted(["nb_hermite_ensemble_workspace_bytes"] + [f"nb_hermite_ensemble_{name}_{sfx}" for name in ("plan", "eval", "step", "timestep", "begin", "advance")
                                                            for sfx in ("f32", "f64")])
DONE, STALLED = 1, 2
# the sizes of the bit tests: 1, 2, one tile and a ragged second, then on and around every switch of S (kernel_matrix.N_BY_WAVES)
BIT_SIZES = (1, 2, 129, 255, 256, 257, 511, 512, 700, 1023, 1024, 1025)
SYSTEM_DT = (1.0 / 64, 1.0 / 128, 1.0 / 32)
SYSTEM_EPS2 = (0.01, 1e-6, 0.0)
LONG_DOUBLE_SIZES = {255: 1, 511: 2, 700: 4, 1025: 8}  # n -> S: one system per S against the long double bounds


def fns(pkg, dtype):
    lib = pkg.hermite_ensemble_lib()
    sfx = "f32" if np.dtype(dtype) == np.float32 else "f64"
    scalar = np.float32 if sfx == "f32" else float
    return {name: getattr(lib, f"nb_hermite_ensemble_{name}_{sfx}") for name in ("plan", "eval", "step", "timestep", "begin", "advance")}, scalar


def workspace_bytes(n, b, size):
    return 8 * n * b * size + 8 * b * -(-n // 256) + 64 * -(-b // 256)


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_hermite_ensemble_header_library_and_binding_agree(pkg):
    declared = declared_symbols(HEADER)
    assert declared == SYMBOLS and len(declared) == 13
    assert exported_symbols(pkg.HERMITE_ENSEMBLE_LIB_PATH) == declared
    assert sorted(pkg.HERMITE_ENSEMBLE_SIGNATURES) == declared
    assert os.path.basename(pkg.HERMITE_ENSEMBLE_LIB_PATH) == "libnbody_hip_hermite_ensemble.so" or "NBODY_HIP_HERMITE_ENSEMBLE_LIB" in os.environ
    needed = subprocess.run(["readelf", "-d", pkg.HERMITE_ENSEMBLE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnbody_hip" not in needed  # it links none of the other libraries


def test_every_other_library_exports_what_it_did(pkg):
    ours = set(SYMBOLS)
    for path, header, count in ((pkg.ENSEMBLE_LIB_PATH, "nbody_hip_ensemble.h", 4), (pkg.HERMITE_LIB_PATH, "nbody_hip_hermite.h", 9),
                                (pkg.HERMITE_BLOCK_LIB_PATH, "nbody_hip_hermite_block.h", 9), (pkg.NEIGHBOUR_LIB_PATH, "nbody_hip_neighbour.h", None),
                                (pkg.FIELD_LIB_PATH, "nbody_hip_field.h", None), (pkg.KNN_LIB_PATH, "nbody_hip_knn.h", 5)):
        exported = exported_symbols(path)
        assert exported == declared_symbols(header), header
        assert count is None or len(exported) == count, header
        assert not ours & set(exported), header
    product = exported_symbols(pkg.LIB_PATH)
    assert len(product) == 96 and not ours & set(product)
    assert not ours & set(exported_symbols(pkg.LAB_LIB_PATH))


def test_hermite_ensemble_records_match_the_header(pkg):
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    for struct, mirror, size in (("plan", pkg.HermiteEnsemblePlan, 40), ("clock", pkg.HermiteEnsembleClock, 32), ("status", pkg.HermiteEnsembleStatus, 64)):
        body = re.search(r"typedef struct nb_hermite_ensemble_%s \{.*?\*/(.*?)\} nb_hermite_ensemble_%s_t;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(?:int|unsigned long long|unsigned|double|uint32_t|uint64_t)\s+(\w+)(?:\[\d+\])?;", body)
        assert fields == [f for f, _ in mirror._fields_], struct
        assert ctypes.sizeof(mirror) == size, struct
    assert pkg.HERMITE_ENSEMBLE_CLOCK_DTYPE.itemsize == 32 and list(pkg.HERMITE_ENSEMBLE_CLOCK_DTYPE.names) == [f for f, _ in pkg.HermiteEnsembleClock._fields_]
    assert re.search(r"#define NB_HERMITE_ENSEMBLE_MAX_BODIES 65536u", text) and pkg.HERMITE_ENSEMBLE_MAX_BODIES == MAX_N
    assert re.search(r"#define NB_HERMITE_ENSEMBLE_MAX_TOTAL \(1u << 28\)", text) and pkg.HERMITE_ENSEMBLE_MAX_TOTAL == MAX_TOTAL
    assert re.search(r"#define NB_HERMITE_ENSEMBLE_DONE 1u", text) and re.search(r"#define NB_HERMITE_ENSEMBLE_STALLED 2u", text)
    assert (pkg.HERMITE_ENSEMBLE_DONE, pkg.HERMITE_ENSEMBLE_STALLED) == (DONE, STALLED)
    # what the issue wants said: the padding is stepped and enters the time-step minimum; the rule of advance, word for word
    flat = " ".join(text.replace("*", " ").split())
    for phrase in ("THE PADDING BODIES ARE STEPPED", "THEY ENTER THE TIME-STEP MINIMUM", "Per-system body counts are not built",
                   "A system whose flags hold DONE or STALLED is left bit-identical. Its workgroups leave after one scalar load.",
                   "Otherwise remaining = t_stop - time, in double.", "If remaining is not > 0, or (T)remaining is 0: set DONE, time = t_stop, state untouched.",
                   "Else cand = min(dt_next, dt_max). If cand >= remaining, then dt = (T)remaining and this is the system's last step. Otherwise dt = (T)cand.",
                   "If dt_next is not > 0 and DONE is not set, set STALLED. +inf counts as > 0."):
        assert phrase in flat, phrase


def test_hermite_ensemble_argument_errors_are_caught_on_the_host(pkg):
    """Everything refused here is refused before a HIP call (the addresses are never dereferenced)."""
    lib = pkg.hermite_ensemble_lib()
    out = ctypes.c_size_t(0)
    for n, b, size in ((1000, 7, 4), (1000, 7, 8), (1, 1, 4), (65536, 2, 8), (256, 300, 4)):
        assert lib.nb_hermite_ensemble_workspace_bytes(n, b, size, ctypes.byref(out)) == 0 and out.value == workspace_bytes(n, b, size), (n, b, size)
    # N, B, N * B out of range; B * groups_per_system * block_threads > 2^31 (N = 1: one group of 64 threads per system)
    for bad in ((0, 1, 4), (1, 0, 4), (MAX_N + 1, 1, 4), (MAX_N, MAX_TOTAL // MAX_N + 1, 4), (1000, 7, 2), (1000, 7, 16), (1, (1 << 25) + 1, 4), (1, (1 << 25) + 1, 8)):
        assert lib.nb_hermite_ensemble_workspace_bytes(*bad, ctypes.byref(out)) == ERR, bad
    assert lib.nb_hermite_ensemble_workspace_bytes(1, 1 << 25, 4, ctypes.byref(out)) == 0
    assert lib.nb_hermite_ensemble_workspace_bytes(1000, 7, 4, None) == ERR
    count = ctypes.c_int(0)
    no_gpu = pkg.lib().nb_device_count(ctypes.byref(count)) != 0 or count.value == 0
    for dtype in (np.float32, np.float64):
        f, scalar = fns(pkg, dtype)
        size = np.dtype(dtype).itemsize
        n, b = 1024, 3
        span, ws_bytes = 4 * n * b * size, workspace_bytes(n, b, size)
        ok = dict(new=0x100000000, old=0x200000000, vel=0x300000000, acc=0x400000000, jerk=0x500000000, ws=0x600000000, params=0x700000000, clocks=0x800000000,
                  status=0x900000000, eps=0xa00000000, dt=0xb00000000, ws_bytes=ws_bytes, n=n, b=b, t_stop=1.0, dt_max=0.5)
        length = dict(new=span, old=span, vel=span, acc=span, jerk=span, ws=ws_bytes, params=4 * b * size, clocks=32 * b, status=64, eps=b * size, dt=b * size)
        align = dict(new=4 * size, old=4 * size, vel=4 * size, acc=4 * size, jerk=4 * size, ws=4 * size, params=4 * size, clocks=8, status=8, eps=size, dt=size)
        sizes_bad = (dict(n=0), dict(b=0), dict(n=MAX_N + 1), dict(n=MAX_N, b=MAX_TOTAL // MAX_N + 1))

        def step(**kw):
            a = {**ok, **kw}
            return f["step"](a["new"], a["old"], a["vel"], a["acc"], a["jerk"], a["ws"], a["ws_bytes"], a["n"], a["b"], scalar(0.01), scalar(0.01), a["params"], None)

        def evaluate(**kw):
            a = {**ok, **kw}
            return f["eval"](a["acc"], a["jerk"], a["old"], a["vel"], a["n"], a["b"], scalar(0.01), a["eps"], None)

        def timestep(**kw):
            a = {**ok, **kw}
            return f["timestep"](a["acc"], a["jerk"], a["n"], a["b"], scalar(0.02), a["dt"], a["ws"], a["ws_bytes"], None)

        def begin(**kw):
            a = {**ok, **kw}
            return f["begin"](a["acc"], a["jerk"], a["old"], a["vel"], a["clocks"], a["n"], a["b"], scalar(0.01), a["eps"], scalar(0.02), a["ws"], a["ws_bytes"], None)

        def advance(**kw):
            a = {**ok, **kw}
            return f["advance"](a["new"], a["old"], a["vel"], a["acc"], a["jerk"], a["clocks"], a["status"], a["ws"], a["ws_bytes"], a["n"], a["b"], a["t_stop"], a["dt_max"],
                                scalar(0.02), scalar(0.01), a["eps"], None)

        calls = ((step, ("new", "old", "vel", "acc", "jerk", "ws", "params"), ("params",)),
                 (evaluate, ("acc", "jerk", "old", "vel", "eps"), ("eps",)),
                 (timestep, ("acc", "jerk", "dt", "ws"), ()),
                 (begin, ("acc", "jerk", "old", "vel", "clocks", "ws", "eps"), ("eps",)),
                 (advance, ("new", "old", "vel", "acc", "jerk", "clocks", "status", "ws", "eps"), ("status", "eps")))
        for call, names, optional in calls:
            for name in names:
                if name not in optional:
                    assert call(**{name: None}) == ERR, (call.__name__, name, "null")
                assert call(**{name: ok[name] + align[name] // 2}) == ERR, (call.__name__, name, "misaligned")
            for bad in sizes_bad:
                assert call(**bad) == ERR, (call.__name__, bad)
            if "ws" in names:
                assert call(ws_bytes=ws_bytes - 1) == ERR and call(ws_bytes=0) == ERR, call.__name__
            for x in names:  # every pair of arrays, overlapping by one element at either end
                for y in names:
                    if x == y:
                        continue
                    assert call(**{x: ok[y] + length[y] - align[x]}) == ERR, (call.__name__, x, "on the end of", y)
                    assert call(**{x: ok[y] - length[x] + align[x]}) == ERR, (call.__name__, x, "running into", y)
                    if {x, y} != {"new", "old"}:
                        assert call(**{x: ok[y]}) == ERR, (call.__name__, x, "==", y)
        assert step(new=ok["old"] + 4 * size) == ERR and advance(new=ok["old"] + 4 * size) == ERR  # the SAME array, not a shifted one
        for bad in (dict(t_stop=float("nan")), dict(dt_max=0.0), dict(dt_max=-1.0), dict(dt_max=float("nan"))):
            assert advance(**bad) == ERR, bad
        if no_gpu:  # past the argument check: a HIP error
            assert step(new=ok["old"]) not in (0, ERR) and advance(new=ok["old"], status=None, eps=None, dt_max=float("inf")) not in (0, ERR)
            assert step(params=None) not in (0, ERR) and evaluate(eps=None) not in (0, ERR)


def test_hermite_ensemble_plan_is_hermite_plan_per_system(pkg):
    for dtype in (np.float32, np.float64):
        f, _ = fns(pkg, dtype)
        for n in (1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 8229, 65536):
            solo = pkg.hermite_plan(n, dtype)
            seen = set()
            for b in (1, 3, 256, 4096):
                p = pkg.hermite_ensemble_plan(n, b, dtype)
                assert (p.waves_per_group, p.bodies_per_lane, p.unroll, p.lds_bytes, p.groups, p.block_threads) == \
                    (solo.waves_per_group, solo.bodies_per_lane, solo.unroll, solo.lds_bytes, solo.groups, solo.block_threads), (n, b)
                assert p.groups_per_system == solo.groups and p.grid_blocks == solo.groups * b and p.reserved == 0
                seen.add((p.bodies_per_lane, p.waves_per_group, p.unroll, p.groups, p.block_threads, p.lds_bytes, p.groups_per_system))
            assert len(seen) == 1, n  # independent of B
        p = pkg.HermiteEnsemblePlan()
        for bad in ((0, 1), (1, 0), (MAX_N + 1, 1), (MAX_N, MAX_TOTAL // MAX_N + 1), (1, (1 << 25) + 1)):
            assert f["plan"](*bad, ctypes.byref(p)) == ERR, bad
        assert f["plan"](16, 16, None) == ERR


def ensemble_listing():
    subprocess.run(["make", "-s", "-C", CSRC, "hermite_ensemble.s"], check=True, capture_output=True)
    return open(os.path.join(CSRC, "hermite_ensemble.s")).read()


def test_hermite_ensemble_streaming_loops_keep_hermite_evals_mix():
    """Every streaming loop of the fp32 hermite_ensemble_eval kernels, as test_hermite_streaming_loops_keep_their_mix counts hermite_eval's:
    2 v_rsq_f32 and 25 (no mass multiply) or 26 v_pk_* per packed pair, bodies j by s_load, no LDS, scratch or barrier instruction and no
    v_mov; no kernel of the file uses scratch or more than 128 VGPRs."""
    text = ensemble_listing()
    seen = 0
    for name, lines in kernels_of(text):
        if "hermite_ensemble_evalIf" not in name:
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
    assert len(sizes) == 23 and max(sizes) == 0, sizes
    assert len(vgprs) == 23 and max(vgprs) <= 128, vgprs
    assert "_atomic" not in text


# ---------------------------------------------------------------------------------------------------------------- the registry of hermite_ensemble.s
# Every kernel of the listing, once, with the GPU test of this file that reaches it and the shapes (N, B) it is reached with there.
def ensemble_registry():
    out = {}
    for dtype in (F32, F64):
        t = "float" if dtype == F32 else "double"
        for s, sizes in N_BY_WAVES.items():
            shapes = [(n, 3) for n in sizes if n in BIT_SIZES] + ([(1, 3), (2, 3), (129, 3)] if s == 1 else []) + (list(ENSEMBLE_LARGE) if s == 8 else [])
            assert shapes
            out[("hermite_ensemble_eval", (t, s, False))] = ("test_bits_against_the_solo_calls", shapes)
            out[("hermite_ensemble_eval", (t, s, True))] = ("test_bits_against_the_solo_calls", shapes)
        out[("hermite_ensemble_predict", (t,))] = ("test_bits_against_the_solo_calls", [(n, 3) for n in BIT_SIZES])
        out[("hermite_ensemble_timestep_partial", (t,))] = ("test_bits_against_the_solo_calls", [(n, 3) for n in BIT_SIZES])
        out[("hermite_ensemble_clock", (t,))] = ("test_adaptive_advance_follows_the_rule", [(ADAPTIVE_N, ADAPTIVE_B)])
    out[("hermite_ensemble_status", ())] = ("test_adaptive_advance_follows_the_rule", [(ADAPTIVE_N, ADAPTIVE_B)])
    return out


ADAPTIVE_N, ADAPTIVE_B = 300, 4


def test_every_kernel_of_the_listing_is_in_the_registry(pkg):
    listed = listed_kernels(ensemble_listing())
    assert len(listed) == len(set(listed)) == 23
    registry = ensemble_registry()
    missing = sorted(kernel_name(k) for k in set(listed) - set(registry))
    stale = sorted(kernel_name(k) for k in set(registry) - set(listed))
    assert not missing, f"kernels of hermite_ensemble.s no case reaches: {missing}"
    assert not stale, f"cases that name no kernel of hermite_ensemble.s: {stale}"
    for (family, args), (test, shapes) in registry.items():
        assert test in globals(), test
        if family == "hermite_ensemble_eval":  # the shapes reach the instantiation: S follows N
            for n, b in shapes:
                assert pkg.hermite_ensemble_plan(n, b, F32 if args[0] == "float" else F64).waves_per_group == args[1], (family, args, n)
    sizes = {n for n, _ in registry[("hermite_ensemble_predict", ("float",))][1]}
    assert sizes == set(BIT_SIZES)


def test_hermite_ensemble_sources_use_no_atomics_and_share_the_text():
    source = open(os.path.join(CSRC, "hermite_ensemble.hip")).read()
    for fragment in ('#include "hermite_stream.inc"', '#include "hermite_correct.inc"', '#include "hermite_body.h"', '#include "hermite_stream.h"', '#include "hermite_ratio.h"'):
        assert fragment in source, fragment
    for name in ("hermite_ensemble.hip", "hermite_ensemble_capi.hip", "hermite_ensemble_boundary.h", "hermite_ensemble_kernels.h"):
        text = open(os.path.join(CSRC, name)).read()
        for word in ("atomic", "hipMalloc", "hipFree", "Synchronize", "mutex", "static "):
            assert word not in text.replace("static_assert", "").replace("static_cast", "").replace("No atomics", "").replace("no atomics", ""), (name, word)


# ---------------------------------------------------------------------------------------------------------------- GPU
gpu_only = pytest.mark.gpu


class Ensemble:
    """the arrays of B systems on the device, through the C calls; `pad` canary bodies on either side of every array"""

    def __init__(self, gpu, pos, vel, eps2, pad=0, ws_fill=None):
        self.gpu, self.dtype = gpu, pos.dtype
        self.b, self.n = pos.shape[0], pos.shape[1]
        self.f, self.scalar = fns(gpu, self.dtype)
        self.pad = pad
        size = self.dtype.itemsize
        self.ws_bytes = gpu.hermite_ensemble_workspace_bytes(self.n, self.b, self.dtype)
        assert self.ws_bytes == workspace_bytes(self.n, self.b, size)
        self.canary = np.full(4 * pad, 1234.5, self.dtype)
        self.bufs = {}
        bodies = 4 * self.n * self.b
        for name, count in (("pos", bodies), ("pos2", bodies), ("vel", bodies), ("acc", bodies), ("jerk", bodies), ("ws", self.ws_bytes // size), ("eps", self.b),
                            ("params", 4 * self.b), ("dt", self.b), ("clocks", 32 * self.b // size), ("status", 64 // size)):
            host = np.concatenate([self.canary, np.zeros(count, self.dtype), self.canary])
            if name == "ws" and ws_fill is not None:
                host[4 * pad:4 * pad + count] = ws_fill
            buf = gpu.DeviceBuffer(host.nbytes)
            buf.upload(host)
            self.bufs[name] = buf
        self.eps2 = np.broadcast_to(np.asarray(eps2, self.dtype), (self.b,)).copy()
        self.put("pos", pos), self.put("vel", vel), self.put("eps", self.eps2)

    def ptr(self, name):
        return self.bufs[name].ptr.value + 4 * self.pad * self.dtype.itemsize

    def put(self, name, data):
        data = np.ascontiguousarray(data)
        self.gpu.check(self.gpu.lib().nb_h2d(self.ptr(name), data.ctypes.data, data.nbytes, None), "nb_h2d")

    def read(self, name, out):
        self.gpu.check(self.gpu.lib().nb_d2h(out.ctypes.data, self.ptr(name), out.nbytes, None), "nb_d2h")
        return out

    def get(self, name):
        return self.read(name, np.empty((self.b, self.n, 4), self.dtype))

    def predicted(self):
        return self.read("ws", np.empty((self.b, self.n, 8), self.dtype))

    def canaries_intact(self):
        for buf in self.bufs.values():
            host = buf.download(np.empty(buf.nbytes // self.dtype.itemsize, self.dtype))
            if self.pad and not (host[:4 * self.pad].tobytes() == self.canary.tobytes() and host[-4 * self.pad:].tobytes() == self.canary.tobytes()):
                return False
        return True

    def eval(self, stream=None):
        self.gpu.check(self.f["eval"](self.ptr("acc"), self.ptr("jerk"), self.ptr("pos"), self.ptr("vel"), self.n, self.b, self.scalar(0), self.ptr("eps"), stream),
                       "nb_hermite_ensemble_eval")

    def step(self, dt, new="pos", old="pos", stream=None):
        """dt: one value per system -> system_params; a scalar -> the scalar arguments (then every system has eps2[0])"""
        if np.ndim(dt) == 0:
            args = (self.scalar(dt), self.scalar(self.eps2[0]), None)
        else:
            table = np.zeros((self.b, 4), self.dtype)
            table[:, 0], table[:, 1], table[:, 2:] = dt, self.eps2, 77.0  # (the last two are ignored)
            self.put("params", table)
            args = (self.scalar(0), self.scalar(0), self.ptr("params"))
        self.gpu.check(self.f["step"](self.ptr(new), self.ptr(old), self.ptr("vel"), self.ptr("acc"), self.ptr("jerk"), self.ptr("ws"), self.ws_bytes, self.n, self.b, *args,
                                      stream), "nb_hermite_ensemble_step")

    def timestep(self, eta, stream=None):
        self.gpu.check(self.f["timestep"](self.ptr("acc"), self.ptr("jerk"), self.n, self.b, self.scalar(eta), self.ptr("dt"), self.ptr("ws"), self.ws_bytes, stream),
                       "nb_hermite_ensemble_timestep")
        return self.read("dt", np.empty(self.b, self.dtype))

    def begin(self, eta, stream=None):
        self.gpu.check(self.f["begin"](self.ptr("acc"), self.ptr("jerk"), self.ptr("pos"), self.ptr("vel"), self.ptr("clocks"), self.n, self.b, self.scalar(0), self.ptr("eps"),
                                       self.scalar(eta), self.ptr("ws"), self.ws_bytes, stream), "nb_hermite_ensemble_begin")

    def advance(self, t_stop, dt_max, eta, stream=None, status=True):
        self.gpu.check(self.f["advance"](self.ptr("pos"), self.ptr("pos"), self.ptr("vel"), self.ptr("acc"), self.ptr("jerk"), self.ptr("clocks"),
                                         self.ptr("status") if status else None, self.ptr("ws"), self.ws_bytes, self.n, self.b, float(t_stop), float(dt_max), self.scalar(eta),
                                         self.scalar(0), self.ptr("eps"), stream), "nb_hermite_ensemble_advance")

    def clocks(self):
        return self.read("clocks", np.empty(self.b, self.gpu.HERMITE_ENSEMBLE_CLOCK_DTYPE))

    def status(self):
        return self.read("status", np.empty(64, np.uint8)).tobytes()

    def state(self, pos="pos"):
        return tuple(self.get(k) for k in (pos, "vel", "acc", "jerk"))

    def free(self):
        for buf in self.bufs.values():
            buf.free()


def solo_timestep(gpu, d, eta):
    """nb_hermite_timestep_* of a tests/test_hermite.py Device"""
    f, scalar = solo_fns(gpu, d.dtype)
    out, scratch = gpu.DeviceBuffer(8), gpu.DeviceBuffer(8192)
    gpu.check(f["timestep"](d.ptr("acc"), d.ptr("jerk"), d.n, scalar(eta), out.ptr, scratch.ptr, 8192, None), "nb_hermite_timestep")
    dt = out.download(np.empty(1, d.dtype))[0]
    out.free(), scratch.free()
    return dt


def systems_of(n, b, dtype, seed=500):
    """B clouds of tests/test_hermite.py, one kind of masses (kernel_matrix.MASSES) per system"""
    clouds = [cloud(n, dtype, seed + 10 * s + n, MASSES[s % len(MASSES)]) for s in range(b)]
    return np.stack([c[0] for c in clouds]), np.stack([c[1] for c in clouds])


def same_bits(got, want, what):
    for g, w, name in zip(got, want, ("pos", "vel", "acc", "jerk")):
        assert g.tobytes() == w.tobytes(), (what, name)


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,b", [(n, 3) for n in BIT_SIZES] + list(ENSEMBLE_LARGE))
def test_bits_against_the_solo_calls(gpu, dtype, n, b):
    """eval, one step and the time step of every system are the bits of nb_hermite_eval_* / _step_* / _timestep_* on that system alone, with a dt
    and a softening^2 (0 among them: the floor) per system; one system per S also meets the long double bounds of tests/test_hermite.py"""
    pos, vel = systems_of(n, b, dtype)
    dts, eps2 = np.array(SYSTEM_DT[:b], dtype), np.array(SYSTEM_EPS2[:b], dtype)
    eta = dtype(0.02)
    e = Ensemble(gpu, pos, vel, eps2)
    e.eval()
    acc0, jerk0 = e.get("acc"), e.get("jerk")
    dt0 = e.timestep(eta)
    e.step(dts, new="pos2", old="pos")
    stepped, predicted = e.state("pos2"), e.predicted()
    dt1 = e.timestep(eta)
    assert e.get("pos").tobytes() == pos.tobytes()
    e.free()
    for s in range(b):
        d = Device(gpu, pos[s], vel[s], eps2[s])
        d.eval()
        assert acc0[s].tobytes() == d.get("acc").tobytes() and jerk0[s].tobytes() == d.get("jerk").tobytes(), ("eval", n, s)
        assert dt0[s].tobytes() == solo_timestep(gpu, d, eta).tobytes(), ("timestep", n, s)
        d.step(dts[s], new="pos2", old="pos")
        same_bits([q[s] for q in stepped], d.state("pos2"), ("step", n, s))
        assert predicted[s].tobytes() == d.get("ws").tobytes(), ("predicted", n, s)
        assert dt1[s].tobytes() == solo_timestep(gpu, d, eta).tobytes(), ("timestep after the step", n, s)
        d.free()
    if n == 1:
        assert np.isposinf(dt0).all()  # a body alone has no jerk
    if n in LONG_DOUBLE_SIZES:
        assert gpu.hermite_ensemble_plan(n, b, dtype).waves_per_group == LONG_DOUBLE_SIZES[n]
        s = 0  # (softening^2 0.01, equal masses)
        check_eval(acc0[s], jerk0[s], pos[s], vel[s], eps2[s], f"ensemble n {n} system {s}")
        want, bounds = ld_step(pos[s], vel[s], acc0[s], jerk0[s], dts[s], eps2[s], predicted[s])
        for name, g, w, bound in zip(("position", "velocity", "acceleration", "jerk"), stepped, want, bounds):
            assert (np.abs(g[s][:, :3].astype(LD) - w) <= bound).all(), (n, name)


def garbage(n, dtype):
    rng = np.random.default_rng(99)
    bad = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype), size=(n, 4))
    return bad, bad.copy()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_system_does_not_depend_on_where_it_is(gpu, dtype):
    """N = 517 (S = 4, five tiles fp32, the last ragged): the system's four arrays after eval + one step are the same bits alone (B = 1), at
    index 3 of 5, between systems of NaN and inf, called twice, on another stream, with a workspace of NaN, in place and ping-pong."""
    n, eps2, dt = 517, dtype(0.01), dtype(1.0 / 64)
    pos, vel = cloud(n, dtype, 4242, "species")
    lib = gpu.lib()

    def run(b, index, others, new="pos2", stream=None, **kw):
        p, v = systems_of(n, b, dtype, seed=900)
        if others == "garbage":
            for s in range(b):
                p[s], v[s] = garbage(n, dtype)
        p[index], v[index] = pos, vel
        e = Ensemble(gpu, p, v, eps2, pad=64, **kw)
        if stream is not None:
            gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
        e.eval(stream=stream)
        e.step(dt, new=new, old="pos", stream=stream)
        if stream is not None:
            gpu.check(lib.nb_stream_synchronize(stream), "nb_stream_synchronize")
        got = [q[index] for q in e.state(new)]
        assert e.canaries_intact()
        if new == "pos2":
            assert e.get("pos").tobytes() == p.tobytes()  # old positions untouched by a ping-pong step
        if others == "garbage":  # ... and the garbage stays garbage, it does not fault
            assert not np.isfinite(e.get("acc")[(index + 1) % b, :, :3]).any()
        e.free()
        return got

    want = run(1, 0, "clouds")
    assert want[0][:, 3].tobytes() == pos[:, 3].tobytes() and want[1][:, 3].tobytes() == vel[:, 3].tobytes()  # masses and velocity .w come through
    assert not want[2][:, 3].any() and not want[3][:, 3].any()
    d = Device(gpu, pos, vel, eps2)
    d.eval(), d.step(dt, new="pos2", old="pos")
    same_bits(want, d.state("pos2"), "the solo calls")
    d.free()
    same_bits(run(5, 3, "clouds"), want, "index 3 of 5")
    same_bits(run(5, 3, "garbage"), want, "between systems of NaN and inf")
    same_bits(run(5, 3, "clouds"), want, "called twice")
    same_bits(run(5, 3, "clouds", ws_fill=np.nan), want, "NaN in the workspace")
    same_bits(run(5, 3, "clouds", new="pos", ws_fill=1e30), want, "in place")
    stream = ctypes.c_void_p()
    gpu.check(lib.nb_stream_create(ctypes.byref(stream)), "nb_stream_create")
    same_bits(run(5, 3, "clouds", stream=stream), want, "another stream")
    gpu.check(lib.nb_stream_destroy(stream), "nb_stream_destroy")


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_time_step_edge_cases_per_system(gpu, dtype):
    """What test_shared_time_step plants, per system: a zero-jerk body and a NaN jerk are left out, a zero acceleration is the minimum; a system
    of one body has no jerk: +inf.  Each system against nb_hermite_timestep_* on it alone (bits) and the long double minimum (2 ulp)."""
    eta, u = dtype(0.02), UNIT_ROUNDOFF[dtype]
    one = Ensemble(gpu, *systems_of(1, 3, dtype), dtype(0.01))
    one.eval()
    assert np.isposinf(one.timestep(eta)).all()
    one.free()
    n, b = 300, 3
    pos, vel = systems_of(n, b, dtype, seed=1300)
    e = Ensemble(gpu, pos, vel, dtype(0.01), ws_fill=np.nan)
    e.eval()
    acc, jerk = e.get("acc"), e.get("jerk")
    jerk[0, 5] = 0               # system 0: a zero-jerk body is left out
    jerk[1, 9, 0] = np.nan       # system 1: a non-finite ratio is left out
    jerk[2, 5], jerk[2, 9, 0] = 0, np.nan
    acc[2, 7, :3] = 0            # system 2: both, and a zero acceleration is the minimum
    e.put("acc", acc), e.put("jerk", jerk)
    got = e.timestep(eta)
    assert got.tobytes() == e.timestep(eta).tobytes()
    e.free()
    for s in range(b):
        d = Device(gpu, pos[s], vel[s], dtype(0.01))
        d.put("acc", acc[s]), d.put("jerk", jerk[s])
        assert got[s].tobytes() == solo_timestep(gpu, d, eta).tobytes(), s
        d.free()
        a2, j2 = (acc[s][:, :3].astype(LD) ** 2).sum(axis=1), (jerk[s][:, :3].astype(LD) ** 2).sum(axis=1)
        with np.errstate(all="ignore"):
            ratio = np.sqrt(a2 / j2)
        want = LD(eta) * ratio[(j2 > 0) & np.isfinite(ratio)].min()
        assert abs(LD(got[s]) - want) <= 2 * u * want, (s, got[s], want)
    assert got[2] == 0 and got[0] > 0 and got[1] > 0


# ---------------------------------------------------------------------------------------------------------------- the adaptive form
ADAPTIVE_ETA, ADAPTIVE_T_STOP, ADAPTIVE_DT_MAX, ADAPTIVE_CALLS = 0.02, 1.0 / 16, 0.6 / 16, 12
ADAPTIVE_EPS2 = (0.01, 1e-6, 0.01, 1.0)


def adaptive_systems(dtype):
    """N = 300, B = 4: a calm cloud; the same cloud with the hard binary of DESIGN.md 5.7 (bodies 0 and 1 a circular binary of separation 0.01
    and four times the mass each); a cloud so light and slow that dt_max bounds its steps: t_stop reached after two; a cloud at rest with a
    large softening: every jerk is 0 after begin, dt_next = +inf, and dt_max is the first step."""
    n = ADAPTIVE_N
    calm = cloud(n, np.float64, 1992)
    pos, vel = calm[0].copy(), calm[1].copy()
    sep, m = 0.01, 4 * pos[0, 3]
    pos[0, 3] = pos[1, 3] = m
    c, cv = pos[0, :3].copy(), vel[0, :3].copy()
    pos[0, :3], pos[1, :3] = c + [sep / 2, 0, 0], c - [sep / 2, 0, 0]
    orbit = np.sqrt(m / (2 * sep))
    vel[0, :3], vel[1, :3] = cv + [0, orbit, 0], cv - [0, orbit, 0]
    light = cloud(n, np.float64, 7)
    light[0][:, 3] *= 1e-6
    light[1][:, :3] *= 1e-3
    rest = cloud(n, np.float64, 8)
    rest[1][:, :3] = 0
    systems = (calm, (pos, vel), light, rest)
    return np.stack([s[0] for s in systems]).astype(dtype), np.stack([s[1] for s in systems]).astype(dtype)


def numpy_rule(clock, t_stop, dt_max, dtype):
    """The rule of the header as far as it is a function of the clock before the call: ("skip" | "finish" | "step" | "last", dt)"""
    if clock["flags"] & (DONE | STALLED):
        return "skip", None
    remaining = np.float64(t_stop) - np.float64(clock["time"])
    if not remaining > 0 or dtype(remaining) == 0:
        return "finish", None
    cand = min(np.float64(clock["dt_next"]), np.float64(dt_max))
    if cand >= remaining:
        return "last", dtype(remaining)
    return "step", dtype(cand)


class SoloRun:
    """B systems driven one by one through nb_hermite_eval_* / _step_* / _timestep_* by the rule of the header restated in numpy"""

    def __init__(self, gpu, pos, vel, eps2, eta):
        self.gpu, self.dtype, self.eta = gpu, pos.dtype.type, pos.dtype.type(eta)
        self.devices = [Device(gpu, pos[s], vel[s], pos.dtype.type(eps2[s])) for s in range(pos.shape[0])]
        self.clocks = []
        for d in self.devices:
            d.eval()
            dt = solo_timestep(gpu, d, self.eta)
            self.clocks.append(dict(time=0.0, dt_next=float(dt), dt_last=0.0, steps=0, flags=0 if dt > 0 else STALLED))

    def advance(self, t_stop, dt_max):
        """one call; returns the status record it should leave, as a dict"""
        stepped, dt_last = 0, np.inf
        for d, c in zip(self.devices, self.clocks):
            what, dt = numpy_rule(c, t_stop, dt_max, self.dtype)
            if what == "finish":
                c["flags"] |= DONE
                c["time"] = float(t_stop)
            elif what in ("step", "last"):
                d.step(dt)
                c["time"] = float(t_stop) if what == "last" else float(np.float64(c["time"]) + np.float64(dt))
                c["dt_last"] = float(dt)
                c["steps"] += 1
                c["dt_next"] = float(solo_timestep(self.gpu, d, self.eta))
                if what == "last":
                    c["flags"] |= DONE
                if not c["dt_next"] > 0 and not c["flags"] & DONE:
                    c["flags"] |= STALLED
                stepped += 1
                dt_last = min(dt_last, c["dt_last"])
        return dict(systems=len(self.clocks), done=sum(1 for c in self.clocks if c["flags"] & DONE), stalled=sum(1 for c in self.clocks if c["flags"] & STALLED),
                    stepped=stepped, total_steps=sum(c["steps"] for c in self.clocks), min_time=min(c["time"] for c in self.clocks), min_dt_last=dt_last)

    def state(self):
        return tuple(np.stack([d.get(k) for d in self.devices]) for k in ("pos", "vel", "acc", "jerk"))

    def free(self):
        for d in self.devices:
            d.free()


def clocks_as_bytes(gpu, clocks):
    out = np.zeros(len(clocks), gpu.HERMITE_ENSEMBLE_CLOCK_DTYPE)
    for i, c in enumerate(clocks):
        out[i] = (c["time"], c["dt_next"], c["dt_last"], c["steps"], c["flags"])
    return out.tobytes()


def status_as_bytes(gpu, s):
    record = gpu.HermiteEnsembleStatus(s["systems"], s["done"], s["stalled"], s["stepped"], s["total_steps"], s["min_time"], s["min_dt_last"])
    return bytes(record)


_ADAPTIVE = {}


def adaptive_single_calls(gpu, dtype):
    """begin + 12 single calls, clocks, status and state read after each and held to the numpy restatement; what they leave, for the tests after"""
    key = np.dtype(dtype).name
    if key in _ADAPTIVE:
        return _ADAPTIVE[key]
    pos, vel = adaptive_systems(dtype)
    eps2 = np.array(ADAPTIVE_EPS2, dtype)
    e = Ensemble(gpu, pos, vel, eps2, pad=16, ws_fill=np.nan)
    solo = SoloRun(gpu, pos, vel, eps2, ADAPTIVE_ETA)
    e.begin(ADAPTIVE_ETA)
    assert e.clocks().tobytes() == clocks_as_bytes(gpu, solo.clocks), (e.clocks(), solo.clocks)
    same_bits(e.state(), solo.state(), "begin")
    assert np.isposinf(solo.clocks[3]["dt_next"]) and solo.clocks[3]["flags"] == 0  # the cloud at rest: no jerk, +inf counts as > 0
    history = []
    for call in range(ADAPTIVE_CALLS):
        before = e.state()
        flags = e.clocks()["flags"].copy()
        e.advance(ADAPTIVE_T_STOP, ADAPTIVE_DT_MAX, ADAPTIVE_ETA)
        want_status = solo.advance(ADAPTIVE_T_STOP, ADAPTIVE_DT_MAX)
        clocks, state = e.clocks(), e.state()
        assert clocks.tobytes() == clocks_as_bytes(gpu, solo.clocks), (call, clocks, solo.clocks)
        assert e.status() == status_as_bytes(gpu, want_status), (call, want_status)
        same_bits(state, solo.state(), f"call {call}")
        for s in range(ADAPTIVE_B):  # a system that was done before the call is left bit-identical
            if flags[s] & DONE:
                same_bits([q[s] for q in state], [q[s] for q in before], f"call {call}: done system {s}")
        history.append(clocks.copy())
    assert e.canaries_intact()
    final = dict(state=e.state(), clocks=e.clocks().tobytes(), status=e.status(), history=history, steps=e.clocks()["steps"].copy())
    e.free(), solo.free()
    _ADAPTIVE[key] = final
    return final


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_adaptive_advance_follows_the_rule(gpu, dtype):
    final = adaptive_single_calls(gpu, dtype)
    history = final["history"]
    # the light cloud: dt_max, then what remains -- done after two steps, and left alone from then on
    assert history[0]["steps"][2] == 1 and history[1]["steps"][2] == 2 and history[1]["flags"][2] == DONE and history[-1]["steps"][2] == 2
    assert history[0]["dt_last"][2] == dtype(ADAPTIVE_DT_MAX) and history[1]["time"][2] == ADAPTIVE_T_STOP
    # the cloud at rest: +inf after begin, so dt_max is its first step
    assert history[0]["dt_last"][3] == dtype(ADAPTIVE_DT_MAX) and np.isfinite(history[0]["dt_next"][3])
    # the binary sets the step of its own system only
    assert history[-1]["dt_last"][1] < history[-1]["dt_last"][0]
    assert not (history[-1]["flags"] & STALLED).any()
    # run to the end: every system done at t_stop exactly, and the system with the binary took more steps than the calm one
    pos, vel = adaptive_systems(dtype)
    e = Ensemble(gpu, pos, vel, np.array(ADAPTIVE_EPS2, dtype))
    e.begin(ADAPTIVE_ETA)
    for _ in range(80):  # batches of 25 calls, 64 bytes read after each
        for _ in range(25):
            e.advance(ADAPTIVE_T_STOP, ADAPTIVE_DT_MAX, ADAPTIVE_ETA)
        status = gpu.HermiteEnsembleStatus.from_buffer_copy(e.status())
        if status.done + status.stalled == status.systems:
            break
    e.advance(ADAPTIVE_T_STOP, ADAPTIVE_DT_MAX, ADAPTIVE_ETA)  # (a call that finds every system done)
    status = gpu.HermiteEnsembleStatus.from_buffer_copy(e.status())
    clocks = e.clocks()
    e.free()
    print("steps per system", clocks["steps"], "status", status.done, status.stalled, status.total_steps)
    assert status.done == ADAPTIVE_B and status.stalled == 0 and status.stepped == 0 and status.min_time == ADAPTIVE_T_STOP and np.isposinf(status.min_dt_last)
    assert (clocks["flags"] == DONE).all() and (clocks["time"] == ADAPTIVE_T_STOP).all() and status.total_steps == clocks["steps"].sum()
    assert clocks["steps"][1] > clocks["steps"][0] and clocks["steps"][2] == 2


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_adaptive_calls_in_a_graph_and_in_a_batch(gpu, dtype):
    """The 12 calls recorded in one stream capture and replayed, and begin + 12 enqueued without a host read between them, leave the bits of
    the 12 single calls."""
    final = adaptive_single_calls(gpu, dtype)
    pos, vel = adaptive_systems(dtype)
    eps2 = np.array(ADAPTIVE_EPS2, dtype)
    lib = gpu.lib()

    def same(e, what):
        same_bits(e.state(), final["state"], what)
        assert e.clocks().tobytes() == final["clocks"] and e.status() == final["status"], what

    batch = Ensemble(gpu, pos, vel, eps2)
    batch.begin(ADAPTIVE_ETA)
    for _ in range(ADAPTIVE_CALLS):
        batch.advance(ADAPTIVE_T_STOP, ADAPTIVE_DT_MAX, ADAPTIVE_ETA)
    same(batch, "a batch")
    batch.free()

    stream = ctypes.c_void_p()
    gpu.check(lib.nb_stream_create(ctypes.byref(stream)), "nb_stream_create")
    hip = hip_runtime()
    captured = Ensemble(gpu, pos, vel, eps2)
    captured.begin(ADAPTIVE_ETA)
    begun = captured.clocks().tobytes()
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    graph, graph_exec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0
    for _ in range(ADAPTIVE_CALLS):
        captured.advance(ADAPTIVE_T_STOP, ADAPTIVE_DT_MAX, ADAPTIVE_ETA, stream=stream)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
    assert captured.clocks().tobytes() == begun  # recorded, not run
    assert hip.hipGraphInstantiate(ctypes.byref(graph_exec), graph, None, None, 0) == 0
    assert hip.hipGraphLaunch(graph_exec, stream) == 0
    gpu.check(lib.nb_stream_synchronize(stream), "nb_stream_synchronize")
    same(captured, "captured and replayed")
    assert hip.hipGraphExecDestroy(graph_exec) == 0 and hip.hipGraphDestroy(graph) == 0
    captured.free()
    gpu.check(lib.nb_stream_destroy(stream), "nb_stream_destroy")

    # without a status record the clocks and the state are the same
    quiet = Ensemble(gpu, pos, vel, eps2)
    quiet.begin(ADAPTIVE_ETA)
    for _ in range(ADAPTIVE_CALLS):
        quiet.advance(ADAPTIVE_T_STOP, ADAPTIVE_DT_MAX, ADAPTIVE_ETA, status=False)
    same_bits(quiet.state(), final["state"], "no status")
    assert quiet.clocks().tobytes() == final["clocks"] and quiet.status() == bytes(64)
    quiet.free()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_python_class_gives_the_c_calls_bits(gpu, dtype):
    n, b = 333, 3
    pos, vel = systems_of(n, b, dtype, seed=70)
    eps2, dts, eta = np.array(SYSTEM_EPS2, dtype), np.array(SYSTEM_DT, dtype), dtype(0.02)
    e = Ensemble(gpu, pos, vel, eps2)
    e.eval()
    e.step(dts), e.step(dts)
    want, want_dt = e.state(), e.timestep(eta)
    system = gpu.HermiteEnsemble(n, b, dtype, softening_sq=eps2)
    system.set_state(pos, vel)
    system.eval()
    system.step(dts), system.step(dts)
    same_bits((system.get_positions(), system.get_velocities(), system.get_accelerations(), system.get_jerks()), want, "eval and two steps")
    assert system.suggested_dt(eta).tobytes() == want_dt.tobytes()
    # a scalar dt and a scalar softening^2 take the scalar arguments
    e.put("eps", np.full(b, eps2[0], dtype)), setattr(e, "eps2", np.full(b, eps2[0], dtype))
    e.put("pos", pos), e.put("vel", vel)
    e.eval(), e.step(dts[0])
    want = e.state()
    scalars = gpu.HermiteEnsemble(n, b, dtype, softening_sq=eps2[0])
    scalars.set_state(pos, vel)
    scalars.eval(), scalars.step(dts[0])
    same_bits((scalars.get_positions(), scalars.get_velocities(), scalars.get_accelerations(), scalars.get_jerks()), want, "scalars")
    scalars.free()
    # the adaptive form
    e.put("eps", eps2), setattr(e, "eps2", eps2)
    e.put("pos", pos), e.put("vel", vel)
    e.begin(eta)
    for _ in range(3):
        e.advance(0.05, 0.01, eta)
    system.set_state(pos, vel)
    system.begin(eta)
    system.advance(0.05, eta, dt_max=0.01, calls=3)
    same_bits((system.get_positions(), system.get_velocities(), system.get_accelerations(), system.get_jerks()), e.state(), "three adaptive calls")
    assert system.clocks().tobytes() == e.clocks().tobytes() and bytes(system.status()) == e.status()
    assert system.status().systems == b and (system.clocks()["steps"] == 3).all()
    system.free(), e.free()
    with pytest.raises(gpu.NBodyHipError):
        gpu.HermiteEnsemble(0, 3, dtype)
    with pytest.raises(gpu.NBodyHipError):
        gpu.HermiteEnsemble(MAX_N + 1, 1, dtype)


@gpu_only
def test_ensemble_step_beats_the_solo_steps(gpu):
    """N = 1 024, B = 256, fp32, device events, the median of 5 after warm-up: one ensemble step takes less time than the 256 nb_hermite_step_f32
    calls on the same systems, measured in the same process.  That ratio is the library's reason to exist, so the bar is 1."""
    n, b, dtype = 1024, 256, np.float32
    one = cloud(n, dtype, 1, "equal")
    pos, vel = np.broadcast_to(one[0], (b, n, 4)).copy(), np.broadcast_to(one[1], (b, n, 4)).copy()
    eps2, dt = dtype(0.01), dtype(1e-3)
    e = Ensemble(gpu, pos, vel, eps2)
    e.eval()
    solo, scalar = solo_fns(gpu, dtype)
    size = 4 * n * 4  # bytes of one system in an array of bodies

    def ensemble_step():
        e.step(dt)

    def solo_steps():
        for s in range(b):
            gpu.check(solo["step"](e.ptr("pos") + s * size, e.ptr("pos") + s * size, e.ptr("vel") + s * size, e.ptr("acc") + s * size, e.ptr("jerk") + s * size,
                                   e.ptr("ws") + 2 * s * size, 2 * size, n, scalar(dt), scalar(eps2), None), "nb_hermite_step")

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

    t_ensemble, t_solo = median_ms(ensemble_step), median_ms(solo_steps)
    e.free()
    print(f"ensemble step of {b} x {n}: {t_ensemble:.3f} ms; {b} solo steps: {t_solo:.3f} ms; ratio {t_solo / t_ensemble:.2f}")
    assert t_ensemble < t_solo, (t_ensemble, t_solo)


# ---------------------------------------------------------------------------------------------------------------- CLI
CLI = os.path.join(ROOT, "cuda-nbody_amd", "nbody")


def test_cli_rejects_what_the_hermite_ensemble_cannot_do(tmp_path):
    tipsy = tmp_path / "model.tipsy"
    tipsy.write_bytes(b"\0" * 64)
    base = ["--integrator=hermite-ensemble", "--systems=3", "--numbodies=1024"]
    run = base + ["--steps=1"]
    for extra in (["--integrator=hermite-ensemble", "--numbodies=1024", "--steps=1"], ["--integrator=hermite-ensemble", "--systems=3", "--steps=1"],
                  ["--integrator=hermite-ensemble", "--systems=3", "--numbodies=65537", "--steps=1"], ["--integrator=hermite-ensemble", "--systems=8192", "--numbodies=65536", "--steps=1"],
                  ["--integrator=hermite-ensemble", "--systems=0", "--numbodies=1024", "--steps=1"],
                  run + ["--mode=strict"], run + ["--numdevices=2"], run + ["--devices=0,1"], run + ["--hostmem"], run + [f"--tipsy={tipsy}"], run + ["--compare"],
                  run + ["--qatest"], run + ["--graph"], run + ["--energy"], run + ["--no-workspace"], run + ["--workspace-mib=64"], run + ["--levels=3"],
                  run + ["--t-end=0.5"], base + ["--benchmark", "--t-end=0.5"], base + ["--t-end=0"], base + ["--t-end=-1"], base + ["--t-end=nan"], base + ["--t-end=soon"],
                  base + ["--t-end=0.5", "--eta=0"], base + ["--t-end=0.5", "--eta=2"],
                  # --t-end elsewhere; --eta outside the block and ensemble integrators
                  ["--numbodies=1024", "--steps=1", "--t-end=0.5"], ["--systems=3", "--numbodies=1024", "--steps=1", "--t-end=0.5"],
                  ["--integrator=hermite", "--numbodies=1024", "--steps=1", "--t-end=0.5"], ["--systems=3", "--numbodies=1024", "--steps=1", "--eta=0.02"],
                  ["-integrator=hermite-ensemble", "-systems=3", "-numbodies=1024", "-steps=1", "-mode=strict"]):
        r = subprocess.run([CLI, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr, (extra, r.returncode, r.stderr[:300])
    # the messages that were there stay
    r = subprocess.run([CLI, "--systems=3", "--numbodies=1024", "--steps=1", "--eta=0.02"], capture_output=True, text=True, timeout=60)
    assert "--eta and --levels belong to --integrator=hermite-block" in r.stderr
    for integrator in ("hermite", "hermite-block"):
        r = subprocess.run([CLI, f"--integrator={integrator}", "--systems=3", "--numbodies=1024", "--steps=1"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--integrator=hermite cannot be combined with --systems" in r.stderr, integrator
    r = subprocess.run([CLI, *run, "--mode=strict"], capture_output=True, text=True, timeout=60)
    assert "--integrator=hermite-ensemble has no strict mode" in r.stderr
    r = subprocess.run([CLI, "--integrator=hermite-ensemble", "--numbodies=1024", "--steps=1"], capture_output=True, text=True, timeout=60)
    assert "--integrator=hermite-ensemble needs --systems" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--integrator TEXT [euler]   euler | hermite | hermite-block." in r.stdout
    assert "--integrator=hermite-ensemble" in r.stdout and "--t-end FLOAT" in r.stdout and "--eta FLOAT [0.02]          hermite-block:" in r.stdout


def cli_systems(oracle, n, b):
    """what `nbody --systems=B --numbodies=N` starts from: the single-system start-up state, then the next draws"""
    from oracle import scales_for
    pos0, vel0 = oracle.startup_state(n, np.float32)
    c, v = scales_for(n)
    draws = [(pos0, vel0)] + [oracle.randomise(1, n, c, v, np.float32) for _ in range(b - 1)]
    return np.stack([d[0].reshape(n, 4) for d in draws]), np.stack([d[1].reshape(n, 4) for d in draws])


@gpu_only
def test_cli_dump_of_fixed_steps_and_benchmark(gpu, oracle, tmp_path):
    """N = 1 024, B = 3, 10 steps of --integrator=hermite's dt: the dump is HermiteEnsemble's bits, and each system HermiteSystem's on it alone"""
    n, b, steps = 1024, 3, 10
    out = tmp_path / "ensemble.bin"
    r = subprocess.run([CLI, "--integrator=hermite-ensemble", f"--systems={b}", f"--numbodies={n}", f"--steps={steps}", f"--dump={out}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    data = np.fromfile(out, dtype=np.float32)
    assert data.size == 2 * 4 * n * b
    got_pos, got_vel = data[:4 * n * b].reshape(b, n, 4), data[4 * n * b:].reshape(b, n, 4)
    pos, vel = cli_systems(oracle, n, b)
    s = np.float32(0.1)
    eps2, dt = s * s, np.float32(0.016)
    ensemble = gpu.HermiteEnsemble(n, b, np.float32, softening_sq=eps2)
    ensemble.set_state(pos, vel)
    ensemble.eval()
    for _ in range(steps):
        ensemble.step(dt)
    assert got_pos.tobytes() == ensemble.get_positions().tobytes() and got_vel.tobytes() == ensemble.get_velocities().tobytes()
    ensemble.free()
    for i in range(b):
        system = gpu.HermiteSystem(n, np.float32, softening_sq=eps2)
        system.set_state(pos[i], vel[i])
        system.eval()
        for _ in range(steps):
            system.step(dt)
        assert got_pos[i].tobytes() == system.get_positions().tobytes() and got_vel[i].tobytes() == system.get_velocities().tobytes(), i
        system.free()
    r = subprocess.run([CLI, "--integrator=hermite-ensemble", f"--systems={b}", f"--numbodies={n}", "--benchmark", "-i=20"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"^(\d+) bodies x (\d+) systems, hermite integrator, total time for (\d+) iterations: ([\d.]+) ms\n= ([\d.]+) ms per step\n= ([\d.]+) billion interactions per second\n"
                  r"= ([\d.]+) single-precision GFLOP/s at 43 flops per acceleration \+ jerk interaction", r.stdout, re.M)
    assert m, r.stdout[-600:]
    assert (int(m[1]), int(m[2]), int(m[3])) == (n, b, 20)
    ms, ips = float(m[4]), float(m[6])
    want = b * n * n * 20 / (ms * 1e-3) * 1e-9  # B N^2 interactions per step
    assert abs(ips - want) <= 0.01 * want + 0.002, (ips, want)


@gpu_only
def test_cli_adaptive_run_to_t_end(gpu, oracle, tmp_path):
    """--t-end with --eta: every system done, the steps per system as HermiteEnsemble counts them, and the dump its bits"""
    n, b, t_end, eta = 512, 3, 0.05, 0.05
    out = tmp_path / "adaptive.bin"
    r = subprocess.run([CLI, "--integrator=hermite-ensemble", f"--systems={b}", f"--numbodies={n}", f"--t-end={t_end}", f"--eta={eta}", f"--dump={out}"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"^(\d+) bodies x (\d+) systems, hermite integrator, eta (\S+), to t = (\S+): (\d+) systems done, (\d+) stalled\n"
                  r"steps per system: fewest (\d+), median (\d+), most (\d+); (\d+) in all$", r.stdout, re.M)
    assert m, r.stdout[-600:]
    assert (int(m[1]), int(m[2]), float(m[3]), float(m[4]), int(m[5]), int(m[6])) == (n, b, eta, t_end, b, 0)
    pos, vel = cli_systems(oracle, n, b)
    s = np.float32(0.1)
    ensemble = gpu.HermiteEnsemble(n, b, np.float32, softening_sq=s * s)
    ensemble.set_state(pos, vel)
    ensemble.begin(np.float32(eta))
    while True:
        ensemble.advance(t_end, np.float32(eta), dt_max=t_end, calls=64)
        status = ensemble.status()
        if status.done + status.stalled == status.systems:
            break
    steps = np.sort(ensemble.clocks()["steps"])
    assert (int(m[7]), int(m[8]), int(m[9]), int(m[10])) == (steps[0], steps[b // 2], steps[-1], steps.sum())
    data = np.fromfile(out, dtype=np.float32)
    assert data[:4 * n * b].tobytes() == ensemble.get_positions().tobytes() and data[4 * n * b:].tobytes() == ensemble.get_velocities().tobytes()
    ensemble.free()
