"""nb_field_* on the MI355X (include/nbody_hip_field.h); the CPU part, the numpy restatement and the registry are tests/test_field.py.

Against long double sums from the same T-typed inputs, per target and component, under the bounds of the sister modules: TOL of
tests/test_fast_domain.py (5e-6 fp32, 1e-14 fp64) times the target's sum of term magnitudes,

    A = sum m s^-3 |r_k|,    J = sum m s^-3 (|w_k| + 3 (sum_c |r_c w_c|) s^-2 |r_k|),    P = sum m s^-1 = |phi|

(the form of tests/test_hermite.py's reference / check_eval).  Every instantiation of the registry, after the plan query selected it; shapes
(N, M) with targets off the sources, on them and excluded, on them and not excluded; the exact properties, bit for bit; the existing
libraries on targets == sources; the Python class and the command line; a speed sanity bound.  The worst error of every comparison is
printed as a fraction of its bound (DESIGN.md 5.9 quotes them)."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from kernel_matrix import F32, F64, TYPE_NAME, kernel_name
from test_fast_domain import TOL
from test_field import CLI, FLOOR, MODEL_JERK, MODEL_PLAIN, NONE, expected_plan, field_cases, plan_dict, scalar_of, suffix
from test_hermite import LD, cloud, hip_runtime

gpu_only = pytest.mark.gpu
WORST = {}  # (output, precision) -> the largest error seen, as a fraction of its bound


# ---------------------------------------------------------------------------------------------------------------- the yardstick


def field_reference(src, src_vel, tgt, tgt_vel, self_index, eps2, rows=None):
    """a, jerk (None without velocities), phi of targets `rows` (default: all) summed in long double from the T-typed inputs, and the sums of
    term magnitudes A, J, P in float64, which is plenty for a bound.  softening 0 is the header's floor."""
    kind = src.dtype.type
    m = tgt.shape[0]
    rows = np.arange(m) if rows is None else np.asarray(rows)
    floor = LD(eps2) if eps2 != 0 else LD(FLOOR[kind])
    with_jerk = src_vel is not None and tgt_vel is not None
    p, mass = src[:, :3].astype(LD), src[:, 3].astype(LD)
    v = src_vel[:, :3].astype(LD) if with_jerk else None
    a, jerk, phi = np.zeros((len(rows), 3), LD), np.zeros((len(rows), 3), LD) if with_jerk else None, np.zeros(len(rows), LD)
    A, J, P = np.zeros((len(rows), 3)), np.zeros((len(rows), 3)) if with_jerk else None, np.zeros(len(rows))
    block = max(1, min(256, (1 << 20) // src.shape[0]))
    for s in range(0, len(rows), block):
        i = rows[s:s + block]
        r = p[None, :, :] - tgt[i, None, :3].astype(LD)
        mk = np.broadcast_to(mass[None, :], (len(i), src.shape[0])).copy()
        if self_index is not None:
            hit = self_index[i] != NONE
            mk[np.nonzero(hit)[0], self_index[i][hit]] = 0
        s2 = (r * r).sum(axis=2) + floor
        inv = 1 / np.sqrt(s2)
        k3 = mk * inv / s2
        a[s:s + len(i)] = (k3[:, :, None] * r).sum(axis=1)
        phi[s:s + len(i)] = -(mk * inv).sum(axis=1)
        k64, r64 = np.abs(k3).astype(np.float64), np.abs(r).astype(np.float64)
        A[s:s + len(i)] = (k64[:, :, None] * r64).sum(axis=1)
        P[s:s + len(i)] = np.abs(mk * inv).astype(np.float64).sum(axis=1)
        if with_jerk:
            w = v[None, :, :] - tgt_vel[i, None, :3].astype(LD)
            t = 3 * (r * w).sum(axis=2) / s2
            jerk[s:s + len(i)] = (k3[:, :, None] * (w - t[:, :, None] * r)).sum(axis=1)
            w64 = np.abs(w).astype(np.float64)
            t64 = 3 * (r64 * w64).sum(axis=2) / s2.astype(np.float64)
            J[s:s + len(i)] = (k64[:, :, None] * (w64 + t64[:, :, None] * r64)).sum(axis=1)
    return dict(a=a, jerk=jerk, phi=phi, A=A, J=J, P=P, rows=rows)


def check_field(out, ref, kind, what):
    """out: dict of acc (M, 4), jerk (M, 4) or None, pot (M,) or None as the device left them"""
    rows, tol = ref["rows"], LD(TOL[kind])
    precision = suffix(kind)
    text = []
    for name, got, want, scale in (("acc", out.get("acc"), ref["a"], ref["A"]), ("jerk", out.get("jerk"), ref["jerk"], ref["J"]), ("pot", out.get("pot"), ref["phi"], ref["P"])):
        if got is None:
            continue
        assert want is not None, name
        assert np.isfinite(want).all(), f"{what}: the yardstick itself is not finite"
        mine = got[rows, :3] if got.ndim == 2 else got[rows]
        assert np.isfinite(mine).all(), (what, name)
        err = np.abs(mine.astype(LD) - want)
        with np.errstate(all="ignore"):
            worst = float(np.nanmax(np.where(scale > 0, err / (tol * scale), np.where(err > 0, np.inf, 0))))
        WORST[(name, precision)] = max(WORST.get((name, precision), 0.0), worst)
        text.append(f"{name} {worst:.3g}")
        assert (err <= tol * scale).all(), f"{what}: {name} at {worst:.3g} x its bound"
        if got.ndim == 2:
            assert not got[rows, 3].any(), f"{what}: .w of {name} is not 0"
    print(f"{what}: " + ", ".join(text) + f" of the bound; worst so far {({k[0] + ' ' + k[1]: round(v, 4) for k, v in sorted(WORST.items())})}")


# ---------------------------------------------------------------------------------------------------------------- the device side


class FieldDevice:
    """the arrays of one call on the device, through the C calls; PAD canary bytes round every array; outputs start as 0xC3 bytes"""
    PAD = 256
    OUTPUTS = ("acc", "jerk", "pot")

    def __init__(self, gpu, src, tgt, src_vel=None, tgt_vel=None, self_index=None, ws_fill=None, alias=False):
        """alias: targets (and target velocities) ARE the sources' arrays, the same addresses"""
        self.gpu, self.dtype, self.n, self.m = gpu, src.dtype, src.shape[0], tgt.shape[0]
        self.scalar, self.lib = scalar_of(self.dtype), gpu.field_lib()
        n, m = self.n, self.m
        self.ws_bytes = gpu.field_workspace_bytes(n, m, self.dtype)
        u32, u8 = np.dtype(np.uint32), np.dtype(np.uint8)
        self.kinds = dict(src=(self.dtype, 4 * n), src_vel=(self.dtype, 4 * n), tgt=(self.dtype, 4 * m), tgt_vel=(self.dtype, 4 * m), self=(u32, m), acc=(self.dtype, 4 * m),
                          jerk=(self.dtype, 4 * m), pot=(self.dtype, m), ws=(u8, max(self.ws_bytes, 32)))
        self.bufs = {}
        for name, (kind, count) in self.kinds.items():
            nbytes = count * kind.itemsize
            host = np.full(nbytes + 2 * self.PAD, 0xA5, np.uint8)
            host[self.PAD:self.PAD + nbytes] = 0xC3 if name in self.OUTPUTS else 0
            if name == "ws" and ws_fill is not None:
                host[self.PAD:self.PAD + nbytes] = ws_fill
            buf = gpu.DeviceBuffer(host.nbytes)
            buf.upload(host)
            self.bufs[name] = buf
        self.alias = alias
        self.has_vel, self.has_self = src_vel is not None, self_index is not None
        self.put("src", src)
        if not alias:
            self.put("tgt", tgt)
        if self.has_vel:
            self.put("src_vel", src_vel)
            if not alias:
                self.put("tgt_vel", tgt_vel)
        if self.has_self:
            self.put("self", self_index)
        self.inputs = {name: self.get(name).tobytes() for name in ("src", "src_vel", "tgt", "tgt_vel", "self")}

    def ptr(self, name):
        if self.alias and name in ("tgt", "tgt_vel"):
            name = "src" if name == "tgt" else "src_vel"
        return self.bufs[name].ptr.value + self.PAD

    def put(self, name, data):
        kind, count = self.kinds[name]
        data = np.ascontiguousarray(data, dtype=kind).reshape(-1)
        assert data.size == count, (name, data.size, count)
        self.gpu.check(self.gpu.lib().nb_h2d(self.ptr(name), data.ctypes.data, data.nbytes, None), "nb_h2d")

    def get(self, name):
        kind, count = self.kinds[name]
        out = np.empty(count, kind)
        self.gpu.check(self.gpu.lib().nb_d2h(out.ctypes.data, self.bufs[name].ptr.value + self.PAD, out.nbytes, None), "nb_d2h")
        return out.reshape(-1, 4) if name in ("src", "src_vel", "tgt", "tgt_vel", "acc", "jerk") else out

    def canaries_intact(self):
        for buf in self.bufs.values():
            host = buf.download(np.empty(buf.nbytes, np.uint8))
            if not ((host[:self.PAD] == 0xA5).all() and (host[-self.PAD:] == 0xA5).all()):
                return False
        return True

    def inputs_unchanged(self):
        return all(self.get(name).tobytes() == before for name, before in self.inputs.items())

    def untouched(self, name):
        return bool((self.get(name).view(np.uint8) == 0xC3).all())

    def eval(self, eps2, outputs=("acc", "jerk", "pot"), stream=None, use_self=True):
        fn = getattr(self.lib, "nb_field_eval_" + suffix(self.dtype))
        out = [self.ptr(name) if name in outputs else None for name in self.OUTPUTS]
        self.gpu.check(fn(self.ptr("src"), self.ptr("src_vel") if self.has_vel else None, self.n, self.ptr("tgt"), self.ptr("tgt_vel") if self.has_vel else None,
                          self.ptr("self") if self.has_self and use_self else None, self.m, self.scalar(eps2), *out, self.ptr("ws") if self.ws_bytes else None, self.ws_bytes,
                          stream), "nb_field_eval")

    def results(self, outputs=("acc", "jerk", "pot")):
        return {name: self.get(name) if name in outputs else None for name in self.OUTPUTS}

    def everything(self):
        return b"".join(self.get(name).tobytes() for name in self.OUTPUTS)

    def free(self):
        for buf in self.bufs.values():
            buf.free()


def points(m, dtype, seed, vscale=0.3):
    """M points of the caller's own, off the sources of cloud(): another stream of the same distribution, with velocities"""
    tgt, vel = cloud(m, dtype, 77000 + seed, "equal", vscale)
    tgt[:, 3] = -5.0  # (.w is ignored)
    return tgt, vel


def some_self_index(m, n, seed):
    """a third of the targets exclude a source chosen at random: exclusion is by index, whatever lies there"""
    rng = np.random.default_rng(seed)
    return np.where(rng.uniform(size=m) < 1 / 3, rng.integers(0, n, m), NONE).astype(np.uint32)


def sampled(m, seed, count=48):
    return None if m <= count else np.sort(np.random.default_rng(seed).choice(m, count, replace=False))


def run(gpu, src, tgt, src_vel, tgt_vel, self_index, eps2, outputs, alias=False):
    d = FieldDevice(gpu, src, tgt, src_vel, tgt_vel, self_index, alias=alias)
    d.eval(eps2, outputs)
    out = d.results(outputs)
    for name in FieldDevice.OUTPUTS:
        if name not in outputs:
            assert d.untouched(name), name
    assert d.canaries_intact() and d.inputs_unchanged()
    d.free()
    return out


# ---------------------------------------------------------------------------------------------------------------- 8: every instantiation


@gpu_only
@pytest.mark.parametrize("case", field_cases(), ids=lambda c: f"{kernel_name(('field_eval', (TYPE_NAME[c[0]], c[1], c[2]))).replace(' ', '')} n={c[3]} m={c[4]}")
def test_every_instantiation_against_long_double(gpu, case):
    dtype, waves, jerk, n, m = case
    plan = plan_dict(gpu, n, m, dtype)
    assert plan["waves_per_group"] == waves and plan == expected_plan(n, m, dtype), "the plan query selects the claimed instantiation"
    outputs = ("acc", "jerk", "pot") if jerk else ("acc", "pot")
    tgt, tgt_vel = points(m, dtype, n + m)
    self_index = some_self_index(m, n, n * 31 + m)
    rows = sampled(m, n + m)
    for mass in ("equal", "species", "random", "zeros"):
        src, src_vel = cloud(n, dtype, 5000 + n, mass)
        eps2 = dtype(0.01)
        out = run(gpu, src, tgt, src_vel if jerk else None, tgt_vel if jerk else None, self_index, eps2, outputs)
        ref = field_reference(src, src_vel if jerk else None, tgt, tgt_vel if jerk else None, self_index, eps2, rows)
        check_field(out, ref, dtype, f"{suffix(dtype)} S={waves} jerk={jerk} n={n} m={m} J={plan['ranges']} {mass}")


# ---------------------------------------------------------------------------------------------------------------- 9: shapes


SHAPE_SOURCES = (1, 2, 300, 5000, 70000)


def shape_targets(n):
    return (1, 2, 100, 129, 5000, n + 17)


@gpu_only
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n", SHAPE_SOURCES)
def test_shapes_against_long_double(gpu, dtype, n):
    """targets off the sources; the sources themselves (a slice of the positions passed as it is, self_index = arange: softening 0, every
    coincident pair excluded); a mix (every third target ON a source and NOT excluded, softening > 0)"""
    src, src_vel = cloud(n, dtype, 300 + n, "random" if n <= 5000 else "species", 1.0)
    for m in shape_targets(n):
        rows = sampled(m, n * 7 + m, 12 if n > 5000 else 48)
        tgt, tgt_vel = points(m, dtype, n * 3 + m, 1.0)
        for eps2 in (dtype(0.01), dtype(0)):
            out = run(gpu, src, tgt, src_vel, tgt_vel, None, eps2, ("acc", "jerk", "pot"))
            check_field(out, field_reference(src, src_vel, tgt, tgt_vel, None, eps2, rows), dtype, f"{suffix(dtype)} off n={n} m={m} eps2={float(eps2)}")
        if m <= n:
            own = np.arange(m, dtype=np.uint32)
            out = run(gpu, src, src[:m], src_vel, src_vel[:m], own, dtype(0), ("acc", "jerk", "pot"))
            check_field(out, field_reference(src, src_vel, src[:m], src_vel[:m], own, dtype(0), rows), dtype, f"{suffix(dtype)} own slice n={n} m={m} eps2=0")
        mixed, mixed_vel = tgt.copy(), tgt_vel.copy()
        on = np.arange(0, m, 3)
        mixed[on, :3] = src[(on * 7) % n, :3]
        eps2 = dtype(1e-4)
        out = run(gpu, src, mixed, src_vel, mixed_vel, None, eps2, ("acc", "jerk", "pot"))
        check_field(out, field_reference(src, src_vel, mixed, mixed_vel, None, eps2, rows), dtype, f"{suffix(dtype)} mix n={n} m={m}")


@gpu_only
@pytest.mark.parametrize("n,dtype", [(5000, F32), (5000, F64), (70000, F32), (70000, F64), (65536, F32), (65536, F64), (262144, F32)])
def test_targets_are_the_sources(gpu, n, dtype):
    """targets == sources, the same addresses, self_index = arange: at softening 0 (every coincident pair is an excluded one: finite and
    right), and softened; sampled rows"""
    src, src_vel = cloud(n, dtype, 3, "species" if n != 65536 else "random", 1.0)
    own = np.arange(n, dtype=np.uint32)
    rows = sampled(n, n, 16)
    for eps2 in (dtype(0), dtype(0.01)) if n < 100000 else (dtype(0.01),):
        d = FieldDevice(gpu, src, src, src_vel, src_vel, own, alias=True)
        d.eval(eps2)
        out = d.results()
        assert d.canaries_intact() and d.inputs_unchanged()
        d.free()
        assert all(np.isfinite(out[name]).all() for name in out)
        check_field(out, field_reference(src, src_vel, src, src_vel, own, eps2, rows), dtype, f"{suffix(dtype)} targets == sources n={n} eps2={float(eps2)}")


@gpu_only
@pytest.mark.parametrize("n", [65536, 262144])
def test_sampled_targets_of_large_source_sets(gpu, n):
    for m, jerk in ((128, True), (1024, True), (8192, False)):
        src, src_vel = cloud(n, F32, 11, "species", 1.0)
        tgt, tgt_vel = points(m, F32, n + m, 1.0)
        self_index = some_self_index(m, n, m)
        rows = sampled(m, m, 24)
        outputs = ("acc", "jerk", "pot") if jerk else ("acc", "pot")
        out = run(gpu, src, tgt, src_vel if jerk else None, tgt_vel if jerk else None, self_index, F32(0.01), outputs)
        check_field(out, field_reference(src, src_vel if jerk else None, tgt, tgt_vel if jerk else None, self_index, F32(0.01), rows), F32, f"f32 n={n} m={m} jerk={jerk}")


@gpu_only
@pytest.mark.parametrize("dtype", [F32, F64])
def test_an_excluded_coincident_pair_at_no_softening(gpu, dtype):
    """a tracer ON a source, excluding it: finite and right; not excluding it: a still finite and right, phi -m / sqrt(floor) deeper"""
    n = 1000
    src, src_vel = cloud(n, dtype, 21, "random")
    tgt, tgt_vel = points(5, dtype, 21)
    tgt[2, :3], tgt_vel[2, :3] = src[700, :3], src_vel[700, :3]
    self_index = np.array([NONE, NONE, 700, NONE, NONE], np.uint32)
    out = run(gpu, src, tgt, src_vel, tgt_vel, self_index, dtype(0), ("acc", "jerk", "pot"))
    check_field(out, field_reference(src, src_vel, tgt, tgt_vel, self_index, dtype(0)), dtype, f"{suffix(dtype)} excluded coincident pair")
    bare = run(gpu, src, tgt, src_vel, tgt_vel, None, dtype(0), ("acc", "jerk", "pot"))
    assert np.isfinite(bare["acc"]).all() and np.isfinite(bare["jerk"]).all() and np.isfinite(bare["pot"]).all()
    ref = field_reference(src, src_vel, tgt, tgt_vel, None, dtype(0))
    check_field(bare, ref, dtype, f"{suffix(dtype)} coincident pair, not excluded (equal velocities)")
    # the header's figure: the two long double sums differ by m * 2^30 (fp32) / m * 2^150 (fp64), and each result is within TOL x its own P of its sum
    deeper = LD(src[700, 3]) * LD(2.0) ** (30 if dtype == F32 else 150)
    assert abs(LD(bare["pot"][2]) - (LD(out["pot"][2]) - deeper)) <= LD(TOL[dtype]) * (2 * ref["P"][2] - deeper)
    assert bare["acc"][2].tobytes() == out["acc"][2].tobytes() and bare["jerk"][2].tobytes() == out["jerk"][2].tobytes(), "r = 0 and w = 0: exactly 0 either way"


# ---------------------------------------------------------------------------------------------------------------- 10: exact properties


@gpu_only
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n,m", [(2085, 777), (5000, 300), (300, 200)])
def test_field_bits_and_invariants(gpu, dtype, n, m):
    """the same bits from two calls, on another stream, with a NaN-filled workspace, from a captured graph replayed twice; canaries; inputs
    untouched; .w = 0; null outputs leave their arrays untouched and change no bit of the others; permuted and duplicated targets; exclusion
    against mass 0  ((2085, 777) and (5000, 300) have several ranges and the second launch, (300, 200) one launch)"""
    lib = gpu.lib()
    src, src_vel = cloud(n, dtype, 40 + n, "random")
    tgt, tgt_vel = points(m, dtype, 40 + m)
    tgt[::5, :3] = src[(np.arange(0, m, 5) * 3) % n, :3]  # some targets on a source ...
    self_index = some_self_index(m, n, 9)
    self_index[::10] = ((np.arange(0, m, 10) * 3) % n).astype(np.uint32)  # ... half of them excluding it
    eps2 = dtype(1e-3)

    def fresh(ws_fill=None, **kw):
        return FieldDevice(gpu, kw.get("src", src), kw.get("tgt", tgt), src_vel, kw.get("tgt_vel", tgt_vel), kw.get("self_index", self_index), ws_fill=ws_fill)

    base = fresh()
    base.eval(eps2)
    want = base.everything()
    acc, jerk, pot = base.get("acc"), base.get("jerk"), base.get("pot")
    assert base.canaries_intact() and base.inputs_unchanged()
    assert not acc[:, 3].any() and not jerk[:, 3].any() and np.isfinite(acc).all() and np.isfinite(jerk).all() and np.isfinite(pot).all()
    base.eval(eps2)
    assert base.everything() == want, "again, on the workspace the first call left"

    again = fresh(ws_fill=0xFF)
    again.eval(eps2)
    assert again.everything() == want and again.canaries_intact(), "NaN workspace (0xFF bytes: NaN in both precisions)"
    again.free()

    stream = ctypes.c_void_p()
    gpu.check(lib.nb_stream_create(ctypes.byref(stream)), "nb_stream_create")
    other = fresh(ws_fill=0xFF)
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    other.eval(eps2, stream=stream)
    gpu.check(lib.nb_stream_synchronize(stream), "nb_stream_synchronize")
    assert other.everything() == want, "another stream"
    other.free()

    hip = hip_runtime()
    captured = fresh(ws_fill=0xFF)
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    graph, graph_exec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0
    captured.eval(eps2, stream=stream)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
    assert all(captured.untouched(name) for name in FieldDevice.OUTPUTS), "recorded, not run"
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
    for mask in range(1, 7):
        asked = tuple(name for k, name in enumerate(FieldDevice.OUTPUTS) if mask >> k & 1)
        some = fresh()
        some.eval(eps2, asked)
        for name in FieldDevice.OUTPUTS:
            if name in asked:
                assert some.get(name).tobytes() == base.get(name).tobytes(), (asked, name)
            else:
                assert some.untouched(name), (asked, name)
        assert some.canaries_intact()
        some.free()
    # ... and without velocity arrays at all
    bare = FieldDevice(gpu, src, tgt, None, None, self_index)
    bare.eval(eps2, ("acc", "pot"))
    assert bare.get("acc").tobytes() == acc.tobytes() and bare.get("pot").tobytes() == pot.tobytes() and bare.untouched("jerk")
    bare.free()

    # targets permuted, self_index and velocities along: the outputs permuted, bit for bit
    order = np.random.default_rng(3).permutation(m)
    moved = fresh(tgt=tgt[order], tgt_vel=tgt_vel[order], self_index=self_index[order])
    moved.eval(eps2)
    assert moved.get("acc").tobytes() == acc[order].tobytes() and moved.get("jerk").tobytes() == jerk[order].tobytes() and moved.get("pot").tobytes() == pot[order].tobytes()
    moved.free()
    # a duplicated target (one that excludes somebody, copied over one that does not, far away in the array): duplicate bits, the rest unchanged
    a, b = 10, m - 3
    twice_tgt, twice_vel, twice_self = tgt.copy(), tgt_vel.copy(), self_index.copy()
    twice_tgt[b], twice_vel[b], twice_self[b] = tgt[a], tgt_vel[a], self_index[a]
    twice = fresh(tgt=twice_tgt, tgt_vel=twice_vel, self_index=twice_self)
    twice.eval(eps2)
    for name, full in (("acc", acc), ("jerk", jerk), ("pot", pot)):
        got = twice.get(name)
        assert got[b].tobytes() == full[a].tobytes() == got[a].tobytes(), name
        rest = np.setdiff1d(np.arange(m), [b])
        assert got[rest].tobytes() == full[rest].tobytes(), (name, "a target's results do not depend on the targets beside it")
    twice.free()
    # exclusion of j == the same call with m_j = 0 and no exclusion: one target at a time against a source set with that mass cleared
    for k in (0, 10, 20, m - 1):
        j = int(self_index[k])
        if j == NONE:
            j = int(k * 13 % n)
        one_self = np.full(m, NONE, np.uint32)
        one_self[k] = j
        excl = fresh(self_index=one_self)
        excl.eval(eps2)
        lighter = src.copy()
        lighter[j, 3] = 0
        zero = fresh(src=lighter)
        zero.eval(eps2, use_self=False)
        for name in FieldDevice.OUTPUTS:
            assert excl.get(name)[k].tobytes() == zero.get(name)[k].tobytes(), (name, k, j)
        excl.free(), zero.free()
    base.free()


# ---------------------------------------------------------------------------------------------------------------- 11: the existing libraries


@gpu_only
@pytest.mark.parametrize("dtype", [F32, F64])
def test_field_against_the_existing_libraries(gpu, dtype):
    """targets == sources, self_index = arange, 65 536 bodies: a and jerk against nb_hermite_eval_* within the sum of both tolerances (each is
    within TOL x its magnitude sum of the long double sum); phi against nb_neighbour_survey_*'s potentials likewise; (1/2) sum m phi against
    nb_energy_*'s potential energy under the bound of test_neighbour.test_potentials_against_nb_energy; sources split in two halves:
    field(all) = field(A) + field(B) within the tolerances of the three calls -- the caller who shards sources over devices"""
    from test_hermite import evaluate
    from test_neighbour import NeighbourDevice
    n = 65536
    src, src_vel = cloud(n, dtype, 17, "species", 1.0)
    eps2 = dtype(0.01)
    own = np.arange(n, dtype=np.uint32)
    d = FieldDevice(gpu, src, src, src_vel, src_vel, own, alias=True)
    d.eval(eps2)
    mine = d.results()
    rows = sampled(n, 5, 64)
    ref = field_reference(src, src_vel, src, src_vel, own, eps2, rows)
    check_field(mine, ref, dtype, f"{suffix(dtype)} n={n} against long double")
    tol = TOL[dtype]
    acc, jerk = evaluate(gpu, src, src_vel, eps2)
    assert (np.abs(acc[rows, :3].astype(LD) - mine["acc"][rows, :3].astype(LD)) <= 2 * tol * ref["A"]).all(), "nb_hermite_eval: accelerations"
    assert (np.abs(jerk[rows, :3].astype(LD) - mine["jerk"][rows, :3].astype(LD)) <= 2 * tol * ref["J"]).all(), "nb_hermite_eval: jerks"
    # (every row, against the GPU's own magnitudes where the long double ones are sampled: |a| <= A, so 2 tol A is not available; the
    #  largest component difference relative to the largest |a| is printed, not asserted)
    print(f"{suffix(dtype)}: max |a_field - a_hermite| / max |a| = {np.abs(acc[:, :3] - mine['acc'][:, :3]).max() / np.abs(acc[:, :3]).max():.3g}")
    survey = NeighbourDevice(gpu, src)
    survey.survey(0.0, eps2, outputs=("pot",))
    theirs = survey.get("pot")
    survey.free()
    assert (np.abs(theirs[rows].astype(LD) - mine["pot"][rows].astype(LD)) <= 2 * tol * ref["P"]).all(), "nb_neighbour_survey: potentials"
    assert (np.abs(theirs.astype(LD) - mine["pot"].astype(LD)) <= 2 * tol * np.abs(theirs.astype(LD))).all(), "... every body: P = |phi|"
    half = 0.5 * float((src[:, 3].astype(np.float64) * mine["pot"].astype(np.float64)).sum())
    gpu.set_softening_squared(eps2 if dtype == F32 else float(eps2))
    zeros = gpu.DeviceBuffer(src.nbytes)
    energy = gpu.energy(d.ptr("src"), zeros.ptr, n, dtype)["potential"]
    zeros.free(), d.free()
    print(f"{suffix(dtype)}: (1/2) sum m phi = {half!r}, nb_energy potential = {energy!r}: {abs(half - energy) / abs(energy):.3g} relative")
    assert abs(half - energy) <= (1e-5 if dtype == F32 else 2e-12) * abs(energy)
    # two halves of the sources, the same targets (every body); a target excludes itself in the half that holds it
    parts = []
    for lo, hi in ((0, n // 2), (n // 2, n)):
        inside = (own >= lo) & (own < hi)
        self_index = np.where(inside, own - lo, NONE).astype(np.uint32)
        parts.append(run(gpu, src[lo:hi], src, src_vel[lo:hi], src_vel, self_index, eps2, ("acc", "jerk", "pot")))
    for name, scale in (("acc", ref["A"]), ("jerk", ref["J"]), ("pot", ref["P"])):
        whole = mine[name][rows, :3] if name != "pot" else mine[name][rows]
        added = (parts[0][name].astype(LD) + parts[1][name].astype(LD))
        added = added[rows, :3] if name != "pot" else added[rows]
        # (each half is within TOL x ITS magnitude sum, and the two magnitude sums add to the whole's)
        assert (np.abs(whole.astype(LD) - added) <= 2 * tol * scale).all(), (name, "field(all) = field(A) + field(B)")


# ---------------------------------------------------------------------------------------------------------------- 12: the class, the CLI


@gpu_only
@pytest.mark.parametrize("dtype", [F32, F64])
def test_python_class_gives_the_c_calls_bits(gpu, dtype):
    n, m, eps2 = 3000, 500, dtype(1e-3)
    src, src_vel = cloud(n, dtype, 55, "species")
    tgt, tgt_vel = points(m, dtype, 55)
    self_index = some_self_index(m, n, 55)
    d = FieldDevice(gpu, src, tgt, src_vel, tgt_vel, self_index)
    d.eval(eps2)
    want = d.results()
    probe = gpu.FieldProbe(n, 4096, dtype, softening_sq=eps2)
    for given in ((src, tgt, src_vel, tgt_vel, self_index, None), (d.ptr("src"), d.ptr("tgt"), d.ptr("src_vel"), d.ptr("tgt_vel"), d.ptr("self"), m)):  # host arrays, device addresses
        out = probe.eval(given[0], given[1], given[2], given[3], given[4], jerks=True, potentials=True, num_targets=given[5])
        assert out["accelerations"].tobytes() == want["acc"].tobytes() and out["jerks"].tobytes() == want["jerk"].tobytes() and out["potentials"].tobytes() == want["pot"].tobytes()
    out = probe.eval(src, tgt, self_index=self_index, potentials=False)
    assert out["jerks"] is None and out["potentials"] is None and out["accelerations"].tobytes() == want["acc"].tobytes()
    # another M on the same object: the workspace was sized for every M up to max_targets
    few = probe.eval(src, tgt[:7], src_vel, tgt_vel[:7], self_index[:7], jerks=True)
    check_field(dict(acc=few["accelerations"], jerk=few["jerks"], pot=few["potentials"]), field_reference(src, src_vel, tgt[:7], tgt_vel[:7], self_index[:7], eps2), dtype, "seven targets")
    many, many_vel = points(4096, dtype, 56)
    out = probe.eval(src, many, src_vel, many_vel, jerks=True)
    check_field(dict(acc=out["accelerations"], jerk=out["jerks"], pot=out["potentials"]), field_reference(src, src_vel, many, many_vel, None, eps2, sampled(4096, 1)), dtype, "4 096 targets")
    assert probe.accelerations_ptr and probe.jerks_ptr and probe.potentials_ptr
    with pytest.raises(ValueError):
        probe.eval(src, tgt, jerks=True)
    with pytest.raises(ValueError):
        probe.eval(src, d.ptr("tgt"))
    with pytest.raises(ValueError):
        probe.eval(src[:-1], tgt)
    with pytest.raises(ValueError):
        probe.eval(src, many[:0])
    probe.free(), d.free()
    with pytest.raises(gpu.NBodyHipError):
        gpu.FieldProbe(0, 16, dtype)


def cli_field_lines(stdout):
    number = r"([-+0-9.eE]+|-?inf|-?nan)"
    pattern = rf"^field at \({number}, {number}, {number}\): acceleration \({number}, {number}, {number}\), potential {number}$"
    return np.array([[float(x) for x in m] for m in re.findall(pattern, stdout, re.M)])


@gpu_only
def test_cli_prints_the_field_of_the_final_state(gpu, tmp_path):
    """nbody --field with the three integrators, fp32 and --fp64: the lines give the field of the state the run dumps (evaluated here through
    the Python class) at the file's points, in file order, after the run's own lines, --energy's and --neighbours'"""
    n, steps = 4096, 3
    rng = np.random.default_rng(12)
    coordinates = np.vstack([np.zeros((1, 3)), rng.standard_normal((40, 3)) * 20.0])
    file = tmp_path / "points.txt"
    file.write_text("# 41 points\n" + "\n".join("  ".join(repr(float(x)) for x in p) + ("   # the last" if k == 40 else "") + ("\n" if k == 7 else "") for k, p in enumerate(coordinates)) + "\n")
    for integrator, extra in (("hermite-block", ["--eta=0.05", "--levels=12"]), ("hermite", []), ("euler", []), ("euler", ["--fp64"]), ("hermite", ["--fp64"])):
        dtype = F64 if "--fp64" in extra else F32
        out = tmp_path / "state.bin"
        r = subprocess.run([CLI, f"--integrator={integrator}", f"--numbodies={n}", f"--steps={steps}", f"--dump={out}", "--energy", "--neighbours=0.75", f"--field={file}", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        pos = np.fromfile(out, dtype=dtype)[:4 * n].reshape(n, 4)
        softening = dtype(np.float32(0.1))
        tgt = np.zeros((41, 4), dtype)
        tgt[:, :3] = coordinates
        probe = gpu.FieldProbe(n, 41, dtype, softening_sq=softening * softening)
        want = probe.eval(pos, tgt)
        probe.free()
        lines = cli_field_lines(r.stdout)
        assert lines.shape == (41, 7), r.stdout[-1500:]
        close = dict(rtol=1e-8, atol=0)
        assert np.allclose(lines[:, :3], tgt[:, :3].astype(np.float64), **close), "in file order"
        assert np.allclose(lines[:, 3:6], want["accelerations"][:, :3].astype(np.float64), **close) and np.allclose(lines[:, 6], want["potentials"].astype(np.float64), **close), integrator
        assert r.stdout.index("energy end") < r.stdout.index("closest pair:") < r.stdout.index("deepest potential:") < r.stdout.index("field at ("), "after --energy's and --neighbours' lines"
    r = subprocess.run([CLI, f"--numbodies={n}", "--benchmark", "-i=2", f"--field={file}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert cli_field_lines(r.stdout).shape == (41, 7)
    assert r.stdout.index("billion interactions per second") < r.stdout.index("field at ("), "the reference's benchmark lines stay first"


# ---------------------------------------------------------------------------------------------------------------- 13: speed


@gpu_only
def test_field_speed_sanity(gpu):
    """65 536 sources fp32, device events, median of 5 single calls after warm-up, the yardsticks timed in the same process.  The expected cost
    per packed pair is the issue-cost model of the loops AS COMPILED (tests/test_field.py: 13 packed + 2 v_rsq_f32 without the jerk against the
    one-sided step's 11 + 2: 1.13; 27 + 2 with it against hermite_eval's 25 + 2: 1.07).  M = N without the jerk: at most 2 x model x the
    one-sided nb_integrate_f32 step; M = N with it: at most 2 x model x nb_hermite_eval_f32; M = 128 with it: at most 1/20 of nb_hermite_eval_f32."""
    from test_hermite import Device
    n, dtype = 65536, F32
    src, src_vel = cloud(n, dtype, 1, "equal", 1.0)
    eps2, dt = dtype(0.01), dtype(1e-3)
    gpu.set_softening_squared(eps2)
    d = Device(gpu, src, src_vel, eps2)
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

    t_hermite = median_ms(d.eval)
    t_euler = median_ms(euler)
    d.free()
    own = np.arange(n, dtype=np.uint32)
    full = FieldDevice(gpu, src, src, src_vel, src_vel, own, alias=True)
    t_plain = median_ms(lambda: full.eval(eps2, ("acc", "pot")))
    t_jerk = median_ms(lambda: full.eval(eps2))
    t_unmasked = median_ms(lambda: full.eval(eps2, use_self=False))
    full.free()
    tgt, tgt_vel = points(128, dtype, 1, 1.0)
    few = FieldDevice(gpu, src, tgt, src_vel, tgt_vel, None)
    t_few = median_ms(lambda: few.eval(eps2))
    few.free()
    print(f"one-sided FAST step {t_euler:.3f} ms, nb_hermite_eval_f32 {t_hermite:.3f} ms; field M = N: a + phi {t_plain:.3f} ms = {t_plain / t_euler:.2f}x the step (model "
          f"{MODEL_PLAIN:.2f}x, ratio / model {t_plain / t_euler / MODEL_PLAIN:.2f}); a + jerk + phi {t_jerk:.3f} ms = {t_jerk / t_hermite:.2f}x hermite_eval (model {MODEL_JERK:.2f}x, "
          f"ratio / model {t_jerk / t_hermite / MODEL_JERK:.2f}); without self_index {t_unmasked:.3f} ms (the MASK form costs {(t_jerk - t_unmasked) / t_unmasked * 100:+.1f} %); "
          f"M = 128: {t_few:.4f} ms = 1/{t_hermite / t_few:.0f} of hermite_eval")
    assert t_plain <= 2 * MODEL_PLAIN * t_euler, (t_plain, t_euler, MODEL_PLAIN)
    assert t_jerk <= 2 * MODEL_JERK * t_hermite, (t_jerk, t_hermite, MODEL_JERK)
    assert t_few <= t_hermite / 20, (t_few, t_hermite)


@gpu_only
def test_zz_report_the_worst_errors(gpu):
    """(runs last in the module: prints what DESIGN.md 5.9 quotes)"""
    print("worst error as a fraction of its bound:", {f"{k[0]} {k[1]}": round(v, 4) for k, v in sorted(WORST.items())})
    assert all(v <= 1 for v in WORST.values())
