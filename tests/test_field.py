"""Acceleration, jerk and potential of N sources at M points of the caller's own (nb_field_*, include/nbody_hip_field.h;
libnbody_hip_field.so from csrc/field*.hip).  The CPU part; the GPU part is tests/test_field_gpu.py, which imports the helpers below.

The definition, restated in numpy below (numpy_field): with r = x_j - p_k, w = v_j - u_k, s^2 = r.r + softening_sq (0 -> the floor 2^-60 in
fp32, 2^-300 in fp64), over all sources j,

    a_k = sum m s^-3 r,    jerk_k = sum m s^-3 (w - 3 (r.w) s^-2 r),    phi_k = -sum m s^-1,    m = m_j, but 0 when j == self_index[k]

CPU tests: the boundary (declared, exported, mirrored; the other libraries unchanged), the plan and the workspace as functions of
(N, M, precision), host-side argument checks, the instruction mix of the streaming loops, the registry of field.s (every kernel of the
listing is named once, as a case with the shape that reaches it), the command line's refusals, the numpy restatement on a hand-made state."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from kernel_matrix import F32, F64, LANE_WIDTH, N_BY_WAVES, TYPE_NAME, kernel_name, listed_kernels
from test_capi_symbols import declared_symbols, exported_symbols
from test_hermite import CSRC

ERR = 10001
MAX_N, MAX_M = 1 << 26, 1 << 24
NONE = 0xFFFFFFFF
SYMBOLS = ["nb_field_eval_f32", "nb_field_eval_f64", "nb_field_plan_f32", "nb_field_plan_f64", "nb_field_workspace_bytes"]
FLOOR = {np.float32: 2.0 ** -60, np.float64: 2.0 ** -300}
TARGET = 512  # workgroups the evaluation aims at (taken over from 5.7)
# What the compiler delivers for the fp32 streaming loops, per packed pair of targets and source: packed operations without /
# with the jerk, v_rsq_f32, and what the MASK form adds: two compares, two selects and the copy of the mass into a vector register.
PK_PLAIN, PK_JERK, RSQ, MASK_EXTRA = 13, 27, 2, 5
# fp64, per target and source: vector operations without / with the jerk (v_rsq_f64 among them), and the MASK form's compare, two selects, two copies
DP_PLAIN, DP_JERK, DP_MASK_EXTRA = 19, 35, 5
# The S = 1 jerk kernel in fp32 (fewer than 256 sources) keeps part of the two source sets in spilled scalar registers: its plain loop
# moves them with v_readlane / v_writelane, at most this many per packed pair.  No other loop has a vector operation beyond its mix.
LANE_MOVES_S1 = 10
# issue cycles (docs/history.md: packed fp32 op 4.08, v_rsq_f32 8.3); the one-sided step: 11 packed + 2 v_rsq_f32, hermite_eval: 25 + 2
PK_CYCLES, RSQ_CYCLES = 4.08, 8.3
MODEL_PLAIN = (PK_PLAIN * PK_CYCLES + RSQ * RSQ_CYCLES) / (11 * PK_CYCLES + 2 * RSQ_CYCLES)  # against the one-sided FAST step
MODEL_JERK = (PK_JERK * PK_CYCLES + RSQ * RSQ_CYCLES) / (25 * PK_CYCLES + 2 * RSQ_CYCLES)    # against nb_hermite_eval_f32


def suffix(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def scalar_of(dtype):
    return np.float32 if np.dtype(dtype) == np.float32 else float


# ---------------------------------------------------------------------------------------------------------------- the definition in numpy


def numpy_field(src, src_vel, tgt, tgt_vel, self_index, eps2):
    """The definition in T arithmetic, pair by pair (small states only).  src (N, 4), tgt (M, 4) of T; the velocities (., 4) or None;
    self_index (M,) of uint32 or None.  -> a (M, 4), jerk (M, 4) or None, phi (M,)"""
    kind = src.dtype.type
    n, m = src.shape[0], tgt.shape[0]
    s2_floor = kind(eps2) if eps2 != 0 else kind(FLOOR[kind])
    with_jerk = src_vel is not None and tgt_vel is not None
    a, jerk, phi = np.zeros((m, 4), kind), np.zeros((m, 4), kind) if with_jerk else None, np.zeros(m, kind)
    for k in range(m):
        for j in range(n):
            mass = kind(0) if self_index is not None and self_index[k] == j else src[j, 3]
            r = src[j, :3] - tgt[k, :3]
            s2 = (r * r).sum(dtype=kind) + s2_floor
            inv = kind(1) / np.sqrt(s2)
            inv2, inv3 = inv * inv, inv * inv * inv
            a[k, :3] += mass * inv3 * r
            phi[k] -= mass * inv
            if with_jerk:
                w = src_vel[j, :3] - tgt_vel[k, :3]
                jerk[k, :3] += mass * inv3 * (w - kind(3) * (r * w).sum(dtype=kind) * inv2 * r)
    return a, jerk, phi


def test_the_numpy_definition_on_a_hand_made_state():
    """Two sources -- mass 2 at the origin moving with (1, 0, 0), mass 3 at (3, 0, 0) at rest -- and three targets at rest:
    (0, 4, 0) off both (the 3-4-5 triangle); (3, 0, 0), ON source 1 and excluding it by index; the origin, ON source 0 and excluding nobody."""
    for kind in (np.float64, np.float32):
        src = np.array([[0, 0, 0, 2], [3, 0, 0, 3]], kind)
        src_vel = np.array([[1, 0, 0, 0], [0, 0, 0, 0]], kind)
        tgt = np.array([[0, 4, 0, 7], [3, 0, 0, 7], [0, 0, 0, 7]], kind)  # (.w is ignored)
        tgt_vel = np.zeros((3, 4), kind)
        self_index = np.array([NONE, 1, NONE], np.uint32)
        a, jerk, phi = numpy_field(src, src_vel, tgt, tgt_vel, self_index, 0.0)
        close = dict(rtol=8 * np.finfo(kind).eps, atol=0)
        # target 0: source 0 at r = (0, -4, 0), s = 4: a = 2/64 r, phi = -1/2, r.w = 0 so jerk = 2/64 w; source 1 at r = (3, -4, 0), s = 5: a = 3/125 r, phi = -3/5, w = 0
        assert np.allclose(a[0, :3], [0.072, -0.125 - 0.096, 0], **close) and np.isclose(phi[0], -1.1, **close)
        assert np.allclose(jerk[0, :3], [0.03125, 0, 0], **close)
        # target 1: source 1 coincides and is excluded -> exactly nothing of it, at softening 0; source 0 at r = (-3, 0, 0), s = 3, w = (1, 0, 0), r.w = -3:
        # a = 2/27 r, phi = -2/3, jerk = 2/27 (w - 3 (-3)/9 r) = 2/27 (-2, 0, 0)
        assert np.allclose(a[1, :3], [-2 / 9, 0, 0], **close) and np.isclose(phi[1], -2 / 3, **close)
        assert np.allclose(jerk[1, :3], [-4 / 27, 0, 0], **close) and np.isfinite(jerk[1]).all()
        # target 2: source 0 coincides and is NOT excluded: a gets exactly 0 of it, phi -m / sqrt(floor), the jerk m w / floor^(3/2) (w != 0);
        # source 1 at r = (3, 0, 0): a = 3/27 r, phi = -1, w = 0
        assert np.allclose(a[2, :3], [1 / 3, 0, 0], **close)
        big = 2.0 ** (30 if kind == np.float32 else 150)
        assert np.isclose(phi[2], -2 * big - 1, **close) and np.isclose(jerk[2, 0], 2 * big ** 3, **close) and not jerk[2, 1:].any()
        # excluding by index is "mass 0", bit for bit
        lighter = src.copy()
        lighter[1, 3] = 0
        b = numpy_field(lighter, src_vel, tgt[1:2], tgt_vel[1:2], None, 0.0)
        assert a[1].tobytes() == b[0][0].tobytes() and jerk[1].tobytes() == b[1][0].tobytes() and phi[1].tobytes() == b[2][0].tobytes()
        assert not a[:, 3].any() and not jerk[:, 3].any()
        assert numpy_field(src, None, tgt, None, self_index, 0.0)[1] is None


# ---------------------------------------------------------------------------------------------------------------- the boundary


def test_field_header_library_and_binding_agree(pkg):
    declared = declared_symbols("nbody_hip_field.h")
    assert declared == SYMBOLS
    assert exported_symbols(pkg.FIELD_LIB_PATH) == declared
    assert sorted(pkg.FIELD_SIGNATURES) == declared
    # the other libraries export what they did, none of it ours
    others = {pkg.LIB_PATH: 96, pkg.ENSEMBLE_LIB_PATH: 4, pkg.HERMITE_LIB_PATH: 9, pkg.HERMITE_BLOCK_LIB_PATH: 9, pkg.NEIGHBOUR_LIB_PATH: 7}
    for path, count in others.items():
        assert len(exported_symbols(path)) == count, path
        assert not set(declared) & set(exported_symbols(path)), path
    assert not set(declared) & set(exported_symbols(pkg.LAB_LIB_PATH))
    assert set(exported_symbols(pkg.LIB_PATH)) <= set(exported_symbols(pkg.LAB_LIB_PATH))
    needed = subprocess.run(["readelf", "-d", pkg.FIELD_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnbody_hip" not in needed


def test_field_plan_mirror_and_constants_match_the_header(pkg):
    text = open(os.path.join(ROOT, "include", "nbody_hip_field.h")).read()
    body = re.search(r"typedef struct nb_field_plan \{(.*?)\} nb_field_plan_t;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(unsigned long long|int|unsigned)\s+(\w+);", body)
    ctype = {"unsigned long long": ctypes.c_ulonglong, "int": ctypes.c_int, "unsigned": ctypes.c_uint}
    assert [f for _, f in fields] == [f for f, _ in pkg.FieldPlan._fields_]
    for (kind, field), (_, mirrored) in zip(fields, pkg.FieldPlan._fields_):
        assert mirrored == ctype[kind], field
    assert ctypes.sizeof(pkg.FieldPlan) == 56
    assert re.search(r"#define NB_FIELD_MAX_SOURCES \(1u << 26\)", text) and pkg.FIELD_MAX_SOURCES == MAX_N
    assert re.search(r"#define NB_FIELD_MAX_TARGETS \(1u << 24\)", text) and pkg.FIELD_MAX_TARGETS == MAX_M
    assert re.search(r"#define NB_FIELD_NONE 0xFFFFFFFFu", text) and pkg.FIELD_NONE == NONE
    for phrase in ("a_k    =  sum m s^-3 r", "jerk_k =  sum m s^-3 (w - 3 (r.w) s^-2 r)", "phi_k  = -sum m s^-1", "2^-60 (fp32) / 2^-300 (fp64)", "-m * 2^30 (fp32) / -m * 2^150 (fp64)",
                   "Exclusion is by INDEX, never by distance", "Permuting the\n * targets permutes the outputs bit for bit"):
        assert phrase in text, phrase


# ---------------------------------------------------------------------------------------------------------------- plan and workspace


def expected_plan(n, m, dtype):
    """the geometry rule of the header, restated"""
    W, size = LANE_WIDTH[dtype], np.dtype(dtype).itemsize
    S = 1
    while S < 8 and 2 * S * 128 <= n:
        S *= 2
    tiles, chunks = -(-m // (64 * W)), -(-n // 128)
    cap = 1
    while 2 * cap <= chunks // S:
        cap *= 2
    J = 1
    while tiles * J < TARGET and J < cap:
        J *= 2
    partial = J * 7 * tiles * 64 * W * size if J > 1 else 0
    return dict(bodies_per_lane=W, waves_per_group=S, unroll=4 if W == 2 else 2, tiles=tiles, ranges=J, groups=tiles * J, block_threads=64 * S,
                lds_bytes=max(S - 1, 1) * 7 * 64 * W * size, launches=2 if J > 1 else 1, reserved=0, partial_offset=0, partial_bytes=partial)


def expected_workspace(n, m, dtype):
    return (expected_plan(n, m, dtype)["partial_bytes"] + 255) & ~255


def plan_dict(pkg, n, m, dtype):
    p = pkg.field_plan(n, m, dtype)
    return {name: getattr(p, name) for name, _ in pkg.FieldPlan._fields_}


def test_field_plan_and_workspace_are_functions_of_n_m_and_precision(pkg):
    """The grid crosses every switch point: S at N = 256, 512, 1 024; the tile edges of M (128 fp32, 64 fp64); the J target (tiles x J >= 512: M
    around 256 and 512 tiles, and around the tile counts where J halves) and its cap (the largest power of two <= chunks / S: N where
    chunks / S passes 2, 4, 64)."""
    lib = pkg.field_lib()
    sources = sorted({1, 2, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 5000, 8191, 8192, 8193, 65535, 65536, 65537, 70000, 262144, MAX_N})
    for dtype in (F32, F64):
        per = 64 * LANE_WIDTH[dtype]
        targets = sorted({1, 2, 63, 64, 65, 100, 127, 128, 129, 5000, per * 3, per * 4, per * 4 + 1, per * 8, per * 8 + 1, per * 255, per * 256, per * 256 + 1, per * 511, per * 512,
                          per * 512 + 1, 65536, 262144, MAX_M})
        for n in sources:
            for m in targets:
                plans = {tuple(plan_dict(pkg, n, m, dtype).items()) for _ in range(2)}
                assert len(plans) == 1
                got = dict(plans.pop())
                assert got == expected_plan(n, m, dtype), (n, m, dtype)
                chunks = -(-n // 128)
                assert got["ranges"] * got["waves_per_group"] <= max(chunks, got["waves_per_group"]), "every wave of every range has a chunk"
                assert got["lds_bytes"] <= 64 * 1024 and got["ranges"] & (got["ranges"] - 1) == 0
                assert pkg.field_workspace_bytes(n, m, dtype) == expected_workspace(n, m, dtype), (n, m, dtype)
        p = pkg.FieldPlan()
        fn = getattr(lib, "nb_field_plan_" + suffix(dtype))
        for n, m in ((0, 1), (1, 0), (MAX_N + 1, 1), (1, MAX_M + 1)):
            assert fn(n, m, ctypes.byref(p)) == ERR, (n, m)
        assert fn(16, 16, None) == ERR
    shape = lambda n, m: (plan_dict(pkg, n, m, F32)["tiles"], plan_dict(pkg, n, m, F32)["ranges"], plan_dict(pkg, n, m, F32)["launches"])  # noqa: E731
    assert shape(65536, 128) == (1, 64, 2) and shape(262144, 1024) == (8, 64, 2) and shape(65536, 65536) == (512, 1, 1)
    out = ctypes.c_size_t(0)
    for bad in ((0, 1, 4), (1, 0, 4), (MAX_N + 1, 1, 4), (1, MAX_M + 1, 8), (1000, 1000, 2), (1000, 1000, 16)):
        assert lib.nb_field_workspace_bytes(*bad, ctypes.byref(out)) == ERR, bad
    assert lib.nb_field_workspace_bytes(1000, 1000, 4, None) == ERR


# ---------------------------------------------------------------------------------------------------------------- argument errors


def test_field_argument_errors_are_caught_on_the_host(pkg):
    """Everything refused here is refused before a HIP call: the made-up addresses are never dereferenced."""
    lib = pkg.field_lib()
    count = ctypes.c_int(0)
    no_gpu = pkg.lib().nb_device_count(ctypes.byref(count)) != 0 or count.value == 0
    for dtype in (F32, F64):
        scalar, size, n, m = scalar_of(dtype), np.dtype(dtype).itemsize, 4096, 1000
        ws_bytes = pkg.field_workspace_bytes(n, m, dtype)
        assert ws_bytes > 0
        ok = dict(src=0x100000000, src_vel=0x200000000, tgt=0x300000000, tgt_vel=0x400000000, self=0x500000000, acc=0x600000000, jerk=0x700000000, pot=0x800000000,
                  ws=0x900000000, ws_bytes=ws_bytes, n=n, m=m, eps2=0.01)
        length = dict(src=4 * n * size, src_vel=4 * n * size, tgt=4 * m * size, tgt_vel=4 * m * size, self=4 * m, acc=4 * m * size, jerk=4 * m * size, pot=m * size, ws=ws_bytes)
        align = dict(src=4 * size, src_vel=4 * size, tgt=4 * size, tgt_vel=4 * size, self=4, acc=4 * size, jerk=4 * size, pot=size, ws=32)
        inputs, outputs = ("src", "src_vel", "tgt", "tgt_vel", "self"), ("acc", "jerk", "pot", "ws")

        def call(**kw):
            a = {**ok, **kw}
            return getattr(lib, "nb_field_eval_" + suffix(dtype))(a["src"], a["src_vel"], a["n"], a["tgt"], a["tgt_vel"], a["self"], a["m"], scalar(a["eps2"]), a["acc"], a["jerk"],
                                                                  a["pot"], a["ws"], a["ws_bytes"], None)

        for null in ("src", "tgt", "ws"):
            assert call(**{null: None}) == ERR, null
        for bad in (dict(n=0), dict(m=0), dict(n=MAX_N + 1), dict(m=MAX_M + 1), dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0), dict(eps2=-0.01), dict(eps2=float("nan"))):
            assert call(**bad) == ERR, bad
        for name in inputs + outputs:
            assert call(**{name: ok[name] + align[name] // 2}) == ERR, f"{name} misaligned"
        for x in outputs:  # an output against every other array: the same start, x on the last bytes of y, x running into y (32 is a multiple of every alignment)
            for y in inputs + outputs:
                if x == y:
                    continue
                assert call(**{x: ok[y]}) == ERR, (x, "==", y)
                assert call(**{x: ok[y] + (length[y] - 1) // 32 * 32}) == ERR, (x, "on the end of", y)
                assert call(**{x: ok[y] - (length[x] - 1) // 32 * 32}) == ERR, (x, "running into", y)
                assert call(**{y: ok[x]}) == ERR, (y, "==", x)
        assert call(acc=ok["src"]) == ERR, "an output overlapping sources"
        assert call(src_vel=None) == ERR and call(tgt_vel=None) == ERR and call(src_vel=None, tgt_vel=None) == ERR, "jerks without both velocity arrays"
        assert call(acc=None, jerk=None, pot=None) == ERR, "no output at all"
        if no_gpu:  # (with a GPU the made-up addresses would be used) past the argument check: a HIP error
            square = pkg.field_workspace_bytes(n, n, dtype)
            assert call(tgt=ok["src"], m=n, ws_bytes=square) not in (0, ERR), "targets == sources is accepted"
            assert call(tgt=ok["src"], tgt_vel=ok["src_vel"], m=n, ws_bytes=square) not in (0, ERR) and call(src_vel=ok["src"], tgt_vel=ok["src"]) not in (0, ERR), "inputs may alias each other"
            assert call(src_vel=None, tgt_vel=None, jerk=None) not in (0, ERR) and call(self=None) not in (0, ERR) and call(acc=None, jerk=None) not in (0, ERR)
            # a geometry of one range needs no workspace at all
            assert pkg.field_workspace_bytes(100, 5, dtype) == 0 and call(n=100, m=5, ws=None, ws_bytes=0) not in (0, ERR)


# ---------------------------------------------------------------------------------------------------------------- the listing


def field_listing():
    subprocess.run(["make", "-s", "-C", CSRC, "field.s"], check=True, capture_output=True)
    return open(os.path.join(CSRC, "field.s")).read()


def kernels_of(text):
    lines = text.split("\n")
    for i, line in enumerate(lines):
        m = re.match(r"^(_ZN2nb12_GLOBAL__N_1\d+field_\w+):", line)
        if m:
            end = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            yield m.group(1), lines[i:end]


def inner_loops(lines):
    """(label, instructions) of every innermost loop of a kernel's listing"""
    for i, line in enumerate(lines):
        if "Inner Loop Header" not in line:
            continue
        label = lines[i - 1].split(":")[0].strip()
        stop = next((k for k in range(i, len(lines)) if ("s_cbranch" in lines[k] or "s_branch" in lines[k]) and label in lines[k]), None)
        if stop is not None:
            yield label, [l.strip() for l in lines[i + 1:stop]]


def test_field_streaming_loops_keep_their_mix():
    """Every streaming loop of the field_eval kernels.  fp32 (8 packed pairs per trip: two groups of 4 sources against a packed pair of
    targets): 13 v_pk_* + 2 v_rsq_f32 per packed pair without the jerk, 27 + 2 with it, and nothing else in the plain form (but the
    scalar-register moves of the S = 1 jerk kernel, stated above); the MASK form has the same packed operations and v_rsq and, per packed pair,
    two v_cmp, two v_cndmask and one v_mov (the mass, now a vector) more.  fp64 (4 interactions per trip): 19 / 35 vector operations per
    interaction, the MASK form one v_cmp, two v_cndmask and two v_mov more.  Sources by s_load; no LDS, scratch or barrier instruction, no vector
    memory access; no kernel of the file uses scratch or more than 128 VGPRs (hermite_eval's occupancy: four waves per SIMD)."""
    text = field_listing()
    seen = 0
    for name, lines in kernels_of(text):
        if "field_evalI" not in name:
            continue
        seen += 1
        fp32, jerk, single = "field_evalIf" in name, "ELb1E" in name, "Li1E" in name
        forms = []
        for label, body in inner_loops(lines):
            count = lambda prefix: sum(1 for l in body if l.startswith(prefix))  # noqa: E731
            rsq = count("v_rsq_f32") if fp32 else count("v_rsq_f64")
            if rsq < 4:
                continue  # (the one-source loop of the ragged end, the fold)
            assert count("ds_") == 0 and count("scratch_") == 0 and count("s_barrier") == 0, (name, label)
            assert count("s_load") >= 2 and count("global_") == 0 and count("buffer_") == 0 and count("flat_") == 0, (name, label)
            select = (count("v_cmp"), count("v_cndmask"), count("v_mov"))
            moves = count("v_readlane") + count("v_writelane")
            if fp32:
                pairs = rsq // RSQ
                assert pairs == 8 and rsq == RSQ * pairs, (name, label)
                assert count("v_pk_") == (PK_JERK if jerk else PK_PLAIN) * pairs, (name, label, count("v_pk_") / pairs)
                rest = count("v_") - count("v_pk_") - rsq
                assert select in ((0, 0, 0), (2 * pairs, 2 * pairs, pairs)), (name, label, select)
            else:
                pairs = rsq
                assert pairs == 4, (name, label)
                rest = count("v_") - (DP_JERK if jerk else DP_PLAIN) * pairs
                assert select in ((0, 0, 0), (pairs, 2 * pairs, 2 * pairs)), (name, label, select)
            masked = select[0] > 0
            assert moves <= (LANE_MOVES_S1 * pairs if fp32 and jerk and single and not masked else 0), (name, label, moves)
            assert rest == sum(select) + moves, (name, label, "the forms differ by the compare / select operations only")
            if masked:
                assert sum(select) == (MASK_EXTRA if fp32 else DP_MASK_EXTRA) * pairs
            forms.append(masked)
        assert sorted(forms) == [False, True], (name, forms)
    assert seen == 16  # S = 1, 2, 4, 8 x (without, with the jerk) x two precisions: the compiled forms do not multiply per requested output
    sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    vgprs = [int(m) for m in re.findall(r"\.vgpr_count:\s+(\d+)", text)]
    assert len(sizes) == 20 and max(sizes) == 0, sizes
    assert len(vgprs) == 20 and max(vgprs) <= 128, vgprs


def test_field_sources_keep_the_scalar_unit_to_loads():
    for name in ("field.hip", "field_capi.hip", "field_kernels.h"):
        src = open(os.path.join(CSRC, name)).read().lower()
        for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_dcache_" + "wb", "s_dcache_" + "discard", "atomicadd"):
            assert word not in src, (name, word)
    text = field_listing()
    assert "s_" + "store" not in text and "_atomic" not in text and "s_dcache_" + "wb" not in text
    assert "s_load_dword" in text


# ---------------------------------------------------------------------------------------------------------------- the registry of field.s
# Every kernel of the listing, once: field_eval<T, S, JERK> with the (N, M) that reach it -- S follows N (kernel_matrix.N_BY_WAVES: on and
# around every switch point), JERK follows the call --, and field_finish<T, JERK>, which runs whenever the plan has more than one range.
# A case names what the plan query must report for it; tests/test_field_gpu.py asserts that on the device, then runs it.
FIELD_TARGETS = {1: (37, 130), 2: (1, 300, 129), 4: (64, 200, 1000, 130), 8: (129, 77)}  # M per N of N_BY_WAVES[S], in order: tile edges, ragged tiles, M > N
FIELD_LARGE = ((5000, 300), (1024, 65536))  # S = 8: four ranges and a second launch; 512 tiles of one range, one launch


def field_cases():
    """(dtype, S, jerk, n, m)"""
    out = []
    for dtype in (F32, F64):
        for s, sizes in N_BY_WAVES.items():
            shapes = list(zip((100,) + sizes if s == 1 else sizes, FIELD_TARGETS[s])) + (list(FIELD_LARGE) if s == 8 else [])
            for jerk in (False, True):
                out += [(dtype, s, jerk, n, m) for n, m in shapes]
    return out


def field_registry():
    """kernel -> the cases that reach it"""
    out = {}
    for dtype, s, jerk, n, m in field_cases():
        out.setdefault(("field_eval", (TYPE_NAME[dtype], s, jerk)), []).append((n, m))
        if expected_plan(n, m, dtype)["launches"] == 2:
            out.setdefault(("field_finish", (TYPE_NAME[dtype], jerk)), []).append((n, m))
    return out


def test_every_kernel_of_the_listing_is_in_the_registry(pkg):
    listed = listed_kernels(field_listing())
    assert len(listed) == len(set(listed)) == 20
    registry = field_registry()
    missing = sorted(kernel_name(k) for k in set(listed) - set(registry))
    stale = sorted(kernel_name(k) for k in set(registry) - set(listed))
    assert not missing, f"kernels of field.s no case reaches: {missing}"
    assert not stale, f"cases that name no kernel of field.s: {stale}"
    for dtype, s, jerk, n, m in field_cases():
        plan = plan_dict(pkg, n, m, dtype)
        assert plan["waves_per_group"] == s, (n, m, s)
    for (family, args), shapes in registry.items():
        if family == "field_eval":  # both ways of storing are reached where the geometry has them: J = 1 needs no finish, J > 1 does
            dtype = F32 if args[0] == "float" else F64
            launches = {plan_dict(pkg, n, m, dtype)["launches"] for n, m in shapes}
            assert launches == {1, 2}, (kernel_name((family, args)), launches)


# ---------------------------------------------------------------------------------------------------------------- CLI
CLI = os.path.join(ROOT, "cuda-nbody_amd", "nbody")


def test_cli_refuses_field_where_it_refuses_energy(tmp_path):
    """--field is single-device, not for --compare / --qatest / --systems (the refusals of --energy and --neighbours), and wants a readable
    file of 1 to 65 536 finite points"""
    good = tmp_path / "points.txt"
    good.write_text("# three points\n0 0 0\n\n  1.5 -2 3e-1   # the second\n1e3\t2\t3\n")
    base = ["--numbodies=1024", "--steps=1", f"--field={good}"]
    for extra in (base + ["--numdevices=2"], base + ["--devices=0,1"], ["--numdevices=2"] + base, base + ["--compare"], base + ["--qatest"], base + ["--systems=3"],
                  base + ["--integrator=hermite", "--numdevices=2"], base + ["--integrator=hermite-block", "--devices=0,1"], base + ["--integrator=hermite", "--compare"],
                  ["-numbodies=1024", "-steps=1", f"-field={good}", "-compare"]):
        r = subprocess.run([CLI, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr, (extra, r.returncode, r.stderr[:300])
        for other in ("--energy", "--neighbours=0.5"):
            twin = [other if a.lstrip("-").startswith("field=") else a for a in extra]
            e = subprocess.run([CLI, *twin], capture_output=True, text=True, timeout=60)
            assert e.returncode == 1 and "CRITICAL ERROR" in e.stderr, (other, "is refused there too", twin)
    r = subprocess.run([CLI, *base, "--numdevices=2"], capture_output=True, text=True, timeout=60)
    assert "--field is single-device" in r.stderr
    files = {"empty.txt": "", "comments.txt": "# nothing\n\n   \n", "two.txt": "1 2\n", "four.txt": "1 2 3 4\n", "word.txt": "0 0 0\n1 x 3\n", "nan.txt": "0 0 nan\n", "inf.txt": "inf 0 0\n",
             "huge.txt": "1e999 0 0\n", "long.txt": "0 0 0\n" * 65537}
    for name, content in files.items():
        (tmp_path / name).write_text(content)
        r = subprocess.run([CLI, "--numbodies=1024", "--steps=1", f"--field={tmp_path / name}"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr and "--field" in r.stderr, (name, r.returncode, r.stderr[:300])
    for extra in ([f"--field={tmp_path / 'missing.txt'}"], [f"--field={tmp_path}"], ["--field="], ["--field"]):
        r = subprocess.run([CLI, "--numbodies=1024", "--steps=1", *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr, (extra, r.returncode, r.stderr[:300])
    (tmp_path / "full.txt").write_text("0 0 0\n" * 65536)
    r = subprocess.run([CLI, "--numbodies=1024", "--steps=1", f"--field={tmp_path / 'full.txt'}", "--compare"], capture_output=True, text=True, timeout=60)
    assert "--field cannot be combined with --compare" in r.stderr, "65 536 points are read; the refusal is the combination's"
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--field FILE" in r.stdout
