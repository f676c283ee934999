"""6th-order block time steps of many independent systems in the launches of one call (nb_hermite6_block_ensemble_*,
include/nbody_hip_hermite6_block_ensemble.h; libnbody_hip_hermite6_block_ensemble.so from csrc/hermite6_block_ensemble*.hip).

The reference of every GPU test is the solo library (nb_hermite6_block_*; tests/test_hermite6_block.py and tests/test_hermite6_domain.py
hold it to long double and to the numpy restatement of the scheme) on each system alone, in the same process: the contract is
bit-identity, so every comparison is of bytes and there is no tolerance anywhere.

CPU tests: the boundary (declared, exported, mirrored), host-side argument checks with the cube rule, the plan against the solo plan, the
workspace formula, the streaming loops of hermite6_block_ensemble_eval against those of hermite6_block_eval in the two listings, the
command line's refusals.

GPU tests: one and 12 calls from hand-made schedules (three systems with different contents, `now` and n_act; every switch of S, ragged
chunks, J up to 16, the grid cap); independence of B, index, neighbours, workspace, stream; t_stop per system and the summary; init and
sync; a captured graph; a whole run of four binary clouds; the Python class and the command line; one call against the solo calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_capi_symbols import declared_symbols, exported_symbols
from test_hermite import CLI, CSRC, cloud, hip_runtime
from test_hermite6_block import STATE, Block6Device, hermite6_init, kernels_of
from test_hermite_block import BINARY_DT_MAX, BINARY_EPS2, BINARY_ETA_START, BINARY_LEVELS, hand_made_schedule
from test_hermite_block_ensemble import EnsembleDevice, expected_summary, scaled_binary, stack, streaming_loops, summary_dict

ERR = 10001
MAX_N, MAX_TOTAL = 65536, 1 << 28
NS = 9
SYMBOLS = ["nb_hermite6_block_ensemble_init_f32", "nb_hermite6_block_ensemble_init_f64", "nb_hermite6_block_ensemble_plan_f32", "nb_hermite6_block_ensemble_plan_f64",
           "nb_hermite6_block_ensemble_step_f32", "nb_hermite6_block_ensemble_step_f64", "nb_hermite6_block_ensemble_summary", "nb_hermite6_block_ensemble_sync_f32",
           "nb_hermite6_block_ensemble_sync_f64", "nb_hermite6_block_ensemble_workspace_bytes"]
ARRAYS = ("pos", "vel", "acc", "jerk", "snap", "crackle")
gpu_only = pytest.mark.gpu


def fns(pkg, dtype):
    lib = pkg.hermite6_block_ensemble_lib()
    sfx = "f32" if np.dtype(dtype) == np.float32 else "f64"
    scalar = np.float32 if sfx == "f32" else float
    return {name: getattr(lib, f"nb_hermite6_block_ensemble_{name}_{sfx}") for name in ("init", "step", "sync", "plan")}, scalar


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_header_library_and_binding_agree(pkg):
    declared = declared_symbols("nbody_hip_hermite6_block_ensemble.h")
    assert declared == SYMBOLS and len(declared) == 10
    assert exported_symbols(pkg.HERMITE6_BLOCK_ENSEMBLE_LIB_PATH) == declared, "exactly the ten exports: the ensemble evaluation linked in for init exports nothing"
    assert sorted(pkg.HERMITE6_BLOCK_ENSEMBLE_SIGNATURES) == declared
    needed = subprocess.run(["readelf", "-d", pkg.HERMITE6_BLOCK_ENSEMBLE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libnbody_hip" not in needed
    lib = pkg.hermite6_block_ensemble_lib()
    assert all(hasattr(lib, name) for name in declared)
    # every other library exports what its header declares, as before, and none of the new names
    others = set(exported_symbols(pkg.LIB_PATH))
    for path, header, count in ((pkg.ENSEMBLE_LIB_PATH, "nbody_hip_ensemble.h", 4), (pkg.HERMITE_LIB_PATH, "nbody_hip_hermite.h", 9), (pkg.HERMITE_BLOCK_LIB_PATH, "nbody_hip_hermite_block.h", 9),
                                (pkg.HERMITE6_LIB_PATH, "nbody_hip_hermite6.h", 11), (pkg.HERMITE6_BLOCK_LIB_PATH, "nbody_hip_hermite6_block.h", 9),
                                (pkg.NEIGHBOUR_LIB_PATH, "nbody_hip_neighbour.h", None), (pkg.FIELD_LIB_PATH, "nbody_hip_field.h", None), (pkg.KNN_LIB_PATH, "nbody_hip_knn.h", None),
                                (pkg.HERMITE_ENSEMBLE_LIB_PATH, "nbody_hip_hermite_ensemble.h", None), (pkg.HERMITE6_ENSEMBLE_LIB_PATH, "nbody_hip_hermite6_ensemble.h", None),
                                (pkg.HERMITE_BLOCK_ENSEMBLE_LIB_PATH, "nbody_hip_hermite_block_ensemble.h", 10)):
        names = exported_symbols(path)
        assert names == declared_symbols(header), header
        assert count is None or len(names) == count, header
        others |= set(names)
    assert len(exported_symbols(pkg.LIB_PATH)) == 96
    assert not set(declared) & others
    # the header takes the 4th-order block ensemble header's types and constants and declares no struct of its own
    text = open(os.path.join(ROOT, "include", "nbody_hip_hermite6_block_ensemble.h")).read()
    assert '#include "nbody_hip_hermite_block_ensemble.h"' in text and "typedef" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "#define" not in re.sub(r"#define NBODY_HIP_HERMITE6_BLOCK_ENSEMBLE_H", "", text)
    assert "A B-DEPENDENT TARGET" in text and "DELIBERATELY NOT" in text, "the header says why the geometry does not shrink with B"
    assert "FRONT of the workspace" in text, "the header says where init packs"
    assert os.path.exists(os.path.join(CSRC, "hermite6_block_ensemble_boundary.hip")) and not os.path.exists(os.path.join(CSRC, "hermite6_block_ensemble_capi.hip"))
    # the two "Not built" notes point here
    for header in ("nbody_hip_hermite6_block.h", "nbody_hip_hermite6_ensemble.h"):
        assert "nbody_hip_hermite6_block_ensemble.h" in open(os.path.join(ROOT, "include", header)).read(), header


def test_argument_errors_are_caught_on_the_host(pkg):
    """Everything refused here is refused before a HIP call: the addresses are never dereferenced."""
    lib = pkg.hermite6_block_ensemble_lib()
    out = ctypes.c_size_t(0)
    for bad in ((0, 3, 4), (MAX_N + 1, 1, 4), (1000, 0, 4), (MAX_N, 4097, 4), (1, MAX_TOTAL + 1, 4), (1000, 3, 2), (1000, 3, 16)):
        assert lib.nb_hermite6_block_ensemble_workspace_bytes(*bad, ctypes.byref(out)) == ERR, bad
    assert lib.nb_hermite6_block_ensemble_workspace_bytes(1000, 3, 4, None) == ERR
    assert lib.nb_hermite6_block_ensemble_workspace_bytes(MAX_N, 4096, 4, ctypes.byref(out)) == 0, "N B = 2^28 is allowed"
    # a grid over 2^31 threads with N B = 2^28: 2^15 systems of 8 192 bodies are 2^15 x 512 (fp32) evaluation workgroups of 512 threads
    for size, dtype in ((4, np.float32), (8, np.float64)):
        solo = pkg.hermite6_block_plan(8192, 1, dtype)
        assert solo.launch_groups * solo.block_threads * (1 << 15) > 1 << 31
        assert lib.nb_hermite6_block_ensemble_workspace_bytes(8192, 1 << 15, size, ctypes.byref(out)) == ERR, "N B = 2^28, but the evaluation grid is over 2^31 threads"
    good = pkg.HermiteBlockParams(0.2, 0.01, 0.125, 30, 0)
    for dtype in (np.float32, np.float64):
        f, scalar = fns(pkg, dtype)
        size = np.dtype(dtype).itemsize
        n, b = 1024, 3
        span = 4 * n * b * size
        ws_bytes = pkg.hermite6_block_ensemble_workspace_bytes(n, b, dtype)
        assert ws_bytes >= 12 * n * b * size, "the front of the workspace holds init's packed state"
        ok = dict(pos=0x100000000, vel=0x200000000, acc=0x300000000, jerk=0x400000000, snap=0x500000000, crackle=0x600000000, ticks=0x700000000, levels=0x800000000,
                  status=0x900000000, ws=0xa00000000, eps=0xd00000000, ws_bytes=ws_bytes, n=n, b=b, params=good, t_stop=1.0)
        length = dict(**{k: span for k in ARRAYS}, ticks=8 * n * b, levels=4 * n * b, status=64 * b, ws=ws_bytes, eps=b * size)
        align = dict(**{k: 4 * size for k in ARRAYS}, ticks=8, levels=4, status=8, ws=32, eps=size)

        def args(a):
            return [a[k] for k in STATE] + [a["status"], a["ws"], a["ws_bytes"], a["n"], a["b"], scalar(0.01), a["eps"], None if a["params"] is None else ctypes.byref(a["params"])]

        def step(**kw):
            a = {**ok, **kw}
            return f["step"](*args(a), a["t_stop"], None)

        def init(**kw):
            return f["init"](*args({**ok, **kw}), None)

        for call in (step, init):
            for null in length:
                if null != "eps":  # (NULL there means: the scalar for every system)
                    assert call(**{null: None}) == ERR, null
            assert call(params=None) == ERR
            for bad in (dict(n=0), dict(n=MAX_N + 1), dict(b=0), dict(n=MAX_N, b=4097), dict(n=8192, b=1 << 15), dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0)):
                assert call(**bad) == ERR, bad
            for name in length:
                assert call(**{name: ok[name] + align[name] // 2}) == ERR, f"{name} misaligned"
            for x in length:  # every pair of arrays, snaps and crackles included, overlapping at either end or equal
                for y in length:
                    if x == y:
                        continue
                    assert call(**{x: ok[y] + length[y] - align[x]}) == ERR, (x, "on the end of", y)
                    assert call(**{x: ok[y] - length[x] + align[x]}) == ERR, (x, "running into", y)
                    assert call(**{x: ok[y]}) == ERR, (x, "==", y)
            for eta, eta_start, dt_max, level in ((0, 0.01, 0.125, 30), (-1, 0.01, 0.125, 30), (float("nan"), 0.01, 0.125, 30), (0.2, 0, 0.125, 30), (0.2, float("inf"), 0.125, 30),
                                                  (0.2, 0.01, 0, 30), (0.2, 0.01, float("inf"), 30), (0.2, 0.01, 0.125, -1), (0.2, 0.01, 0.125, 41), (0.2, 0.01, 1e-305, 40)):
                assert call(params=pkg.HermiteBlockParams(eta, eta_start, dt_max, level, 0)) == ERR, (eta, eta_start, dt_max, level)
        assert step(t_stop=float("nan")) == ERR

        def sync(**kw):
            a = {"pos_out": 0xb00000000, "vel_out": 0xc00000000, **ok, **kw}
            return f["sync"](a["pos_out"], a["vel_out"], *[a[k] for k in ARRAYS], a["ticks"], a["status"], a["n"], a["b"], None if a["params"] is None else ctypes.byref(a["params"]), None)

        for null in ("pos_out", "vel_out", *ARRAYS, "ticks", "status", "params"):
            assert sync(**{null: None}) == ERR, null
        sync_length = {**{k: length[k] for k in (*ARRAYS, "ticks", "status")}, "pos_out": span, "vel_out": span}
        sync_at = {**ok, "pos_out": 0xb00000000, "vel_out": 0xc00000000}
        for x in sync_length:
            assert sync(**{x: sync_at[x] + (4 if x in ("ticks", "status") else 2 * size)}) == ERR, f"{x} misaligned"
            for y in sync_length:
                if x != y:
                    assert sync(**{x: sync_at[y] + sync_length[y] - (8 if x in ("ticks", "status") else 4 * size)}) == ERR, (x, "on the end of", y)
                    assert sync(**{x: sync_at[y]}) == ERR, (x, "==", y)
        for bad in (dict(n=0), dict(n=MAX_N + 1), dict(b=0), dict(n=MAX_N, b=4097), dict(params=pkg.HermiteBlockParams(0.2, 0.01, 0.125, 41, 0))):
            assert sync(**bad) == ERR, bad
        # the "Range of h" of nbody_hip_hermite6_block.h: fp32 refuses dt_max = 2^-10 with 33 levels in init, step and sync.  (fp64 takes
        # them: an accepted call goes on to the device, so that half is test_fp64_takes_the_parameters_fp32_refuses_for_their_cube.)
        cube = pkg.HermiteBlockParams(0.2, 0.01, 2.0 ** -10, 33, 0)
        if dtype == np.float32:
            assert step(params=cube) == ERR and init(params=cube) == ERR and sync(params=cube) == ERR
            for dt_max, level in ((2.0 ** -3, 40), (1.5 * 2.0 ** -43, 0), (2.0 ** 43, 0)):
                p = pkg.HermiteBlockParams(0.2, 0.01, dt_max, level, 0)
                assert step(params=p) == ERR and init(params=p) == ERR and sync(params=p) == ERR, (dt_max, level)
        else:
            for dt_max, level in ((2.0 ** -301, 40), (2.0 ** -341, 0), (2.0 ** 342, 0)):
                p = pkg.HermiteBlockParams(0.2, 0.01, dt_max, level, 0)
                assert step(params=p) == ERR and init(params=p) == ERR and sync(params=p) == ERR, (dt_max, level)
        plan = pkg.HermiteBlockEnsemblePlan()
        for bad in ((0, 3, 1), (MAX_N + 1, 1, 1), (100, 0, 1), (MAX_N, 4097, 1), (8192, 1 << 15, 1), (100, 3, 0), (100, 3, 101)):
            assert f["plan"](*bad, ctypes.byref(plan)) == ERR, bad
        assert f["plan"](16, 3, 1, None) == ERR
    summary = lib.nb_hermite6_block_ensemble_summary
    status, record = 0x900000000, 0xe00000000
    for bad in ((None, 3, record), (status, 3, None), (status, 0, record), (status, MAX_TOTAL + 1, record), (status + 4, 3, record), (status, 3, record + 4),
                (status, 3, status), (status, 3, status + 3 * 64 - 8), (status, 3, status - 56)):
        assert summary(bad[0], bad[1], bad[2], None) == ERR, bad


@gpu_only
def test_fp64_takes_the_parameters_fp32_refuses_for_their_cube(gpu):
    """dt_max = 2^-10 with 33 levels: a tick of 2^-43, whose cube is no normal float but a normal double.  fp32 refuses (no HIP call); fp64
    runs init, a step and sync."""
    cube = gpu.HermiteBlockParams(0.2, 0.01, 2.0 ** -10, 33, 0)
    pos, vel = stack([cloud(64, np.float64, 7 + s, "equal") for s in range(2)])
    e = Ensemble6Device(gpu, pos, vel, 0.01, cube)
    e.init(), e.step(), e.sync()
    assert [s.block_steps for s in e.statuses()] == [1, 1] and e.canaries_intact()
    e.free()
    with pytest.raises(gpu.NBodyHipError):
        e = Ensemble6Device(gpu, pos.astype(np.float32), vel.astype(np.float32), np.float32(0.01), cube)
        try:
            e.init()
        finally:
            e.free()


PLAN_SIZES = (1, 2, 255, 256, 300, 512, 1024, 5000, 16384, 65536)


def test_plan_is_the_solo_plan_times_the_number_of_systems(pkg):
    solo_names = [name for name, _ in pkg.HermiteBlockPlan._fields_]
    names = [name for name, _ in pkg.HermiteBlockEnsemblePlan._fields_]
    shared = [name for name in solo_names if name in names]
    assert shared == [name for name in solo_names if name != "launches"], "every field of the solo plan but its launch count, which this library undercuts"
    for dtype in (np.float32, np.float64):
        size, tile = np.dtype(dtype).itemsize, 128 if dtype == np.float32 else 64
        for n in PLAN_SIZES:
            for n_act in sorted({a for a in (1, 129, n) if a <= n}):
                solo = pkg.hermite6_block_plan(n, n_act, dtype)
                for b in (1, 3, 1000):
                    p = pkg.hermite6_block_ensemble_plan(n, b, n_act, dtype)
                    for name in shared:
                        assert getattr(p, name) == getattr(solo, name), (n, b, n_act, name)
                    assert p.partial_offset == solo.partial_offset and p.partial_bytes == p.ranges * NS * p.slots * size
                    assert p.lds_bytes == max(p.waves_per_group - 1, 1) * NS * tile * size + 128
                    assert p.groups_per_system == solo.launch_groups and p.blocks_per_system == -(-n // 256)
                    assert p.eval_grid == b * solo.launch_groups and p.schedule_grid == b * -(-n // 256)
                    assert p.step_launches == 5 and solo.launches == 6
                    assert p.workspace_stride * b == pkg.hermite6_block_ensemble_workspace_bytes(n, b, dtype)
                    assert p.partial_offset + p.partial_bytes <= p.workspace_stride


def test_workspace_size_is_monotone_and_the_documented_formula(pkg):
    def up(v):
        return -(-v // 256) * 256

    for dtype in (np.float32, np.float64):
        size, tile = np.dtype(dtype).itemsize, 128 if dtype == np.float32 else 64
        last = 0
        for n in sorted(set(PLAN_SIZES) | {3, 127, 511, 513, 1023, 1025, 2085, 4096, 40000}):
            groups = max(pkg.hermite6_block_plan(m, 1, dtype).launch_groups for m in (n, 255, 511, 1023) if m <= n)
            blocks = -(-n // 256)
            stride = up(12 * n * size) + up(groups * NS * tile * size) + up(4 * n) + up(4 * blocks) + up(8 * blocks) + up(4 * blocks) + up(64)
            sizes = [pkg.hermite6_block_ensemble_workspace_bytes(n, b, dtype) for b in (1, 2, 3, 64, 1000)]
            assert sizes == [stride * b for b in (1, 2, 3, 64, 1000)], (n, sizes[0], stride)
            assert stride >= last and stride % 256 == 0, "monotone in N (the launch grid alone is not: it shrinks where S doubles)"
            assert stride >= 12 * n * size, "B strides hold init's contiguous T[12 N B]"
            last = stride
        for below, at in ((255, 256), (511, 512), (1023, 1024)):
            assert pkg.hermite6_block_ensemble_workspace_bytes(below, 1, dtype) <= pkg.hermite6_block_ensemble_workspace_bytes(at, 1, dtype), (below, at)


def test_streaming_loops_are_those_of_the_solo_kernel():
    """hermite6_block_ensemble_eval<T, S> against hermite6_block_eval<T, S>, loop by loop, from the two listings: the same numbers of v_pk_*,
    v_rsq_* and scalar loads, and of vector arithmetic altogether; no LDS, scratch, barrier, v_mov or vector load inside, and no more lane
    moves of parked scalar registers than the solo loop has; no scratch in any kernel of the new unit; the occupancy hermite6_block_eval is
    compiled for.  Nothing is counted by hand: the solo listing is the yardstick."""
    subprocess.run(["make", "-s", "-C", CSRC, "hermite6_block.s", "hermite6_block_ensemble.s"], check=True, capture_output=True)
    solo = dict(kernels_of(open(os.path.join(CSRC, "hermite6_block.s")).read()))
    text = open(os.path.join(CSRC, "hermite6_block_ensemble.s")).read()
    ours = dict(kernels_of(text))
    seen = 0
    for t in ("f", "d"):
        for s in (1, 2, 4, 8):
            theirs = [lines for name, lines in solo.items() if f"hermite6_block_evalI{t}Li{s}E" in name]
            mine = [lines for name, lines in ours.items() if f"hermite6_block_ensemble_evalI{t}Li{s}E" in name]
            assert len(theirs) == 1 and len(mine) == 1, (t, s)
            want, got = streaming_loops(theirs[0]), streaming_loops(mine[0])
            assert len(want) >= 2, (t, s, "the unit and the mixed loop")
            assert len(got) == len(want), (t, s, got, want)
            for mine_loop, their_loop in zip(got, want):
                assert {k: v for k, v in mine_loop.items() if k != "lane_moves"} == {k: v for k, v in their_loop.items() if k != "lane_moves"}, (t, s, mine_loop, their_loop)
                assert mine_loop["lane_moves"] <= their_loop["lane_moves"], (t, s, mine_loop, their_loop)
            for loop in got:
                assert loop["lds"] == 0 and loop["scratch"] == 0 and loop["barrier"] == 0 and loop["v_mov"] == 0 and loop["vector_loads"] == 0, (t, s, loop)
            seen += 1
    assert seen == 8
    sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(sizes) == len(ours) and max(sizes) == 0, sizes
    assert all(int(m) == 0 for m in re.findall(r"; ScratchSize: (\d+)", text))
    records = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text)
    evals = {name: int(vgprs) for name, vgprs in records if "hermite6_block_ensemble_evalI" in name}
    assert len(evals) == 8
    for name, vgprs in evals.items():
        assert vgprs <= (168 if "evalId" in name else 128), (name, vgprs)  # 3 (fp64) / 4 (fp32) waves per SIMD of 512 registers
    # the occupancy line of every instantiation: what the attribute asks for
    for name, vgprs in evals.items():
        block = text[text.index(name + ":"):]
        occupancy = int(re.search(r"; Occupancy: (\d+)", block).group(1))
        assert occupancy == (3 if "evalId" in name else 4), (name, occupancy)
    src = open(os.path.join(CSRC, "hermite6_block_ensemble.hip")).read()
    assert "amdgpu_waves_per_eu(kWavesPerSimd<T>, kWavesPerSimd<T>)" in src and "kWavesPerSimd = sizeof(T) == 8 ? 3 : 4" in src
    assert "_atomic" not in text


CLI_NAME = "--integrator=hermite6-block-ensemble"


def test_cli_rejects_what_the_block6_ensemble_cannot_do():
    """hermite-block-ensemble's restrictions and messages, and the cube rule of hermite6-block on dt and --levels"""
    base = [CLI_NAME, "--numbodies=256", "--systems=3", "--t-end=0.1"]

    def refused(args, message):
        r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "CRITICAL ERROR" in r.stderr and message in r.stderr, (args, r.returncode, r.stderr[:300])

    refused([CLI_NAME, "--numbodies=256", "--t-end=0.1"], "--integrator=hermite-block-ensemble needs --systems")
    refused([CLI_NAME, "--numbodies=65537", "--systems=3", "--t-end=0.1"], "--systems: --numbodies must be at most 65536")
    refused([CLI_NAME, "--numbodies=65536", "--systems=4097", "--t-end=0.1"], "--integrator=hermite-block-ensemble: numbodies * systems must be at most 2^28")
    refused(base + ["--mode=strict"], "--integrator=hermite-block-ensemble has no strict mode")
    refused(base + ["--numdevices=2"], "--systems is single-device")
    refused(base + ["--devices=0,1"], "--systems is single-device")
    refused(base + ["--steps=3"], "--t-end cannot be combined with --benchmark or --steps")
    refused(base + ["--energy"], "--systems cannot be combined with")
    refused(base + ["--eta=0"], "")
    refused(base + ["--levels=41"], "--levels: Value not in range 0 to 40")
    refused(["--integrator=hermite6-block-ensembles", "--numbodies=256", "--systems=3"], "")
    # single precision: --demo=2 steps by dt = 0.0006, about 2^-10.7, and 33 levels below that a tick's cube is no normal float
    cube = "--integrator=hermite6-block-ensemble: dt * 2^-levels must have a normal cube in the run's precision"
    refused(base + ["--demo=2", "--levels=33"], cube)
    refused(base + ["--demo=2", "--levels=32"], cube)
    refused(base + ["--levels=37"], cube)
    for accepted in (base + ["--demo=2", "--levels=33", "--fp64"], base + ["--demo=2", "--levels=31"], base + ["--levels=36"]):
        r = subprocess.run([CLI, *accepted], capture_output=True, text=True, timeout=60)
        assert cube not in r.stderr, accepted  # (what the run does then is the GPU tests' matter)
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--integrator=hermite6-block-ensemble  hermite-block-ensemble's run" in r.stdout and "--eta [0.2]" in r.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU


class Ensemble6Device(EnsembleDevice):
    """EnsembleDevice of tests/test_hermite_block_ensemble.py with the snaps and crackles, through the C calls of this library: PAD canary bytes
    round every array; the workspace filled with 0xFF bytes (NaN in both precisions) unless ws_fill says otherwise, and what the calls never
    write of it -- the padding that ends every system's slice -- must still hold them afterwards."""

    def __init__(self, gpu, pos, vel, eps2, params, ws_fill=0xFF):
        self.gpu, self.dtype = gpu, pos.dtype
        self.b, self.n = pos.shape[0], pos.shape[1]
        self.f, self.scalar = fns(gpu, self.dtype)
        self.params, self.ws_fill = params, ws_fill
        self.ws_bytes = gpu.hermite6_block_ensemble_workspace_bytes(self.n, self.b, self.dtype)
        count = self.n * self.b
        self.kinds = {name: (self.dtype, 4) for name in (*ARRAYS, "pos_out", "vel_out")}
        self.kinds.update(ticks=(np.dtype(np.uint64), 1), levels=(np.dtype(np.int32), 1))
        sizes = {name: count * cols * kind.itemsize for name, (kind, cols) in self.kinds.items()}
        sizes.update(status=64 * self.b, ws=self.ws_bytes, eps=self.b * self.dtype.itemsize, summary=64)
        self.sizes, self.bufs = sizes, {}
        for name, nbytes in sizes.items():
            host = np.full(nbytes + 2 * self.PAD, 0xA5, np.uint8)
            host[self.PAD:self.PAD + nbytes] = ws_fill if name == "ws" else 0
            buf = gpu.DeviceBuffer(host.nbytes)
            buf.upload(host)
            self.bufs[name] = buf
        self.put("pos", pos), self.put("vel", vel)
        if np.ndim(eps2) == 0:
            self.eps2, self.eps_ptr = eps2, None
        else:
            self.eps2, self.eps_ptr = 123.0, self.ptr("eps")  # (the scalar is ignored when the array is given)
            self.raw_put("eps", np.ascontiguousarray(eps2, dtype=self.dtype))

    def _args(self):
        return [self.ptr(k) for k in STATE + ("status", "ws")] + [self.ws_bytes, self.n, self.b, self.scalar(self.eps2), self.eps_ptr, ctypes.byref(self.params)]

    def init(self, stream=None):
        self.packed = 12 * self.n * self.b * self.dtype.itemsize  # init packs a contiguous T[12 N B] into the front of the workspace
        self.gpu.check(self.f["init"](*self._args(), stream), "nb_hermite6_block_ensemble_init")

    def canaries_intact(self):
        """the PAD bytes round every array; and between the systems, where a slice ends with a control record of 64 bytes in a section of
        256: the 192 bytes no call writes -- but for those that lie in the front of the workspace after an init, which packs there"""
        for name, buf in self.bufs.items():
            host = buf.download(np.empty(buf.nbytes, np.uint8))
            assert (host[:self.PAD] == 0xA5).all() and (host[-self.PAD:] == 0xA5).all(), f"canary of {name}"
        stride = self.ws_bytes // self.b
        ws = self.get("ws").reshape(self.b, stride)
        checked = 0
        for s in range(self.b):
            if s * stride + stride - 192 >= getattr(self, "packed", 0):
                assert (ws[s, -192:] == self.ws_fill).all(), f"the end of slice {s}"
                checked += 1
        assert checked >= 1, "the last slice ends behind init's packed state"
        return True

    def step(self, t_stop=float("inf"), stream=None):
        self.gpu.check(self.f["step"](*self._args(), float(t_stop), stream), "nb_hermite6_block_ensemble_step")

    def sync(self, stream=None):
        self.gpu.check(self.f["sync"](*[self.ptr(k) for k in ("pos_out", "vel_out", *ARRAYS, "ticks", "status")], self.n, self.b, ctypes.byref(self.params), stream),
                       "nb_hermite6_block_ensemble_sync")

    def summary(self, stream=None):
        self.gpu.check(self.gpu.hermite6_block_ensemble_lib().nb_hermite6_block_ensemble_summary(self.ptr("status"), self.b, self.ptr("summary"), stream),
                       "nb_hermite6_block_ensemble_summary")
        if stream is not None:
            return None
        return self.gpu.HermiteBlockEnsembleSummary.from_buffer_copy(self.get("summary").tobytes())

    def everything(self):
        """per system, the bytes Block6Device.everything() gives of it: the eight arrays, then the status record"""
        arrays = [self.get(k) for k in STATE]
        status = self.get("status")
        return [b"".join(a[s].tobytes() for a in arrays) + status[s].tobytes() for s in range(self.b)]


_STARTS = {}


def solo_start(gpu, pos, vel, eps2):
    """accelerations, jerks, snaps and crackles (0) of one system from the solo library's initial evaluation; computed once per system"""
    key = (pos.tobytes(), vel.tobytes(), pos.dtype.str, float(eps2))
    if key not in _STARTS:
        _STARTS[key] = hermite6_init(gpu, pos, vel, pos.dtype.type(eps2))
    return _STARTS[key]


def hand_made_systems(gpu, dtype, n, actives, eps2s, seed0=0, masses=("equal", "species", "random")):
    """hand_made_systems of tests/test_hermite_block_ensemble.py for this scheme: len(actives) systems of n bodies with different contents and
    masses, each with the hand-made schedule of tests/test_hermite_block.py for its own n_act, moved in time by 256 ticks (a level-0 step)
    per system, so that every system has its own `now`.  Accelerations to crackles come from the solo initial evaluation.
    -> params, then per system (pos, vel, acc, jerk, snap, crackle, ticks, levels, now)"""
    params = gpu.HermiteBlockParams(0.2, 0.01, 0.125, 8, 0)
    out = []
    for s, n_act in enumerate(actives):
        pos, vel = cloud(n, dtype, seed0 + 100 * s + n, masses[s % len(masses)])
        now, max_level, active, levels, ticks = hand_made_schedule(n, n_act, seed0 + n * 7 + n_act + s)
        assert max_level == params.max_level
        acc, jerk, snap, crackle = solo_start(gpu, pos, vel, eps2s[s])
        out.append((pos, vel, acc, jerk, snap, crackle, (ticks + 256 * s).astype(np.uint64), levels.astype(np.int32), now + 256 * s))
    return params, out


def load_ensemble(gpu, params, systems, eps2, **kw):
    e = Ensemble6Device(gpu, np.stack([s[0] for s in systems]), np.stack([s[1] for s in systems]), eps2, params, **kw)
    for k, name in enumerate(STATE[2:], start=2):
        e.put(name, np.stack([s[k] for s in systems]))
    return e


def load_solo(gpu, params, system, eps2, **kw):
    d = Block6Device(gpu, system[0], system[1], system[0].dtype.type(eps2), params, **kw)
    for k, name in enumerate(STATE[2:], start=2):
        d.put(name, system[k])
    return d


def solo_bytes(gpu, params, system, eps2, calls, t_stop=float("inf")):
    """{k: Block6Device.everything() after k solo calls} for k in `calls`, from the hand-made state of one system"""
    d = load_solo(gpu, params, system, eps2, ws_fill=np.nan)
    out = {}
    for k in range(1, max(calls) + 1):
        d.step(t_stop)
        if k in calls:
            out[k] = d.everything()
    assert d.canaries_intact()
    d.free()
    return out


def check_against_solo(gpu, dtype, n, actives, calls=(1, 12)):
    eps2s = [0.01, 0.003, 0.02][:len(actives)]
    params, systems = hand_made_systems(gpu, dtype, n, actives, eps2s)
    e = load_ensemble(gpu, params, systems, np.array(eps2s, dtype))
    got = {}
    for k in range(1, max(calls) + 1):
        e.step()
        if k in calls:
            got[k] = e.everything()
        if k == 1:
            first = e.statuses()
            assert [(s.now_ticks, s.last_active, s.block_steps, s.flags) for s in first] == [(system[8], a, 1, 0) for system, a in zip(systems, actives)], "own now and n_act per system"
            assert len({s.now_ticks for s in first}) == len(actives)
    assert e.canaries_intact()
    assert summary_dict(e.summary()) == expected_summary(gpu, e.statuses())
    e.free()
    for s, system in enumerate(systems):
        want = solo_bytes(gpu, params, system, eps2s[s], calls)
        for k in calls:
            assert got[k][s] == want[k], f"N {n}, system {s} (n_act {actives[s]}) after {k} call(s): not the solo step's bits"


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [2, 127, 256, 300, 512, 1024, 5000])
def test_three_systems_take_the_solo_steps_bit_for_bit(gpu, dtype, n):
    """n_act = 1, 129 (or N) and N in one call; S switches at 256 / 512 / 1 024, 127 and 300 and 5 000 end in a ragged chunk, J reaches 4 at 5 000"""
    check_against_solo(gpu, dtype, n, [1, min(129, n), n])
    if n == 5000:
        assert max(gpu.hermite6_block_ensemble_plan(n, 3, a, dtype).ranges for a in (1, 129, n)) == 4


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [16384, 65536])
def test_two_large_systems_take_the_solo_steps_bit_for_bit(gpu, dtype, n):
    """16 384: J = 16 with 129 due bodies; 65 536: the launch grid of a system at its cap, all of it working when every body is due"""
    few, every = gpu.hermite6_block_ensemble_plan(n, 2, 129, dtype), gpu.hermite6_block_ensemble_plan(n, 2, n, dtype)
    if n == 16384:
        assert few.ranges == 16
    else:
        assert every.groups == every.launch_groups or dtype == np.float32, "fp64: 1 024 tiles are the whole grid"
        assert every.launch_groups == max(1023, every.tiles)
    check_against_solo(gpu, dtype, n, [129, n])


def run_from_init(gpu, pos, vel, eps2, params, calls, stream=None, **kw):
    e = Ensemble6Device(gpu, pos, vel, eps2, params, **kw)
    if stream is not None:
        gpu.check(gpu.lib().nb_device_synchronize(), "nb_device_synchronize")
    e.init(stream)
    for _ in range(calls):
        e.step(stream=stream)
    if stream is not None:
        gpu.check(gpu.lib().nb_stream_synchronize(stream), "nb_stream_synchronize")
    return e


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_system_does_not_depend_on_the_others(gpu, dtype):
    """init and 12 calls: the same bits alone (B = 1) and as system 3 of 5 whose others are NaN, inf and huge; with another workspace content;
    on another stream; when run twice -- and the solo library's bits in every case"""
    n, calls = 300, 12
    params = gpu.HermiteBlockParams(0.2, 0.01, 0.016, 12, 0)
    pos, vel = cloud(n, dtype, 91, "species")
    eps2 = dtype(1e-3)
    solo = Block6Device(gpu, pos, vel, eps2, params)
    solo.init()
    for _ in range(calls):
        solo.step()
    want, status = solo.everything(), solo.status()
    solo.free()
    assert status.block_steps == calls and status.body_steps < calls * n, "a mixed schedule"

    alone = run_from_init(gpu, pos[None], vel[None], eps2, params, calls)
    assert alone.everything() == [want] and alone.canaries_intact()
    alone.free()

    others_pos, others_vel = np.empty((5, n, 4), dtype), np.empty((5, n, 4), dtype)
    for s, fill in enumerate((np.nan, np.inf, 1e30, None, -np.inf)):
        others_pos[s], others_vel[s] = (pos, vel) if fill is None else (fill, fill)
    lib = gpu.lib()
    stream = ctypes.c_void_p()
    gpu.check(lib.nb_stream_create(ctypes.byref(stream)), "nb_stream_create")
    for what, kw in (("NaN workspace", {}), ("zero workspace", dict(ws_fill=0)), ("again", {}), ("another stream", dict(stream=stream))):
        crowd = run_from_init(gpu, others_pos, others_vel, eps2, params, calls, **kw)
        assert crowd.everything()[3] == want, f"system 3 of 5, {what}"
        assert crowd.canaries_intact(), what
        crowd.free()
    gpu.check(lib.nb_stream_destroy(stream), "nb_stream_destroy")


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_t_stop_holds_each_system_at_its_own_last_step(gpu, dtype):
    """Three clouds of equal masses whose bodies all start at level 2, 5 and 7 of 8 (ticks 0): to t_stop = dt_max the deeper a system starts, the
    more calls it needs.  A system that has stopped keeps every byte while the others go on; a larger t_stop resumes it; the summary counts."""
    n = 300
    eps2s = [0.01, 0.01, 0.01]
    params, systems = hand_made_systems(gpu, dtype, n, [n, n, n], eps2s, seed0=5, masses=("equal",))
    systems = [(*system[:6], np.zeros(n, np.uint64), np.full(n, level, np.int32), 0) for system, level in zip(systems, (2, 5, 7))]
    e = load_ensemble(gpu, params, systems, dtype(0.01))
    t_stop = params.dt_max
    stopped_at, frozen, history = {}, {}, []
    for call in range(1, 400):
        e.step(t_stop)
        statuses = e.statuses()
        history.append([s.block_steps for s in statuses])
        for s, status in enumerate(statuses):
            if status.flags & gpu.HERMITE_BLOCK_STOPPED and s not in stopped_at:
                stopped_at[s] = call
                frozen[s] = e.everything()[s]
        if call == 8:
            assert summary_dict(e.summary()) == expected_summary(gpu, statuses)
        if len(stopped_at) == 3:
            break
    early, late = min(stopped_at, key=stopped_at.get), max(stopped_at, key=stopped_at.get)
    print("stopped at call", stopped_at)
    assert len(stopped_at) == 3 and stopped_at[early] + 1 < stopped_at[late], f"one system reaches t_stop calls before another: {stopped_at}"
    final, statuses = e.everything(), e.statuses()
    for s in range(3):
        assert final[s] == frozen[s], f"system {s} stopped at call {stopped_at[s]} and changed afterwards"
        assert statuses[s].now_ticks == 1 << 8 and statuses[s].block_steps == stopped_at[s] - 1, "it stopped at t = dt_max, where all its bodies are due"
    first, last = stopped_at[early], stopped_at[late]
    assert history[last - 2][late] > history[first - 1][late] and history[last - 2][early] == history[first - 1][early], "the late system kept stepping while the early one stood"
    record = summary_dict(e.summary())
    assert record == expected_summary(gpu, statuses) and record["stopped"] == 3 and record["min_now_ticks"] == record["max_now_ticks"] == 1 << 8
    # the solo library, the same number of calls with the same t_stop: the same bits, the flag and deepest_level included
    for s, system in enumerate(systems):
        assert solo_bytes(gpu, params, system, eps2s[s], (last,), t_stop=t_stop)[last] == final[s], s
    # a later, larger t_stop resumes every system
    e.step(2 * t_stop)
    resumed = e.statuses()
    assert all(not r.flags & gpu.HERMITE_BLOCK_STOPPED and r.block_steps == b.block_steps + 1 and r.now_ticks > b.now_ticks for r, b in zip(resumed, statuses))
    record = summary_dict(e.summary())
    assert record == expected_summary(gpu, resumed) and record["stopped"] == 0
    assert e.canaries_intact()
    e.free()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [2, 300, 1024])
def test_init_and_sync_are_the_solo_calls_per_system(gpu, dtype, n):
    """init from garbage in every output array (its crackle is 0); sync after 5 calls, every system at a time of its own, velocities.w kept.
    Softening per system (one of them 0: the floor) and, at 300 bodies, as a scalar 0 too."""
    params = gpu.HermiteBlockParams(0.2, 0.01, 0.016, 12, 0)
    systems = [cloud(n, dtype, 40 + n + s, ("random", "equal", "species")[s]) for s in range(3)]
    for s, (_, v) in enumerate(systems):
        v[:, 3] = np.arange(n) + 1000 * s + 0.5  # velocities.w: a payload of the caller's
    for eps2 in ([1e-4, 0.0, 0.01],) + ((0.0,) if n == 300 else ()):
        per_system = np.ndim(eps2) != 0
        pos, vel = stack(systems)
        e = Ensemble6Device(gpu, pos, vel, np.array(eps2, dtype) if per_system else dtype(eps2), params)
        for name in ("acc", "jerk", "snap", "crackle"):
            e.put(name, np.full((3, n, 4), 3.25, dtype))
        e.put("ticks", np.full((3, n), 77, np.uint64)), e.put("levels", np.full((3, n), -5, np.int32))
        e.raw_put("status", np.full((3, 64), 0x5A, np.uint8))
        e.init()
        started = e.everything()
        assert not e.get("crackle").any(), "init's crackle is 0"
        for _ in range(5):
            e.step()
        e.sync()
        stepped, snapshot = e.everything(), (e.get("pos_out"), e.get("vel_out"))
        assert e.canaries_intact()
        e.free()
        assert snapshot[1][..., 3].tobytes() == vel[..., 3].tobytes(), "velocities.w preserved"
        for s, (p, v) in enumerate(systems):
            d = Block6Device(gpu, p, v, dtype(eps2[s] if per_system else eps2), params, ws_fill=np.nan)
            d.init()
            assert d.everything() == started[s], (n, s, "init")
            for _ in range(5):
                d.step()
            d.sync()
            assert d.everything() == stepped[s], (n, s, "5 calls")
            assert d.get("pos_out").tobytes() == snapshot[0][s].tobytes() and d.get("vel_out").tobytes() == snapshot[1][s].tobytes(), (n, s, "sync")
            d.free()


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_captured_graph_gives_the_direct_calls_bits(gpu, dtype):
    """init + steps + summary captured on ONE stream and replayed"""
    n, calls = 300, 12
    params = gpu.HermiteBlockParams(0.2, 0.01, 0.016, 12, 0)
    pos, vel = stack([cloud(n, dtype, 60 + s, ("equal", "random", "species")[s]) for s in range(3)])
    eps2 = np.array([1e-3, 2e-3, 1e-2], dtype)
    direct = run_from_init(gpu, pos, vel, eps2, params, calls)
    want, want_summary = direct.everything(), direct.summary()
    direct.free()
    lib, hip = gpu.lib(), hip_runtime()
    stream = ctypes.c_void_p()
    gpu.check(lib.nb_stream_create(ctypes.byref(stream)), "nb_stream_create")
    captured = Ensemble6Device(gpu, pos, vel, eps2, params)
    gpu.check(lib.nb_device_synchronize(), "nb_device_synchronize")
    graph, graph_exec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 0) == 0
    captured.init(stream)
    for _ in range(calls):
        captured.step(stream=stream)
    captured.summary(stream)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
    assert not captured.get("acc").any(), "recorded, not run"
    assert hip.hipGraphInstantiate(ctypes.byref(graph_exec), graph, None, None, 0) == 0
    assert hip.hipGraphLaunch(graph_exec, stream) == 0
    gpu.check(lib.nb_stream_synchronize(stream), "nb_stream_synchronize")
    assert captured.everything() == want, "captured and replayed"
    assert captured.get("summary").tobytes() == bytes(want_summary)
    assert captured.canaries_intact()
    assert hip.hipGraphExecDestroy(graph_exec) == 0 and hip.hipGraphDestroy(graph) == 0
    captured.free()
    gpu.check(lib.nb_stream_destroy(stream), "nb_stream_destroy")


CLASS_STATE = ("positions", "velocities", "accelerations", "jerks", "snaps", "crackles", "ticks", "levels")


def class_state(system):
    return [getattr(system, "get_" + name)() for name in CLASS_STATE]


@gpu_only
def test_a_whole_run_of_four_binary_clouds(gpu):
    """fp64, eta = 0.2, to t = 1/8 through Hermite6BlockEnsemble.advance: every system's final state, levels, status and snapshot are those of
    Hermite6BlockSystem.advance on it alone, and the summary adds the solo counters up"""
    systems = [scaled_binary(scale) for scale in (1, 2, 4, 8)]
    n, t_stop = systems[0][0].shape[0], 0.125
    ensemble = gpu.Hermite6BlockEnsemble(n, 4, np.float64, gpu.HermiteBlockParams(0.2, BINARY_ETA_START, BINARY_DT_MAX, BINARY_LEVELS, 0), BINARY_EPS2)
    ensemble.set_state(*stack(systems))
    ensemble.init()
    summary = ensemble.advance(t_stop)
    got = class_state(ensemble)
    statuses, snapshot = ensemble.statuses(), ensemble.snapshot()
    ensemble.free()
    solo_steps, solo_bodies = [], []
    for s, (pos, vel) in enumerate(systems):
        system = gpu.Hermite6BlockSystem(n, np.float64, softening_sq=BINARY_EPS2, eta=0.2, eta_start=BINARY_ETA_START, dt_max=BINARY_DT_MAX, max_level=BINARY_LEVELS)
        system.set_state(pos, vel)
        system.init()
        status = system.advance(t_stop)
        want = class_state(system)
        want_snapshot = system.snapshot()
        system.free()
        for name, g, w in zip(CLASS_STATE, got, want):
            assert g[s].tobytes() == w.tobytes(), (s, name)
        assert bytes(statuses[s]) == bytes(status), s
        assert snapshot[0][s].tobytes() == want_snapshot[0].tobytes() and snapshot[1][s].tobytes() == want_snapshot[1].tobytes(), s
        assert status.now_ticks == 1 << BINARY_LEVELS
        solo_steps.append(status.block_steps), solo_bodies.append(status.body_steps)
    print("block steps per system:", solo_steps)
    assert len(set(solo_steps)) > 1, "the harder binaries take more block steps"
    assert (summary.block_steps, summary.body_steps, summary.stopped, summary.systems) == (sum(solo_steps), sum(solo_bodies), 4, 4)
    assert summary.min_now_ticks == summary.max_now_ticks == 1 << BINARY_LEVELS


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_python_class_gives_the_c_calls_bits(gpu, dtype):
    n, b = 777, 3
    params = gpu.HermiteBlockParams(0.3, 0.02, 0.016, 9, 0)
    pos, vel = stack([cloud(n, dtype, 55 + s, "random") for s in range(b)])
    eps2 = np.array([1e-3, 2e-3, 4e-3], dtype)
    d = run_from_init(gpu, pos, vel, eps2, params, 30)
    d.sync()
    want, want_snapshot, want_status, want_summary = [d.get(k) for k in STATE], (d.get("pos_out"), d.get("vel_out")), d.get("status").tobytes(), bytes(d.summary())
    d.free()
    ensemble = gpu.Hermite6BlockEnsemble(n, b, dtype, params, eps2)
    assert isinstance(ensemble, gpu.HermiteBlockEnsemble)
    ensemble.set_state(pos, vel)
    ensemble.init()
    for _ in range(30):
        ensemble.step()
    for name, g, w in zip(CLASS_STATE, class_state(ensemble), want):
        assert g.tobytes() == w.tobytes(), name
    snap = ensemble.snapshot()
    assert snap[0].tobytes() == want_snapshot[0].tobytes() and snap[1].tobytes() == want_snapshot[1].tobytes()
    assert b"".join(bytes(s) for s in ensemble.statuses()) == want_status and bytes(ensemble.summary()) == want_summary
    # advance() ends with every system at the last block step not past t_stop
    ensemble.set_state(pos, vel)
    ensemble.init()
    summary = ensemble.advance(5 * 0.016, batch=16)
    assert summary.stopped == b and summary.min_now_ticks == summary.max_now_ticks == 5 << 9 and np.allclose(ensemble.times(), 5 * 0.016, rtol=0, atol=1e-15)
    ensemble.free()
    default = gpu.Hermite6BlockEnsemble(16, 2, dtype)
    assert (default.params.eta, default.params.eta_start, default.params.dt_max, default.params.max_level) == (0.2, 0.01, 0.125, 30)
    default.free()
    with pytest.raises(gpu.NBodyHipError):
        gpu.Hermite6BlockEnsemble(0, 3, dtype)
    with pytest.raises(gpu.NBodyHipError):
        gpu.Hermite6BlockEnsemble(65537, 1, dtype)


@gpu_only
def test_cli_dump_equals_the_class_snapshot(gpu, oracle, tmp_path):
    """the start-up states of `nbody --systems` (tests/test_hermite_ensemble.py), to t = 3 dt: --dump is the class's snapshot, the counters are
    the summary's, the integrator is named hermite6-block and --eta defaults to 0.2; --benchmark prints its figures"""
    from test_hermite_ensemble import cli_systems
    n, b, levels = 512, 3, 12
    dt_max = float(np.float32(0.016))
    s = np.float32(0.1)
    pos, vel = cli_systems(oracle, n, b)
    out = tmp_path / "block6_ensemble.bin"
    for eta in (0.3, None):
        ensemble = gpu.Hermite6BlockEnsemble(n, b, np.float32, gpu.HermiteBlockParams(0.2 if eta is None else eta, 0.01, dt_max, levels, 0), s * s)
        ensemble.set_state(pos, vel)
        ensemble.init()
        summary = ensemble.advance(3 * dt_max)
        want = ensemble.snapshot()
        ensemble.free()
        assert summary.min_now_ticks == 3 << levels
        for how in ("--steps=3", f"--t-end={3 * dt_max!r}"):
            r = subprocess.run([CLI, CLI_NAME, f"--numbodies={n}", f"--systems={b}", how, f"--levels={levels}", f"--dump={out}"] + ([] if eta is None else [f"--eta={eta}"]),
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            data = np.fromfile(out, dtype=np.float32)
            assert data.size == 2 * 4 * n * b
            assert data[:4 * n * b].tobytes() == want[0].tobytes() and data[4 * n * b:].tobytes() == want[1].tobytes(), (eta, how)
            m = re.search(r"^(\d+) block steps, (\d+) body steps = ", r.stdout, re.M)
            assert m and (int(m[1]), int(m[2])) == (summary.block_steps, summary.body_steps), r.stdout[-600:]
            assert f"{b} systems stopped" in r.stdout and f"{n} bodies x {b} systems, hermite6-block integrator, eta {0.2 if eta is None else eta:g}, {levels} levels" in r.stdout
    r = subprocess.run([CLI, CLI_NAME, f"--numbodies={n}", f"--systems={b}", "--benchmark", "-i=2", "--fp64"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"^%d bodies x %d systems, hermite6-block integrator, total time for 2 intervals of dt_max: ([\d.e+-]+) ms\n= ([\d.e+-]+) ms per interval\n"
                  r"= (\d+) block steps, (\d+) body steps = " % (n, b), r.stdout, re.M)
    assert m and int(m[3]) >= 2 * b and int(m[4]) >= 2 * b * n, r.stdout[-600:]


@gpu_only
def test_one_call_beats_the_solo_calls_back_to_back(gpu):
    """fp32, 64 systems of 1 024 bodies, 128 of each due (a hand-made schedule, put back before every timed call, outside the timed region):
    one ensemble call against the 64 nb_hermite6_block_step_f32 calls it replaces, on the same arrays' contents, device events, median of
    9 after warm-up, in the same process.

    Measured on an MI355X: 87.0 us against 2 849.4 us, 32.8x (the solo calls are 384 launches, the ensemble call five).  The bound is half of
    that gain."""
    n, b, n_act, dtype = 1024, 64, 128, np.float32
    params, systems = hand_made_systems(gpu, dtype, n, [n_act], [0.01])
    system = systems[0]
    e = load_ensemble(gpu, params, [system] * b, dtype(0.01))
    solos = [load_solo(gpu, params, system, 0.01) for _ in range(b)]
    ticks, levels = np.stack([system[6]] * b), np.stack([system[7]] * b)

    def rewind_ensemble():
        e.put("ticks", ticks), e.put("levels", levels)

    def rewind_solos():
        for d in solos:
            d.put("ticks", system[6]), d.put("levels", system[7])

    def median_ms(fn, prepare):
        for _ in range(2):
            prepare(), fn()
        times = []
        for _ in range(9):
            prepare()
            gpu.check(gpu.lib().nb_device_synchronize(), "nb_device_synchronize")
            start, stop = gpu.Event(), gpu.Event()
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_ms(stop))
        return sorted(times)[4]

    t_ensemble = median_ms(e.step, rewind_ensemble)
    assert [s.last_active for s in e.statuses()] == [n_act] * b

    def all_solos():
        for d in solos:
            d.step()

    t_solo = median_ms(all_solos, rewind_solos)
    assert all(d.status().last_active == n_act for d in solos)
    assert e.everything()[b - 1] == solos[b - 1].everything(), "the timed calls computed the same thing"
    e.free()
    for d in solos:
        d.free()
    print(f"64 x 1024 bodies, 128 due: one ensemble call {t_ensemble * 1e3:.1f} us, 64 solo calls {t_solo * 1e3:.1f} us ({t_solo / t_ensemble:.1f}x)")
    assert 16.4 * t_ensemble <= t_solo, (t_ensemble, t_solo)
