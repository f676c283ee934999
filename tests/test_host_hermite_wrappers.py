"""The C++ host wrappers of the eight Hermite integrators (cuda-nbody_amd/host/bodysystemhip_hermite*.hpp, bodyensemblehip_hermite*.hpp),
each in both precisions, through the command line: `nbody --dump` is, byte for byte, the snapshot of the matching Python class driven with
the command line's own conversions.  Both sides end in the same C calls on the same start-up state, so there is no tolerance: what the
test holds is the choice of precision and order (host/hermite_calls.hpp, with_precision_and_order of host/cli_common.hpp) and the
argument lists the wrappers hand on.

N = 300 is a multiple neither of 64 nor of the 128- / 256-body tiles, so every kernel's ragged end is in play; the ensembles run 3 systems;
the fixed-step integrators take 3 steps, the block integrators run to 2 dt_max."""
import subprocess

import numpy as np
import pytest

from test_hermite import CLI, gpu_only

N, SYSTEMS = 300, 3
FIXED_STEPS, BLOCK_STEPS = 3, 2
ETA_START, LEVELS = 0.01, 30  # the command line's eta_start and its default --levels

# --integrator=<name>: the Python class, whether it steps B systems, whether it takes block time steps, and the default --eta of the block runs
INTEGRATORS = {
    "hermite": ("HermiteSystem", False, False, None),
    "hermite6": ("Hermite6System", False, False, None),
    "hermite-block": ("HermiteBlockSystem", False, True, 0.02),
    "hermite6-block": ("Hermite6BlockSystem", False, True, 0.2),
    "hermite-ensemble": ("HermiteEnsemble", True, False, None),
    "hermite6-ensemble": ("Hermite6Ensemble", True, False, None),
    "hermite-block-ensemble": ("HermiteBlockEnsemble", True, True, 0.02),
    "hermite6-block-ensemble": ("Hermite6BlockEnsemble", True, True, 0.2),
}


def startup_systems(oracle, n, b, dtype):
    """what `nbody --numbodies=N [--systems=B] [--fp64]` starts from: the single-system start-up state, then the next draws of the precision"""
    from oracle import scales_for
    pos0, vel0 = oracle.startup_state(n, dtype)
    c, v = scales_for(n)
    draws = [(pos0, vel0)] + [oracle.randomise(1, n, c, v, dtype) for _ in range(b - 1)]
    return np.stack([d[0].reshape(n, 4) for d in draws]), np.stack([d[1].reshape(n, 4) for d in draws])


def class_snapshot(gpu, name, dtype, pos, vel):
    """the Python class of --integrator=<name> on (B, N, 4) arrays, with the command line's conversions: dt and the softening are the demo
    row's floats widened to T, softening^2 = T(0.1) * T(0.1), dt_max = dt"""
    kind, many, block, eta = INTEGRATORS[name]
    dt = dtype(np.float32(0.016))
    s = dtype(np.float32(0.1))
    eps2 = s * s
    if not many:
        pos, vel = pos[0], vel[0]
    if block and many:
        system = getattr(gpu, kind)(N, SYSTEMS, dtype, gpu.HermiteBlockParams(eta, ETA_START, float(dt), LEVELS, 0), eps2)
    elif block:
        system = getattr(gpu, kind)(N, dtype, softening_sq=eps2, eta=eta, eta_start=ETA_START, dt_max=float(dt), max_level=LEVELS)
    elif many:
        system = getattr(gpu, kind)(N, SYSTEMS, dtype, softening_sq=eps2)
    else:
        system = getattr(gpu, kind)(N, dtype, softening_sq=eps2)
    system.set_state(pos, vel)
    if block:
        system.init()
        system.advance(BLOCK_STEPS * float(dt))
        got = system.snapshot()
    else:
        system.eval()
        for _ in range(FIXED_STEPS):
            system.step(dt)
        got = system.get_positions(), system.get_velocities()
    got = got[0].copy(), got[1].copy()
    system.free()
    return got


@gpu_only
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", list(INTEGRATORS))
def test_cli_dump_is_the_python_class_snapshot(gpu, oracle, tmp_path, name, dtype):
    _, many, block, _ = INTEGRATORS[name]
    b = SYSTEMS if many else 1
    out = tmp_path / "dump.bin"
    args = [CLI, f"--integrator={name}", f"--numbodies={N}", f"--steps={BLOCK_STEPS if block else FIXED_STEPS}", f"--dump={out}"]
    args += [f"--systems={SYSTEMS}"] if many else []
    args += ["--fp64"] if dtype is np.float64 else []
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    data = np.fromfile(out, dtype=dtype)
    assert data.size == 2 * 4 * N * b
    pos, vel = startup_systems(oracle, N, b, dtype)
    want_pos, want_vel = class_snapshot(gpu, name, dtype, pos, vel)
    assert want_pos.dtype == dtype and want_pos.size == 4 * N * b
    assert data[:4 * N * b].tobytes() == want_pos.tobytes() and data[4 * N * b:].tobytes() == want_vel.tobytes()
