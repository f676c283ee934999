"""CPU test: the listing of pair_forces_jpacked (csrc/nbody_pair_lead.hip, `make asm`) holds the instruction mix it was written for
-- per rotation step 16 x (14 v_pk_* + 2 v_rsq_f32) + 12 lane moves with one species on both sides, 16 x 16 packed and 14 moves in
the general loop -- in 256 VGPRs at two waves per SIMD; and the kernels it stands beside, pair_forces<float, 8, 8> and <float, 4, 8>
in nbody_pair.s, still hold theirs (the counts of tests/test_capi_symbols.py, asserted here again).

A lane move is an instruction with wave_ror:1.  The positions of the two bodies j (and their masses) move as v_mov_b32_dpp; the six
reaction sums move INSIDE the addition that joins a step's sixteen terms to them (v_add_f32_dpp wave_ror:1: move and addition in
one instruction).  Twelve (fourteen) instructions either way, and nothing else on the vector unit."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cuda-nbody_amd", "csrc")


@pytest.fixture(scope="module")
def listings():
    subprocess.run(["make", "-s", "-C", CSRC, "asm"], check=True, capture_output=True)
    return {name: open(os.path.join(CSRC, name)).read().split("\n") for name in ("nbody_pair_lead.s", "nbody_pair.s")}


def kernel_lines(lines, pattern):
    start = next(i for i, l in enumerate(lines) if re.match(pattern, l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return start, end


def rotation_loops(lines, start, end):
    """per depth-2 loop: (v_pk_*, v_rsq_f32, wave_ror:1 moves, other v_* than plain moves, scratch_*, ds_*) from its header to its back-edge;
    a move is v_mov_b32_dpp or v_add_f32_dpp with wave_ror:1"""
    mixes = []
    for i in range(start, end):
        if "Inner Loop Header: Depth=2" not in lines[i]:
            continue
        label = lines[i - 1].split(":")[0].strip()
        stop = next(k for k in range(i, end) if "s_cbranch" in lines[k] and label in lines[k])
        body = [l.strip() for l in lines[i + 1:stop] if l.strip() and not l.strip().startswith(";")]
        count = lambda what: sum(1 for l in body if what in l.split()[0])  # noqa: E731
        rotations = sum(1 for l in body if l.startswith(("v_mov_b32_dpp", "v_add_f32_dpp")) and "wave_ror:1" in l)
        other = sum(1 for l in body if l.startswith("v_") and not l.startswith(("v_pk_", "v_rsq_f32", "v_mov_b32")) and not (l.startswith("v_add_f32_dpp") and "wave_ror:1" in l))
        mixes.append((count("v_pk_"), count("v_rsq_f32"), rotations, other, count("scratch_"), count("ds_")))
    return mixes


def test_jpacked_rotation_loops_hold_their_instruction_mix(listings):
    lines = listings["nbody_pair_lead.s"]
    start, end = kernel_lines(lines, r"_ZN2nb\S*pair_forces_jpackedILi8EE\S*:")
    source = open(os.path.join(CSRC, "nbody_pair_lead.hip")).read()
    unr = int(re.search(r"#define NB_PAIR_LEAD_UNR (\d+)", source).group(1))  # steps per trip of the rotation loop
    mixes = rotation_loops(lines, start, end)
    # two loops: one species on both sides (no mass multiply), and the general one (+2 v_pk_mul per body i, the masses of the bodies j rotate too)
    assert sorted(mixes) == [(unr * 224, unr * 32, unr * 12, 0, 0, 0), (unr * 256, unr * 32, unr * 14, 0, 0, 0)], mixes


def test_jpacked_register_budget(listings):
    lines = listings["nbody_pair_lead.s"]
    _, end = kernel_lines(lines, r"_ZN2nb\S*pair_forces_jpackedILi8EE\S*:")
    tail = "\n".join(lines[end:end + 60])
    assert int(re.search(r"; NumVgprs: (\d+)", tail).group(1)) == 256
    assert int(re.search(r"; NumAgprs: (\d+)", tail).group(1)) == 0
    assert int(re.search(r"; Occupancy: (\d+)", tail).group(1)) == 2


def test_pair_forces_listing_is_what_it_was(listings):
    """pair_forces<float, 4, 8> and <float, 8, 8>, four steps per trip: the mixes tests/test_capi_symbols.py pins"""
    lines = listings["nbody_pair.s"]
    mixes = rotation_loops(lines, *kernel_lines(lines, r"_ZN2nb\S*pair_forcesIfLi4ELi8EE\S*:"))
    assert sorted(mixes) == [(224, 32, 36, 0, 0, 0), (240, 32, 36, 0, 0, 0), (240, 32, 40, 0, 0, 0), (256, 32, 40, 0, 0, 0)], mixes
    start, end = kernel_lines(lines, r"_ZN2nb\S*pair_forcesIfLi8ELi8EE\S*:")
    mixes = rotation_loops(lines, start, end)
    assert sorted(mixes) == [(448, 64, 36, 0, 0, 0), (480, 64, 36, 0, 0, 0), (480, 64, 40, 0, 0, 0), (512, 64, 40, 0, 0, 0)], mixes
    tail = "\n".join(lines[end:end + 60])
    assert int(re.search(r"; NumVgprs: (\d+)", tail).group(1)) == 256 and int(re.search(r"; NumAgprs: (\d+)", tail).group(1)) == 0
    assert int(re.search(r"; Occupancy: (\d+)", tail).group(1)) == 2
    # no new __global__ in this listing: the forces kernel of the headline geometry lives in a translation unit of its own
    assert not [l for l in lines if ".amdhsa_kernel" in l and "jpacked" in l]
