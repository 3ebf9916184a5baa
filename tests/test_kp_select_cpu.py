"""CPU: the workgroup-parallel partition of the keypoint selection (kp_introselect_block, df-vo_amd/csrc/solver_kp.hip)
restated in lock step on the host (tests/host_harness/kp_block_lockstep.h) against the scalar selection
sm::kp_introselect_cp, through the stand-alone program tests/host_harness/kp_block_lockstep_check.cpp built with
AddressSanitizer and UBSan: whole (key, tosort) state, both position types (packed 16-bit scan, two int scans), reads
confined to the documented slack of four floats on either side of the keys."""
import os
import subprocess

import numpy as np
import pytest

import select_world as S

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "kp_block_lockstep_check.cpp")
DEPS = [SRC, os.path.join(HERE, "host_harness", "kp_block_lockstep.h"),
        os.path.join(HERE, "..", "df-vo_amd", "csrc", "kp_select.h"), os.path.join(HERE, "..", "df-vo_amd", "csrc", "solver_math.h")]


@pytest.fixture(scope="module")
def checker():
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "kp_block_lockstep_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in DEPS):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    return exe


def test_lockstep_partition_exhaustive_over_three_values(checker):
    """every sequence over {0, 1, 2} of length 6 .. 11 with every kth in 3 .. num - 2, parallel passes down to ranges of
    6: all tie patterns around the pivot, self-pairs first / last / in a row, crossings next to either end"""
    r = subprocess.run([checker, "exhaustive"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.strip().endswith("exhaustive: ok"), r.stdout[-4000:]


def test_lockstep_partition_on_the_case_inventory(checker, tmp_path):
    """select_world.cases() (killers, structured, special keys) at the real switch of 256"""
    cases = [c for c in S.cases() if len(S.selection_keys(c)) > 0]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            keys = S.selection_keys(c)
            f.write(np.asarray([len(keys), min(c[2], len(keys)) - 1], np.int32).tobytes())
            f.write(np.ascontiguousarray(keys, np.float32).tobytes())
    r = subprocess.run([checker, "cases", path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.strip().endswith("cases: ok"), r.stdout[-4000:]
    assert "cases: %d selections" % len(cases) in r.stdout
