"""CPU: the lifetimes of the solver chain's device buffers (df-vo_amd/csrc/dev_mem.h, solver_buffers.hip) -- every buffer
set under a failure of each of its allocations, growth by dimension, the on-demand arrays, and which side streams and
events a TrackerBuffers destroys -- through the stand-alone program tests/host_harness/solver_buffers_check.cpp: the
host-only unit compiled as plain C++ against HIP entry points the program defines itself, with AddressSanitizer and UBSan."""
import glob
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "df-vo_amd", "csrc")
SRC = os.path.join(HERE, "host_harness", "solver_buffers_check.cpp")
UNIT = os.path.join(CSRC, "solver_buffers.hip")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

CASES = ["%s_fail_each" % w for w in ("ransac", "pnp", "bestn", "rigid", "tracker_kp")] + \
        ["parts_fail_releases_all", "fits_no_calls", "grow_one_dimension", "grow_on_demand_fail", "devarr_moves",
         "streams_init_own", "streams_init_given", "streams_borrowed_aliased", "streams_rebind", "streams_shared"]


@pytest.fixture(scope="module")
def checker():
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers under %s (ROCM_PATH)" % ROCM)
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "solver_buffers_check")
    deps = [SRC, UNIT] + glob.glob(os.path.join(CSRC, "*.h"))
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"),
                        "-o", exe, SRC, "-x", "c++", UNIT], check=True)
    return exe


def test_every_case_is_listed(checker):
    r = subprocess.run([checker, "--list"], stdout=subprocess.PIPE, text=True, check=True)
    assert sorted(r.stdout.split()) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_solver_buffers(checker, case):
    r = subprocess.run([checker, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith(case + ": ok"), r.stdout
