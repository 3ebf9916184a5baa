"""CPU: the lifetimes of the nets' layer packings (df-vo_amd/csrc/dev_mem.h, net_layers.hip) -- a conv layer under a failure of
each of its allocations in every precision, packed twice, moved inside a std::vector, and DevArr's alloc_zeroed / detach --
through the stand-alone program tests/host_harness/net_layers_check.cpp: the host-only unit compiled as plain C++ against HIP
entry points and weight packers the program defines itself, with AddressSanitizer and UBSan."""
import glob
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "df-vo_amd", "csrc")
SRC = os.path.join(HERE, "host_harness", "net_layers_check.cpp")
STUB = os.path.join(HERE, "host_harness", "hip_stub.h")
UNIT = os.path.join(CSRC, "net_layers.hip")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

CASES = ["fail_each_fp32", "fail_each_f16x3", "fail_each_fp32_wino2", "repack_frees_first", "vector_of_layers", "alloc_zeroed",
         "detach"]


@pytest.fixture(scope="module")
def checker():
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers under %s (ROCM_PATH)" % ROCM)
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "net_layers_check")
    deps = [SRC, STUB, UNIT] + glob.glob(os.path.join(CSRC, "*.h"))
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"),
                        "-o", exe, SRC, "-x", "c++", UNIT], check=True)
    return exe


def test_every_case_is_listed(checker):
    r = subprocess.run([checker, "--list"], stdout=subprocess.PIPE, text=True, check=True)
    assert sorted(r.stdout.split()) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_net_layers(checker, case):
    r = subprocess.run([checker, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith(case + ": ok"), r.stdout
