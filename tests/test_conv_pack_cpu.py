"""CPU: the ring kernels' host packers after the k-group walk became one function (df-vo_amd/csrc/conv_pack.hip) --
conv_pack_weights_f16g, conv_pack_weights_f32g, conv_build_f16g_table and conv_pack_weights against the loops they replaced,
byte for byte over the whole output, padding included -- through the stand-alone program
tests/host_harness/conv_pack_check.cpp: the host-only unit compiled as plain C++ (the ROCm clang++, for _Float16 on the host;
no HIP library, no GPU), with AddressSanitizer and UBSan linked in."""
import glob
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "df-vo_amd", "csrc")
SRC = os.path.join(HERE, "host_harness", "conv_pack_check.cpp")
UNIT = os.path.join(CSRC, "conv_pack.hip")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def checker():
    cxx = next((c for c in (os.path.join(ROCM, "llvm", "bin", "clang++"), os.path.join(ROCM, "lib", "llvm", "bin", "clang++"))
                if os.path.exists(c)), None)
    if cxx is None or not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip("no ROCm clang++ / HIP headers under %s (ROCM_PATH)" % ROCM)
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "conv_pack_check")
    deps = [SRC, UNIT] + glob.glob(os.path.join(CSRC, "*.h"))
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"),
                        "-o", exe, SRC, "-x", "c++", UNIT], check=True)
    return exe


def test_packed_weights_are_byte_identical_to_the_loops_they_replaced(checker):
    r = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("conv_pack_check: ok (6 shapes x 2)"), r.stdout
