"""CPU: the host-only half of dfvo_pipeline_set_iterative (df-vo_amd/csrc/pipeline_iter.h: option refusals, the keypoint counts
the loop's scale stage can meet, the rigid-flow keypoint configuration, the "not run" record) in a stand-alone program
(tests/host_harness/pipeline_iter_check.cpp) built with AddressSanitizer and UBSan; the HIP entry points the headers name are
tests/host_harness/hip_stub.h's."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "df-vo_amd", "csrc")
SRC = os.path.join(HERE, "host_harness", "pipeline_iter_check.cpp")
DEPS = [SRC, os.path.join(HERE, "host_harness", "hip_stub.h"), os.path.join(HERE, "..", "include", "dfvo_hip.h")] + [
    os.path.join(CSRC, n) for n in ("pipeline_iter.h", "pipeline_setup.h", "tracker.h", "solver.h", "dev_mem.h", "dfvo_common.h")]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_pipeline_iter_host_logic(tmp_path):
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pipeline_iter_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in DEPS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"),
                        "-o", exe, SRC], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("pipeline_iter: ok"), r.stdout
