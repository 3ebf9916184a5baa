"""CPU: the fused pipeline's option rules (df-vo_amd/csrc/pipeline_setup.h: which combinations of the option, iterative, depth-source
and pose blocks the four setters take, in either setter order, and the edge values of every range check) in a stand-alone program
(tests/host_harness/pipeline_setup_check.cpp) built with AddressSanitizer and UBSan.  The header names no HIP entry point."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "pipeline_setup_check.cpp")
DEPS = [SRC, os.path.join(HERE, "..", "include", "dfvo_hip.h"), os.path.join(HERE, "..", "df-vo_amd", "csrc", "pipeline_setup.h")]


def test_pipeline_setup_host_logic():
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pipeline_setup_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in DEPS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("pipeline_setup: ok"), r.stdout
