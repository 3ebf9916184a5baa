"""CPU: the host-only stream logic (df-vo_amd/csrc/stream_layout.h) -- the stream pool's classification of probe times into
dispatch-pipe groups and hardware queues, and the fused pipeline's role -> stream plan per queue count -- through the
stand-alone program tests/host_harness/stream_layout_check.cpp, built with AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "stream_layout_check.cpp")
HDR = os.path.join(HERE, "..", "df-vo_amd", "csrc", "stream_layout.h")

CASES = ["classify_twelve_on_four_queues", "classify_twelve_queues_four_pipes", "classify_five_queues_uneven",
         "classify_positive_not_repeated", "classify_inconsistent", "classify_thresholds", "pick_too_few_queues"] + \
        ["plan_nqueues_%d" % n for n in (1, 2, 3, 4, 5, 7, 8, 12)]


@pytest.fixture(scope="module")
def checker():
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "stream_layout_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    return exe


def test_every_case_is_listed(checker):
    r = subprocess.run([checker, "--list"], stdout=subprocess.PIPE, text=True, check=True)
    assert sorted(r.stdout.split()) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_stream_layout(checker, case):
    r = subprocess.run([checker, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith(case + ": ok"), r.stdout
