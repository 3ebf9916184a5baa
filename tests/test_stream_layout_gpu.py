"""GPU: the fused pipeline computes the same thing in every stream layout (df-vo_amd/csrc/stream_layout.h).  Three fresh
processes -- the hardware-queue count is read once, when HIP starts -- run tests/stream_layout_child.py: four queues (lane
layout), four queues with the wide layout forced, twelve queues (wide layout); their reports must agree bit for bit."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ENVS = [("4", "auto"), ("4", "wide"), ("12", "auto")]


def run_child(queues, layout):
    env = dict(os.environ, GPU_MAX_HW_QUEUES=queues, DFVO_STREAM_LAYOUT=layout)
    for k in ("DFVO_STREAM_POOL", "DFVO_STREAM_POOL_FORCE_FAIL", "DFVO_FLOW_INSTANCES"):
        env.pop(k, None)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "stream_layout_child.py")], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=240)
    except subprocess.TimeoutExpired as e:
        pytest.fail("child (%s queues, %s) ran out of time; no further child is started\n%s" % (queues, layout, e.stderr))
    if r.returncode < 0:
        pytest.fail("child (%s queues, %s) died from signal %d; no further child is started\n%s" % (queues, layout, -r.returncode, r.stderr))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines and lines[-1] == "DONE", r.stdout + r.stderr
    layouts = [json.loads(l[7:]) for l in lines if l.startswith("LAYOUT ")]
    assert len(layouts) == 1
    return layouts[0], [l for l in lines if l.startswith(("PAIR ", "RNG "))]


def test_layouts_agree_bit_for_bit(gpu):
    results = []
    for queues, layout in ENVS:  # one after the other; a child that died or hung has ended the test above
        results.append(run_child(queues, layout))
    for (queues, layout), (lay, rows) in zip(ENVS, results):
        print(queues, layout, lay["text"])
        pairs = [json.loads(r[5:]) for r in rows if r.startswith("PAIR ")]
        assert [(p["run"], p["pair"]) for p in pairs] == [("coded", k) for k in range(7)] + \
            [(t, k) for t in ("rigid_prefetch", "rigid_late") for k in range(3)]
        assert len([r for r in rows if r.startswith("RNG ")]) == 3
        # whether the pre-part was prefetched or left to track_begin changes nothing
        strip = lambda p: {k: v for k, v in p.items() if k != "run"}
        assert [strip(p) for p in pairs[7:10]] == [strip(p) for p in pairs[10:13]]
        assert any(p["status"] == 3 for p in pairs[7:]), "no pair of the rigid scene took the PnP fallback"
        assert all(p["status"] in (0, 3) for p in pairs) and all(p["n_kp"] > 10 for p in pairs)
    lanes = results[0][0]
    assert lanes["layout"] == "lanes" and lanes["streams"] == 4 and lanes["queues"] >= 4, lanes["text"]
    assert lanes["trk"] == lanes["rep0"] == lanes["rep1"] and lanes["pre0"] == lanes["pre1"] == lanes["depth"], lanes["text"]
    assert len({lanes["flow"], lanes["flow_x"], lanes["depth"], lanes["trk"]}) == 4, lanes["text"]
    for lay, _ in results[1:]:
        assert lay["layout"] == "wide" and lay["streams"] == 8, lay["text"]
    assert results[2][0]["queues"] >= 8, results[2][0]["text"]
    assert results[0][1] == results[1][1], "four queues: lanes vs wide"
    assert results[0][1] == results[2][1], "lanes on four queues vs wide on twelve"
