"""The cases of tests/test_pipeline_refine_gpu.py and their expected values (tests/pipeline_refine_oracle.solve_pair over three
pairs, the depths rolled over as the pipeline rolls them), computed once per process and shared with the CPU tests that assert
what the cases exercise.  No GPU, no torch call in here."""
import numpy as np

import pipeline_refine_oracle as RO
from pipeline_configs_oracle import SOURCES

FLOW_OPEN = dict(validity="flow", validity_thre=1.0)


def scene_inputs(name):
    from test_pipeline_configs_gpu import scene  # (the 128 x 416 rigid scene, the 192 x 640 tunnel)
    return scene(name)


def opts(source, **kw):
    o = dict(SOURCES[source])
    o.update(kw)
    return o


def refine(e=False, s=False, p=False, score="opt_flow", **kw):
    ro = dict(e_iterative_kp=e, scale_iterative_kp=s, pnp_iterative_kp=p, e_iterative_score=score, pnp_iterative_score=score)
    ro.update(kw)
    return ro


# (id, scene, TrackingPipeline options, refinement keys, pairs whose processed current depth is zeroed)
PARITY = [
    ("e-opt", "rigid", opts("local_bestN", **FLOW_OPEN), refine(e=True, rigid_flow_thre=0.5), ()),
    ("e-rigid", "rigid", opts("local_bestN", **FLOW_OPEN), refine(e=True, score="rigid_flow", rigid_flow_thre=0.5), ()),
    ("e_scale-opt", "rigid", opts("local_bestN", **FLOW_OPEN), refine(e=True, s=True, rigid_flow_thre=0.5), ()),
    ("e_scale-rigid-tunnel", "tunnel", opts("local_bestN"), refine(e=True, s=True, score="rigid_flow"), ()),
    ("pnp-rigid", "rigid", opts("local_bestN", tracking_method="PnP"), refine(p=True, score="rigid_flow", rigid_flow_thre=0.5), ()),
    ("pnp-opt", "rigid", opts("bestN", tracking_method="PnP"), refine(p=True, rigid_flow_thre=0.5), ()),
    ("minus_one-rigid", "rigid", opts("local_bestN", **FLOW_OPEN), refine(e=True, s=True, p=True, score="rigid_flow", rigid_flow_thre=0.5), (0, 1)),
    ("minus_one-opt", "rigid", opts("local_bestN", **FLOW_OPEN), refine(e=True, p=True, rigid_flow_thre=0.5), (0, 2)),
    ("e_scale-sampled", "rigid", opts("sampled", **FLOW_OPEN), refine(e=True, s=True, rigid_flow_thre=0.5), ()),
    ("abs_diff-e_scale", "rigid", opts("local_bestN", scale_method="abs_diff", **FLOW_OPEN), refine(e=True, s=True, rigid_flow_thre=0.5), ()),
]
# a flow gate nothing passes: E is rejected in pass one, so nothing refines and the plain PnP fallback runs with 5 repeats
REJECTED_FIRST = ("rejected-first", "rigid", opts("local_bestN", validity="flow", validity_thre=1e3), refine(e=True, s=True), ())
# GRIC on the tunnel with thresholds that leave 10 or fewer kp_depth keypoints: the second pass returns t = 0 (E_tracker.py:196)
REJECTED_SECOND = ("rejected-second", "tunnel", opts("local_bestN"), refine(e=True, s=True, p=True, optical_flow_thre=5e-6), ())
# the same scene with hundreds of kp_depth keypoints on which GRIC prefers the homography: rejected by the validity rule itself
REJECTED_SECOND_GRIC = ("rejected-second-gric", "tunnel", opts("local_bestN"), refine(e=True, s=True, p=True, score="rigid_flow",
                                                                                     rigid_flow_thre=0.01), ())
# scale -1 in pass one, refinement on [R | 0]; with scale_iterative_kp the second scale decides: pair 1 has the real depth again
MINUS_ONE_SCALE = ("minus-one-scale", "rigid", opts("local_bestN", **FLOW_OPEN), refine(e=True, s=True, rigid_flow_thre=0.5), (0,))
EMPTY = ("empty", "rigid", opts("local_bestN", **FLOW_OPEN), refine(e=True, rigid_flow_thre=1e-6), ())
EMPTY_PNP = ("empty-pnp", "rigid", opts("local_bestN", tracking_method="PnP"), refine(p=True, rigid_flow_thre=1e-6), ())


def depth_plan(sc, zero_pairs=()):
    """per pair (processed depth of the current frame, its raw float32 depth); the raw map stays the scene's where the
    processed one is zeroed"""
    raw = sc["depth_cur"].astype(np.float32)
    return [(np.zeros_like(sc["depth_cur"]) if f in zero_pairs else sc["depth_cur"], raw) for f in range(3)]


_chains = {}


def chain(case, n_pairs=3):
    """the oracle's pairs of a case, once: [(record, RandomState after)]; a pair that raises ends like any other (the depths
    roll over, the RandomState stays where the raise left it)"""
    key, name, o, ro, zero = case
    if key not in _chains:
        sc = scene_inputs(name)
        plan = depth_plan(sc, zero)
        np.random.seed(4869)
        depth_ref, raw_ref = sc["depth_ref"], sc["depth_ref"].astype(np.float32)
        out = []
        for f in range(n_pairs):
            depth_cur, raw_cur = plan[f]
            r = RO.solve_pair(o, ro, sc["flow"], sc["diff"], depth_cur, depth_ref, raw_ref, sc["K"])
            out.append((r, np.random.get_state()))
            depth_ref, raw_ref = depth_cur, raw_cur
        _chains[key] = out
    return _chains[key]


def gpu_case_pnp_poses():
    """(R, t) of every PnP first pass a GPU case refines from"""
    out = []
    for case in PARITY + [REJECTED_SECOND, REJECTED_SECOND_GRIC, MINUS_ONE_SCALE, EMPTY_PNP]:
        out += [(r["pnp1"]["R"], r["pnp1"]["t"]) for r, _ in chain(case) if r["pnp1"] is not None]
    return out
