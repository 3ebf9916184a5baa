"""CPU: scale_recovery.method iterative in the fused pipeline's host layer -- pipeline.options_from_cfg on the edits of
options/examples/ablation_scale_iterative.yml (written out here), the scale_recovery.kp_src combinations it takes and refuses,
the value checks of TrackingPipeline's iterative keys (raised before the device or the library is touched), the multi-rank
refusal of sequence.run_sequence(s), and the oracle helper of the GPU test against oracle.tracker_np.scale_recovery_iterative."""
import importlib

import numpy as np
import pytest

from test_pipeline_options_cpu import default_cfg, uniform

K0 = [[100.0, 0, 208], [0, 100.0, 64], [0, 0, 1]]


@pytest.fixture(scope="module")
def pmod():
    import __graft_entry__ as g
    g.dfvo_amd()
    return importlib.import_module("df-vo_amd.pipeline")


def scale_iterative(c):  # ablation_scale_iterative.yml
    c.kp_selection.rigid_flow_kp.enable = True
    c.kp_selection.rigid_flow_kp.num_bestN = 2000
    c.kp_selection.rigid_flow_kp.num_row = 10
    c.kp_selection.rigid_flow_kp.num_col = 10
    c.kp_selection.rigid_flow_kp.score_method = "opt_flow"
    c.kp_selection.rigid_flow_kp.rigid_flow_thre = 5
    c.kp_selection.rigid_flow_kp.optical_flow_thre = 0.1
    c.scale_recovery.method = "iterative"


def test_the_shipped_ablation_maps_to_the_iterative_keys(pmod):
    c = default_cfg()
    scale_iterative(c)
    assert pmod.options_from_cfg(c) == {"scale_recovery": "iterative"}
    c.kp_selection.rigid_flow_kp.num_bestN = 1500
    c.kp_selection.rigid_flow_kp.num_row = 5
    c.kp_selection.rigid_flow_kp.rigid_flow_thre = 3
    c.kp_selection.rigid_flow_kp.optical_flow_thre = 0.2
    assert pmod.options_from_cfg(c) == {"scale_recovery": "iterative", "rigid_num_bestN": 1500, "rigid_num_row": 5,
                                        "rigid_flow_thre": 3, "optical_flow_thre": 0.2}
    assert pmod.options_from_cfg(default_cfg()) == {}
    assert not set(pmod.ITER_DEFAULTS) & set(pmod.OPTION_DEFAULTS), "the iterative keys stay out of capi.PipelineOpts' table"


def test_scale_kp_src_under_the_iterative_method(pmod):
    c = default_cfg()
    scale_iterative(c)
    c.scale_recovery.kp_src = "kp_depth"  # each round's scale from that round's rigid-flow keypoints
    assert pmod.options_from_cfg(c) == {"scale_recovery": "iterative", "iter_kp_src": "kp_depth"}
    c = default_cfg()
    scale_iterative(c)
    uniform(c)  # all three trackers on kp_list: the scale from the tracked (sampled) keypoints
    assert pmod.options_from_cfg(c) == {"scale_recovery": "iterative", "kp_source": "sampled"}
    c.scale_recovery.kp_src = "kp_depth"
    assert pmod.options_from_cfg(c) == {"scale_recovery": "iterative", "iter_kp_src": "kp_depth", "kp_source": "sampled"}
    c.scale_recovery.kp_src = "kp_best"  # neither kp_depth nor the trackers' source
    with pytest.raises(NotImplementedError, match="kp_src"):
        pmod.options_from_cfg(c)


@pytest.mark.parametrize("path,value", [("e_tracker.kp_src", "kp_depth"), ("pnp_tracker.kp_src", "kp_depth"),
                                        ("e_tracker.iterative_kp.enable", True), ("scale_recovery.iterative_kp.enable", True),
                                        ("pnp_tracker.iterative_kp.enable", True)])
def test_what_stays_refused_under_the_iterative_method(pmod, path, value):
    c = default_cfg()
    scale_iterative(c)
    node = c
    keys = path.split(".")
    for k in keys[:-1]:
        node = node[k]
    node[keys[-1]] = value
    with pytest.raises(NotImplementedError) as e:
        pmod.options_from_cfg(c)
    assert path in str(e.value), str(e.value)


def test_iterative_without_rigid_flow_kp_is_refused_by_that_key(pmod):
    c = default_cfg()
    c.scale_recovery.method = "iterative"  # (the reference dies with a KeyError in its first round)
    with pytest.raises(NotImplementedError) as e:
        pmod.options_from_cfg(c)
    assert "kp_selection.rigid_flow_kp.enable" in str(e.value)
    c.scale_recovery.method = "recursive"
    with pytest.raises(NotImplementedError, match="scale_recovery.method"):
        pmod.options_from_cfg(c)


@pytest.mark.parametrize("key,value", [("scale_recovery", "iter"), ("scale_recovery", True), ("iter_kp_src", "kp_list"),
                                       ("rigid_num_bestN", 0), ("rigid_num_bestN", 99), ("rigid_num_bestN", 2000.5),
                                       ("rigid_num_row", 0), ("rigid_num_row", "10"), ("rigid_num_col", -1), ("rigid_num_col", True),
                                       ("rigid_flow_thre", float("nan")), ("rigid_flow_thre", None), ("optical_flow_thre", float("inf")),
                                       ("optical_flow_thre", "0.1")])
def test_bad_iterative_values_raise_value_error(pmod, key, value):
    """raised before the constructor touches the device or the library, so this runs anywhere; with the method off as well"""
    for method in ("iterative", "simple"):
        o = {"scale_recovery": method}
        o[key] = value
        with pytest.raises(ValueError, match=key):
            pmod.TrackingPipeline(128, 416, 64, 96, K0, {}, {}, **o)


def test_more_than_one_rank_is_refused_naming_prev_scale():
    import __graft_entry__ as g
    g.dfvo_amd()
    smod = importlib.import_module("df-vo_amd.sequence")

    class Pipe:  # (refused before the pipeline is touched)
        iterative = True

    with pytest.raises(NotImplementedError, match="prev_scale"):
        smod.run_sequence(Pipe(), [], 10, world=2, rank=0)
    with pytest.raises(NotImplementedError, match="prev_scale"):
        smod.run_sequences(Pipe(), [("a", [], 10)], world=2, rank=1)


def test_oracle_helper_loop_is_the_oracles_loop():
    """tests/pipeline_iter_oracle.iterative_loop against oracle.tracker_np.scale_recovery_iterative on a committed scene: scale,
    rounds, keypoints, distance map and np.random afterwards -- for both keypoint sources, and from a carried scale"""
    from golden.make_golden import rigid_case
    from golden.make_golden_rigid_iter import unit_E_pose
    from oracle import tracker_np as T
    import pipeline_iter_oracle as IO
    c = rigid_case(60, 100, 2)
    E = unit_E_pose(c["T_ref_to_cur"])
    lb = T.local_bestN(c["flow"], c["diff"][..., None])
    best = (lb["kp1_best"][0], lb["kp2_best"][0])
    for src, prev in (("kp_depth", 0.0), ("kp_best", 0.0), ("kp_depth", 1.3)):
        kw = dict(kp_src=src, kp_best=best) if src == "kp_best" else {}
        np.random.seed(7)
        want = T.scale_recovery_iterative(c["flow"], c["diff"][..., None], c["raw_depth"], c["depth_cur"], E, c["K"], prev_scale=prev,
                                          score_method="opt_flow", **kw)
        want_rng = IO.rng_words()
        np.random.seed(7)
        rec = IO.iterative_loop(c["flow"], c["diff"].reshape(60, 100), c["raw_depth"], c["depth_cur"], E, c["K"], prev, src, best)
        assert rec["error"] is None and rec["n_iter"] == want["n_iter"] and rec["scale"] == want["scale"], (src, prev)
        assert np.array_equal(rec["ref_kp"], want["ref_kp"]) and np.array_equal(rec["cur_kp"], want["cur_kp"])
        assert np.array_equal(rec["mask"], want["rigid_flow_mask"]) and np.array_equal(IO.rng_words(), want_rng)
        assert len(rec["n_kp"]) == len(rec["scale_out"]) == rec["n_iter"] and rec["scale_in"][0] == prev
        assert rec["scale_in"][1:] == rec["scale_out"][:-1]
