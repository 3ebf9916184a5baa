"""CPU: pipeline.options_from_cfg -- the reference's configuration object as the override dict of TrackingPipeline.
The configurations are default_cfg.default_configuration(...) edited the way each shipped ablation file edits
default_configuration.yml (options/examples/ablation_*.yml; the values are written out here), plus every key the fused
pipeline does not run, which must be refused by name.  Neither the GPU nor the shared library is touched."""
import importlib

import pytest


@pytest.fixture(scope="module")
def pmod():
    import __graft_entry__ as g
    g.dfvo_amd()
    return importlib.import_module("df-vo_amd.pipeline")


def default_cfg():
    import __graft_entry__ as g
    g.dfvo_amd()
    dc = importlib.import_module("df-vo_amd.default_cfg")
    return dc.default_configuration(376, 1241, "network-default.pytorch", "mono_640x192")


def best_n(c):  # ablation_correspondences_best_n.yml
    c.kp_selection.local_bestN.enable = False
    c.kp_selection.bestN.enable = True
    c.kp_selection.bestN.num_bestN = 2000


def uniform(c):  # ablation_correspondences_uniform.yml
    c.kp_selection.local_bestN.enable = False
    c.kp_selection.sampled_kp.enable = True
    c.kp_selection.sampled_kp.num_kp = 2000
    c.e_tracker.kp_src = "kp_list"
    c.scale_recovery.kp_src = "kp_list"
    c.pnp_tracker.kp_src = "kp_list"


def model_sel_flow(c):  # ablation_model_sel_flow.yml
    c.e_tracker.validity.method = "flow"
    c.e_tracker.validity.thre = 5


def tracker_pnp(c):  # ablation_tracker_pnp.yml
    c.tracking_method = "PnP"


def test_default_configuration_maps_to_no_overrides(pmod):
    assert pmod.options_from_cfg(default_cfg()) == {}
    o = dict(pmod.DEFAULTS)
    o.update(pmod.OPTION_DEFAULTS)
    f = pmod.check_options(o)
    assert f == dict(kp_source=0, kp_score_method=0, kp_sampled_num=2000, flow_crop=[0.0, 1.0, 0.0, 1.0], validity_method=0,
                     validity_thre=0.0, scale_method=0, tracking_method=0)


@pytest.mark.parametrize("edit,want", [
    (best_n, {"kp_source": "bestN"}),
    (uniform, {"kp_source": "sampled"}),
    (model_sel_flow, {"validity": "flow", "validity_thre": 5}),
    (tracker_pnp, {"tracking_method": "PnP"}),
], ids=["best_n", "uniform", "model_sel_flow", "tracker_pnp"])
def test_shipped_ablations(pmod, edit, want):
    c = default_cfg()
    edit(c)
    assert pmod.options_from_cfg(c) == want


def test_values_travel(pmod):
    """non-default numbers of the keys the pipeline reads end up under the pipeline's own names"""
    c = default_cfg()
    best_n(c)
    c.kp_selection.bestN.num_bestN = 777
    c.seed = 7
    c.pnp_tracker.ransac.iter = 50
    c.scale_recovery.ransac.method = "abs_diff"
    assert pmod.options_from_cfg(c) == {"kp_source": "bestN", "kp_num_bestN": 777, "seed": 7, "pnp_iters": 50,
                                        "scale_method": "abs_diff"}
    c = default_cfg()
    uniform(c)
    c.kp_selection.sampled_kp.num_kp = 1999
    c.crop.flow_crop = [[0.1, 0.9], [0.05, 0.95]]
    assert pmod.options_from_cfg(c) == {"kp_source": "sampled", "kp_sampled_num": 1999, "flow_crop": ((0.1, 0.9), (0.05, 0.95))}
    c = default_cfg()
    c.kp_selection.local_bestN.score_method = "flow_ratio"
    c.kp_selection.local_bestN.thre = 0.05
    c.e_tracker.validity.method = "homo_ratio"
    c.e_tracker.validity.thre = 0.5
    assert pmod.options_from_cfg(c) == {"kp_score_method": "flow_ratio", "kp_thre": 0.05, "validity": "homo_ratio",
                                        "validity_thre": 0.5}


def _set(path, value):
    def edit(c):
        node = c
        keys = path.split(".")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = value
    return edit


@pytest.mark.parametrize("path,value", [
    ("e_tracker.iterative_kp.enable", True), ("scale_recovery.iterative_kp.enable", True),
    ("pnp_tracker.iterative_kp.enable", True), ("kp_selection.rigid_flow_kp.enable", True),
    ("kp_selection.depth_consistency.enable", True), ("deep_pose.enable", True), ("online_finetune.enable", True),
    ("e_tracker.kp_src", "kp_depth"), ("scale_recovery.kp_src", "kp_depth"), ("pnp_tracker.kp_src", "kp_depth")])
def test_unsupported_keys_are_refused_by_name(pmod, path, value):
    c = default_cfg()
    _set(path, value)(c)
    with pytest.raises(NotImplementedError) as e:
        pmod.options_from_cfg(c)
    assert path in str(e.value), str(e.value)


def test_mixed_kp_src_is_refused(pmod):
    c = default_cfg()
    uniform(c)
    c.scale_recovery.kp_src = "kp_best"  # E-tracker and PnP on the uniform samples, the scale on kp_best
    with pytest.raises(NotImplementedError, match="kp_src"):
        pmod.options_from_cfg(c)
    c = default_cfg()
    uniform(c)
    c.kp_selection.sampled_kp.enable = False  # every tracker reads kp_list, which nothing produces
    with pytest.raises(NotImplementedError, match="kp_src"):
        pmod.options_from_cfg(c)
    c = default_cfg()
    c.kp_selection.local_bestN.enable = False  # kp_best without local_bestN or bestN
    with pytest.raises(NotImplementedError, match="kp_src"):
        pmod.options_from_cfg(c)


@pytest.mark.parametrize("key,value", [("kp_source", "best_n"), ("kp_score_method", "ratio"), ("validity", "gric"),
                                       ("scale_method", "simple"), ("tracking_method", "pnp"), ("kp_sampled_num", 0),
                                       ("kp_sampled_num", 2.5), ("flow_crop", [[0.5, 0.5], [0, 1]]), ("flow_crop", [0, 1, 0, 1]),
                                       ("validity_thre", float("nan"))])
def test_bad_option_values_raise_value_error(pmod, key, value):
    """raised before the constructor touches the device or the library, so this runs anywhere"""
    o = {key: value}
    if key == "validity_thre":
        o["validity"] = "flow"
    with pytest.raises(ValueError, match=key):
        pmod.TrackingPipeline(128, 416, 64, 96, [[100.0, 0, 208], [0, 100.0, 64], [0, 0, 1]], {}, {}, **o)
    with pytest.raises(ValueError, match="validity_thre"):
        pmod.TrackingPipeline(128, 416, 64, 96, [[100.0, 0, 208], [0, 100.0, 64], [0, 0, 1]], {}, {}, validity="flow")
