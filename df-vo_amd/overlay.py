"""Drop-in overlay: makes the reference's unchanged `apis/run.py` / `libs/dfvo.py` use the MI355X
classes.  `install()` registers this package's mirrors under the reference's module names, so that

    from libs.deep_models.deep_models import DeepModel          (libs/dfvo.py:24)
    from libs.matching.keypoint_sampler import KeypointSampler  (libs/dfvo.py:27)
    from libs.tracker import EssTracker, PnpTracker             (libs/dfvo.py:28)

resolve to df-vo_amd.libs.*, while every other `libs.*` module (dfvo, datasets, general, geometry, ...)
still comes from the reference checkout on sys.path.  See INTEGRATION.md.

The drawer is the one class that is overlaid in part:

    from libs.general.frame_drawer import FrameDrawer           (libs/dfvo.py:24)

resolves to a stand-in module whose attributes are looked up lazily.  On first use it loads the reference's own
frame_drawer.py (found on the `libs.general` package path) under a private module name and hands out `FrameDrawer` as a
subclass of the reference's class in which only the four dense panels -- draw_depth, draw_flow, draw_flow_consistency,
draw_rigid_flow_consistency -- come from df-vo_amd.libs.general.frame_drawer; every other attribute of the module
(draw_match_temporal, draw_match_side, ...) and of the class (draw_traj, main, interface, ...) is the reference's.  cv2 is
imported when the reference's file is, not before.
"""
import importlib
import importlib.util
import os
import sys
import types

PKG = __name__.rsplit(".", 1)[0]

_MAP = {
    "libs.deep_models.deep_models": ".libs.deep_models.deep_models",
    "libs.matching.keypoint_sampler": ".libs.matching.keypoint_sampler",
    "libs.matching.depth_consistency": ".libs.matching.depth_consistency",
    "libs.tracker": ".libs.tracker",
    "libs.tracker.E_tracker": ".libs.tracker.E_tracker",
    "libs.tracker.pnp_tracker": ".libs.tracker.pnp_tracker",
}


REF_DRAWER = "libs.general.frame_drawer"
_PRIVATE_DRAWER = "libs.general._dfvo_reference_frame_drawer"


def _drawer_module():
    mod = types.ModuleType(REF_DRAWER)
    mod.__doc__ = "stand-in for the reference's libs/general/frame_drawer.py: its own module, FrameDrawer's dense panels on the device"
    state = {}

    def resolve():
        if not state:
            pkg = importlib.import_module("libs.general")  # the reference's package, from the checkout on sys.path
            path = next((os.path.join(d, "frame_drawer.py") for d in pkg.__path__ if os.path.exists(os.path.join(d, "frame_drawer.py"))), None)
            if path is None:
                raise ImportError("libs/general/frame_drawer.py not found on the libs.general package path %s" % list(pkg.__path__))
            spec = importlib.util.spec_from_file_location(_PRIVATE_DRAWER, path)
            ref = importlib.util.module_from_spec(spec)
            sys.modules[_PRIVATE_DRAWER] = ref
            spec.loader.exec_module(ref)
            ours = importlib.import_module(".libs.general.frame_drawer", PKG)
            state["ref"] = ref
            state["cls"] = type("FrameDrawer", (ours.DenseMixin, ref.FrameDrawer), {"__module__": REF_DRAWER, "__doc__": ref.FrameDrawer.__doc__})
        return state

    def module_getattr(name):
        if name.startswith("__") and name.endswith("__"):
            raise AttributeError(name)
        st = resolve()
        return st["cls"] if name == "FrameDrawer" else getattr(st["ref"], name)

    mod.__getattr__ = module_getattr
    return mod


def install():
    for ref_name, ours in _MAP.items():
        sys.modules[ref_name] = importlib.import_module(ours, PKG)
    sys.modules[REF_DRAWER] = _drawer_module()
    return sorted(_MAP)
