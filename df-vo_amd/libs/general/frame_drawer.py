"""The dense panels of the reference's FrameDrawer (/root/reference/libs/general/frame_drawer.py:410-512) on the device.

`DenseMixin` holds the four methods that colour whole maps -- draw_depth, draw_flow, draw_flow_consistency,
draw_rigid_flow_consistency -- with the reference's signatures and guards, over the dfvo_vis_* entry points
(include/dfvo_hip.h, csrc/vis.hip): Middlebury wheel, matplotlib magma / jet, cv2.resize into the cell, with the reference's
arithmetic.  Each writes its cell into self.data[item], the view of the host window the rest of the drawer (trajectory,
matches, imshow: the reference's own code, see overlay.py) keeps drawing on.

Arrays that are still the frame session's (generation token + whole contents, the test kp_selection applies) are not
uploaded: the panels of a generation are drawn from the session's device buffers, all in one launch at the first dense call
of the frame, and the later calls fetch their cell.  Anything else is uploaded and drawn by itself.

`DensePanels(cfg)` is the mixin with the window and the layout of its own, for hosts without the reference checkout."""
import ctypes as C

import numpy as np

from ... import capi
from ..tracker import _ctx

CELLS = {"depth": 0, "flow1": 1, "flow2": 2, "rigid_flow_diff": 2, "warp_diff": 2, "opt_flow_diff": 3}
_SESSION_BUFFER = {"flow1": "fwd", "flow2": "bwd", "opt_flow_diff": "diff"}
MAP_VALUE, MAP_DISPARITY = 0, 1
MAGMA, JET = 0, 1


def _absent(d, key):
    """`d.get(key, -1) is -1` of the reference"""
    v = d.get(key, -1)
    return isinstance(v, int) and not isinstance(v, bool) and v == -1


def _float_map(a, what):
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        raise TypeError("%s: float32 or float64 expected, got %s" % (what, a.dtype))
    return np.ascontiguousarray(a)


class DenseMixin:
    """needs self.h, self.w (window), self.data / self.display (FrameDrawer.initialize_drawer)"""
    _vis_handle = None

    # -- device drawer ---------------------------------------------------------------------------------------------------
    def _vis(self):
        if self._vis_handle is None:
            capi.require_gpu()
            h = C.c_void_p()
            capi.check(capi.lib().dfvo_vis_create(int(self.h), int(self.w), C.byref(h)))
            self._vis_handle = h
            self._vis_lib = capi.lib()
            self._on_cell = {}       # cell id -> what the device canvas holds there (None: unknown / blank)
            self._tmp = {}
            self.stats = {"resident": 0, "uploaded": 0, "session_launches": 0, "blanked": 0}
            rect = (C.c_int * 4)()
            for item, cell in CELLS.items():
                capi.check(self._vis_lib.dfvo_vis_cell_rect(h, cell, rect))
                if item in self.data and self.data[item].shape[:2] != (rect[2] - rect[0], rect[3] - rect[1]):
                    raise ValueError("drawer layout: cell '%s' is %s, the device drawer has %s" % (
                        item, self.data[item].shape[:2], (rect[2] - rect[0], rect[3] - rect[1])))
        return self._vis_handle

    def close(self):
        if self._vis_handle is not None:
            self._vis_lib.dfvo_vis_destroy(self._vis_handle)
            self._vis_handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    def vis_counters(self):
        out = (C.c_longlong * 8)()
        capi.check(self._vis_lib.dfvo_vis_counters(self._vis(), out))
        return dict(zip(("panels_resident", "panels_uploaded", "launches", "selects", "cleared", "bytes_up", "bytes_down"), out))

    def vis_device_ms(self):
        ms = C.c_float()
        capi.check(self._vis_lib.dfvo_vis_device_ms(self._vis(), C.byref(ms)))
        return float(ms.value)

    def _fetch(self, item):
        v = self._vis()
        shape = self.data[item].shape
        tmp = self._tmp.get(shape)
        if tmp is None:
            tmp = self._tmp[shape] = np.empty(shape, np.uint8)
        capi.check(self._vis_lib.dfvo_vis_fetch(v, CELLS[item], capi.as_ptr(tmp)))
        self.data[item][...] = tmp

    def _blank(self, item):
        v = self._vis()
        h, w, c = self.data[item][...].shape
        self.data[item][...] = np.zeros((h, w, c))
        capi.check(self._vis_lib.dfvo_vis_clear_cell(v, CELLS[item]))
        self._on_cell[CELLS[item]] = None
        self.stats["blanked"] += 1

    # -- upload path -------------------------------------------------------------------------------------------------
    def _draw_map(self, item, a, kind, cmap, vmax):
        a = _float_map(a, item)
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
        if a.ndim != 2:
            raise ValueError("%s: a [H,W] map expected, got %s" % (item, a.shape))
        if kind == MAP_VALUE and vmax < 0:
            raise ValueError("minvalue must be less than or equal to maxvalue")  # matplotlib.colors.Normalize.__call__
        out = C.c_double()
        v = self._vis()
        self._on_cell[CELLS[item]] = None
        capi.check(self._vis_lib.dfvo_vis_draw_map(v, CELLS[item], capi.as_ptr(a), int(a.dtype == np.float64), a.shape[0], a.shape[1],
                                                   kind, cmap, float(vmax), C.byref(out)))
        self.stats["uploaded"] += 1
        if out.value < 0:
            raise ValueError("minvalue must be less than or equal to maxvalue")
        self._fetch(item)

    def _flow_writeback(self, flow_data, n_unknown):
        """flow_to_image's u[idxUnknow] = 0 / v[idxUnknow] = 0 act on views of the caller's array (flowlib.py:203-205)"""
        if n_unknown:
            with np.errstate(invalid="ignore"):
                unknown = (np.abs(flow_data[0]) > 1e7) | (np.abs(flow_data[1]) > 1e7)
            flow_data[:, unknown] = 0

    # -- resident path -----------------------------------------------------------------------------------------------
    def _session_of(self, arr, item):
        """the frame session, if `arr` still holds the contents of its buffer for `item` (token, then the whole contents) AND
        the device buffer behind it still holds that generation: the arrays are compared with the session's pinned host
        copies, the kernels read the nets' output buffers, which any other pass on the same net overwrites"""
        s = _ctx.session
        if s is None or not s.active or s.handle is None or s.gen < 0:
            return None
        ok = s.vis_is_depth(arr) if item == "depth" else s.vis_is_buffer(arr, _SESSION_BUFFER[item])
        return s if ok and (self._session_cells(s) >> CELLS[item]) & 1 else None

    def _session_cells(self, s):
        cells = C.c_int()
        capi.check(self._vis_lib.dfvo_vis_session_cells(s.handle, s.gen, C.byref(cells)))
        return int(cells.value)

    def _asked_for(self, item):
        """will FrameDrawer.main ask for `item`?  (the drawer is constructed with cfg.visualization, dfvo.py:93: its `flow`
        switches are main's conditions; a configuration without them asks for everything)"""
        if not self.display.get(item, False):
            return False
        key = {"flow1": "vis_forward_flow", "flow2": "vis_backward_flow", "opt_flow_diff": "vis_flow_diff"}[item]
        try:
            return bool(getattr(self.cfg.flow, key))
        except (AttributeError, KeyError):
            return True

    def forget_resident(self):
        """drop what is known about the device canvas: the next resident call launches again (benchmarks)"""
        self._vis()
        self._resident_gen = None
        self._on_cell = {}

    def _session_draw(self, s, item, params=None):
        """make the device canvas hold `item` of the session's generation; the first call of a generation draws, in the same
        launch, every other flow panel FrameDrawer.main will ask for and the session can serve.  Returns what the draw of
        `item` reported."""
        cell = CELLS[item]
        gen_key = (s.sid, s.gen)
        diff_default = 0.1 if (s.kp_cfg is not None and int(s.kp_cfg.score_method) == 1) else 1.0
        want = {item: params}
        if getattr(self, "_resident_gen", None) != gen_key:
            self._resident_gen = gen_key
            self._resident_info = {}
            servable = self._session_cells(s)
            for other in ("flow1", "flow2", "opt_flow_diff"):
                if (servable >> CELLS[other]) & 1 and self._asked_for(other):
                    want.setdefault(other, diff_default if other == "opt_flow_diff" else None)
        tag = (gen_key, item, params)
        if self._on_cell.get(cell) == tag:
            return self._resident_info[item]
        mask, diff_vmax, depth_kind, depth_vmax = 0, 1.0, MAP_VALUE, 0.0
        for it, par in want.items():
            mask |= 1 << CELLS[it]
            if it == "opt_flow_diff":
                diff_vmax = float(par)
            if it == "depth":
                depth_kind, depth_vmax = par
        unk = (C.c_longlong * 2)()
        dv = C.c_double()
        capi.check(self._vis_lib.dfvo_vis_draw_session(self._vis(), s.handle, s.gen, mask, diff_vmax, depth_kind, float(depth_vmax),
                                                       unk, C.byref(dv)))
        self.stats["session_launches"] += 1
        for it, par in want.items():
            self._on_cell[CELLS[it]] = (gen_key, it, par)
            self._resident_info[it] = {"flow1": int(unk[0]), "flow2": int(unk[1]), "depth": float(dv.value)}.get(it)
        return self._resident_info[item]

    # -- the four methods (frame_drawer.py:410-512) --------------------------------------------------------------------
    def draw_depth(self, vo):
        """Draw depth/disparity map"""
        self._vis()
        if self.display['depth']:
            if vo.cfg.visualization.depth.use_tracking_depth:
                if _absent(vo.cur_data, 'depth'):
                    return
                tmp_vis_depth = vo.cur_data['depth']
            else:
                if _absent(vo.cur_data, 'raw_depth'):
                    return
                tmp_vis_depth = vo.cur_data['raw_depth']
            mode = vo.cfg.visualization.depth.depth_disp
            if mode not in ('depth', 'disp'):
                return
            kind, vmax = (MAP_VALUE, float(vo.cfg.depth.max_depth)) if mode == 'depth' else (MAP_DISPARITY, 0.0)
            s = self._session_of(tmp_vis_depth, "depth")
            if s is not None and not (kind == MAP_VALUE and vmax < 0):
                used = self._session_draw(s, "depth", (kind, vmax))
                if used < 0:
                    raise ValueError("minvalue must be less than or equal to maxvalue")
                self.stats["resident"] += 1
                self._fetch("depth")
            else:
                self._draw_map("depth", tmp_vis_depth, kind, MAGMA, vmax)
        else:
            self._blank("depth")

    def draw_flow(self, flow_data, flow_name):
        """Draw optical flow map; flow_data [2xHxW]"""
        self._vis()
        if self.display[flow_name]:
            s = self._session_of(flow_data, flow_name) if flow_name in _SESSION_BUFFER else None
            if s is not None:
                n_unknown = self._session_draw(s, flow_name)
                self.stats["resident"] += 1
            else:
                a = np.asarray(flow_data)
                if a.dtype != np.float32 or a.ndim != 3 or a.shape[0] != 2:
                    raise TypeError("draw_flow: a float32 [2,H,W] flow expected, got %s %s" % (a.dtype, a.shape))
                a = np.ascontiguousarray(a)
                n = C.c_longlong()
                self._on_cell[CELLS[flow_name]] = None
                capi.check(self._vis_lib.dfvo_vis_draw_flow(self._vis(), CELLS[flow_name], capi.as_ptr(a), a.shape[1], a.shape[2],
                                                            C.byref(n)))
                self.stats["uploaded"] += 1
                n_unknown = int(n.value)
            self._fetch(flow_name)
            self._flow_writeback(flow_data, n_unknown)
        else:
            self._blank(flow_name)

    def _draw_jet(self, item, mask, vmax):
        s = self._session_of(mask, item) if item in _SESSION_BUFFER else None
        if s is not None and not vmax < 0:
            self._session_draw(s, item, float(vmax))
            self.stats["resident"] += 1
            self._fetch(item)
        else:
            self._draw_map(item, mask, MAP_VALUE, JET, float(vmax))

    def draw_flow_consistency(self, vo):
        """Draw forward-backward flow consistency map"""
        if _absent(vo.cur_data, 'fb_flow_mask'):
            return
        if vo.cfg.kp_selection.local_bestN.enable and vo.cfg.kp_selection.local_bestN.score_method == "flow_ratio":
            vmax = 0.1
        else:
            vmax = 1
        self._vis()
        self._draw_jet("opt_flow_diff", vo.cur_data['fb_flow_mask'], vmax)

    def draw_rigid_flow_consistency(self, vo):
        """Draw optical-rigid flow consistency map"""
        if _absent(vo.cur_data, 'rigid_flow_mask'):
            return
        vmax = vo.cfg.kp_selection.rigid_flow_kp.rigid_flow_thre
        self._vis()
        self._draw_jet("rigid_flow_diff", vo.cur_data['rigid_flow_mask'], vmax)


class DensePanels(DenseMixin):
    """the dense half of the drawer by itself: the window (uint8 BGR [window_h, window_w, 3]) and initialize_drawer's
    rectangles for the dense items, then the four methods.  `main(vo)` calls them in FrameDrawer.main's order and conditions."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.h, self.w = cfg.window_h, cfg.window_w
        self.img = np.zeros((self.h, self.w, 3), dtype=np.uint8)
        self.data, self.display = {}, {}
        h, w = self.h, self.w
        q = lambda e, k: int(e / 4 * k)  # noqa: E731
        for item, (r, c) in {"depth": (2, 2), "flow1": (2, 3), "flow2": (3, 2), "rigid_flow_diff": (3, 2), "opt_flow_diff": (3, 3),
                             "warp_diff": (3, 2)}.items():
            self.data[item] = self.img[q(h, r):q(h, r + 1), q(w, c):q(w, c + 1)]
            self.display[item] = True

    def main(self, vo):
        vis = vo.cfg.visualization
        if vis.depth.depth_disp is not None:
            self.draw_depth(vo)
        if vis.flow.vis_forward_flow and vo.tracking_stage >= 1 and vo.ref_data.get('flow') is not None:
            self.draw_flow(vo.ref_data['flow'], 'flow1')
        if vis.flow.vis_backward_flow and vo.tracking_stage >= 1 and vo.cur_data.get('flow') is not None:
            self.draw_flow(vo.cur_data['flow'], 'flow2')
        if vis.flow.vis_flow_diff and vo.cfg.deep_flow.forward_backward and vo.tracking_stage >= 1:
            self.draw_flow_consistency(vo)
        if vis.flow.vis_rigid_diff and vo.tracking_stage >= 1:
            self.draw_rigid_flow_consistency(vo)
        return vo
