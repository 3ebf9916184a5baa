"""DepthConsistency with the reference's surface (/root/reference/libs/matching/depth_consistency.py:18-163) over
dfvo_depth_consistency: the reference's Backprojection / Reprojection layers, grid_sample and the depth_ratio difference run
as one launch."""
import numpy as np

from ... import capi


class DepthConsistency:
    def __init__(self, cfg, cam_intrinsics):
        self.cfg = cfg
        self.cam_intrinsics = cam_intrinsics

    def prepare_depth_consistency_data(self, cur_data, ref_data):
        """depth_consistency.py:31-67, as float32 host arrays: 'K' / 'inv_K' [1, 4, 4], ('depth', id) [1, 1, H, W] of both
        frames, ('pose_T', cur_id, ref_id) [1, 4, 4] (ref_data['deep_pose']: current -> reference), 'cur_id', 'ref_id'"""
        data = {}
        for key, mat in (('inv_K', self.cam_intrinsics.inv_mat), ('K', self.cam_intrinsics.mat)):
            m = np.eye(4)
            m[:3, :3] = mat
            data[key] = m[None].astype(np.float32)
        data['cur_id'], data['ref_id'] = cur_data['id'], ref_data['id']
        data[('depth', cur_data['id'])] = np.asarray(cur_data['raw_depth'], dtype=np.float32)[None, None]
        data[('depth', ref_data['id'])] = np.asarray(ref_data['raw_depth'], dtype=np.float32)[None, None]
        data[('pose_T', cur_data['id'], ref_data['id'])] = np.asarray(ref_data['deep_pose'], dtype=np.float32)[None]
        return data

    def _depth_diff(self, inputs):
        cur = np.ascontiguousarray(inputs[('depth', inputs['cur_id'])][0, 0], dtype=np.float32)
        ref = np.ascontiguousarray(inputs[('depth', inputs['ref_id'])][0, 0], dtype=np.float32)
        assert cur.shape == ref.shape and cur.ndim == 2
        K = np.ascontiguousarray(inputs['K'][0, :3, :3], dtype=np.float32)
        Kinv = np.ascontiguousarray(inputs['inv_K'][0, :3, :3], dtype=np.float32)
        T = np.ascontiguousarray(inputs[('pose_T', inputs['cur_id'], inputs['ref_id'])][0], dtype=np.float32)
        out = np.zeros(cur.shape, np.float32)
        capi.check(capi.lib().dfvo_depth_consistency_host(capi.as_ptr(cur), capi.as_ptr(ref), cur.shape[0], cur.shape[1], capi.as_ptr(K),
                                                          capi.as_ptr(Kinv), capi.as_ptr(T), capi.as_ptr(out)))
        return out

    def warp_and_reproj_depth(self, inputs):
        """depth_consistency.py:69-116.  The warped and the reprojected depth are intermediate values of the one device
        launch and never leave it: what this returns carries the finished map, which compute_depth_diff hands on."""
        return {('depth_diff', inputs['cur_id'], inputs['ref_id']): self._depth_diff(inputs)}

    def compute_depth_diff(self, depth_data, inputs):
        """depth_consistency.py:118-151, method depth_ratio: {('depth_diff', cur_id, ref_id): float32 [H, W]}"""
        key = ('depth_diff', inputs['cur_id'], inputs['ref_id'])
        return {key: depth_data[key]}

    def compute(self, cur_data, ref_data):
        """depth_consistency.py:153-163: ref_data['depth_diff'], float32 [H, W]"""
        inputs = self.prepare_depth_consistency_data(cur_data, ref_data)
        depth_outputs = self.warp_and_reproj_depth(inputs)
        depth_consistency = self.compute_depth_diff(depth_outputs, inputs)
        ref_data['depth_diff'] = depth_consistency[('depth_diff', cur_data['id'], ref_data['id'])]
