#!/usr/bin/env python3
"""Fixture for the LiDAR -> multi-view depth step: run the REAL PointToMultiViewDepth.__call__
(mmdet3d/datasets/pipelines/loading.py:876-966) on the exact-layer inputs of tests/points_depth_cases.py
(ds2_ties, edges, stride5_batch, keyties), one sample at a time as the pipeline does.

The module file is loaded by path with inert stand-ins for mmcv / mmdet / mmdet3d.core / PIL / cv2 / torchvision.  One stand-in
carries arithmetic: `pyquaternion` is not installed, so `Quaternion(q).rotation_matrix` is served by a restatement of its
published definition (normalise, then the product of the left and the conjugate right multiplication matrices) -- the fixture pins
everything EXCEPT that class.  The info dicts hold dyadic unit quaternions (tests/points_depth_cases.exact_info), for which any
correct quaternion -> matrix formula is exact.

lidar2img is a local of __call__: it is recorded through the `points` object the class multiplies it with (`points.tensor[:, :3]
.matmul(lidar2img[:3, :3].T) + lidar2img[:3, 3].unsqueeze(0)`), whose stand-in logs the two operands and returns torch's own result.

Writes tests/golden/points_depth_ref.npz: per case the points of every sample, post_rots, post_trans, lidar2img (B, N, 3, 4) as the
reference computed it, and the maps (keyties: rows 187-191 only, the others are asserted to be zero).

Run in the build container:  python tests/golden/make_golden_points_depth.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import make_golden as MG  # noqa: E402
import points_depth_cases as PC  # noqa: E402


class Quaternion:
    """stand-in for pyquaternion.Quaternion: (w, x, y, z) -> rotation_matrix of the normalised quaternion"""

    def __init__(self, q):
        self.q = np.array(q, dtype=np.float64)

    @property
    def rotation_matrix(self):
        q = self.q
        n = np.linalg.norm(q)
        if abs(1.0 - n) >= 1e-14 and n > 0:
            q = q / n
        w, x, y, z = q
        left = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
        right_conj = np.array([[w, x, y, z], [-x, w, -z, y], [-y, z, w, -x], [-z, -y, x, w]])
        return np.dot(left, right_conj)[1:][:, 1:]


class _Sum:
    def __init__(self, t, log):
        self.t, self.log = t, log

    def __add__(self, other):
        self.log.append(other.clone())
        return self.t + other


class _Rows:
    def __init__(self, t, log):
        self.t, self.log = t, log

    def __getitem__(self, idx):
        return _Rows(self.t[idx], self.log)

    def matmul(self, other):
        self.log.append(other.clone())
        return _Sum(self.t.matmul(other), self.log)


class _Points:
    def __init__(self, t, log):
        self.tensor = _Rows(t, log)


def main():
    MG.install_stubs()

    class _Base(object):
        pass
    MG._mod('PIL', Image=None)
    MG._mod('pyquaternion', Quaternion=Quaternion)
    MG._mod('mmdet3d.core'); MG._mod('mmdet3d.core.points', BasePoints=None, get_points_type=None)
    MG._mod('mmdet3d.core.bbox', LiDARInstance3DBoxes=None)
    MG._mod('mmdet.datasets'); MG._mod('mmdet.datasets.pipelines', LoadAnnotations=_Base, LoadImageFromFile=_Base)
    MG._mod('mmdet3d.datasets'); MG._mod('mmdet3d.datasets.builder', PIPELINES=MG._Registry())
    pk = MG._mod('mmdet3d.datasets.pipelines')
    pk.__path__ = []
    MG._mod('torchvision'); MG._mod('torchvision.transforms'); MG._mod('torchvision.transforms.functional', rotate=None)
    ref = MG.load_ref('mmdet3d.datasets.pipelines.loading', 'mmdet3d/datasets/pipelines/loading.py')
    out = {}
    for name in PC.FIXTURE_CASES:
        case = PC.by_name(name)
        pts_list, M, R, T = PC.exact_inputs(case)
        B, N, h, w = PC.dims(case)
        step = ref.PointToMultiViewDepth(grid_config=dict(depth=list(case['cfg'])), downsample=case['ds'])
        maps, mats = [], []
        for b in range(B):
            curr, names, intrins = PC.exact_info(case, b)
            log = []
            imgs = torch.zeros(N, 3, case['H'], case['W'])
            results = dict(points=_Points(torch.from_numpy(pts_list[b]), log), curr=curr, cam_names=names,
                           img_inputs=(imgs, None, None, intrins, torch.from_numpy(R[b]), torch.from_numpy(T[b]), None))
            maps.append(step(results)['gt_depth'].numpy())
            assert len(log) == 2 * N
            mats.append(np.stack([np.concatenate([log[2 * n].T.numpy(), log[2 * n + 1].numpy().reshape(3, 1)], 1) for n in range(N)]))
            out[f'{name}.points{b}'] = pts_list[b]
        maps, mats = np.stack(maps), np.stack(mats)
        assert maps.shape == (B, N, h, w) and maps.dtype == np.float32 and mats.shape == (B, N, 3, 4)
        if name == 'keyties':
            r0, r1 = PC.KEYTIES_ROWS
            assert not maps[:, :, :r0].any() and not maps[:, :, r1:].any()
            maps = maps[:, :, r0:r1]
        out[f'{name}.map'], out[f'{name}.lidar2img'] = maps, mats.astype(np.float32)
        out[f'{name}.post_rots'], out[f'{name}.post_trans'] = R, T
        print(name, 'non-empty pixels', int((maps != 0).sum()), 'lidar2img equals the exact layer\'s', np.array_equal(mats, M[:, :, :3]))
    path = os.path.join(MG.OUT, 'points_depth_ref.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
