#!/usr/bin/env python3
"""Fixture for fb_bev_amd/occ_metrics.py: run the REAL reference Metric_mIoU (mmdet3d/datasets/occ_metrics.py, loaded by path) on three
synthetic frames of the grid it hard-codes for its range ring (200 x 200 columns, here 2 cells deep) and record, for three rings
(min_d, max_d), the accumulated confusion matrix and the count_miou() dict.

termcolor is absent here and gets a stand-in module (the reference only colours a string with it); sklearn, tqdm and numpy are the
installed ones.  The generator also runs the reference's 1-D call form (pred[mask_camera], nuscenes_dataset.py:746) and checks that it
leaves the same matrix, so the test may hold both forms against one record.

Run in the build container:  python tests/golden/make_golden_occ_metric.py
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

RINGS = ((-1, 100), (0, 30), (10, 40))
GRID = (200, 200, 2)
N = 18


def frames():
    """labels: mostly free (17), 255 where unlabelled; predictions: the label with errors; mask_camera: two thirds visible"""
    rng = np.random.default_rng(20231)
    out = []
    for _ in range(3):
        gt = np.where(rng.random(GRID) < 0.75, N - 1, rng.integers(0, N, GRID)).astype(np.uint8)
        pred = np.where(rng.random(GRID) < 0.8, gt, rng.integers(0, N, GRID)).astype(np.uint8)
        gt[rng.random(GRID) < 0.03] = 255
        out.append((pred, gt, rng.random(GRID) < 0.66))
    return out


def main():
    MG._mod('termcolor', colored=lambda s, *a, **k: s)
    ref = MG.load_ref('ref_occ_metrics', 'mmdet3d/datasets/occ_metrics.py')
    data = frames()
    rec = {}
    for i, (pred, gt, cam) in enumerate(data):
        rec[f'pred_{i}'], rec[f'gt_{i}'], rec[f'mask_camera_{i}'] = pred, gt, cam
    for r, (min_d, max_d) in enumerate(RINGS):
        m = ref.Metric_mIoU(num_classes=N, use_image_mask=True, min_d=min_d, max_d=max_d)
        m1 = ref.Metric_mIoU(num_classes=N, use_image_mask=True, min_d=min_d, max_d=max_d)
        for pred, gt, cam in data:
            m.add_batch(pred, gt, None, cam)
            m1.add_batch(pred[cam], gt, None, cam)
        assert np.array_equal(m.hist, m1.hist)
        assert np.array_equal(m.hist, np.round(m.hist)) and m.hist.max() < 2 ** 53
        with contextlib.redirect_stdout(io.StringIO()):
            res = m.count_miou()
        rec[f'hist_{r}'] = m.hist.astype(np.int64)
        rec[f'miou_keys_{r}'] = np.array(list(res.keys()))
        rec[f'miou_values_{r}'] = np.array([float(v) for v in res.values()], dtype=np.float64)
        print(f'ring {(min_d, max_d)}: counted {int(m.hist.sum())}, mIoU {res["Overall"]}')
    rec['rings'] = np.array(RINGS, dtype=np.float64)
    path = os.path.join(MG.OUT, 'occ_metric_miou.npz')
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
