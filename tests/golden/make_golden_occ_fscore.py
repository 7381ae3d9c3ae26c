#!/usr/bin/env python3
"""Fixture for fb_bev_amd/occ_metrics.Metric_FScore: run the REAL reference Metric_FScore (mmdet3d/datasets/occ_metrics.py, loaded by
path; its KD-trees are scikit-learn's) on four synthetic frames of the 200 x 200 x 16 grid and record, for three threshold pairs, the
running totals after every frame, the count_fscore() dict, the sizes of both point sets per frame, and the constructor's signature.

The frames are structured blocks in free space (the file compresses to a fraction of its 10 MB):
  0  labels = blocks, prediction = the blocks moved, grown, shrunk or dropped, plus a few stray voxels
  1  an empty prediction (the reference's `prediction.shape[0] == 0` branch)
  2  prediction = the labels shifted by one cell along x: every nearest pair is exactly one cell apart, the case that float64
     rounding decides at threshold 0.4
  3  as 0 with other blocks, ids above 17 and unlabelled (255) voxels among them
mask_camera hides a third of the columns, in 5 x 5 patches.  Every frame is handed to the reference as a COPY: its add_batch writes
255 into the arrays it is given.  The generator also runs the reference's 1-D call form (pred[mask_camera]) and checks that it leaves
the same totals, so the test may hold both forms against one record.

termcolor is absent here and gets a stand-in module (the reference only colours a string with it).

Run in the build container:  python tests/golden/make_golden_occ_fscore.py
"""
import contextlib
import inspect
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

PAIRS = ((0.4, 0.4), (0.6, 0.6), (0.4, 0.8))          # (threshold_acc, threshold_complete)
GRID = (200, 200, 16)
FREE = 17


def _blocks(rng, n, ids):
    """n boxes (x0, x1, y0, y1, z0, z1, id), some touching the faces of the grid"""
    out = []
    for k in range(n):
        sx, sy, sz = rng.integers(1, 12), rng.integers(1, 12), rng.integers(1, 6)
        x0, y0, z0 = rng.integers(0, GRID[0] - sx + 1), rng.integers(0, GRID[1] - sy + 1), rng.integers(0, GRID[2] - sz + 1)
        if k % 7 == 0:
            x0 = 0 if k % 2 else GRID[0] - sx
        if k % 11 == 0:
            z0 = 0 if k % 2 else GRID[2] - sz
        out.append((x0, x0 + sx, y0, y0 + sy, z0, z0 + sz, int(ids[k % len(ids)])))
    return out


def _paint(blocks):
    vol = np.full(GRID, FREE, dtype=np.uint8)
    for x0, x1, y0, y1, z0, z1, c in blocks:
        vol[max(x0, 0):max(x1, 0), max(y0, 0):max(y1, 0), max(z0, 0):max(z1, 0)] = c
    return vol


def _mask(rng):
    coarse = rng.random((GRID[0] // 5, GRID[1] // 5)) < 0.66
    return np.repeat(np.repeat(coarse, 5, 0), 5, 1)[:, :, None].repeat(GRID[2], 2)


def frames():
    rng = np.random.default_rng(20240)
    out = []
    for f in range(4):
        ids = np.arange(0, 17) if f != 3 else np.array([0, 3, 18, 4, 200, 11, 255, 16])
        blocks = _blocks(rng, 120, ids)
        gt = _paint(blocks)
        if f == 1:
            pred = np.full(GRID, FREE, dtype=np.uint8)
        elif f == 2:
            pred = np.full(GRID, FREE, dtype=np.uint8)
            pred[1:] = gt[:-1]
        else:
            moved = []
            for k, (x0, x1, y0, y1, z0, z1, c) in enumerate(blocks):
                if k % 9 == 0:
                    continue                                          # missed
                d = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (2, 0, 0), (-1, 0, -1), (0, 3, 0)][k % 8]
                g = 1 if k % 5 == 0 else (-1 if k % 5 == 1 and x1 - x0 > 2 else 0)    # grown / shrunk along x
                moved.append((x0 + d[0], x1 + d[0] + g, y0 + d[1], y1 + d[1], z0 + d[2], z1 + d[2], c))
            pred = _paint(moved)
            stray = rng.random(GRID) < 0.0005
            pred[stray] = rng.integers(0, 17, int(stray.sum()))
        out.append((pred, gt, _mask(rng)))
    return out


def main():
    MG._mod('termcolor', colored=lambda s, *a, **k: s)
    ref = MG.load_ref('ref_occ_metrics', 'mmdet3d/datasets/occ_metrics.py')
    data = frames()
    rec = {}
    for i, (pred, gt, cam) in enumerate(data):
        rec[f'pred_{i}'], rec[f'gt_{i}'], rec[f'mask_camera_{i}'] = pred, gt, cam
    sig = inspect.signature(ref.Metric_FScore.__init__)
    params = [p for p in sig.parameters.values() if p.name != 'self']
    rec['ctor_names'] = np.array([p.name for p in params])
    rec['ctor_defaults'] = np.array([repr(p.default) for p in params])
    for r, (t_acc, t_cmpl) in enumerate(PAIRS):
        m = ref.Metric_FScore(threshold_acc=t_acc, threshold_complete=t_cmpl, use_image_mask=True)
        m1 = ref.Metric_FScore(threshold_acc=t_acc, threshold_complete=t_cmpl, use_image_mask=True)
        totals, sizes = [], []
        for pred, gt, cam in data:
            g, p = gt.copy(), pred.copy()
            m.add_batch(p, g, None, cam.copy())
            m1.add_batch(pred[cam], gt.copy(), None, cam.copy())
            assert (m.tot_acc, m.tot_cmpl, m.tot_f1_mean) == (m1.tot_acc, m1.tot_cmpl, m1.tot_f1_mean)
            totals.append((m.tot_acc, m.tot_cmpl, m.tot_f1_mean))
            sizes.append((len(m.voxel2points(g)), len(m.voxel2points(p))))       # g, p now hold 255 where the mask hides them
        with contextlib.redirect_stdout(io.StringIO()):
            res = m.count_fscore()
        assert list(res.keys()) == ['f-score']
        rec[f'totals_{r}'] = np.array(totals, dtype=np.float64)                   # (frames, 3): tot_acc, tot_cmpl, tot_f1_mean
        rec[f'fscore_{r}'] = np.float64(res['f-score'])
        rec[f'sizes_{r}'] = np.array(sizes, dtype=np.int64)                       # (frames, 2): ground truth, prediction
        print(f'thresholds {(t_acc, t_cmpl)}: sizes {sizes}, totals {totals[-1]}, f-score {res["f-score"]}')
    for i, (pred, gt, cam) in enumerate(data):                                    # the generator kept its own frames intact
        assert np.array_equal(rec[f'pred_{i}'], pred) and np.array_equal(rec[f'gt_{i}'], gt)
    assert rec['sizes_0'][1, 1] == 0 and rec['sizes_0'][1, 0] > 0                 # frame 1: the empty prediction
    rec['pairs'] = np.array(PAIRS, dtype=np.float64)
    rec['cnt'] = np.int64(len(data))
    path = os.path.join(MG.OUT, 'occ_fscore.npz')
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
