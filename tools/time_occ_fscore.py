#!/usr/bin/env python3
"""Time the occupancy F-score of one 200 x 200 x 16 frame, for thresholds 0.4 and 0.6 and for a sparse (2 % occupied) and a dense (60 %)
frame:
  (a) device: Metric_FScore.add_batch on CUDA class maps -- one launch of fbbev_occ_fscore_counts plus the append of the counts --
              by HIP events, and the launch alone
  (b) host:   Metric_FScore.add_batch on the same frames as numpy arrays (shifted boolean arrays), by the wall clock
  (c) where scikit-learn is importable: the two KDTree builds and the two queries the reference's add_batch makes on the same point
      sets (leaf_size 10), by the wall clock; written out here, the reference is not read
The three sides are checked to count the same hits before anything is timed.  Writes p50 (p10 - p90) of the timed iterations in
microseconds to a .md.

    python tools/time_occ_fscore.py [--out profiles/r18_occ_fscore.md] [--iters 30] [--warmup 5]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fb_bev_amd import _capi  # noqa: E402
from fb_bev_amd.occ_metrics import Metric_FScore  # noqa: E402

GRID = (200, 200, 16)
FREE = 17


def pct(us):
    us = np.array(us)
    return tuple(float(np.percentile(us, q)) for q in (50, 10, 90))


def events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return pct([a.elapsed_time(b) * 1e3 for a, b in ev])


def wall(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t) * 1e6)
    return pct(us)


def frame(density, seed):
    rng = np.random.default_rng(seed)
    G = rng.random(GRID) < density
    P = np.where(rng.random(GRID) < 0.5, G, rng.random(GRID) < density)
    ids = lambda occ: np.where(occ, rng.integers(0, 17, GRID), FREE).astype(np.uint8)  # noqa: E731
    return ids(P), ids(G), rng.random(GRID) < 0.66


def points(m, ids, cam):
    """voxel2points of the reference on the effective ids"""
    idx = np.argwhere(m._occupied(ids, cam))
    return np.stack([idx[:, a] * m.voxel_size[a] + m.voxel_size[a] / 2 + m.range[a] for a in range(3)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r18_occ_fscore.md'))
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    try:
        from sklearn.neighbors import KDTree
    except ImportError:
        KDTree = None
    dev = torch.device('cuda:0')
    t = lambda r: 'n/a' if r is None else f'{r[0]:.0f} ({r[1]:.0f} - {r[2]:.0f})'  # noqa: E731
    rows = []
    for name, density in (('sparse', 0.02), ('dense', 0.6)):
        pred, gt, cam = frame(density, 7)
        d_pred, d_gt, d_cam = (torch.from_numpy(a).to(dev) for a in (pred, gt, cam))
        for thr in (0.4, 0.6):
            new = lambda: Metric_FScore(threshold_acc=thr, threshold_complete=thr, use_image_mask=True)  # noqa: E731
            m_dev, m_host = new(), new()
            m_dev.add_batch(d_pred, d_gt, None, d_cam)
            m_host.add_batch(pred, gt, None, cam)
            counts = m_host.frame_counts()[0]
            assert np.array_equal(m_dev.frame_counts()[0], counts)
            tree = None
            if KDTree is not None:
                p_pts, g_pts = points(m_host, pred, cam), points(m_host, gt, cam)

                def tree():
                    pt, gtree = KDTree(p_pts, leaf_size=10), KDTree(g_pts, leaf_size=10)
                    return (int((pt.query(g_pts)[0].flatten() < thr).sum()), int((gtree.query(p_pts)[0].flatten() < thr).sum()))

                assert tree() == (int(counts[2]), int(counts[3])), (tree(), counts)
            tab, dtab = m_dev.tables(GRID), m_dev._device_tables(GRID, dev)
            mask8 = d_cam.view(torch.uint8)
            out = torch.zeros((1, 4), dtype=torch.int32, device=dev)
            launch = lambda: _capi.occ_fscore_counts(d_pred[None], d_gt[None], mask8[None], dtab['void_bits'], *dtab['sq'],  # noqa: E731
                                                     dtab['offsets'], tab['R'], tab['T_acc'], tab['T_cmpl'], counts=out)
            rows.append((name, thr, counts.tolist(), len(tab['offsets']),
                         events(launch, args.iters, args.warmup),
                         events(lambda: m_dev.add_batch(d_pred, d_gt, None, d_cam), args.iters, args.warmup),
                         wall(lambda: new().add_batch(pred, gt, None, cam), args.iters, args.warmup),
                         None if tree is None else wall(tree, max(3, args.iters // 10), 1)))
            print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# Occupancy F-score of one 200 x 200 x 16 frame: device, host, KD-trees\n\n')
        f.write(f'`tools/time_occ_fscore.py`, {torch.cuda.get_device_name(0)}, {args.iters} timed iterations after {args.warmup} warm-up '
                '(the KD-tree column: a tenth as many, after one).  Times are p50 (p10 - p90) in microseconds.  The device columns are '
                'HIP-event intervals: the launch of `fbbev_occ_fscore_counts` alone, and `Metric_FScore.add_batch` (the launch, a zeroed '
                'int32 row and its append to the int64 tensor).  The host column is `Metric_FScore.add_batch` on numpy arrays, the last '
                'column the two `KDTree(..., leaf_size=10)` builds and two `query` calls of the reference on the same point sets '
                f'(scikit-learn {"not importable here" if KDTree is None else "on the host CPU"}); both by the wall clock.  All sides '
                'were checked to give the same counts first.\n\n')
        f.write('| frame | threshold | n_gt, n_pred, n_cmpl, n_acc | offsets | kernel | device add_batch | host add_batch | KD-trees |\n')
        f.write('|---|---|---|---|---|---|---|---|\n')
        for name, thr, counts, n_off, k, d, h, kd in rows:
            f.write(f'| {name} | {thr} | {counts} | {n_off} | {t(k)} | {t(d)} | {t(h)} | {t(kd)} |\n')


if __name__ == '__main__':
    main()
