#!/usr/bin/env python3
"""Time the LiDAR -> multi-view depth step with HIP events, in ONE process, the two sides ALTERNATING iteration by iteration:
  (a) argsort: a torch restatement of the reference's route (PointToMultiViewDepth, loading.py:883-907 and :951-957) on the SAME GPU:
               per sample and camera two matmuls, a division, round, six comparisons, argsort of rank + depth / 100, first-of-run
               mask, scatter -- what a straight port of the pipeline step to the device would launch
  (b) entry:   fb_bev_amd.points_depth.points_to_depth on GPU tensors = fbbev_points_to_depth (a memset, the splat kernel, the
               resolve kernel)
at B = 4, N = 6, 256 x 704, downsample 1, depth [2, 42), 34 720 points of 5 floats per sample, nuScenes-like calibration (the real
layer of tests/points_depth_cases.py).  A CPU run of the same restatement -- what a loader worker does today, followed by 4.3 MB per
sample through the loader and over PCIe -- is a stated baseline outside the timed region (wall clock, one thread pool as torch
finds it).  Writes p10 / p50 / p90 in microseconds, the device operations of one call with their durations as torch.profiler
records them, and the bytes each of the entry's three operations moves, to a .json and a .md.

    python tools/time_points_depth.py [--out profiles/r22_points_depth.json] [--iters 30] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import points_depth_cases as PC  # noqa: E402
from fb_bev_amd.points_depth import points_to_depth  # noqa: E402

B, N, H, W, P, STRIDE, CFG = 4, 6, 256, 704, 34720, 5, (2.0, 42.0)


def pct(us):
    us = np.array(us)
    return {k: round(float(np.percentile(us, q)), 2) for k, q in (('p10_us', 10), ('p50_us', 50), ('p90_us', 90))}


def alternate(fns, iters, warmup):
    for _ in range(warmup):
        for fn in fns:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(iters)]
    torch.cuda.synchronize()
    for row in ev:
        for fn, (a, b) in zip(fns, row):
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return [pct([row[i][0].elapsed_time(row[i][1]) * 1e3 for row in ev]) for i in range(len(fns))]


def device_ops(fn):
    """[(name, microseconds)] of the device operations of one call, as torch.profiler records them"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(e.name[:60], round(float(e.device_time), 2)) for e in prof.events() if str(e.device_type).endswith('CUDA')]


def argsort_route(points, lidar2img, post_rots, post_trans, counts=None):
    """the reference's route in torch on the tensors' device -> (B, N, H, W); counts: a list that receives the kept pairs"""
    lo, hi = CFG
    out = torch.zeros((B, N, H, W), dtype=torch.float32, device=points[0].device)
    for b in range(B):
        xyz = points[b][:, :3]
        for n in range(N):
            m = lidar2img[b, n]
            p = xyz.matmul(m[:3, :3].T) + m[:3, 3].unsqueeze(0)
            p = torch.cat([p[:, :2] / p[:, 2:3], p[:, 2:3]], 1)
            p = p.matmul(post_rots[b, n].T) + post_trans[b, n:n + 1]
            coor = torch.round(p[:, :2] / 1)
            depth = p[:, 2]
            kept = (coor[:, 0] >= 0) & (coor[:, 0] < W) & (coor[:, 1] >= 0) & (coor[:, 1] < H) & (depth < hi) & (depth >= lo)
            coor, depth = coor[kept], depth[kept]
            if counts is not None:
                counts.append(int(kept.sum()))
            ranks = coor[:, 0] + coor[:, 1] * W
            order = (ranks + depth / 100.).argsort()
            coor, depth, ranks = coor[order], depth[order], ranks[order]
            first = torch.ones(coor.shape[0], device=coor.device, dtype=torch.bool)
            first[1:] = ranks[1:] != ranks[:-1]
            coor, depth = coor[first].to(torch.long), depth[first]
            out[b, n][coor[:, 1], coor[:, 0]] = depth
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r22_points_depth.json'))
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    pts0, M, R, T = PC.real_inputs(PC.by_name('shipped'))
    rng = np.random.default_rng(5)
    cpu_pts = []
    for b in range(B):                                               # the sweep of the test case, turned about the vertical per sample
        a = rng.uniform(0, 2 * np.pi)
        rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        rows = pts0[0].copy()
        rows[:, :3] = (rows[:, :3].astype(np.float64) @ rot.T).astype(np.float32)
        cpu_pts.append(torch.from_numpy(rows))
    cpu_m = [torch.from_numpy(np.repeat(a, B, 0).copy()) for a in (M, R, T)]
    points = [p.to(dev) for p in cpu_pts]
    mats = [t.to(dev) for t in cpu_m]
    flat = torch.cat(points, 0)
    offsets = torch.arange(B + 1, dtype=torch.int32, device=dev) * P

    entry = lambda: points_to_depth(flat, *mats, H, W, 1, CFG, offsets=offsets)  # noqa: E731
    route = lambda: argsort_route(points, *mats)  # noqa: E731
    counts = []
    want, got = argsort_route(points, *mats, counts=counts), entry()
    differ = int((want != got).sum())
    assert bool((got <= want).all()) and bool(((got != 0) == (want != 0)).all())       # only key ties and last-bit dot products differ
    t_route, t_entry = alternate([route, entry], args.iters, args.warmup)
    t0 = time.perf_counter()
    cpu = argsort_route(cpu_pts, *cpu_m)
    t_cpu = time.perf_counter() - t0
    plane = 4 * B * N * H * W
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
               shape=dict(B=B, N=N, H=H, W=W, downsample=1, points_per_sample=P, point_stride=STRIDE, depth=list(CFG)),
               non_empty_pixels=int((got != 0).sum()), kept_pairs=int(sum(counts)), pixels_that_differ_from_the_argsort_route=differ,
               argsort_route_gpu=t_route, entry=t_entry,
               device_ops=dict(argsort_route_gpu=len(device_ops(route)), entry=device_ops(entry)),
               cpu_argsort_route_ms=round(1e3 * t_cpu, 1), cpu_threads=torch.get_num_threads(),
               cpu_equals_gpu_route_pixels=int((cpu == want.cpu()).sum()),
               bytes=dict(memset_written=plane, resolve_read_and_written=2 * plane,
                          splat_points_read_once=4 * STRIDE * B * P, splat_points_rows_touched_by_all_cameras=4 * STRIDE * B * P * N,
                          splat_atomics=4 * int(sum(counts)), map_through_the_loader_today=plane, sweep_instead=4 * STRIDE * B * P))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    t = lambda r: f'{r["p50_us"]:.0f} ({r["p10_us"]:.0f} - {r["p90_us"]:.0f})'  # noqa: E731
    with open(os.path.splitext(args.out)[0] + '.md', 'w') as f:
        f.write('# LiDAR points to multi-view depth maps: the argsort route against the z-buffer entry\n\n')
        f.write(f'`tools/time_points_depth.py`, {res["device"]}, {args.iters} timed iterations after {args.warmup} warm-up, the sides '
                f'alternating in one process; B = {B}, N = {N}, {H} x {W}, downsample 1, {P} points of {STRIDE} floats per sample.  Times are '
                'p50 (p10 - p90) in microseconds between HIP events around one call.\n\n')
        f.write('| side | time | device operations |\n|---|---|---|\n')
        f.write(f'| argsort route in torch on the GPU | {t(t_route)} | {res["device_ops"]["argsort_route_gpu"]} |\n')
        f.write(f'| `fbbev_points_to_depth` | {t(t_entry)} | {len(res["device_ops"]["entry"])} |\n\n')
        f.write('The entry\'s device operations of one call (torch.profiler): ' +
                '; '.join(f'`{n}` {us} us' for n, us in res['device_ops']['entry']) + '.\n\n')
        bt = res['bytes']
        f.write(f'Bytes: the memset writes {bt["memset_written"] / 2 ** 20:.1f} MiB; the resolve pass reads and writes '
                f'{bt["resolve_read_and_written"] / 2 ** 20:.1f} MiB; the splat reads the sweeps once from memory '
                f'({bt["splat_points_read_once"] / 2 ** 20:.2f} MiB, each row touched by all {N} cameras: '
                f'{bt["splat_points_rows_touched_by_all_cameras"] / 2 ** 20:.1f} MiB of requests) and issues {res["kept_pairs"]} '
                f'4-byte atomics ({bt["splat_atomics"] / 2 ** 10:.0f} KiB).  {res["non_empty_pixels"]} pixels are non-empty; '
                f'{differ} differ from the argsort route (ties of its fp32 key, and dot products associated otherwise).\n\n')
        f.write(f'Baseline outside the timed region: the same restatement on the CPU ({res["cpu_threads"]} threads, one wall-clock run) takes '
                f'{res["cpu_argsort_route_ms"]} ms for the {B} samples, and the loader then ships {bt["map_through_the_loader_today"] / 2 ** 20:.1f} MiB '
                f'of maps instead of {bt["sweep_instead"] / 2 ** 20:.2f} MiB of points.\n\n')
        f.write('An interval spans a side\'s launches as the GPU sees them: where the GPU work is shorter than the time the host needs to issue '
                'it, the interval measures the host, not the kernels.  The resolve variant that scatters from the points into a second plane '
                'was not built and not measured.  The effect on the whole training step is not measured.\n')


if __name__ == '__main__':
    main()
