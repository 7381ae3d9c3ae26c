#!/usr/bin/env python3
"""Time the occupancy head's three sum-shaped voxel losses at the shipped training shape, (B, 19, 200, 200, 16) with B = 1 and 4, on both
head layouts, in focal and cross-entropy mode, with HIP events, in ONE process, the two sides ALTERNATING iteration by iteration:
  (a) parent: what OccHead.loss_voxel runs for them -- nan_to_num, CustomFocalLoss or CE_ssc_loss, sem_scal_loss, geo_scal_loss --
              forward + backward to the gradient of the logits
  (b) fused:  occ_loss.voxel_losses_fused, forward + backward (fbbev_occ_loss_stats, the torch epilogue, fbbev_occ_loss_grad)
and the two kernels alone.  The yardstick is (a) in the same process.  Writes p10 / p50 / p90 in microseconds, the peak of
torch.cuda.max_memory_allocated above the inputs for one iteration of each side (the gradient of the logits included), the bytes of the traffic floors (forward
4 B N C + B N, backward 8 B N C + B N) and each kernel's share of the 8 TB/s peak (floor / p50) to a .json and a .md.

    python tools/time_occ_loss.py [--out profiles/r15_occ_loss.json] [--iters 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fb_bev_amd import _capi  # noqa: E402
from fb_bev_amd import occ_loss as L  # noqa: E402

H = W = 200
D, C, EMPTY = 16, 19, 18
PEAK_BYTES_PER_US = 8e6                    # 8 TB/s


def pct(us):
    us = np.array(us)
    return {k: round(float(np.percentile(us, q)), 2) for k, q in (('p10_us', 10), ('p50_us', 50), ('p90_us', 90))}


def alternate(fns, iters, warmup):
    """the functions in turn, iteration by iteration -> one percentile record each"""
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


def peak_above_inputs(fn, logits):
    """peak of one forward + backward above the inputs; the gradient of the logits it leaves behind is counted"""
    logits.grad = None                     # the previous iteration's: else the base holds it and the new one replaces it unseen
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15_occ_loss.json'))
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    cw = L.class_weights(C).float().to(dev)
    focal_mod = L.CustomFocalLoss(bev_hw=(H, W)).to(dev)
    rows = []
    for B in (1, 4):
        N = H * W * D
        base = (torch.randn(B, H, W, D, C, generator=g) * 2).to(dev)                # channels-last memory
        gt = torch.randint(0, C - 1, (B, H, W, D), generator=g)
        gt[torch.rand(gt.shape, generator=g) < 0.9] = EMPTY                         # real frames: almost every voxel is free
        gt[torch.rand(gt.shape, generator=g) < 0.2] = 255
        gt = gt.to(dev)
        labels = gt.to(torch.uint8)
        layouts = {'channels_last': base.permute(0, 4, 1, 2, 3), 'planes': base.permute(0, 4, 1, 2, 3).contiguous()}
        for layout, data in layouts.items():
            for focal in (True, False):
                logits = data.detach().requires_grad_()

                def parent():
                    x = torch.nan_to_num(logits.float(), nan=0.0, posinf=0.0, neginf=0.0)
                    ce = focal_mod(x, gt, cw, ignore_index=255) if focal else L.CE_ssc_loss(x, gt, cw, ignore_index=255)
                    total = ce + L.sem_scal_loss(x, gt, ignore_index=255) + L.geo_scal_loss(x, gt, ignore_index=255, non_empty_idx=EMPTY)
                    logits.grad = None
                    total.backward()
                    return total

                def fused():
                    ce, sem, geo = L.voxel_losses_fused(logits, gt, cw, focal_mod.c if focal else None, EMPTY, focal, focal_mod.gamma,
                                                        focal_mod.alpha, focal_mod.loss_weight)
                    logits.grad = None
                    (ce + sem + geo).backward()
                    return ce + sem + geo

                a, b = float(parent()), float(fused())
                assert abs(a - b) <= 1e-4 * abs(a), (a, b)
                plane = focal_mod.c if focal else None
                sf = torch.empty(3 * C + 4, device=dev)
                si = torch.empty(C + 1, dtype=torch.int32, device=dev)
                ws = torch.empty(_capi.lib().fbbev_occ_loss_ws_bytes(B, C, H, W, D), dtype=torch.uint8, device=dev)
                gs = torch.randn(3 * C + 4, generator=g).to(dev)
                out = torch.empty_strided(data.shape, data.stride(), device=dev)
                t_parent, t_fused, t_stats, t_grad = alternate(
                    [parent, fused,
                     lambda: _capi.occ_loss_stats(data, labels, cw, plane, EMPTY, focal, stats_f=sf, stats_i=si, ws=ws),
                     lambda: _capi.occ_loss_grad(data, labels, gs, cw, plane, EMPTY, focal, out=out)], args.iters, args.warmup)
                floor_f, floor_b = 4 * B * N * C + B * N, 8 * B * N * C + B * N
                rows.append(dict(B=B, layout=layout, mode='focal' if focal else 'ce', shape=[B, C, H, W, D], parent_fwd_bwd=t_parent,
                                 fused_fwd_bwd=t_fused, kernel_stats=t_stats, kernel_grad=t_grad,
                                 peak_bytes=dict(parent=peak_above_inputs(parent, logits), fused=peak_above_inputs(fused, logits)),
                                 bytes=dict(logits=4 * B * N * C, floor_forward=floor_f, floor_backward=floor_b),
                                 share_of_8TBps=dict(kernel_stats=round(floor_f / t_stats['p50_us'] / PEAK_BYTES_PER_US, 3),
                                                     kernel_grad=round(floor_b / t_grad['p50_us'] / PEAK_BYTES_PER_US, 3))))
                logits.grad = None
                print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, rows=rows), f, indent=1)
        f.write('\n')
    with open(os.path.splitext(args.out)[0] + '.md', 'w') as f:
        f.write('# Occupancy voxel losses: parent chain against the fused path\n\n')
        f.write(f'`tools/time_occ_loss.py`, {torch.cuda.get_device_name(0)}, {args.iters} timed iterations after {args.warmup} warm-up, '
                'the sides alternating in one process.  Times are p50 (p10 - p90) in microseconds; peak = '
                '`torch.cuda.max_memory_allocated` above the inputs for one forward + backward, the gradient of the logits (4 B N C bytes) included; share = traffic floor / p50 / 8 TB/s.\n\n')
        f.write('| B | layout | mode | parent fwd+bwd | fused fwd+bwd | ratio | stats kernel | share | grad kernel | share | peak parent | peak fused |\n')
        f.write('|---|---|---|---|---|---|---|---|---|---|---|---|\n')
        t = lambda r: f'{r["p50_us"]:.0f} ({r["p10_us"]:.0f} - {r["p90_us"]:.0f})'  # noqa: E731
        for r in rows:
            f.write(f'| {r["B"]} | {r["layout"]} | {r["mode"]} | {t(r["parent_fwd_bwd"])} | {t(r["fused_fwd_bwd"])} | '
                    f'{r["parent_fwd_bwd"]["p50_us"] / r["fused_fwd_bwd"]["p50_us"]:.1f}x | {t(r["kernel_stats"])} | '
                    f'{r["share_of_8TBps"]["kernel_stats"]:.3f} | {t(r["kernel_grad"])} | {r["share_of_8TBps"]["kernel_grad"]:.3f} | '
                    f'{r["peak_bytes"]["parent"] / 2 ** 20:.0f} MiB | {r["peak_bytes"]["fused"] / 2 ** 20:.0f} MiB |\n')
        f.write("\nAn interval spans a side's launches as the GPU sees them: where the GPU work is shorter than the time the host needs to issue it (B = 1: a hundred small launches on either side) the interval measures the host, not the kernels; the kernel columns are single launches.\n")


if __name__ == '__main__':
    main()
