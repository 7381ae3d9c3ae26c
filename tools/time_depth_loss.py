#!/usr/bin/env python3
"""Time the depth supervision loss of CM_DepthNet, forward + backward to the gradient of depth_preds, with HIP events, in ONE process,
the two sides ALTERNATING iteration by iteration:
  (a) parent: CM_DepthNet(fused_depth_loss=False).get_depth_loss -- the ATen chain (view / permute copies, where, min, one_hot,
              binary_cross_entropy, mask, reductions) and autograd's mirror of it
  (b) fused:  CM_DepthNet(fused_depth_loss=True).get_depth_loss -- fbbev_depth_loss_fwd + fbbev_depth_loss_grad
and the two entries alone, at
  BN = 24, 256 x 704, downsample 16, D = 80,  depth [2, 42, 0.5]      (4 samples x 6 cameras of the shipped config)
  BN = 6,  512 x 1408, downsample 16, D = 118, depth [1, 60, 0.5]
The yardstick is (a) in the same process.  Writes p10 / p50 / p90 in microseconds, the kernel launches of one step (the device
kernels torch.profiler sees), the peak of torch.cuda.max_memory_allocated above the inputs for one step of each side (the gradient
of depth_preds included) and the bytes either side must move at least, to a .json and a .md.

    python tools/time_depth_loss.py [--out profiles/r21_depth_loss.json] [--iters 30] [--warmup 5]
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
from fb_bev_amd.depth_net import CM_DepthNet  # noqa: E402

SHAPES = [dict(BN=24, H=256, W=704, ds=16, D=80, cfg=[2.0, 42.0, 0.5]), dict(BN=6, H=512, W=1408, ds=16, D=118, cfg=[1.0, 60.0, 0.5])]


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


def peak_above_inputs(fn, x):
    """peak of one forward + backward above the inputs; the gradient it leaves behind is counted"""
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def launches(fn):
    """device kernels (memsets and copies included) of one call, as torch.profiler records them"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_depth_loss.json'))
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    rows = []
    for s in SHAPES:
        BN, H, W, ds, D, cfg = (s[k] for k in ('BN', 'H', 'W', 'ds', 'D', 'cfg'))
        h, w = H // ds, W // ds
        gt = torch.rand((1, BN, H, W), generator=g) * (cfg[1] + 5)
        gt[torch.rand(gt.shape, generator=g) < 0.985] = 0.0                             # a projected lidar sweep: ~1.5 % of the pixels
        gt = gt.to(dev)
        x = torch.softmax(3 * torch.randn((1, BN, D, h, w), generator=g), dim=2).to(dev).requires_grad_()
        mk = lambda fused: CM_DepthNet(in_channels=8, context_channels=4, depth_channels=D, mid_channels=8, use_dcn=False,  # noqa: E731
                                       use_aspp=False, downsample=ds, grid_config=dict(depth=cfg), loss_depth_weight=3.0,
                                       fused_depth_loss=fused).to(dev)
        nets = {False: mk(False), True: mk(True)}

        def step(fused):
            loss = nets[fused].get_depth_loss(gt, x)['loss_depth']
            x.grad = None
            loss.backward()
            return loss

        parent, fused = (lambda: step(False)), (lambda: step(True))
        a, b = float(parent()), float(fused())
        assert abs(a - b) <= 1e-5 * abs(a), (a, b)
        gt3, probs = gt.view(BN, H, W), x.detach().view(BN, D, h, w)
        labels = torch.empty((BN, h, w), dtype=torch.int32, device=dev)
        out_f, out_i = torch.empty(2, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(_capi.lib().fbbev_depth_loss_ws_bytes(BN, h, w, D), dtype=torch.uint8, device=dev)
        gl, out = torch.ones(1, device=dev), torch.empty_like(probs)
        t_parent, t_fused, t_fwd, t_grad = alternate(
            [parent, fused, lambda: _capi.depth_loss_fwd(gt3, probs, ds, D, cfg[0], cfg[2], labels=labels, out_f=out_f, out_i=out_i, ws=ws),
             lambda: _capi.depth_loss_grad(probs, labels, out_i, gl, out=out)], args.iters, args.warmup)
        n_gt, n_p = 4 * BN * H * W, 4 * BN * D * h * w
        rows.append(dict(shape=s, foreground_cells=int(out_i), cells=BN * h * w, loss=b, parent_fwd_bwd=t_parent, fused_fwd_bwd=t_fused,
                         kernel_fwd=t_fwd, kernel_grad=t_grad, launches=dict(parent=launches(parent), fused=launches(fused)),
                         peak_bytes=dict(parent=peak_above_inputs(parent, x), fused=peak_above_inputs(fused, x)),
                         bytes=dict(gt=n_gt, probs=n_p, floor_forward=n_gt + n_p + 4 * BN * h * w, floor_backward=2 * n_p + 4 * BN * h * w)))
        x.grad = None
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, rows=rows), f, indent=1)
        f.write('\n')
    with open(os.path.splitext(args.out)[0] + '.md', 'w') as f:
        f.write('# Depth supervision loss: the ATen chain against the fused route\n\n')
        f.write(f'`tools/time_depth_loss.py`, {torch.cuda.get_device_name(0)}, {args.iters} timed iterations after {args.warmup} warm-up, the '
                'sides alternating in one process.  Times are p50 (p10 - p90) in microseconds for forward + backward to the gradient of '
                'depth_preds; launches = device kernels of one step as torch.profiler records them; peak = `torch.cuda.max_memory_allocated` '
                'above the inputs for one step, the gradient of depth_preds included; floor = the bytes a pass must move (forward: gt + '
                'probs + labels, backward: probs + grad_probs + labels).\n\n')
        f.write('| BN | image | ds | D | parent fwd+bwd | fused fwd+bwd | ratio | fwd entry | grad entry | launches parent | launches fused | '
                'peak parent | peak fused | floor fwd | floor bwd |\n')
        f.write('|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n')
        t = lambda r: f'{r["p50_us"]:.0f} ({r["p10_us"]:.0f} - {r["p90_us"]:.0f})'  # noqa: E731
        for r in rows:
            s = r['shape']
            f.write(f'| {s["BN"]} | {s["H"]} x {s["W"]} | {s["ds"]} | {s["D"]} | {t(r["parent_fwd_bwd"])} | {t(r["fused_fwd_bwd"])} | '
                    f'{r["parent_fwd_bwd"]["p50_us"] / r["fused_fwd_bwd"]["p50_us"]:.1f}x | {t(r["kernel_fwd"])} | {t(r["kernel_grad"])} | '
                    f'{r["launches"]["parent"]} | {r["launches"]["fused"]} | {r["peak_bytes"]["parent"] / 2 ** 20:.1f} MiB | '
                    f'{r["peak_bytes"]["fused"] / 2 ** 20:.1f} MiB | {r["bytes"]["floor_forward"] / 2 ** 20:.1f} MiB | '
                    f'{r["bytes"]["floor_backward"] / 2 ** 20:.1f} MiB |\n')
        f.write("\nAn interval spans a side's launches as the GPU sees them: where the GPU work is shorter than the time the host needs to "
                'issue it, the interval measures the host, not the kernels; the entry columns are the C entries alone (forward: two '
                'launches, gradient: one).\n')


if __name__ == '__main__':
    main()
