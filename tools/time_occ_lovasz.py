#!/usr/bin/env python3
"""Time the occupancy head's Lovasz-softmax term at the shipped training shape, (B, 19, 200, 200, 16) with B = 1 and 4, on both head
layouts, with HIP events, in ONE process, the two sides ALTERNATING iteration by iteration:
  (a) parent: what OccHead.loss_voxel runs for it -- nan_to_num, torch.softmax, occ_loss.lovasz_softmax -- forward + backward to the
              gradient of the logits
  (b) fused:  occ_loss.lovasz_softmax_fused, forward + backward (fbbev_occ_lovasz_fwd, fbbev_occ_lovasz_grad)
and the two entries alone (the forward entry is a chain of launches: keys, three launches per radix pass, fg sums, coefficients,
loss, per class group).  The yardstick is (a) in the same process.  Writes p10 / p50 / p90 in microseconds, the peak of
torch.cuda.max_memory_allocated above the inputs for one iteration of each side (the gradient of the logits included), the bytes of
the traffic floors and each entry's share of the 8 TB/s peak (floor / p50) to a .json and a .md.
  forward floor:  4 B N C (logits) + 8 B N C (key words and cleared coefficients written) + passes x 16 C n_valid (pairs read and
                  written) + 12 C n_valid (pairs read, coefficients scattered) + B N (labels)
  backward floor: 12 B N C (logits, coefficients, gradient) + B N

    python tools/time_occ_lovasz.py [--out profiles/r16_occ_lovasz.json] [--iters 30] [--warmup 5] [--digit-bits 10|8]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 200
D, C, EMPTY = 16, 19, 18
PEAK_BYTES_PER_US = 8e6                    # 8 TB/s


def pct(us):
    us = np.array(us)
    return {k: round(float(np.percentile(us, q)), 2) for k, q in (('p10_us', 10), ('p50_us', 50), ('p90_us', 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_occ_lovasz.json'))
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--digit-bits', type=int, default=10, choices=(8, 10))
    args = ap.parse_args()
    os.environ['FBBEV_OCC_LOVASZ_DIGIT_BITS'] = str(args.digit_bits)             # the library reads it once, at its first forward
    import torch
    from fb_bev_amd import _capi
    from fb_bev_amd import occ_loss as L

    def alternate(fns):
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(args.iters)]
        torch.cuda.synchronize()
        for row in ev:
            for fn, (a, b) in zip(fns, row):
                a.record()
                fn()
                b.record()
        torch.cuda.synchronize()
        return [pct([row[i][0].elapsed_time(row[i][1]) * 1e3 for row in ev]) for i in range(len(fns))]

    def peak_above_inputs(fn, logits):
        logits.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    passes = 3 if args.digit_bits == 10 else 4
    rows = []
    for B in (1, 4):
        N = H * W * D
        base = (torch.randn(B, H, W, D, C, generator=g) * 2).to(dev)                # channels-last memory
        gt = torch.randint(0, C - 1, (B, H, W, D), generator=g)
        gt[torch.rand(gt.shape, generator=g) < 0.9] = EMPTY                         # real frames: almost every voxel is free
        gt[torch.rand(gt.shape, generator=g) < 0.2] = 255
        gt = gt.to(dev)
        labels = gt.to(torch.uint8)
        n_valid = int((gt != 255).sum())
        layouts = {'channels_last': base.permute(0, 4, 1, 2, 3), 'planes': base.permute(0, 4, 1, 2, 3).contiguous()}
        for layout, data in layouts.items():
            logits = data.detach().requires_grad_()

            def parent():
                x = torch.nan_to_num(logits.float(), nan=0.0, posinf=0.0, neginf=0.0)
                loss = L.lovasz_softmax(torch.softmax(x, dim=1), gt, ignore=255)
                logits.grad = None
                loss.backward()
                return loss

            def fused():
                loss = L.lovasz_softmax_fused(logits, gt)
                logits.grad = None
                loss.backward()
                return loss

            a, b = float(parent().detach()), float(fused().detach())
            assert abs(a - b) <= 2e-5 * abs(a) + 1e-6, (a, b)
            loss_c = torch.empty(C, device=dev)
            fg = torch.empty(C + 1, dtype=torch.int32, device=dev)
            coef = torch.empty((C, B, H, W, D), device=dev)
            ws_bytes = _capi.lib().fbbev_occ_lovasz_ws_bytes(B, C, H, W, D)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            scale = torch.full((1,), 0.25, device=dev)
            out = torch.empty_strided(data.shape, data.stride(), device=dev)
            t_parent, t_fused, t_fwd, t_grad = alternate(
                [parent, fused, lambda: _capi.occ_lovasz_fwd(data, labels, loss_c=loss_c, fg_count=fg, coef=coef, ws=ws),
                 lambda: _capi.occ_lovasz_grad(data, labels, coef, scale, out=out)])
            floor_f = 12 * B * N * C + passes * 16 * C * n_valid + 12 * C * n_valid + B * N
            floor_b = 12 * B * N * C + B * N
            rows.append(dict(B=B, layout=layout, digit_bits=args.digit_bits, shape=[B, C, H, W, D], n_valid=n_valid, loss=dict(parent=a, fused=b),
                             parent_fwd_bwd=t_parent, fused_fwd_bwd=t_fused, entry_fwd=t_fwd, entry_grad=t_grad,
                             peak_bytes=dict(parent=peak_above_inputs(parent, logits), fused=peak_above_inputs(fused, logits)),
                             bytes=dict(logits=4 * B * N * C, workspace=ws_bytes, floor_forward=floor_f, floor_backward=floor_b),
                             share_of_8TBps=dict(entry_fwd=round(floor_f / t_fwd['p50_us'] / PEAK_BYTES_PER_US, 3),
                                                 entry_grad=round(floor_b / t_grad['p50_us'] / PEAK_BYTES_PER_US, 3))))
            logits.grad = None
            del ws, coef, out
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, digit_bits=args.digit_bits, rows=rows), f,
                  indent=1)
        f.write('\n')
    with open(os.path.splitext(args.out)[0] + '.md', 'w') as f:
        f.write('# Lovasz-softmax occupancy loss: parent chain against the fused path\n\n')
        f.write(f'`tools/time_occ_lovasz.py --digit-bits {args.digit_bits}`, {torch.cuda.get_device_name(0)}, {args.iters} timed iterations '
                f'after {args.warmup} warm-up, the sides alternating in one process.  Times are p50 (p10 - p90) in microseconds; peak = '
                '`torch.cuda.max_memory_allocated` above the inputs for one forward + backward, the gradient of the logits (4 B N C bytes) '
                'included; share = traffic floor / p50 / 8 TB/s.\n\n')
        f.write('| B | layout | parent fwd+bwd | fused fwd+bwd | ratio | forward entry | share | grad entry | share | peak parent | peak fused | workspace |\n')
        f.write('|---|---|---|---|---|---|---|---|---|---|---|---|\n')
        t = lambda r: f'{r["p50_us"]:.0f} ({r["p10_us"]:.0f} - {r["p90_us"]:.0f})'  # noqa: E731
        for r in rows:
            f.write(f'| {r["B"]} | {r["layout"]} | {t(r["parent_fwd_bwd"])} | {t(r["fused_fwd_bwd"])} | '
                    f'{r["parent_fwd_bwd"]["p50_us"] / r["fused_fwd_bwd"]["p50_us"]:.1f}x | {t(r["entry_fwd"])} | '
                    f'{r["share_of_8TBps"]["entry_fwd"]:.3f} | {t(r["entry_grad"])} | {r["share_of_8TBps"]["entry_grad"]:.3f} | '
                    f'{r["peak_bytes"]["parent"] / 2 ** 20:.0f} MiB | {r["peak_bytes"]["fused"] / 2 ** 20:.0f} MiB | '
                    f'{r["bytes"]["workspace"] / 2 ** 20:.0f} MiB |\n')
        f.write('\nThe forward entry is a chain of launches per class group (keys; histogram, column scan and scatter per radix pass; fg sums, '
                'coefficients, loss); its time includes what the host needs to issue them.\n')


if __name__ == '__main__':
    main()
