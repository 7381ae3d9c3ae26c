#!/usr/bin/env python3
"""Time the occupancy class map at the shipped grid, (B, 200, 200, 16) with 19 logits, B = 1 and 4, on both head layouts, with HIP
events (20 warm-up, 100 timed iterations each), in ONE process:
  (a) parent:  the chain of FBOCC.predict_occupancy exactly as it runs (slice, softmax, argmax, permute / flip / rot90 / permute),
               with and without the contiguous copy a host transfer of the result needs
  (b) classes: fbbev_occ_classes alone
  (c) scored:  fbbev_occ_classes with gt, mask_camera, the range ring and the confusion table, on a skewed label set (almost every
               voxel (free, free)) and on a uniform one
The yardstick is (a) on the same box in the same process.  Writes p10 / p50 / p90 in microseconds and the bytes moved to
profiles/r12_occ_classes.json.

    python tools/time_occ_classes.py [--out profiles/r12_occ_classes.json] [--iters 100] [--warmup 20]
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
from fb_bev_amd.occ_metrics import range_ring  # noqa: E402

H = W = 200
D, C, C0 = 16, 19, 1


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return {k: round(float(np.percentile(us, q)), 2) for k, q in (('p10_us', 10), ('p50_us', 50), ('p90_us', 90))}


def parent_chain(occ):
    occ = occ[:, 1:].softmax(1)
    x = occ.argmax(1, keepdim=True)
    x = x.permute(0, 1, 4, 2, 3)
    x = torch.rot90(torch.flip(x, [3]), -1, [3, 4])
    return x.permute(0, 3, 4, 2, 1)[..., 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r12_occ_classes.json'))
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    ring = torch.from_numpy(range_ring((W, H), 0.4, 0, 30).astype(np.uint8)).to(dev)
    rows = []
    for B in (1, 4):
        N = H * W * D
        base = torch.randn(B, H, W, D, C, generator=g).to(dev)                       # channels-last memory
        layouts = {'channels_last': base.permute(0, 4, 1, 2, 3), 'planes': base.permute(0, 4, 1, 2, 3).contiguous()}
        for layout, logits in layouts.items():
            want = parent_chain(logits).to(torch.uint8)
            out = torch.empty(B, W, H, D, dtype=torch.uint8, device=dev)
            assert torch.equal(_capi.occ_classes(logits, c0=C0, out=out), want)
            mask = (torch.rand(B, W, H, D, generator=g) < 0.7).to(torch.uint8).to(dev)
            uniform = torch.randint(0, C - C0, (B, W, H, D), generator=g, dtype=torch.uint8).to(dev)
            skewed = torch.where(torch.rand(B, W, H, D, generator=g).to(dev) < 0.97, want, uniform)   # 97 % on the diagonal ...
            hist = torch.zeros(C - C0, C - C0, dtype=torch.int32, device=dev)
            free = logits.clone()
            free[:, C - 1] += 8.0                                                     # ... and, for `skewed_free`, in ONE bin: (free, free)
            free_gt = torch.where(torch.rand(B, W, H, D, generator=g).to(dev) < 0.97, torch.full_like(want, C - C0 - 1), uniform)
            res = {
                'parent_chain': timed(lambda: parent_chain(logits), args.iters, args.warmup),
                'parent_chain_contiguous': timed(lambda: parent_chain(logits).contiguous(), args.iters, args.warmup),
                'occ_classes': timed(lambda: _capi.occ_classes(logits, c0=C0, out=out), args.iters, args.warmup),
                'occ_classes_scored_uniform': timed(lambda: _capi.occ_classes(logits, c0=C0, gt=uniform, mask=mask, column_mask=ring, hist=hist,
                                                                              out=out), args.iters, args.warmup),
                'occ_classes_scored_diagonal': timed(lambda: _capi.occ_classes(logits, c0=C0, gt=skewed, mask=mask, column_mask=ring, hist=hist,
                                                                               out=out), args.iters, args.warmup),
                'occ_classes_scored_skewed_free': timed(lambda: _capi.occ_classes(free, c0=C0, gt=free_gt, mask=mask, column_mask=ring, hist=hist,
                                                                                  out=out), args.iters, args.warmup),
            }
            n = C - C0
            rows.append(dict(B=B, layout=layout, shape=[B, C, H, W, D], **res,
                             bytes=dict(kernel_floor=4 * B * N * C + B * N, kernel_scored=4 * B * N * C + 3 * B * N + W * H,
                                        parent_chain=B * N * (4 * C + 4 * n + 4 * n + 8 + 8 + 8 + 8 + 8),
                                        host_copy_int64=8 * B * N, host_copy_uint8=B * N)))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, rows=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
