#!/usr/bin/env python3
"""Deterministic mode against the default mode, interleaved step by step on the same inputs: the path's training step
(bench.py `fb_projection_train`, configs[2]: BL2, B = 4, 4 levels).  Prints one JSON line: p50 / p10 / p90 of each mode in ms.

    python tools/time_deterministic.py [--steps 50] [--warmup 5]

Also one MConv3d weight gradient and the MSDA boundary backward, interleaved the same way.  Kernel times: run under
`rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fb_bev_amd as F                                                  # noqa: E402
from fb_bev_amd import synthetic as S                                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--config', default='BL2')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--levels', type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing to measure')
    dev = torch.device('cuda:0')
    d = S.fb_path_step(a.config, a.batch, a.levels, dev)
    step = d['step']
    times = {False: [], True: []}
    try:
        for mode in (False, True):
            F.set_deterministic(mode)
            for _ in range(a.warmup):
                step()
        torch.cuda.synchronize()
        for _ in range(a.steps):
            for mode in (False, True):
                F.set_deterministic(mode)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step()
                e1.record()
                torch.cuda.synchronize()
                times[mode].append(e0.elapsed_time(e1))
    finally:
        F.set_deterministic(None)

    def q(v, p):
        v = sorted(v)
        return round(v[min(len(v) - 1, int(p * len(v)))], 4)

    def summary(t, workload):
        r = {'workload': workload, 'steps': a.steps}
        for mode, key in ((False, 'off'), (True, 'on')):
            r[key] = {'p50_ms': q(t[mode], 0.5), 'p10_ms': q(t[mode], 0.1), 'p90_ms': q(t[mode], 0.9)}
        r['ratio_on_off'] = round(r['on']['p50_ms'] / r['off']['p50_ms'], 4)
        return r
    res = summary(times, f'fb_projection_train {a.config} B={a.batch} L={a.levels}')
    res['overhead'] = round(res['ratio_on_off'] - 1.0, 4)
    res['note'] = 'every step ends in a device synchronise (both modes): absolute times sit above bench.py\'s'
    res['conv3d_wgrad'] = summary(interleaved(a, *conv3d_wgrad_call(dev)), 'MConv3d 3x3x3 80->80 at 100x100x8, B=1: weight gradient')
    res['msda_boundary_bwd'] = summary(interleaved(a, *msda_bwd_call(dev)),
                                       'ms_deform_attn_backward as mmcv calls it: B=4, 40000 queries, 8 heads, Dh 32, 4 levels, 4 points')
    print(json.dumps(res))


def interleaved(a, fn, _):
    times = {False: [], True: []}
    try:
        for mode in (False, True):
            F.set_deterministic(mode)
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.steps):
            for mode in (False, True):
                F.set_deterministic(mode)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[mode].append(e0.elapsed_time(e1))
    finally:
        F.set_deterministic(None)
    return times


def conv3d_wgrad_call(dev):
    from fb_bev_amd import _capi
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 8, 100, 100, 80, generator=g).to(dev)
    dy = torch.randn(1, 8, 100, 100, 80, generator=g).to(dev)
    dw = torch.zeros(27, 80, 80, device=dev)
    return (lambda: _capi.conv3d_wgrad_ndhwc(x, dy, dw.zero_(), ksize=3, stride=1, pad=1)), None


def msda_bwd_call(dev):
    from fb_bev_amd.ms_deform_attn import ms_deform_attn_backward
    g = torch.Generator().manual_seed(0)
    B, M, Dh, L, P, Q = 4, 8, 32, 4, 4, 40000
    shapes = torch.tensor([[32, 88], [16, 44], [8, 22], [4, 11]])
    ls = torch.cat([shapes.new_zeros(1), (shapes[:, 0] * shapes[:, 1]).cumsum(0)[:-1]]).to(dev)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    shapes = shapes.to(dev)
    value = torch.randn(B, S, M, Dh, generator=g).to(dev)
    loc = torch.rand(B, Q, M, L, P, 2, generator=g).to(dev)
    attn = torch.rand(B, Q, M, L, P, generator=g).to(dev)
    go = torch.randn(B, Q, M * Dh, generator=g).to(dev)
    outs = [torch.zeros_like(t) for t in (value, loc, attn)]

    def fn():
        for t in outs:
            t.zero_()
        ms_deform_attn_backward(value, shapes, ls, loc, attn, go, *outs)
    return fn, None


if __name__ == '__main__':
    main()
