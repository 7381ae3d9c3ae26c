#!/usr/bin/env python3
"""The exact-fp32 TRAINING route of the row-wise linear layers (mode f32_mfma under autograd: _RowsLinearF32 -- forward and input
gradient on fbbev_rows_linear_f32, weight / bias gradient on fbbev_rows_wgrad_f32) against mode f32 (the vendor GEMMs of
rows_linear._RowsLinear: the route a training step in f32_mfma mode took before), interleaved step by step: the path's training step
at BASELINE configs[2] (BL2, B = 4, 4 levels; synthetic.fb_path_step(..., train=True).step -- the step bench.py's
`fb_projection_train` leg times).  Each mode times its OWN copy of the model (same seed: same parameters, same inputs), so no weight
cache is rebuilt inside a timed step.  Then the weight-gradient launch of every layer shape of that step on its own, beside the
split-K vendor form it replaces and the compute floor 2 rows I O / 157.3 TFLOP/s.  Prints one JSON line.

    python tools/time_rows_linear_f32_train.py [--steps 50] [--warmup 5]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fb_bev_amd import _capi, rows_linear as RL, synthetic as S         # noqa: E402
from time_rows_linear_f32 import PEAK_F32_MATRIX_TFLOPS, interleaved, layer_cases   # noqa: E402

STEP_MODES = ('f32', 'f32_mfma')


def time_wgrad(dev, name, rows, I, O, steps, warmup):
    g = torch.Generator().manual_seed(I + O)
    gy = torch.randn(rows, O, generator=g).to(dev)
    x = torch.randn(rows, I, generator=g).to(dev)
    floor_ms = 2.0 * rows * I * O / (PEAK_F32_MATRIX_TFLOPS * 1e12) * 1e3
    rec = {'layer': name, 'rows': rows, 'in': I, 'out': O, 'compute_floor_ms': round(floor_ms, 5)}
    if not (_capi.rows_wgrad_f32_supported(gy, x)):
        return {**rec, 'unsupported': True}
    fns = {'wgrad_f32': lambda: _capi.rows_wgrad_f32(gy, x),
           'vendor_split_k': lambda: (RL.weight_grad(gy, x), RL.bias_grad(gy))}
    with torch.no_grad():
        t = interleaved(fns, steps, warmup)
    L = _capi.rows_wgrad_f32_slice_rows(rows, I, O)
    return {**rec, **t, 'slice_rows': L, 'slices': (rows + L - 1) // L,
            'fraction_of_floor_reached': round(floor_ms / t['wgrad_f32']['p50_ms'], 4),
            'wgrad_f32_over_vendor': round(t['wgrad_f32']['p50_ms'] / t['vendor_split_k']['p50_ms'], 4)}


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
    first = RL.mode()
    ds = {}
    try:
        for k in STEP_MODES:
            RL.set_mode(k)
            ds[k] = S.fb_path_step(a.config, a.batch, a.levels, dev, train=True)    # seeded: the same parameters and inputs in every copy

        def step_in(mode):
            def fn():
                RL.set_mode(mode)
                return ds[mode]['step']()
            return fn
        out = {k: step_in(k)().detach().float().clone() for k in STEP_MODES}
        grads = {k: {n: t.grad.detach().clone() for n, t in zip(ds[k]['names'], ds[k]['leaves']) if t.grad is not None} for k in STEP_MODES}
        t = interleaved({k: step_in(k) for k in STEP_MODES}, a.steps, a.warmup)
    finally:
        RL.set_mode(first)
    rel = {}
    for n, g in grads['f32_mfma'].items():
        if n in grads['f32'] and float(grads['f32'][n].abs().max()) > 0:
            rel[n] = float((g - grads['f32'][n]).abs().max() / grads['f32'][n].abs().max())
    band = t['f32']['p90_ms'] - t['f32']['p10_ms']
    res = {'workload': f'fb_projection training step {a.config} B={a.batch} L={a.levels}', 'steps': a.steps, 'warmup': a.warmup, 'modes': t,
           'f32_mfma_over_f32': round(t['f32_mfma']['p50_ms'] / t['f32']['p50_ms'], 4),
           'f32_mfma_minus_f32_ms': round(t['f32_mfma']['p50_ms'] - t['f32']['p50_ms'], 4), 'f32_p10_p90_band_ms': round(band, 4),
           'slower_than_f32_by_more_than_its_band': bool(t['f32_mfma']['p50_ms'] - t['f32']['p50_ms'] > band),
           'max_abs_output_diff': float((out['f32'] - out['f32_mfma']).abs().max()), 'output_scale': float(out['f32_mfma'].abs().max()),
           'largest_gradient_diff_relative_to_tensor_peak': max(rel.values()) if rel else None,
           'note': 'one model copy per mode (no weight cache is rebuilt inside a timed step); every step ends in a device synchronise'}
    d = ds['f32']
    X, Y, _ = d['pc'].grid_xyz
    rows = a.batch * X * Y
    tokens = a.batch * d['pc'].n_cams * sum(h * w for h, w in d['shapes'])
    del d, ds, out, grads
    torch.cuda.empty_cache()
    res['wgrad_layers'] = [time_wgrad(dev, name, r, I, O, a.steps, a.warmup) for name, r, I, O, _ in layer_cases(dev, rows, tokens)]
    done = [l for l in res['wgrad_layers'] if 'wgrad_f32' in l]
    res['wgrad_layers_sum_ms'] = {k: round(sum(l[k]['p50_ms'] for l in done), 4) for k in ('wgrad_f32', 'vendor_split_k')}
    res['peak_f32_matrix_tflops'] = PEAK_F32_MATRIX_TFLOPS
    print(json.dumps(res))


if __name__ == '__main__':
    main()
