#!/usr/bin/env python3
"""The three routes of the row-wise linear layers (FBBEV_ROWS_LINEAR = x3 | f32 | f32_mfma) interleaved step by step on the same
inputs: the path's INFERENCE step at BASELINE configs[2] (BL2, B = 4, 4 levels; the step bench.py's `fb_projection` leg times:
model and inputs of synthetic.fb_path_step(..., train=False), called under no_grad).  Then every layer shape of that step on its
own: the exact-fp32 kernel (fbbev_rows_linear_f32*) against F.linear + the separate ATen passes it replaces (`vendor_gemm_and_passes`)
and, for the LayerNorm layers, against what the module's f32 route really runs (`module_f32_route`: F.linear, then the library's own
residual + LayerNorm kernel), with the layer's compute floor 2 rows I O / 157.3 TFLOP/s (the FP32 matrix peak both use) and the
fraction of it reached.  Prints one JSON line.

Steady state: every mode times its OWN copy of the model (built from the same seed: same parameters, same inputs).  The weight caches hold one entry keyed on
the mode, so one model switched between modes step by step would rebuild its caches (fragments, padded value weights, permuted
rows: ~20 small launches) inside every timed x3 and f32_mfma step, and none inside the f32 steps.

    python tools/time_rows_linear_f32.py [--steps 50] [--warmup 5]

Kernel times of the new route's step: `rocprofv3 --kernel-trace --stats -- python tools/time_rows_linear_f32.py --only f32_mfma`."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fb_bev_amd import _capi, rows_linear as RL, synthetic as S         # noqa: E402

PEAK_F32_MATRIX_TFLOPS = 157.3


def q(v, p):
    v = sorted(v)
    return round(v[min(len(v) - 1, int(p * len(v)))], 4)


def interleaved(fns, steps, warmup):
    """fns: {name: callable}; one launch of each per round, HIP events around each, a device synchronise behind each"""
    times = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(steps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: {'p50_ms': q(t, 0.5), 'p10_ms': q(t, 0.1), 'p90_ms': q(t, 0.9)} for k, t in times.items()}


def layer_cases(dev, rows, tokens):
    """(name, rows, I, O, kind) of the encoder layer at configs[2]: kind = plain | relu | add | ln"""
    return [('self_attn sampling_offsets 80->64 (+ query_pos)', rows, 80, 64, 'add'),
            ('self_attn attention_weights 80->32 (+ query_pos)', rows, 80, 32, 'add'),
            ('self_attn value_proj 80->96 (head-padded)', rows, 80, 96, 'plain'),
            ('cross_attn sampling_offsets 80->512 (+ query_pos)', rows, 80, 512, 'add'),
            ('cross_attn attention_weights 80->256 (+ query_pos)', rows, 80, 256, 'add'),
            ('cross_attn value_proj 80->96 on the camera tokens', tokens, 80, 96, 'plain'),
            ('output_proj 80->80 + residual + LayerNorm', rows, 80, 80, 'ln'),
            ('FFN 80->320 + ReLU', rows, 80, 320, 'relu'),
            ('FFN 320->80 + residual + LayerNorm', rows, 320, 80, 'ln')]


def time_layer(dev, name, rows, I, O, kind, steps, warmup):
    g = torch.Generator().manual_seed(I + O)
    x = torch.randn(rows, I, generator=g).to(dev)
    w = (torch.randn(O, I, generator=g) / I ** 0.5).to(dev)
    b = torch.randn(O, generator=g).to(dev)
    P = rows // 4 if rows % 4 == 0 else rows
    add = torch.randn(P, I, generator=g).to(dev)
    res = torch.randn(rows, O, generator=g).to(dev)
    norm = torch.nn.LayerNorm(O).to(dev)
    out = torch.empty(rows, O, device=dev)
    module = None
    if kind == 'ln':
        kernel = lambda: _capi.rows_linear_f32_ln(x, w, b, res, norm.weight, norm.bias, norm.eps, out=out)             # noqa: E731
        vendor = lambda: F.layer_norm(F.linear(x, w, b) + res, (O,), norm.weight, norm.bias, norm.eps)                  # noqa: E731
        module = lambda: _capi.layernorm(F.linear(x, w, b), norm.weight, norm.bias, norm.eps, residual=res)             # noqa: E731
    elif kind == 'add':
        add3 = add.unsqueeze(0).expand(rows // P, P, I)
        kernel = lambda: _capi.rows_linear_f32(x, w, b, out=out, addend=add)                                             # noqa: E731
        vendor = lambda: F.linear((x.view(rows // P, P, I) + add3).view(rows, I), w, b)                                   # noqa: E731
    elif kind == 'relu':
        kernel = lambda: _capi.rows_linear_f32(x, w, b, relu=True, out=out)                                              # noqa: E731
        vendor = lambda: torch.relu_(F.linear(x, w, b))                                                                  # noqa: E731
    else:
        kernel = lambda: _capi.rows_linear_f32(x, w, b, out=out)                                                         # noqa: E731
        vendor = lambda: F.linear(x, w, b)                                                                               # noqa: E731
    with torch.no_grad():
        fns = {'f32_mfma_kernel': kernel, 'vendor_gemm_and_passes': vendor}
        if module is not None:
            fns['module_f32_route'] = module
        t = interleaved(fns, steps, warmup)
    floor_ms = 2.0 * rows * I * O / (PEAK_F32_MATRIX_TFLOPS * 1e12) * 1e3
    return {'layer': name, 'rows': rows, 'in': I, 'out': O, 'kind': kind, **t, 'compute_floor_ms': round(floor_ms, 5),
            'fraction_of_floor_reached': round(floor_ms / t['f32_mfma_kernel']['p50_ms'], 4),
            'kernel_over_vendor': round(t['f32_mfma_kernel']['p50_ms'] / t['vendor_gemm_and_passes']['p50_ms'], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--config', default='BL2')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--levels', type=int, default=4)
    ap.add_argument('--only', default=None, help='run the step in this one mode only (for a kernel trace); no JSON line')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing to measure')
    dev = torch.device('cuda:0')
    first = RL.mode()
    ds = {}
    for k in ([a.only] if a.only else RL.MODES):
        RL.set_mode(k)                         # before the model's first forward: a trace of one mode holds that route's kernels only
        ds[k] = S.fb_path_step(a.config, a.batch, a.levels, dev, train=False)      # seeded: the same parameters and inputs in every copy
    d = ds[a.only or 'x3']

    def step_in(mode):
        m, cam, ctx, depth, mlvl = (ds[mode][n] for n in ('model', 'cam', 'ctx', 'depth', 'mlvl'))

        def fn():
            RL.set_mode(mode)
            return m(cam, ctx, depth, mlvl_feats=mlvl)
        return fn
    try:
        with torch.no_grad():
            if a.only:
                fn = step_in(a.only)
                for _ in range(a.warmup + a.steps):
                    fn()
                torch.cuda.synchronize()
                return
            ref = {k: step_in(k)().float().clone() for k in RL.MODES}
            t = interleaved({k: step_in(k) for k in RL.MODES}, a.steps, a.warmup)
    finally:
        RL.set_mode(first)
    res = {'workload': f'fb_projection inference step {a.config} B={a.batch} L={a.levels}', 'steps': a.steps, 'warmup': a.warmup,
           'modes': t,
           'f32_mfma_over_f32': round(t['f32_mfma']['p50_ms'] / t['f32']['p50_ms'], 4),
           'f32_mfma_over_x3': round(t['f32_mfma']['p50_ms'] / t['x3']['p50_ms'], 4),
           'max_abs_diff_vs_f32_mfma': {k: float((ref[k] - ref['f32_mfma']).abs().max()) for k in ('x3', 'f32')},
           'output_scale': float(ref['f32_mfma'].abs().max()),
           'note': 'one model copy per mode (no weight cache is rebuilt inside a timed step); every step ends in a device '
                   'synchronise (all modes): absolute times sit a little above bench.py\'s'}
    X, Y, _ = d['pc'].grid_xyz
    rows = a.batch * X * Y
    tokens = a.batch * d['pc'].n_cams * sum(h * w for h, w in d['shapes'])
    del d, ds, ref
    torch.cuda.empty_cache()
    res['layers'] = [time_layer(dev, *c, a.steps, a.warmup) for c in layer_cases(dev, rows, tokens)]
    res['layers_sum_ms'] = {k: round(sum(l[k]['p50_ms'] for l in res['layers']), 4) for k in ('f32_mfma_kernel', 'vendor_gemm_and_passes')}
    res['layers_sum_ms']['module_f32_route'] = round(sum(l.get('module_f32_route', l['vendor_gemm_and_passes'])['p50_ms'] for l in res['layers']), 4)
    res['peak_f32_matrix_tflops'] = PEAK_F32_MATRIX_TFLOPS
    print(json.dumps(res))


if __name__ == '__main__':
    main()
