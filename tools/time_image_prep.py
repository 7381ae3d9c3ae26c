#!/usr/bin/env python3
"""Time the camera-frames step (fbbev_image_prep) with HIP events, warm, in ONE process:
  24 frames of 900 x 1600 (B = 4, N = 6) -> 256 x 704, with training-range parameters (resize 0.38 .. 0.55, crop, flip, +-5.4
  degrees; seeded) and with the test pipeline's (0.44, centred crop, no flip, 0 degrees), into planes and into channels-last.
Per variant: p10 / p50 / p90 of single launches (an event pair each), the mean of 20 launches back to back under one event pair (the
event overhead shared by 20), the kernel's ALGORITHMIC bytes -- the source rows and columns the crop window actually needs, once,
plus the float output; not what the tiles re-read through the caches -- and the bytes/s that makes at the p50.  Beside them: the
host time of build_plan (wall clock; cold tables, and with the tables cached), the size of the plan, and, where PIL is importable,
the same 24 frames through PIL + numpy on one thread (wall clock, the reference's img_transform_core + the normalisation) as a stated
baseline.  The outputs of the two layouts are compared, and the first frames are held against the numpy restatement, before
anything is timed.  Needs a GPU: there is no fallback.

    python tools/time_image_prep.py [--out profiles/r26_image_prep.md] [--iters 200] [--warmup 20]
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
from fb_bev_amd import _capi, image_prep as IP  # noqa: E402

B, N, HS, WS, FH, FW = 4, 6, 900, 1600, 256, 704
DATA_CONFIG = dict(input_size=(FH, FW), resize=(-0.06, 0.11), rot=(-5.4, 5.4), flip=True, crop_h=(0.0, 0.0), resize_test=0.0)


def pct(us):
    us = np.array(us)
    return {k: round(float(np.percentile(us, q)), 2) for k, q in (('p10_us', 10), ('p50_us', 50), ('p90_us', 90))}


def time_launches(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    single = pct([a.elapsed_time(b) * 1e3 for a, b in ev])
    groups = []
    for _ in range(max(iters // 20, 5)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            fn()
        b.record()
        torch.cuda.synchronize()
        groups.append(a.elapsed_time(b) * 1e3 / 20)
    single['back_to_back_20_mean_us'] = round(float(np.median(groups)), 2)
    return single


def algorithmic_bytes(augs):
    src = 0
    for a in augs:
        newW, newH, crop = a[1][0], a[1][1], a[2]
        hx, hn, _ = IP.resample_table(WS, newW, crop[0], FW)
        vx, vn, _ = IP.resample_table(HS, newH, crop[1], FH)
        src += (int(vx[-1]) + int(vn[-1]) - int(vx[0])) * (int(hx[-1]) + int(hn[-1]) - int(hx[0])) * 3
    return src, len(augs) * 3 * FH * FW * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r26_image_prep.md'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_image_prep.py needs a GPU')
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(26)
    frames = torch.randint(0, 256, (B * N, HS, WS, 3), generator=g, dtype=torch.uint8)
    d_frames = frames.to(dev)
    np.random.seed(26)
    sets = {'train': [IP.sample_augmentation(DATA_CONFIG, HS, WS, True) for _ in range(B * N)],
            'test': [IP.sample_augmentation(DATA_CONFIG, HS, WS, False) for _ in range(B * N)]}
    mean, inv = IP.norm_constants()
    res = dict(device=torch.cuda.get_device_name(0), frames=B * N, source=[HS, WS], output=[FH, FW], iters=args.iters, warmup=args.warmup,
               limits=_capi.image_prep_limits(), variants={}, build_plan={})
    for name, augs in sets.items():
        IP.resample_table.cache_clear()
        t0 = time.perf_counter()
        plan, need = IP.build_plan(augs, HS, WS, FH, FW)
        cold = time.perf_counter() - t0
        warm = []
        for _ in range(20):
            t0 = time.perf_counter()
            IP.build_plan(augs, HS, WS, FH, FW)
            warm.append(time.perf_counter() - t0)
        res['build_plan'][name] = dict(cold_ms=round(cold * 1e3, 3), cached_tables_p50_ms=round(float(np.median(warm)) * 1e3, 3),
                                       plan_bytes=int(plan.numel()) * 4, need=list(need))
        d_plan = plan.to(dev)
        src_b, out_b = algorithmic_bytes(augs)
        outs = {}
        for cl in (False, True):
            out = torch.empty((B * N, 3, FH, FW), dtype=torch.float32, device=dev,
                              memory_format=torch.channels_last if cl else torch.contiguous_format)
            fn = lambda: _capi.image_prep(d_frames, d_plan, need, FH, FW, mean, inv, True, cl, False, out=out)  # noqa: E731
            fn()
            torch.cuda.synchronize()
            outs[cl] = out.clone()
            t = time_launches(fn, args.iters, args.warmup)
            t.update(source_bytes=src_b, output_bytes=out_b, gb_per_s_at_p50=round((src_b + out_b) / (t['p50_us'] * 1e-6) / 1e9, 1))
            res['variants'][f'{name}/{"channels_last" if cl else "planes"}'] = t
            print(name, 'channels_last' if cl else 'planes', t, flush=True)
        assert torch.equal(outs[False], outs[True]), 'the two layouts differ'
        want = IP.prepare_images_reference(frames[:2], augs[:2])
        assert np.array_equal(outs[False][:2].cpu().numpy().view(np.int32), want.view(np.int32)), 'the kernel differs from the restatement'
    try:
        from PIL import Image
        import PIL
        torch.set_num_threads(1)
        fr = frames.numpy()
        for name, augs in sets.items():
            t0 = time.perf_counter()
            for i, (resize, dims, crop, flip, rot) in enumerate(augs):
                img = Image.fromarray(fr[i]).resize(dims).crop(crop)
                if flip:
                    img = img.transpose(method=Image.FLIP_LEFT_RIGHT)
                IP.normalize_reference(np.array(img.rotate(rot)))
            res.setdefault('pil_one_thread_ms', {})[name] = round((time.perf_counter() - t0) * 1e3, 1)
        res['pil_version'] = PIL.__version__
    except ImportError:
        res['pil_one_thread_ms'] = 'PIL is not installed on this machine: not measured'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(os.path.splitext(args.out)[0] + '.json', 'w') as f:
        json.dump(res, f, indent=1)
    with open(args.out, 'w') as f:
        f.write('# fbbev_image_prep: 24 frames of 900 x 1600 to 256 x 704 in one launch\n\n')
        f.write(f'`tools/time_image_prep.py`, {res["device"]}, HIP events, {args.iters} timed launches after {args.warmup} warm-up; '
                f'outputs checked against the numpy restatement (bit equality) before timing.\n\n')
        f.write('| parameters / layout | p10 µs | p50 µs | p90 µs | 20 back to back, µs each | source bytes needed | output bytes | GB/s at p50 |\n')
        f.write('|---|---|---|---|---|---|---|---|\n')
        for k, t in res['variants'].items():
            f.write(f'| {k} | {t["p10_us"]} | {t["p50_us"]} | {t["p90_us"]} | {t["back_to_back_20_mean_us"]} | {t["source_bytes"]} | '
                    f'{t["output_bytes"]} | {t["gb_per_s_at_p50"]} |\n')
        f.write('\nThe bytes are algorithmic: the source rows and columns the crop windows need, counted once, plus the float output; '
                'neighbouring tiles re-read their shared source rows through the caches, which is not counted.\n\n')
        f.write('| build_plan (host, wall clock) | cold tables ms | cached tables p50 ms | plan bytes (one H2D copy) | need (taps, box w, box h, rows, cols) |\n')
        f.write('|---|---|---|---|---|\n')
        for k, t in res['build_plan'].items():
            f.write(f'| {k} | {t["cold_ms"]} | {t["cached_tables_p50_ms"]} | {t["plan_bytes"]} | {t["need"]} |\n')
        f.write(f'\nPIL + numpy on one thread, the same 24 frames (wall clock, ms): {res["pil_one_thread_ms"]}'
                f'{" (Pillow " + res["pil_version"] + ")" if "pil_version" in res else ""}\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
