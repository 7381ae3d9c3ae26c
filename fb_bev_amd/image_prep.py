"""Camera frames -> network input: the reference's PrepareImageInputs (mmdet3d/datasets/pipelines/loading.py:988-1312) without PIL
and without the CPU.

The reference resizes, crops, flips and rotates every frame with PIL and normalises it with mmcv, on the host.  Every pixel of that
chain is integer arithmetic on tables the host builds in float64, so it can be equalled bit for bit:

  img.resize(resize_dims)      bicubic, the support stretched by the downscale factor; two 8-bit passes (horizontal, then vertical)
                               with 22-bit fixed-point coefficients: v = clamp((2^21 + sum_k tap_k * p_k) >> 22, 0, 255) per pass
  img.crop(crop)               zeros outside the resized image
  transpose(FLIP_LEFT_RIGHT)
  img.rotate(rotate)           nearest neighbour, a 16.16 fixed-point affine walk, black fill
  imnormalize(., to_rgb)       (float32(v) - mean) * (1 / std) in fp32 after the channel swap

  sample_augmentation(...)     the reference's draw, in its order from np.random
  post_transform(...)          post_rot (3, 3), post_tran (3,) of img_transform
  resample_table(...)          PIL's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter, float64, cached
  rotate_fixed(w, h, angle)    Image.rotate's matrix as the six 16.16 integers of PIL's affine_fixed
  build_plan(...)              per-image records + tables as ONE int32 host tensor (layout: include/fbbev.h), validated
  prepare_images(...)          GPU: fbbev_image_prep, one launch for all frames.  CPU tensors are refused: there is no fallback
  prepare_images_reference     the numpy restatement: THE DEFINITION the kernel is held to
  PrepareImageInputs           the pipeline step under its reference name; frames come decoded in results['frames'][cam_name]

This module does not import PIL.  What is NOT pinned against the reference's own code: mmcv.image.photometric.imnormalize (neither
mmcv nor cv2 is available where the fixture is made; tests/golden/make_golden_image_prep.py serves it by a stand-in with the
arithmetic above) and pyquaternion (as in points_depth).
"""
import functools
import math

import numpy as np
import torch

from .points_depth import quaternion_rotation_matrix

__all__ = ['sample_augmentation', 'post_transform', 'resample_table', 'rotate_fixed', 'build_plan', 'prepare_images',
           'prepare_images_reference', 'transform_reference', 'normalize_reference', 'norm_constants', 'PrepareImageInputs',
           'PIPELINES', 'build_pipeline_step', 'limits', 'NORMALIZE_CFG', 'PLAN_REC']

NORMALIZE_CFG = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True, debug=False)
PRECISION_BITS = 32 - 8 - 2
PLAN_REC = 16                    # int32 words of a plan record (FBBEV_IP_REC)
# the kernel's tile and LDS plan (fbbev_image_prep_limits returns the same numbers; tests/test_image_prep_abi.py holds them together):
# a launch must not need the library to PLAN, so that a loader worker without a GPU can build plans
LIMITS = dict(tile_w=64, tile_h=16, max_taps=20, max_box_w=72, max_box_h=32, max_src_rows=152, max_src_cols=336)


def limits():
    return dict(LIMITS)


# ---------------------------------------------------------------------------------------------------------------- augmentation
def sample_augmentation(data_config, H, W, is_train, flip=None, scale=None):
    """loading.py:1064-1089 -> (resize, resize_dims, crop, flip, rotate); draws from np.random in the reference's order"""
    fH, fW = data_config['input_size']
    if is_train:
        resize = float(fW) / float(W)
        resize += np.random.uniform(*data_config['resize'])
        resize_dims = (int(W * resize), int(H * resize))
        newW, newH = resize_dims
        crop_h = int((1 - np.random.uniform(*data_config['crop_h'])) * newH) - fH
        crop_w = int(np.random.uniform(0, max(0, newW - fW)))
        crop = (crop_w, crop_h, crop_w + fW, crop_h + fH)
        flip = data_config['flip'] and np.random.choice([0, 1])
        rotate = np.random.uniform(*data_config['rot'])
    else:
        resize = float(fW) / float(W)
        resize += data_config.get('resize_test', 0.0)
        if scale is not None:
            resize = scale
        resize_dims = (int(W * resize), int(H * resize))
        newW, newH = resize_dims
        crop_h = int((1 - np.mean(data_config['crop_h'])) * newH) - fH
        crop_w = int(max(0, newW - fW) / 2)
        crop = (crop_w, crop_h, crop_w + fW, crop_h + fH)
        flip = False if flip is None else flip
        rotate = 0
    return resize, resize_dims, crop, flip, rotate


def post_transform(resize, crop, flip, rotate):
    """img_transform's homography (loading.py:1028-1040) and its 3 x 3 form (:1236-1239), with the same torch ops"""
    post_rot = torch.eye(2)
    post_tran = torch.zeros(2)
    post_rot *= resize
    post_tran -= torch.Tensor(crop[:2])
    if flip:
        A = torch.Tensor([[-1, 0], [0, 1]])
        b = torch.Tensor([crop[2] - crop[0], 0])
        post_rot = A.matmul(post_rot)
        post_tran = A.matmul(post_tran) + b
    h = rotate / 180 * np.pi
    A = torch.Tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])
    b = torch.Tensor([crop[2] - crop[0], crop[3] - crop[1]]) / 2
    b = A.matmul(-b) + b
    post_rot = A.matmul(post_rot)
    post_tran = A.matmul(post_tran) + b
    rot3, tran3 = torch.eye(3), torch.zeros(3)
    tran3[:2] = post_tran
    rot3[:2, :2] = post_rot
    return rot3, tran3


# ---------------------------------------------------------------------------------------------------------------- tables
def _bicubic(x):
    """PIL's bicubic_filter (a = -0.5) on a float64 array, in its order of operations"""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


@functools.lru_cache(maxsize=256)
def resample_table(in_size, out_size, first, count):
    """Outputs first .. first + count - 1 of PIL's bicubic resampling of in_size samples to out_size (precompute_coeffs +
    normalize_coeffs_8bpc) -> (xmin (count,), n (count,), taps (count, ksize)) int32, read-only.  Output i reads input samples
    xmin[i] .. xmin[i] + n[i] - 1 with taps[i, :n[i]]; taps behind n[i] are 0.  An output outside 0 .. out_size - 1 (the crop
    window reaches past the resized image: PIL pads with zeros) has n = 0, and its xmin continues the valid ones so that xmin and
    xmin + n never decrease along the table."""
    in_size, out_size, first, count = int(in_size), int(out_size), int(first), int(count)
    if in_size < 1 or out_size < 1 or count < 0:
        raise ValueError(f'resample_table({in_size}, {out_size}, {first}, {count})')
    scale = float(np.float32(in_size) - np.float32(0)) / out_size           # (double)(in1 - in0) / outSize, the box held as floats
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xx = np.arange(first, first + count, dtype=np.int64)
    valid = (xx >= 0) & (xx < out_size)
    center = 0.0 + (xx + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)         # (int): towards zero; negative values are clipped anyway
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    k = np.zeros((count, ksize), np.float64)
    ww = np.zeros(count, np.float64)
    for x in range(ksize):                                                   # ww += w in tap order, as the C loop
        w = np.where(x < n, _bicubic((x + xmin - center + 0.5) * ss), 0.0)
        k[:, x] = w
        ww = ww + w
    nz = ww != 0.0
    k[nz] = k[nz] / ww[nz, None]
    taps = np.where(k < 0, (-0.5 + k * (1 << PRECISION_BITS)).astype(np.int64), (0.5 + k * (1 << PRECISION_BITS)).astype(np.int64))
    taps[~valid] = 0
    n = np.where(valid, n, 0)
    if valid.any():
        i0, i1 = int(np.argmax(valid)), count - 1 - int(np.argmax(valid[::-1]))
        xmin[:i0] = xmin[i0]
        xmin[i1 + 1:] = xmin[i1] + n[i1]
    else:
        xmin[:] = 0
    out = tuple(a.astype(np.int32) for a in (xmin, n, taps))
    for a in out:
        a.setflags(write=False)
    return out


def _fix(v):
    """PIL's FIX: FLOOR(v * 65536 + 0.5), FLOOR = floor below zero and truncation above"""
    v = v * 65536.0 + 0.5
    return int(math.floor(v)) if v < 0.0 else int(v)


def rotate_fixed(w, h, angle):
    """Image.rotate(angle) of a w x h image (nearest, no expand, centre (w / 2, h / 2)) as PIL's affine_fixed integers
    (a0 .. a5): output pixel (x, y) reads input (xin, yin) = ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16), black outside.
    Angles PIL serves by a copy (0) or a transpose (180) are written as the affine that gives the same pixels."""
    w, h = int(w), int(h)
    angle = float(angle) % 360.0
    if angle == 0:
        return (65536, 0, 32768, 0, 65536, 32768)
    if angle == 180:
        return (-65536, 0, w * 65536 - 32768, 0, -65536, h * 65536 - 32768)
    if angle in (90, 270) and w == h:
        raise ValueError('a quarter turn of a square image is a transpose in PIL, not an affine walk: not planned')
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    if m[1] == 0 and m[3] == 0:
        raise ValueError(f'rotation by {angle!r} rad: PIL takes its scaling route, not the affine walk')
    for x, y in ((0, 0), (w, h), (0, h), (w, 0)):                            # check_fixed
        if not (abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0):
            raise ValueError('image too large for the 16.16 fixed-point walk')
    return (_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


# ---------------------------------------------------------------------------------------------------------------- plan
def _check_aug(aug, Hs, Ws, fH, fW):
    resize, resize_dims, crop, flip, rotate = aug
    newW, newH = (int(v) for v in resize_dims)
    crop = tuple(int(v) for v in crop)
    if newW < 1 or newH < 1:
        raise ValueError(f'resize_dims {resize_dims} must be positive')
    if crop[2] - crop[0] != fW or crop[3] - crop[1] != fH:
        raise ValueError(f'crop {crop} is not {fW} x {fH}')
    if Hs > 100 * Ws and newH < Hs:
        raise ValueError('PIL resizes an image more than 100 times taller than wide in the other order: not planned')
    return newW, newH, crop, bool(flip), float(rotate)


def _tile_need(a, flip, ht, vt, fH, fW):
    """the largest footprint of a tile of the image: (taps, box_w, box_h, src_rows, src_cols), as the kernel computes them"""
    L = LIMITS
    a0, a1, a2, a3, a4, a5 = a
    x0 = np.arange(0, fW, L['tile_w'], dtype=np.int64)
    y0 = np.arange(0, fH, L['tile_h'], dtype=np.int64)
    x1, y1 = np.minimum(x0 + L['tile_w'], fW) - 1, np.minimum(y0 + L['tile_h'], fH) - 1
    xs = np.stack([x0, x1, x0, x1])[:, None, :]                                  # (4, 1, tx)
    ys = np.stack([y0, y0, y1, y1])[:, :, None]                                  # (4, ty, 1)
    xin, yin = (a2 + ys * a1 + xs * a0) >> 16, (a5 + ys * a4 + xs * a3) >> 16
    bx0, bx1 = np.maximum(xin.min(0), 0), np.minimum(xin.max(0), fW - 1)
    by0, by1 = np.maximum(yin.min(0), 0), np.minimum(yin.max(0), fH - 1)
    ok = (bx1 >= bx0) & (by1 >= by0)
    if not ok.any():
        return 0, 0, 0, 0, 0
    bx0, bx1, by0, by1 = bx0[ok], bx1[ok], by0[ok], by1[ok]
    wc0, wc1 = (fW - 1 - bx1, fW - 1 - bx0) if flip else (bx0, bx1)
    cols = (ht[0][wc1].astype(np.int64) + ht[1][wc1]) - ht[0][wc0]
    rows = (vt[0][by1].astype(np.int64) + vt[1][by1]) - vt[0][by0]
    taps = max(int(ht[1].max(initial=0)), int(vt[1].max(initial=0)))
    return taps, int((bx1 - bx0 + 1).max()), int((by1 - by0 + 1).max()), int(rows.max()), int(cols.max())


def build_plan(augs, Hs, Ws, fH, fW):
    """augs: per image (resize, resize_dims, crop, flip, rotate) as sample_augmentation returns them -> (plan, need): plan the int32
    host tensor of fbbev_image_prep (n records of PLAN_REC words, then the tables; pinned where CUDA is available), need the five
    host-side numbers (taps, box_w, box_h, src_rows, src_cols) the entry holds against the kernel's limits.  ValueError when a tap
    window leaves the source, a table is not monotone, or a limit does not hold."""
    Hs, Ws, fH, fW = int(Hs), int(Ws), int(fH), int(fW)
    if min(Hs, Ws, fH, fW) < 1 or max(fH, fW) >= 16384:
        raise ValueError(f'source {Hs} x {Ws}, output {fH} x {fW}')
    n = len(augs)
    words = [np.zeros(n * PLAN_REC, np.int32)]
    at = n * PLAN_REC
    where = {}
    need = [0, 0, 0, 0, 0]

    def table(in_size, out_size, first, count):
        nonlocal at
        key = (in_size, out_size, first, count)
        if key not in where:
            xmin, cnt, taps = resample_table(*key)
            end = xmin.astype(np.int64) + cnt
            if (xmin < 0).any() or (end > in_size).any() or (np.diff(xmin) < 0).any() or (np.diff(end) < 0).any():
                raise ValueError(f'resample_table{key}: a tap window leaves the source or the table is not monotone')
            where[key] = (at, taps.shape[1])
            words.extend([xmin, cnt, taps.reshape(-1)])
            at += 2 * count + taps.size
        return where[key]

    for i, aug in enumerate(augs):
        newW, newH, crop, flip, rotate = _check_aug(aug, Hs, Ws, fH, fW)
        a = rotate_fixed(fW, fH, rotate)
        hk, vk = (Ws, newW, crop[0], fW), (Hs, newH, crop[1], fH)
        (hoff, hks), (voff, vks) = table(*hk), table(*vk)
        got = _tile_need(a, flip, resample_table(*hk), resample_table(*vk), fH, fW)
        need = [max(p, q) for p, q in zip(need, got)]
        words[0][i * PLAN_REC:(i + 1) * PLAN_REC] = [newW, newH, int(flip), 0, *a, hoff, voff, hks, vks, 0, 0]
    L = LIMITS
    for name, v, lim in zip(('taps', 'box width', 'box height', 'source rows', 'source columns'), need,
                            (L['max_taps'], L['max_box_w'], L['max_box_h'], L['max_src_rows'], L['max_src_cols'])):
        if v > lim:
            raise ValueError(f'a tile needs {v} {name}, the kernel holds {lim}: outside the route (resize 0.25 .. 2, |rotate| <= 10 degrees)')
    flat = np.concatenate(words) if words else np.zeros(0, np.int32)
    plan = torch.empty(flat.size, dtype=torch.int32, pin_memory=torch.cuda.is_available())
    plan.numpy()[:] = flat
    return plan, tuple(need)


# ---------------------------------------------------------------------------------------------------------------- restatement
def _pass(src, xmin, cnt, taps, axis, stats):
    """one 8-bit resampling pass along `axis` of an (R, C, 3) uint8 array -> uint8 with len(xmin) samples on that axis"""
    src = np.moveaxis(src, axis, 0).astype(np.int64)
    acc = np.full((len(xmin),) + src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for k in range(taps.shape[1]):
        idx = np.minimum(xmin.astype(np.int64) + k, src.shape[0] - 1)         # taps behind cnt are 0: the index only has to exist
        acc += src[idx] * taps[:, k].astype(np.int64)[:, None, None]
    acc >>= PRECISION_BITS
    if stats is not None:
        stats['lo'], stats['hi'] = min(stats.get('lo', 0), int(acc.min())), max(stats.get('hi', 255), int(acc.max()))
    return np.moveaxis(np.clip(acc, 0, 255).astype(np.uint8), 0, axis)


def transform_reference(src, aug, fH=None, fW=None, stats=None):
    """img_transform_core restated: (Hs, Ws, 3) uint8 -> (fH, fW, 3) uint8, what np.array(img) holds after PIL's resize, crop,
    transpose and rotate.  Only the crop window of the resized image is computed (from the source rows it needs).  stats: a dict
    that receives the smallest and largest unclamped value of the two passes (`lo`, `hi`)."""
    src = np.ascontiguousarray(src)
    Hs, Ws = src.shape[:2]
    crop = aug[2]
    fW = int(crop[2] - crop[0]) if fW is None else fW
    fH = int(crop[3] - crop[1]) if fH is None else fH
    newW, newH, crop, flip, rotate = _check_aug(aug, Hs, Ws, fH, fW)
    hx, hn, ht = resample_table(Ws, newW, crop[0], fW)
    vx, vn, vt = resample_table(Hs, newH, crop[1], fH)
    r0, r1 = int(vx[0]), int(vx[-1]) + int(vn[-1])
    rows = src[r0:max(r1, r0 + 1)] if r1 > r0 else src[:1]
    win = _pass(rows, hx, hn, ht, 1, stats)
    win = _pass(win, np.maximum(vx - r0, 0) if r1 > r0 else vx * 0, vn, vt, 0, stats)
    if flip:
        win = win[:, ::-1]
    a0, a1, a2, a3, a4, a5 = rotate_fixed(fW, fH, rotate)
    y, x = np.meshgrid(np.arange(fH, dtype=np.int64), np.arange(fW, dtype=np.int64), indexing='ij')
    xin, yin = (a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16
    inside = (xin >= 0) & (xin < fW) & (yin >= 0) & (yin < fH)
    out = np.zeros((fH, fW, 3), np.uint8)
    out[inside] = win[yin[inside], xin[inside]]
    return out


def norm_constants(normalize_cfg=None):
    """-> (mean (3,), inv_std (3,)) float32: mean = float32(mean), inv_std = float32(1 / float64(float32(std))), what imnormalize
    makes of the reference's float32 arrays"""
    cfg = NORMALIZE_CFG if normalize_cfg is None else normalize_cfg
    mean = np.array(cfg['mean'], dtype=np.float32)
    std = np.array(cfg['std'], dtype=np.float32)
    return mean, (1.0 / np.float64(std)).astype(np.float32)


def normalize_reference(canvas, normalize_cfg=None):
    """(..., fH, fW, 3) uint8 -> (..., 3, fH, fW) float32: out[c] = (float32(v[2 - c if to_rgb else c]) - mean[c]) * inv_std[c]"""
    cfg = NORMALIZE_CFG if normalize_cfg is None else normalize_cfg
    mean, inv = norm_constants(cfg)
    v = canvas[..., ::-1] if cfg.get('to_rgb', True) else canvas
    out = (v.astype(np.float32) - mean) * inv
    assert out.dtype == np.float32
    return np.ascontiguousarray(np.moveaxis(out, -1, -3))


def prepare_images_reference(frames, augs, normalize_cfg=None, canvas=False):
    """THE DEFINITION the kernel is held to: the numpy restatement of img_transform_core + mmlabNormalize.  frames (n, Hs, Ws, 3)
    uint8 (array or tensor), augs per image -> imgs (n, 3, fH, fW) float32 numpy [, canvas (n, fH, fW, 3) uint8].  Equal, bit for
    bit, to PIL on the uint8 side (tests/test_image_prep_host.py); for scoring saved frames on a host and for the tests."""
    frames = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    cv = np.stack([transform_reference(frames[i], augs[i]) for i in range(len(augs))])
    imgs = normalize_reference(cv, normalize_cfg)
    return (imgs, cv) if canvas else imgs


# ---------------------------------------------------------------------------------------------------------------- GPU route
def prepare_images(frames, augs, normalize_cfg=None, channels_last=False, canvas=False, plan=None):
    """frames (n, Hs, Ws, 3) uint8 on the GPU (a view with a larger image stride is read in place), augs per image -> imgs
    (n, 3, fH, fW) float32 (channels-last strides when asked) [, canvas (n, fH, fW, 3) uint8].  One H2D copy of the plan, one
    launch.  plan: a (plan, need) pair from build_plan to reuse (the test pipeline's never changes).  _capi.FbbevError on CPU
    tensors or when the route declines; there is no fallback."""
    from . import _capi
    if not isinstance(frames, torch.Tensor):
        raise _capi.FbbevError('frames must be a uint8 tensor on the GPU')
    _capi.require_gpu(frames, 'frames')
    if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8 or frames.shape[0] != len(augs):
        raise _capi.FbbevError(f'frames must be ({len(augs)}, Hs, Ws, 3) uint8, got {frames.dtype} {tuple(frames.shape)}')
    cfg = NORMALIZE_CFG if normalize_cfg is None else normalize_cfg
    if cfg.get('debug', False):
        raise _capi.FbbevError('normalize_cfg debug=True (no normalisation) is not part of the route')
    n, Hs, Ws = (int(v) for v in frames.shape[:3])
    if n == 0:
        raise _capi.FbbevError('no frames')
    crop = augs[0][2]
    fH, fW = int(crop[3] - crop[1]), int(crop[2] - crop[0])
    try:
        host, need = build_plan(augs, Hs, Ws, fH, fW) if plan is None else plan
    except ValueError as e:
        raise _capi.FbbevError(f'fbbev_image_prep declines: {e}') from e
    mean, inv = norm_constants(cfg)
    return _capi.image_prep(frames, host.to(frames.device, non_blocking=True), need, fH, fW, mean, inv, bool(cfg.get('to_rgb', True)),
                            bool(channels_last), bool(canvas))


# ---------------------------------------------------------------------------------------------------------------- pipeline step
def _rigid44(rotation, translation):
    m = torch.zeros((4, 4))
    m[3, 3] = 1
    m[:3, :3] = torch.Tensor(quaternion_rotation_matrix(rotation))
    m[:3, -1] = torch.Tensor(translation)
    return m


class PrepareImageInputs(object):
    """The reference's pipeline step (loading.py:988-1312).  The decoded frames come in results['frames'][cam_name] (uint8 HWC
    tensors or arrays, on the device or on the host; JPEG decoding stays the caller's); frames on the GPU take the kernel, host
    frames the restatement.  get_inputs returns the reference's two tuples and sets cam_names, img_augs, canvas, sensor2sensors."""

    def __init__(self, data_config, is_train=False, sequential=False, ego_cam='CAM_FRONT', normalize_cfg=NORMALIZE_CFG):
        if sequential:
            raise NotImplementedError('sequential=True (adjacent frames) is not part of this library; no fb_occ config sets it')
        self.is_train = is_train
        self.data_config = data_config
        self.sequential = sequential
        self.ego_cam = ego_cam
        self.normalize_cfg = normalize_cfg

    def choose_cams(self):
        if self.is_train and self.data_config['Ncams'] < len(self.data_config['cams']):
            return np.random.choice(self.data_config['cams'], self.data_config['Ncams'], replace=False)
        return self.data_config['cams']

    def sample_augmentation(self, H, W, flip=None, scale=None):
        return sample_augmentation(self.data_config, H, W, self.is_train, flip=flip, scale=scale)

    def get_sensor2ego_transformation(self, cam_info, key_info, cam_name, ego_cam=None):
        if ego_cam is None:
            ego_cam = cam_name
        cam, key = cam_info['cams'][cam_name], key_info['cams'][cam_name]
        sweepsensor2sweepego = _rigid44(cam['sensor2ego_rotation'], cam['sensor2ego_translation'])
        sweepego2global = _rigid44(cam['ego2global_rotation'], cam['ego2global_translation'])
        ego = key_info['cams'][ego_cam]
        global2keyego = _rigid44(ego['ego2global_rotation'], ego['ego2global_translation']).inverse()
        sweepsensor2keyego = global2keyego @ sweepego2global @ sweepsensor2sweepego
        global2keyego = _rigid44(key['ego2global_rotation'], key['ego2global_translation']).inverse()
        keyego2keysensor = _rigid44(key['sensor2ego_rotation'], key['sensor2ego_translation']).inverse()
        keysensor2sweepsensor = (keyego2keysensor @ global2keyego @ sweepego2global @ sweepsensor2sweepego).inverse()
        return sweepsensor2keyego, keysensor2sweepsensor

    def get_sensor_transforms(self, cam_info, cam_name):
        cam = cam_info['cams'][cam_name]
        return (_rigid44(cam['sensor2ego_rotation'], cam['sensor2ego_translation']),
                _rigid44(cam['ego2global_rotation'], cam['ego2global_translation']))

    def get_inputs(self, results, scale=None):
        rots, trans, intrins, post_rots, post_trans, sensor2egos, ego2globals, sensor2sensors, frames, augs = ([] for _ in range(10))
        cam_names = self.choose_cams()
        results['cam_names'] = cam_names
        results['img_augs'] = {}
        for cam_name in cam_names:
            cam_data = results['curr']['cams'][cam_name]
            frame = results['frames'][cam_name]
            frame = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frame))
            sensor2keyego, sensor2sensor = self.get_sensor2ego_transformation(results['curr'], results['curr'], cam_name, self.ego_cam)
            sensor2ego, ego2global = self.get_sensor_transforms(results['curr'], cam_name)
            flip = results['tta_config']['tta_flip'] if results.get('tta_config', None) is not None else None
            aug = self.sample_augmentation(H=int(frame.shape[0]), W=int(frame.shape[1]), flip=flip, scale=scale)
            resize, resize_dims, crop, flip, rotate = aug
            results['img_augs'][cam_name] = aug
            post_rot, post_tran = post_transform(resize, crop, flip, rotate)
            frames.append(frame)
            augs.append(aug)
            intrins.append(torch.Tensor(cam_data['cam_intrinsic']))
            rots.append(sensor2keyego[:3, :3])
            trans.append(sensor2keyego[:3, 3])
            post_rots.append(post_rot)
            post_trans.append(post_tran)
            sensor2sensors.append(sensor2sensor)
            sensor2egos.append(sensor2ego)
            ego2globals.append(ego2global)
        stacked = torch.stack(frames)
        if stacked.is_cuda:
            imgs, canvas = prepare_images(stacked, augs, normalize_cfg=self.normalize_cfg, canvas=True)
            results['canvas'] = list(canvas.cpu().numpy())
        else:
            imgs, canvas = prepare_images_reference(stacked, augs, normalize_cfg=self.normalize_cfg, canvas=True)
            imgs = torch.from_numpy(imgs)
            results['canvas'] = list(canvas)
        results['sensor2sensors'] = torch.stack(sensor2sensors)
        return ((imgs, torch.stack(rots), torch.stack(trans), torch.stack(intrins), torch.stack(post_rots), torch.stack(post_trans)),
                (torch.stack(sensor2egos), torch.stack(ego2globals)))

    def __call__(self, results):
        results['img_inputs'], results['aux_cam_params'] = self.get_inputs(results)
        return results


PIPELINES = {'PrepareImageInputs': PrepareImageInputs}


def build_pipeline_step(cfg):
    """dict(type='PrepareImageInputs', ...) -> the step"""
    cfg = dict(cfg)
    typ = cfg.pop('type')
    if typ not in PIPELINES:
        raise KeyError(f'pipeline step {typ!r} is not part of this library')
    return PIPELINES[typ](**cfg)
