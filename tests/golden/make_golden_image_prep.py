#!/usr/bin/env python3
"""Fixture for the camera-frames step: run the REAL PrepareImageInputs (mmdet3d/datasets/pipelines/loading.py:988-1312) with the
REAL PIL on the small sources of tests/image_prep_cases.py.

The module file is loaded by path with the inert stand-ins of make_golden_points_depth.py for mmcv / mmdet / mmdet3d.core / cv2 /
torchvision -- but `PIL.Image` is the installed one, and `Image.open` is patched to serve `Image.fromarray` of the case's source
(JPEG decoding is not part of what is pinned).  Two stand-ins carry arithmetic:
  * `pyquaternion.Quaternion`, as in make_golden_points_depth.py (the info dict holds dyadic unit quaternions, for which any
    correct quaternion -> matrix formula is exact);
  * `mmcv.image.photometric.imnormalize`: neither mmcv nor cv2 is installed where this runs, so it is served by
    (float32(img[..., ::-1] if to_rgb else img) - float32(mean)) * float32(1 / float64(std)), the arithmetic of include/fbbev.h.
The fixture therefore pins everything EXCEPT these two.

Writes tests/golden/image_prep_ref.npz:
  source.<kind>.<Hs>x<Ws>             the sources (image i of a case is its source rolled by 3 i rows and 5 i columns: frames_of)
  <case>.augs / .canvas               img_transform_core per fixture case of tests/image_prep_cases.py
  aug.train / aug.test                sample_augmentation under np.random.seed(s), s in AUG_SEEDS: (seeds, 9) rows
  get_inputs.*                        one whole get_inputs (is_train, seed GET_INPUTS_SEED, 5 of 6 cameras) on info_dict()
  pil_version
The archive is written with fixed time stamps: the same inputs give the same bytes.

Run in the build container:  python tests/golden/make_golden_image_prep.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import make_golden as MG  # noqa: E402
import image_prep_cases as C  # noqa: E402
from make_golden_points_depth import Quaternion as _Q  # noqa: E402


class Quaternion(_Q):
    def __init__(self, *q):
        super().__init__(q[0] if len(q) == 1 else q)


def imnormalize(img, mean, std, to_rgb=True):
    """stand-in for mmcv.image.photometric.imnormalize (a float32 copy, cv2.cvtColor BGR2RGB, subtract, multiply by 1 / std)"""
    img = img.copy().astype(np.float32)
    stdinv = (1 / np.float64(std.reshape(1, -1))).astype(np.float32)
    if to_rgb:
        img = img[..., ::-1]
    out = (img - mean.reshape(1, -1).astype(np.float32)) * stdinv
    assert out.dtype == np.float32
    return np.ascontiguousarray(out)


def save(path, arrays):
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    import PIL
    from PIL import Image
    MG.install_stubs()

    class _Base(object):
        pass
    MG._mod('pyquaternion', Quaternion=Quaternion)
    MG._mod('mmcv.image'); MG._mod('mmcv.image.photometric', imnormalize=imnormalize)
    MG._mod('mmdet3d.core'); MG._mod('mmdet3d.core.points', BasePoints=None, get_points_type=None)
    MG._mod('mmdet3d.core.bbox', LiDARInstance3DBoxes=None)
    MG._mod('mmdet.datasets'); MG._mod('mmdet.datasets.pipelines', LoadAnnotations=_Base, LoadImageFromFile=_Base)
    MG._mod('mmdet3d.datasets'); MG._mod('mmdet3d.datasets.builder', PIPELINES=MG._Registry())
    pk = MG._mod('mmdet3d.datasets.pipelines')
    pk.__path__ = []
    MG._mod('torchvision'); MG._mod('torchvision.transforms'); MG._mod('torchvision.transforms.functional', rotate=None)
    ref = MG.load_ref('mmdet3d.datasets.pipelines.loading', 'mmdet3d/datasets/pipelines/loading.py')
    assert ref.Image is Image
    out = {'pil_version': np.array(PIL.__version__)}

    step = ref.PrepareImageInputs(C.DATA_CONFIG)
    for case in C.FIXTURE_CASES:
        fr = C.frames_of(case)
        cv = np.stack([np.array(step.img_transform_core(Image.fromarray(fr[i]), resize_dims=a[1], crop=a[2], flip=a[3], rotate=a[4]))
                       for i, a in enumerate(case['augs'])])
        assert cv.shape == (len(case['augs']), case['fH'], case['fW'], 3) and cv.dtype == np.uint8
        name = case['name']
        out[f'source.{case["kind"]}.{case["Hs"]}x{case["Ws"]}'] = C.source(case['kind'], case['Hs'], case['Ws'])
        out[f'{name}.augs'], out[f'{name}.canvas'] = C.augs_array(case['augs']), cv
        print(name, cv.shape, 'zero bytes', int((cv == 0).sum()), '255 bytes', int((cv == 255).sum()))

    for is_train in (True, False):
        step = ref.PrepareImageInputs(C.DATA_CONFIG, is_train=is_train)
        rows = []
        for seed in C.AUG_SEEDS:
            np.random.seed(seed)
            rows.append(C.augs_array([step.sample_augmentation(H=90, W=160)])[0])
        out['aug.train' if is_train else 'aug.test'] = np.stack(rows)

    frames = C.pipeline_frames()
    real_open = Image.open
    Image.open = lambda path: Image.fromarray(frames[path])
    try:
        step = ref.PrepareImageInputs(C.DATA_CONFIG, is_train=True)
        np.random.seed(C.GET_INPUTS_SEED)
        results = dict(curr=C.info_dict())
        (imgs, rots, trans, intrins, post_rots, post_trans), (sensor2egos, ego2globals) = step.get_inputs(results)
    finally:
        Image.open = real_open
    names = [str(n) for n in results['cam_names']]
    out['get_inputs.cam_names'] = np.array(names)
    out['get_inputs.augs'] = C.augs_array([results['img_augs'][n] for n in names])
    out['get_inputs.canvas'] = np.stack(results['canvas'])
    for key, t in (('imgs', imgs), ('rots', rots), ('trans', trans), ('intrins', intrins), ('post_rots', post_rots),
                   ('post_trans', post_trans), ('sensor2egos', sensor2egos), ('ego2globals', ego2globals),
                   ('sensor2sensors', results['sensor2sensors'])):
        assert t.dtype == torch.float32
        out[f'get_inputs.{key}'] = t.numpy()
    print('get_inputs', names, tuple(imgs.shape))
    path = os.path.join(MG.OUT, 'image_prep_ref.npz')
    save(path, out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
