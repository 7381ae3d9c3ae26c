"""fbbev_image_prep on the MI355X: the cases of tests/image_prep_cases.py through the C entry (the emulator test runs the same
checks), fb_bev_amd.image_prep on GPU tensors, and FBOCC(execution=dict(images_from_frames=True)).  Bit equality throughout: with the
numpy restatement and with the fixture the reference class wrote with PIL.  Neither PIL nor the reference tree is read here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_prep_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    return C.GpuApi()


def test_limits_are_the_planner_s(api):
    from fb_bev_amd import _capi, image_prep as IP
    assert C.limits_of(api) == IP.limits() == _capi.image_prep_limits()


@pytest.mark.parametrize('case', C.CASES, ids=C.CASE_IDS)
def test_cases(api, case):
    C.check(api, case)


@pytest.mark.parametrize('variant', C.VARIANTS[1:], ids=lambda v: 'cl%d_swap%d_canvas%d' % tuple(int(x) for x in v))
@pytest.mark.parametrize('name', C.VARIANT_CASES + ('full_train6',))
def test_layouts_swap_and_canvas(api, name, variant):
    C.check(api, C.by_name(name), *variant)


@pytest.mark.parametrize('name', ('batch7_strided', 'size_%dx%d' % (2 * C.TW + 3, 2 * C.TH + 3), 'full_train6'))
def test_two_runs_give_identical_bits(api, name):
    C.check_repeat(api, C.by_name(name))


def test_reference_fixture(api):
    C.check_fixture(api)


def test_module_routes_gpu_tensors_to_the_kernel(api):
    """prepare_images: planes and channels-last, with and without the canvas, a strided view of frames, a reused plan"""
    from fb_bev_amd import _capi, image_prep as IP
    case = C.by_name('batch7_strided')
    want, _ = C.expected(case)
    fr = torch.from_numpy(C.frames_of(case)).to(api.device)
    imgs, cv = IP.prepare_images(fr, case['augs'], canvas=True)
    assert imgs.shape == (7, 3, 25, 70) and imgs.is_contiguous() and np.array_equal(cv.cpu().numpy(), want)
    wf = C.expected_floats(want, True, False)
    assert np.array_equal(imgs.cpu().numpy().view(np.int32), wf.view(np.int32))
    assert np.array_equal(IP.prepare_images_reference(fr, case['augs']).view(np.int32), wf.view(np.int32))
    cl = IP.prepare_images(fr, case['augs'], channels_last=True)
    assert cl.shape == imgs.shape and cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(cl, imgs)
    wide = torch.zeros((7, 92, 160, 3), dtype=torch.uint8, device=api.device)
    wide[:, :90] = fr
    plan = IP.build_plan(case['augs'], 90, 160, 25, 70)
    again = IP.prepare_images(wide[:, :90], case['augs'], plan=plan)
    assert torch.equal(again, imgs)
    no_swap = IP.prepare_images(fr, case['augs'], normalize_cfg=dict(IP.NORMALIZE_CFG, to_rgb=False))
    assert np.array_equal(no_swap.cpu().numpy().view(np.int32), C.expected_floats(want, False, False).view(np.int32))
    with pytest.raises(_capi.FbbevError):
        IP.prepare_images(fr.cpu(), case['augs'])
    with pytest.raises(_capi.FbbevError, match='declines'):
        IP.prepare_images(fr[:1], [C._aug(90, 160, 25, 70, 0.1, 0, 0, False, 0)])        # 21 taps and more


def test_pipeline_step_on_gpu_frames_equals_the_fixture(api):
    import test_image_prep_host as H
    H.check_get_inputs(lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(api.device))


def test_detector_takes_raw_frames(api):
    import test_gpu_full_model as FM
    from fb_bev_amd import image_prep as IP
    dev = api.device
    B, N, Hs, Ws = 1, 6, 300, 800
    img_inputs, metas, _, _ = FM._inputs(dev, B, seed=5)
    g = torch.Generator().manual_seed(9)
    frames = torch.randint(0, 256, (B, N, Hs, Ws, 3), generator=g, dtype=torch.uint8).to(dev)
    augs = [C._aug(Hs, Ws, 256, 704, 0.9 + 0.01 * i, 3 * i, 2 + i, i % 2 == 1, (-5.4, 0, 5.4)[i % 3]) for i in range(N)]
    m = FM._small_model(dev, execution=dict(images_from_frames=True)).eval()
    assert m.images_from_frames is True and FM._small_model(dev).images_from_frames is False
    prepared = IP.prepare_images(frames[0], augs, channels_last=bool(getattr(m.img_backbone, 'channels_last', False)))
    want = IP.prepare_images_reference(frames[0, :2], augs[:2])
    assert np.array_equal(prepared[:2].cpu().numpy().view(np.int32), want.view(np.int32))
    with torch.no_grad():
        from_frames = m.predict_occupancy([frames] + img_inputs[1:], metas(True), img_augs=augs)
        m.reset_history()
        nested = m.predict_occupancy_classes([frames] + img_inputs[1:], metas(True), img_augs=[augs])
        m.reset_history()
        given = m.predict_occupancy([prepared.view(B, N, *prepared.shape[1:])] + img_inputs[1:], metas(True), img_augs=augs)
        m.reset_history()
        m.images_from_frames = False
        off = m.predict_occupancy([prepared.view(B, N, *prepared.shape[1:])] + img_inputs[1:], metas(True))
    assert from_frames.shape == (B, 40, 40, 16)
    assert torch.equal(from_frames, given) and torch.equal(given, off) and torch.equal(nested.long(), from_frames.long())
