"""fbbev_points_to_depth on the MI355X: the cases of tests/points_depth_cases.py through fb_bev_amd._capi.points_to_depth (the
emulator test runs the same checks); fb_bev_amd.points_depth on GPU tensors; FBOCC(execution=dict(depth_from_points=True))."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_depth_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    return PC.GpuApi()


@pytest.mark.parametrize('case', PC.CASES, ids=PC.CASE_IDS)
def test_exact_layer(api, case):
    PC.check_exact(api, case)


@pytest.mark.parametrize('case', [PC.by_name(n) for n in ('odd_dims', 'one_pixel', 'blocks', 'shipped')], ids=lambda c: c['name'])
def test_two_runs_give_identical_bits(api, case):
    PC.check_repeat(api, case)


def test_reference_fixture(api):
    PC.check_fixture(api)


@pytest.mark.parametrize('case', PC.REAL_CASES, ids=PC.REAL_IDS)
def test_real_layer(api, case):
    PC.check_real(api, case)


def test_declines_leave_the_guards_alone(api):
    from fb_bev_amd import _capi
    dev = api.device
    pts, off = torch.zeros(4, 3, device=dev), torch.tensor([0, 4], dtype=torch.int32, device=dev)
    M, R, T = torch.eye(4, device=dev).view(1, 1, 4, 4), torch.eye(3, device=dev).view(1, 1, 3, 3), torch.zeros(1, 1, 3, device=dev)
    for hi, code in ((100.0, -4), (float('nan'), -1)):
        with pytest.raises(_capi.FbbevError, match=f'invalid argument {code}'):
            _capi.points_to_depth(pts, off, 4, M, R, T, 4, 4, 1, 1.0, hi)
    with pytest.raises(_capi.FbbevError, match='invalid argument -1'):
        _capi.points_to_depth(pts, off, 4, M, R, T, 4, 4, 1, 0.0, 45.0)
    buf = torch.full((PC.GUARD * 2,), PC.PATTERN, device=dev)
    out = buf[PC.GUARD:PC.GUARD].view(0, 1, 4, 4)                    # B N == 0: 0, no launch
    got = _capi.points_to_depth(pts, off[:1], 0, M[:0], R[:0], T[:0], 4, 4, 1, 1.0, 45.0, out=out)
    assert got.shape == (0, 1, 4, 4) and bool((buf == PC.PATTERN).all())
    empty = _capi.points_to_depth(pts[:0], torch.zeros(2, dtype=torch.int32, device=dev), 0, M, R, T, 4, 4, 1, 1.0, 45.0)
    assert empty.shape == (1, 1, 4, 4) and bool((empty.view(torch.int32) == 0).all())


def test_module_routes_gpu_tensors_to_the_kernel(api):
    """points_to_depth on GPU tensors: a list, and one tensor with offsets on the host or on the device, equal the C entry's bits"""
    from fb_bev_amd.points_depth import points_to_depth
    case = PC.by_name('stride5_batch')
    want, _ = PC.expected_exact(case)
    pts_list, M, R, T = PC.exact_inputs(case)
    dev = api.device
    pts = [torch.from_numpy(p).to(dev) for p in pts_list]
    mats = [torch.from_numpy(a).to(dev) for a in (M, R, T)]
    got = points_to_depth(pts, *mats, case['H'], case['W'], case['ds'], case['cfg'])
    assert got.is_cuda and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    offs = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts_list])])
    flat = torch.cat(pts, 0)
    for o in ([int(v) for v in offs], torch.tensor(offs, dtype=torch.int32, device=dev)):
        again = points_to_depth(flat, *mats, case['H'], case['W'], case['ds'], case['cfg'], offsets=o)
        assert torch.equal(again.cpu().view(torch.int32), want.view(torch.int32))


def test_detector_builds_gt_depth_from_points(api):
    import test_gpu_full_model as FM
    from fb_bev_amd.points_depth import points_to_depth
    dev = api.device
    case = PC.by_name('shipped')
    B = 2
    img_inputs, metas, gt_occ, gt_depth = FM._inputs(dev, B, seed=3)
    pts_list, M, R, T = PC.real_inputs(case)
    points = [torch.from_numpy(pts_list[0][b::2].copy()).to(dev) for b in range(B)]                 # two halves of the sweep
    lidar2img = torch.from_numpy(M).to(dev).expand(B, -1, -1, -1).contiguous()
    img_inputs[4], img_inputs[5] = torch.from_numpy(R).to(dev).expand(B, -1, -1, -1).contiguous(), \
        torch.from_numpy(T).to(dev).expand(B, -1, -1).contiguous()
    grid = [2.0, 42.0, 0.5]
    built = points_to_depth(points, lidar2img, img_inputs[4], img_inputs[5], 256, 704, 1, grid)
    assert built.shape == (B, 6, 256, 704) and int((built != 0).sum()) > 5000

    m = FM._small_model(dev, execution=dict(depth_from_points=True)).train()
    assert m.depth_from_points is True and m.depth_net.grid_config['depth'] == grid

    def loss(flag, **kw):
        m.depth_from_points = flag
        torch.manual_seed(11)                                        # the depth net's ASPP has a Dropout: the same masks for every call
        return m(return_loss=True, img_inputs=img_inputs, img_metas=metas(True), gt_occupancy=gt_occ, **kw)['loss_depth']
    from_points = loss(True, points=points, lidar2img=lidar2img)
    given = loss(True, gt_depth=built)
    assert torch.isfinite(from_points) and float(from_points.detach()) > 0
    assert torch.equal(from_points.view(torch.int32), given.view(torch.int32))
    # a gt_depth that is given wins, and with the flag off nothing changes
    other = loss(True, gt_depth=gt_depth, points=points, lidar2img=lidar2img)
    off = loss(False, gt_depth=gt_depth)
    assert torch.equal(other.view(torch.int32), off.view(torch.int32))
    assert not torch.equal(off.view(torch.int32), given.view(torch.int32))
    assert FM._small_model(dev).depth_from_points is False
