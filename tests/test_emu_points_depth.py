"""fbbev_points_to_depth on the CPU emulator: the kernel source of fb_bev_amd/csrc/points_depth_kernels.h and its launcher, unedited,
at the cases of tests/points_depth_cases.py, through tests/emu/emu_capi.lib().  Also the CPU side of fb_bev_amd.points_depth: the
torch restatement of the reference's argsort route, the host matrix chain, and PointToMultiViewDepth against the fixture the real
class wrote."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_depth_cases as PC  # noqa: E402


@pytest.fixture(scope='module')
def api():
    return PC.EmuApi()


@pytest.mark.parametrize('case', PC.CASES, ids=PC.CASE_IDS)
def test_exact_layer(api, case):
    PC.check_exact(api, case)


@pytest.mark.parametrize('case', [PC.by_name(n) for n in ('odd_dims', 'one_pixel', 'blocks')], ids=lambda c: c['name'])
def test_two_runs_give_identical_bits(api, case):
    PC.check_repeat(api, case)


def test_reference_fixture(api):
    PC.check_fixture(api)


@pytest.mark.parametrize('case', PC.REAL_CASES, ids=PC.REAL_IDS)
def test_real_layer(api, case):
    PC.check_real(api, case)


# ------------------------------------------------------------------------------------------------------------------ declines
def _call(api, **kw):
    a = dict(points=torch.zeros(8), stride=3, offsets=torch.tensor([0, 2], dtype=torch.int32), max_points=2, B=1, N=1,
             M=torch.eye(4).view(1, 1, 4, 4).clone(), R=torch.eye(3).view(1, 1, 3, 3).clone(), T=torch.zeros(1, 1, 3), H=4, W=4, ds=1,
             lo=1.0, hi=45.0, out=None)
    a.update(kw)
    buf = torch.full((PC.GUARD + 16 + PC.GUARD,), PC.PATTERN)
    out = buf[PC.GUARD:PC.GUARD + 16] if a['out'] is None else a['out']
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    code = api.lib.fbbev_points_to_depth(p(a['points']), a['stride'], p(a['offsets']), a['max_points'], a['B'], a['N'], p(a['M']),
                                         p(a['R']), p(a['T']), a['H'], a['W'], a['ds'], a['lo'], a['hi'], p(out), None)
    return code, buf


NONE = object()


def test_return_codes(api):
    untouched = lambda buf: bool((buf == PC.PATTERN).all())  # noqa: E731
    for name in ('points', 'offsets', 'M', 'R', 'T'):
        code, buf = _call(api, **{name: None})
        assert code == -1 and untouched(buf), name
    p = ctypes.c_void_p
    d = torch.zeros(64)
    assert api.lib.fbbev_points_to_depth(p(d.data_ptr()), 3, p(d.data_ptr()), 0, 1, 1, p(d.data_ptr()), p(d.data_ptr()), p(d.data_ptr()),
                                         4, 4, 1, 1.0, 45.0, None, None) == -1                      # a null out
    for kw in (dict(stride=2), dict(ds=0), dict(ds=-1), dict(max_points=-1), dict(B=-1), dict(N=-1), dict(H=-1), dict(W=-1),
               dict(lo=0.0), dict(lo=-1.0), dict(lo=float('nan')), dict(hi=float('nan'))):
        code, buf = _call(api, **kw)
        assert code == -1 and untouched(buf), kw
    for kw in (dict(H=3, ds=4), dict(W=3, ds=4), dict(H=0), dict(B=0), dict(N=0)):                    # nothing to write: 0, guards and out alone
        code, buf = _call(api, **kw)
        assert code == 0 and untouched(buf), kw
    for hi in (100.0, 150.0, float('inf')):
        code, buf = _call(api, hi=hi)
        assert code == -4 and untouched(buf), hi
    code, buf = _call(api, hi=float(np.nextafter(np.float32(100), np.float32(0))))
    assert code == 0
    code, buf = _call(api, H=4096, W=4096)                                                          # h w = 2^24
    assert code == -5 and untouched(buf)
    code, buf = _call(api, H=8192, W=4096, ds=2, B=0)                                                 # nothing to do comes first
    assert code == 0
    code, buf = _call(api, H=8192, W=8192, ds=2)                                                      # (H / ds)(W / ds) = 2^24
    assert code == -5 and untouched(buf)
    code, buf = _call(api, B=4096, N=4096)                                                            # B N = 2^24
    assert code == -2 and untouched(buf)
    assert _call(api, stride=2, hi=100.0)[0] == -1 and _call(api, hi=100.0, H=4096, W=4096)[0] == -4  # the order of the checks


def test_a_batch_without_points_is_zeroed(api):
    code, buf = _call(api, max_points=0, offsets=torch.tensor([0, 0], dtype=torch.int32))
    assert code == 0
    assert (buf[:PC.GUARD] == PC.PATTERN).all() and (buf[PC.GUARD + 16:] == PC.PATTERN).all()
    assert (buf[PC.GUARD:PC.GUARD + 16].view(torch.int32) == 0).all()


# ------------------------------------------------------------------------------------------------------------------ the CPU route
@pytest.mark.parametrize('name', PC.FIXTURE_CASES)
def test_cpu_route_and_pipeline_step_equal_the_fixture(name):
    """points_to_depth on CPU tensors and PointToMultiViewDepth.__call__ against the map of the reference class, under check 2's rule
    (the restatement's argsort may break a tie of the key the other way)"""
    from fb_bev_amd.points_depth import PointToMultiViewDepth, points_to_depth
    case = PC.by_name(name)
    z = PC.fixture()
    want = PC.fixture_map(case, z)
    pts_list, M, R, T = PC.exact_inputs(case)
    B, N, h, w = PC.dims(case)
    pts = [torch.from_numpy(p) for p in pts_list]
    got = points_to_depth(pts, torch.from_numpy(M), torch.from_numpy(R), torch.from_numpy(T), case['H'], case['W'], case['ds'], case['cfg'])
    assert got.shape == (B, N, h, w) and got.dtype == torch.float32
    ties = PC.tie_pixels(case)
    assert np.array_equal((got.numpy() != 0), want != 0)
    assert np.array_equal(PC._keys(got.numpy(), h, w), PC._keys(want, h, w))
    assert (got.numpy().view(np.int32) == want.view(np.int32))[~ties].all()
    flat = torch.cat(pts, 0)
    offs = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])])
    again = points_to_depth(flat, torch.from_numpy(M), torch.from_numpy(R), torch.from_numpy(T), case['H'], case['W'], case['ds'],
                            case['cfg'], offsets=[int(v) for v in offs])
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    step = PointToMultiViewDepth(grid_config=dict(depth=list(case['cfg'])), downsample=case['ds'])
    for b in range(B):
        curr, names, intrins = PC.exact_info(case, b)
        results = dict(points=pts[b], curr=curr, cam_names=names,
                       img_inputs=(torch.zeros(N, 3, case['H'], case['W']), None, None, intrins, torch.from_numpy(R[b]),
                                   torch.from_numpy(T[b]), None))
        m = step(results)['gt_depth'].numpy()
        assert m.shape == (N, h, w)
        assert np.array_equal(m != 0, want[b] != 0)
        assert np.array_equal(PC._keys(m, h, w), PC._keys(want[b], h, w))
        assert (m.view(np.int32) == want[b].view(np.int32))[~ties[b]].all()


def test_points2depthmap_has_the_reference_signature():
    from fb_bev_amd.points_depth import PIPELINES, PointToMultiViewDepth, build_pipeline_step
    step = build_pipeline_step(dict(type='PointToMultiViewDepth', grid_config=dict(depth=[1.0, 45.0, 0.5]), downsample=2))
    assert isinstance(step, PointToMultiViewDepth) and step.downsample == 2 and PIPELINES['PointToMultiViewDepth'] is PointToMultiViewDepth
    pts = torch.tensor([[2.0, 2.0, 5.0], [3.0, 2.0, 4.0], [2.9, 1.1, 50.0], [100.0, 2.0, 5.0]])
    m = step.points2depthmap(pts, 6, 10)
    assert m.shape == (3, 5) and float(m[1, 1]) == 5.0 and float(m[1, 2]) == 4.0 and int((m != 0).sum()) == 2      # 3 / 2 = 1.5 -> 2


def test_lidar2img_from_info_on_dyadic_quaternions_is_the_fixture():
    from fb_bev_amd.points_depth import lidar2img_from_info
    z = PC.fixture()
    for name in PC.FIXTURE_CASES:
        case = PC.by_name(name)
        for b in range(case['B']):
            got = lidar2img_from_info(*PC.exact_info(case, b))
            assert got.shape == (case['N'], 4, 4) and got.dtype == torch.float32
            assert np.array_equal(got.numpy()[:, :3].view(np.int32), z[f'{name}.lidar2img'][b].view(np.int32))
            assert np.array_equal(got.numpy()[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (case['N'], 1)))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_lidar2img_from_info_on_real_quaternions(seed):
    from fb_bev_amd.points_depth import lidar2img_from_info
    info = PC.real_info(seed)
    want, bound = PC.lidar2img_bound(*info)
    got = lidar2img_from_info(*info).numpy().astype(np.float64)
    assert np.abs(got[:, 3] - np.array([0.0, 0.0, 0.0, 1.0])).max() < 1e-6      # the last row is read by nobody: no bound is derived for it
    err, bound = np.abs(got - want)[:, :3], bound[:, :3]
    PC.observed(f'lidar2img_from_info seed {seed}: worst |error| / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3e}, '
                f'largest |error| {float(err.max()):.3e}, largest bound {float(bound.max()):.3e}')
    assert (err <= bound).all()


def test_quaternion_rotation_matrix():
    from fb_bev_amd.points_depth import quaternion_rotation_matrix
    assert np.array_equal(quaternion_rotation_matrix(PC.Q_CYCLE), np.array([[0., 0, 1], [1, 0, 0], [0, 1, 0]]))
    assert np.array_equal(quaternion_rotation_matrix([0.0, 0.0, 2.0, 0.0]), np.diag([-1.0, 1.0, -1.0]))     # normalised first
    r = quaternion_rotation_matrix([0.3, -0.5, 0.7, 0.1])
    assert np.abs(r @ r.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(r) - 1) < 1e-15
    with pytest.raises(ValueError):
        quaternion_rotation_matrix([0, 0, 0, 0])
