"""fbbev_depth_loss_fwd / fbbev_depth_loss_grad on the MI355X: the table of tests/depth_loss_cases.py through fb_bev_amd._capi (the
emulator test runs the same table); the fixture of the reference module; CM_DepthNet(fused_depth_loss=True) against the default
route and against float64 on the shipped geometry; the routes the flag must leave alone (sid, bf16); FBOCC(execution=dict(
fused_depth_loss=True))."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_loss_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    return DC.GpuApi()


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('case', DC.CASES, ids=DC.CASE_IDS)
def test_labels_loss_and_gradient(api, case):
    DC.check(api, case)


@pytest.mark.parametrize('case', DC.CASES, ids=DC.CASE_IDS)
def test_sums_are_exact_where_p_is_0_or_1(api, case):
    DC.check_exact(api, case)


@pytest.mark.parametrize('case', DC.CASES, ids=DC.CASE_IDS)
def test_two_runs_give_identical_bits(api, case):
    DC.check_repeat(api, case)


def test_reference_fixture(api):
    DC.check_fixture(api)


# ------------------------------------------------------------------------------------------------------------------ the module
def _nets(case, dev, **kw):
    from fb_bev_amd.depth_net import CM_DepthNet
    mk = lambda fused: CM_DepthNet(in_channels=8, context_channels=4, depth_channels=case['D'], mid_channels=8, use_dcn=False,  # noqa: E731
                                   use_aspp=False, downsample=case['ds'], grid_config=dict(depth=list(case['cfg'])),
                                   loss_depth_weight=3.0, fused_depth_loss=fused, **kw).to(dev)
    return mk(False), mk(True)


def test_module_matches_the_default_route_and_float64(api):
    case = DC.by_name('shipped_rows')
    gt, lab, probs = DC.reference(case)
    plain, fused = _nets(case, api.device)
    assert fused.fused_depth_loss is True and plain.fused_depth_loss is False
    d_gt = gt[None].to(api.device)
    x = probs[None].to(api.device).requires_grad_()
    want = plain.get_depth_loss(d_gt, x)['loss_depth']
    got = fused.get_depth_loss(d_gt, x)['loss_depth']
    _, ref, count = DC.ref64(probs, lab)
    DC.observed(f'module shipped_rows: fused {float(got)!r}, default route {float(want)!r}, float64 {3.0 * ref!r}')
    assert abs(float(got) - float(want)) <= DC.RHO_F * abs(float(want))
    assert abs(float(got) - 3.0 * ref) <= DC.RHO_F * 3.0 * ref
    (got * 0.37).backward()
    g64 = DC.grad_ref64(probs, lab, 1.0) * (3.0 * float(torch.tensor(0.37, dtype=torch.float32)))
    # autograd hands the kernel grad_loss = fp32(3 * fp32(0.37)): one more rounding than check 4's grad_loss, inside its ten operations
    err = (x.grad[0].cpu().double() - g64).abs()
    live = g64 != 0
    DC.observed(f'module shipped_rows: autograd gradient worst relative error {float((err[live] / g64[live].abs()).max()):.3e}')
    assert (err <= DC.RHO_G * g64.abs()).all()
    assert (x.grad[0].cpu()[(lab < 0)[:, None].expand_as(probs)] == 0).all()


def test_sid_and_bf16_stay_on_the_default_route(api, monkeypatch):
    from fb_bev_amd import _capi
    case = DC.by_name('shipped_rows')
    gt, lab, probs = DC.reference(case)
    d_gt, d_probs = gt[None].to(api.device), probs[None].to(api.device)
    calls = []

    def boom(*a, **k):
        calls.append(1)
        raise AssertionError('the fused route ran')
    plain, fused = _nets(case, api.device)
    plain_sid, fused_sid = _nets(case, api.device, sid=True)
    monkeypatch.setattr(_capi, 'depth_loss_fwd', boom)
    with pytest.raises(AssertionError, match='the fused route ran'):
        fused.get_depth_loss(d_gt, d_probs)                          # the patch is in the fused route's way
    assert calls == [1]
    a, b = plain_sid.get_depth_loss(d_gt, d_probs)['loss_depth'], fused_sid.get_depth_loss(d_gt, d_probs)['loss_depth']
    assert torch.equal(a, b) and torch.isfinite(a)
    a, b = (n.get_depth_loss(d_gt, d_probs.bfloat16())['loss_depth'] for n in (plain, fused))
    assert torch.equal(a, b) and torch.isfinite(a)
    assert calls == [1]


def test_detector_takes_the_flag(api):
    import test_gpu_full_model as FM
    m = FM._small_model(api.device, execution=dict(fused_depth_loss=True)).train()
    assert m.depth_net.fused_depth_loss is True
    assert FM._small_model(api.device).depth_net.fused_depth_loss is False
    img_inputs, metas, gt_occ, gt_depth = FM._inputs(api.device, 2, seed=3)
    losses = m(return_loss=True, img_inputs=img_inputs, img_metas=metas(True), gt_occupancy=gt_occ, gt_depth=gt_depth)
    assert set(losses) == {'loss_voxel_ce_c_0', 'loss_voxel_sem_scal_c_0', 'loss_voxel_geo_scal_c_0', 'loss_voxel_lovasz_c_0', 'loss_depth'}
    total = m.parse_losses(losses)
    total.backward()
    assert torch.isfinite(total)
    params = [(n, p) for n, p in m.named_parameters() if p.requires_grad and 'depth_net' in n]
    assert params and all(p.grad is not None and torch.isfinite(p.grad).all() for _, p in params)
    assert sum(float(p.grad.abs().sum()) for _, p in params) > 0
