"""fbbev_occ_loss_stats / fbbev_occ_loss_grad on the MI355X: the table of tests/occ_loss_cases.py through fb_bev_amd._capi (the emulator
test runs the same table); OccHead(fused_losses=True) against the unfused head on the small detector's logits; the fused losses
against the reference numbers of tests/golden/occ_encoder_head_small.npz; one training step of FBOCC(execution=dict(
fused_occ_losses=True))."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_loss_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu
TERMS = ('ce', 'sem_scal', 'geo_scal')


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    return LC.GpuApi()


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('focal', [False, True], ids=['ce', 'focal'])
@pytest.mark.parametrize('kind', LC.LABEL_KINDS)
@pytest.mark.parametrize('case', LC.CASES, ids=LC.CASE_IDS)
def test_stats_and_gradient(api, case, kind, focal):
    LC.check(api, case, kind, focal)


@pytest.mark.parametrize('case', LC.EXACT_CASES, ids=LC.EXACT_IDS)
def test_sums_are_exact_where_p_is(api, case):
    LC.check_exact(api, case)


@pytest.mark.parametrize('name', LC.REPEAT_IDS)
def test_two_runs_give_identical_bytes(api, name):
    LC.check_repeat(api, LC.by_name(name))


# ------------------------------------------------------------------------------------------------------------------ the head
@pytest.fixture(scope='module')
def small(api):
    """the small detector's head, its logits for two samples (as the head returns them) and the labels"""
    import test_gpu_full_model as FM
    m = FM._small_model(api.device).eval()
    img_inputs, metas, gt_occ, _ = FM._inputs(api.device, 2)
    with torch.no_grad():
        logits = m.occupancy_head(m.extract_feat(None, img_inputs, metas(True))['img_bev_feat'])['output_voxels'][0]
    assert logits.shape == (2, 19, 40, 40, 16)
    LC.observed(f'small detector: logits strides {logits.stride()}')
    return m.occupancy_head, logits.detach(), gt_occ


def _three(head, logits, gt, fused):
    head.fused_losses = fused
    losses = head.loss(output_voxels=[logits], target_voxels=gt)
    assert set(losses) == {f'loss_voxel_{n}_c_0' for n in TERMS + ('lovasz',)}
    return losses


@pytest.mark.parametrize('focal', [True, False], ids=['focal', 'ce'])
def test_fused_head_losses_equal_the_unfused_head(api, small, focal, monkeypatch):
    from fb_bev_amd import _capi, occ_loss as L
    from fb_bev_amd.occ_head import OccHead
    tiny = dict(in_channels=[8], out_channel=19, num_level=1, norm_cfg=dict(type='BN3d', requires_grad=True), use_deblock=False)
    assert OccHead(**tiny, fused_losses=True).fused_losses is True and OccHead(**tiny).fused_losses is False
    head, logits, gt = small
    head.use_focal_loss = focal
    calls = []
    for name in ('occ_loss_stats', 'occ_loss_grad'):                 # the fused side really goes through the two kernels
        monkeypatch.setattr(_capi, name, lambda *a, _real=getattr(_capi, name), _name=name, **kw: (calls.append(_name), _real(*a, **kw))[1])
    try:
        with torch.no_grad():
            want = _three(head, logits, gt, False)
        assert not calls
        grads = []
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            for _ in range(2):
                x = logits.clone().requires_grad_()
                got = _three(head, x, gt, True)
                sum(got[f'loss_voxel_{n}_c_0'] for n in TERMS).backward()
                grads.append(x.grad)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    finally:
        head.use_focal_loss, head.fused_losses = True, False
    assert calls == ['occ_loss_stats', 'occ_loss_grad'] * 2, calls
    for k, v in want.items():
        g, v = float(got[k].detach()), float(v)
        LC.observed(f'head {"focal" if focal else "ce"} {k}: fused {g!r}, unfused {v!r}, err / (2e-5 |v| + 1e-6) = '
                    f'{abs(g - v) / (2e-5 * abs(v) + 1e-6):.3f}')
        assert abs(g - v) <= 2e-5 * abs(v) + 1e-6, (k, g, v)
    assert grads[0].stride() == logits.stride()
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32)), 'two backward passes differ'
    # the gradient of ce + sem_scal + geo_scal (the head's weights) against float64: the statistics, the epilogue and its autograd
    # in float64 on the CPU give grad_stats, the backward formula of occ_loss_cases gives the gradient and every element's A
    Lc, lab = logits.cpu(), gt.cpu().to(torch.uint8)
    cw, plane = head.class_weights.cpu().float(), head.focal_loss.c.cpu().float()
    sf, si = LC.stats_torch(Lc, lab, cw, plane, head.empty_idx, focal, torch.float64)
    sf = sf.requires_grad_()
    three = L.losses_from_stats(sf, si, cw.double(), head.empty_idx, focal, head.focal_loss.loss_weight)
    w = (head.loss_voxel_ce_weight, head.loss_voxel_sem_scal_weight, head.loss_voxel_geo_scal_weight)
    sum(a * b for a, b in zip(w, three)).backward()
    assert LC.GAMMA == head.focal_loss.gamma and LC.ALPHA == head.focal_loss.alpha
    ref, A = LC.grad_ref64(Lc, lab, cw, plane, head.empty_idx, focal, sf.grad)
    err = (grads[0].cpu().double() - ref).abs()
    live = A > 0
    LC.observed(f'head {"focal" if focal else "ce"}: gradient worst err / A = {float((err[live] / A[live]).max()):.3e} '
                f'(RHO = {LC.RHO[focal]:.3e}), largest |grad| = {float(ref.abs().max()):.3e}')
    assert (grads[0].cpu()[~live] == 0).all()
    assert (err <= LC.RHO[focal] * A).all()
    assert float(ref.abs().max()) > 0


@pytest.mark.parametrize('focal', [True, False], ids=['focal', 'ce'])
def test_fused_losses_reproduce_the_reference_fixture(api, focal):
    import test_occ_modules as OM
    gold = np.load(OM.G)
    vf = [torch.from_numpy(gold[f'head.feat{i}']) for i in range(3)]
    gt = torch.from_numpy(gold['head.gt'].astype(np.int64)).to(api.device)
    with torch.no_grad():
        logits = OM._head(gold, True)(vf)['output_voxels'][0].to(api.device)
        head = OM._head(gold, focal).to(api.device)
        head.fused_losses = True
        losses = head.loss(output_voxels=[logits], target_voxels=gt)
    tag = 'focal' if focal else 'ce'
    for n in TERMS:
        k = f'loss_voxel_{n}_c_0'
        got, exp = float(losses[k]), float(gold[f'head.{tag}.{k}'])
        LC.observed(f'fixture {tag} {k}: {got!r} against {exp!r}, err / (2e-5 |v| + 1e-6) = {abs(got - exp) / (2e-5 * abs(exp) + 1e-6):.3f}')
        assert abs(got - exp) <= 2e-5 * abs(exp) + 1e-6, (tag, k, got, exp)


# ------------------------------------------------------------------------------------------------------------------ the detector
def test_detector_trains_with_fused_losses(api):
    import test_gpu_full_model as FM
    m = FM._small_model(api.device, execution=dict(fused_occ_losses=True)).train()
    assert m.occupancy_head.fused_losses is True
    img_inputs, metas, gt_occ, gt_depth = FM._inputs(api.device, 2, seed=3)
    losses = m(return_loss=True, img_inputs=img_inputs, img_metas=metas(True), gt_occupancy=gt_occ, gt_depth=gt_depth)
    assert set(losses) == {'loss_voxel_ce_c_0', 'loss_voxel_sem_scal_c_0', 'loss_voxel_geo_scal_c_0', 'loss_voxel_lovasz_c_0', 'loss_depth'}
    total = m.parse_losses(losses)
    total.backward()
    assert torch.isfinite(total)
    params = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    missing = [n for n, p in params if p.grad is None]
    assert not missing, missing[:5]
    bad = [n for n, p in params if not torch.isfinite(p.grad).all()]
    assert not bad, bad[:5]
    assert sum(float(p.grad.abs().sum()) for n, p in params if 'occupancy_head' in n) > 0
