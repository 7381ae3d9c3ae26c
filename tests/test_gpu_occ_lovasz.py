"""fbbev_occ_lovasz_fwd / fbbev_occ_lovasz_grad on the MI355X: the table of tests/occ_lovasz_cases.py through fb_bev_amd._capi (the
emulator test runs the same checks), occ_loss.lovasz_softmax_fused against the float64 formula, OccHead(fused_lovasz=True) and
FBOCC(execution=dict(fused_lovasz=True)) against the unfused head, and the chain under graph capture."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_lovasz_cases as VC  # noqa: E402

pytestmark = pytest.mark.gpu
TERMS = ('ce', 'sem_scal', 'geo_scal', 'lovasz')


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    return VC.GpuApi()


def _bar(got, want):
    return abs(got - want) / (2e-5 * abs(want) + 1e-6)


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('kind', VC.LABEL_KINDS)
@pytest.mark.parametrize('case', VC.CASES, ids=VC.CASE_IDS)
def test_counts_errors_coefficients_and_gradient(api, case, kind):
    VC.check(api, case, kind, order64=case['name'] in VC.SMALL_IDS)


@pytest.mark.parametrize('case', VC.EXACT_CASES + [VC.by_name('n2_cl')], ids=VC.EXACT_IDS + ['n2_cl'])
def test_ties_are_broken_by_voxel_index_alone(api, case):
    for kind in ('uniform', 'skewed', 'allvalid'):
        VC.check(api, case, kind, exact=True)


@pytest.mark.parametrize('name', VC.REPEAT_IDS)
def test_two_runs_give_identical_bytes(api, name):
    VC.check_repeat(api, VC.by_name(name))


def test_two_class_groups(api):
    """C = 32 over 528 384 voxels: more (class, voxel) pairs than one group holds, so the classes are sorted as 31 + 1.  Held against
    the float64 formula through the Python entry (a bit-for-bit reference of 17 M coefficients would take this test past its seconds)."""
    from fb_bev_amd import occ_loss as L
    g = torch.Generator().manual_seed(11)
    B, C, H, W, D = 1, 32, 64, 64, 129
    assert C * B * H * W * D > 1 << 24 and 31 * B * H * W * D <= 1 << 24
    logits = torch.randn((B, C, H, W, D), generator=g) * 3
    t = torch.randint(0, C, (B, H, W, D), generator=g)
    t[torch.rand((B, H, W, D), generator=g) < 0.04] = 255
    want = float(VC.lovasz64(torch.softmax(logits.double(), 1), t))
    got = float(L.lovasz_softmax_fused(logits.to(api.device), t.to(api.device)))
    VC.observed(f'two class groups: fused {got!r}, float64 {want!r}, err / (2e-5 |v| + 1e-6) = {_bar(got, want):.3f}')
    assert _bar(got, want) <= 1


# ------------------------------------------------------------------------------------------------------------------ through Python
@pytest.mark.parametrize('kind', ['uniform', 'absent', 'all255'])
@pytest.mark.parametrize('name', ['b1_17x33x16_cl', 'b2_8x8x16_padded_planes', 'b1_6x4x5_permuted'])
def test_fused_function_against_the_float64_formula(api, name, kind):
    from fb_bev_amd import occ_loss as L
    case = VC.by_name(name)
    Lc, lab = VC.inputs(case, kind)[:2]
    storage, size, stride, off = VC.LC.lay_out(case, Lc)
    x64 = Lc.double().requires_grad_()
    want = VC.lovasz64(torch.softmax(torch.nan_to_num(x64, nan=0.0, posinf=0.0, neginf=0.0), 1), lab)
    want.backward()
    x = storage.to(api.device).as_strided(size, stride, off).requires_grad_()
    got = L.lovasz_softmax_fused(x, lab.to(api.device).long())
    got.backward()
    VC.observed(f'fused function {name} {kind}: {float(got.detach())!r} against {float(want.detach())!r}, err / (2e-5 |v| + 1e-6) = '
                f'{_bar(float(got.detach()), float(want.detach())):.3f}')
    assert _bar(float(got.detach()), float(want.detach())) <= 1
    # the gradient's bound is layer 4 of the kernel check; here it is reported, and must be finite (zero when nothing is valid)
    g = x.grad.cpu().double()
    assert torch.isfinite(g).all()
    VC.observed(f'fused function {name} {kind}: gradient worst |err| = {float((g - x64.grad).abs().max()):.3e}, largest |grad| = '
                f'{float(x64.grad.abs().max()):.3e}')
    if kind == 'all255':
        assert float(got.detach()) == 0 and (g == 0).all()
    with pytest.raises(Exception, match='GPU tensor'):
        L.lovasz_softmax_fused(Lc, lab.long())


@pytest.fixture(scope='module')
def small(api):
    import test_gpu_full_model as FM
    m = FM._small_model(api.device).eval()
    img_inputs, metas, gt_occ, _ = FM._inputs(api.device, 2)
    with torch.no_grad():
        logits = m.occupancy_head(m.extract_feat(None, img_inputs, metas(True))['img_bev_feat'])['output_voxels'][0]
    assert logits.shape == (2, 19, 40, 40, 16)
    return m.occupancy_head, logits.detach(), gt_occ


def _losses(head, logits, gt, fused, fused_lovasz):
    head.fused_losses, head.fused_lovasz = fused, fused_lovasz
    try:
        losses = head.loss(output_voxels=[logits], target_voxels=gt)
    finally:
        head.fused_losses, head.fused_lovasz = False, False
    assert set(losses) == {f'loss_voxel_{n}_c_0' for n in TERMS}
    return losses


@pytest.mark.parametrize('fused', [False, True], ids=['with_torch_losses', 'with_fused_losses'])
def test_fused_lovasz_head_equals_the_unfused_head(api, small, fused, monkeypatch):
    from fb_bev_amd import _capi
    from fb_bev_amd.occ_head import OccHead
    tiny = dict(in_channels=[8], out_channel=19, num_level=1, norm_cfg=dict(type='BN3d', requires_grad=True), use_deblock=False)
    assert OccHead(**tiny, fused_lovasz=True).fused_lovasz is True and OccHead(**tiny).fused_lovasz is False
    head, logits, gt = small
    calls = []
    for name in ('occ_lovasz_fwd', 'occ_lovasz_grad'):               # the fused side really goes through the kernels
        monkeypatch.setattr(_capi, name, lambda *a, _real=getattr(_capi, name), _name=name, **kw: (calls.append(_name), _real(*a, **kw))[1])
    softmaxes = []
    for mod in (torch, torch.nn.functional):
        monkeypatch.setattr(mod, 'softmax', lambda *a, _real=mod.softmax, **kw: (softmaxes.append(1), _real(*a, **kw))[1])
    with torch.no_grad():
        want = _losses(head, logits, gt, False, False)
    assert not calls and softmaxes
    del softmaxes[:]
    grads = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error' if fused else 'default')   # with both switches on nothing in the head waits for the host
    try:
        for _ in range(2):
            x = logits.clone().requires_grad_()
            got = _losses(head, x, gt, fused, True)
            got['loss_voxel_lovasz_c_0'].backward()
            grads.append(x.grad)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert calls == ['occ_lovasz_fwd', 'occ_lovasz_grad'] * 2, calls
    if fused:
        assert not softmaxes, 'a full-size softmax is left in the head'
    for k, v in want.items():
        g, v = float(got[k].detach()), float(v)
        VC.observed(f'head fused_losses={fused} {k}: fused_lovasz {g!r}, unfused {v!r}, err / (2e-5 |v| + 1e-6) = {_bar(g, v):.3f}')
        assert _bar(g, v) <= 1, (k, g, v)
    assert grads[0].stride() == logits.stride() and torch.isfinite(grads[0]).all() and float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32)), 'two backward passes differ'


def test_forward_and_backward_replay_under_graph_capture(api, small):
    """nothing in the chain waits for the host: forward + backward are captured once and replayed with identical bits"""
    from fb_bev_amd import occ_loss as L
    _, logits, gt = small
    x = logits.clone().requires_grad_()
    labels = gt.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # warm-up outside the capture (allocator, library load)
        for _ in range(2):
            loss = L.lovasz_softmax_fused(x, labels)
            x.grad = None
            loss.backward()
    torch.cuda.current_stream().wait_stream(side)
    eager_loss, eager_grad = loss.detach().clone(), x.grad.detach().clone()
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g = L.lovasz_softmax_fused(x, labels)
        loss_g.backward()
    outs = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        outs.append((loss_g.detach().clone(), x.grad.detach().clone()))
    for lo, gr in outs:
        assert torch.equal(lo.view(torch.int32), eager_loss.view(torch.int32))
        assert torch.equal(gr.view(torch.int32), eager_grad.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the detector
@pytest.mark.parametrize('fused', [False, True], ids=['with_torch_losses', 'with_fused_losses'])
def test_detector_with_fused_lovasz(api, fused):
    """FBOCC(execution=dict(fused_lovasz=True)): the switch reaches the head, the head's terms on the detector's own logits are those
    of the unfused head, and one training step gives finite gradients on every parameter"""
    import test_gpu_full_model as FM
    m = FM._small_model(api.device, execution=dict(fused_occ_losses=fused, fused_lovasz=True))
    head = m.occupancy_head
    assert head.fused_lovasz is True and head.fused_losses is fused
    assert FM._small_model(api.device).occupancy_head.fused_lovasz is False
    img_inputs, metas, gt_occ, gt_depth = FM._inputs(api.device, 2, seed=3)
    m.eval()
    with torch.no_grad():
        logits = head(m.extract_feat(None, img_inputs, metas(True))['img_bev_feat'])['output_voxels'][0]
        got = head.loss(output_voxels=[logits], target_voxels=gt_occ)
        head.fused_losses = head.fused_lovasz = False
        want = head.loss(output_voxels=[logits], target_voxels=gt_occ)
        head.fused_losses, head.fused_lovasz = fused, True
    assert set(got) == set(want) == {f'loss_voxel_{n}_c_0' for n in TERMS}
    for k, v in want.items():
        g, v = float(got[k]), float(v)
        VC.observed(f'detector fused_occ_losses={fused} {k}: fused_lovasz {g!r}, unfused {v!r}, err / (2e-5 |v| + 1e-6) = {_bar(g, v):.3f}')
        assert _bar(g, v) <= 1, (k, g, v)
    m.train()
    losses = m(return_loss=True, img_inputs=img_inputs, img_metas=metas(True), gt_occupancy=gt_occ, gt_depth=gt_depth)
    assert set(losses) == set(want) | {'loss_depth'}
    total = m.parse_losses(losses)
    total.backward()
    assert torch.isfinite(total)
    params = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    missing = [n for n, p in params if p.grad is None]
    assert not missing, missing[:5]
    bad = [n for n, p in params if not torch.isfinite(p.grad).all()]
    assert not bad, bad[:5]
    assert sum(float(p.grad.abs().sum()) for n, p in params if 'occupancy_head' in n) > 0
