"""Deterministic mode on the GPU (fb_bev_amd.deterministic_enabled; include/fbbev.h FBBEV_FLAG_DETERMINISTIC): the path's training step
bit-stable under torch's deterministic flags, the mode against the default atomic form, and the DA backward's other routes."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))


@pytest.fixture
def det_state():
    import fb_bev_amd as F
    assert torch.cuda.is_available()
    saved = (torch.are_deterministic_algorithms_enabled(), torch.backends.cudnn.deterministic, F._deterministic_override)
    yield F
    torch.use_deterministic_algorithms(saved[0])
    torch.backends.cudnn.deterministic = saved[1]
    F.set_deterministic(saved[2])


def _graph_has(t, name):
    seen, todo = set(), [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if name in type(f).__name__:
            return True
        todo += [g for g, _ in f.next_functions]
    return False


def _steps(name, B, levels, n=3, seed=0):
    """n training steps of the path on the same inputs -> list of {gradient name: tensor}, and whether the default route ran"""
    import train_path as T
    dev = torch.device('cuda:0')
    pc, m, cam, depth, ctx, mlvl = T.build(name, B, levels, dev, seed=seed)
    step, leaves, _ = T.make_step(m, cam, depth, ctx, mlvl, dev, pc, B)
    names = [k for k, _ in m.named_parameters()] + ['depth', 'ctx'] + [f'mlvl{i}' for i in range(1, len(mlvl or []))]
    runs, default_route = [], None
    for _ in range(n):
        out = step()
        if default_route is None:
            default_route = _graph_has(out, 'EncoderLayerFn') and _graph_has(out, 'PoolAdd')
        runs.append({k: t.grad.detach().clone() for k, t in zip(names, leaves) if t.grad is not None})
    torch.cuda.synchronize()
    return runs, default_route


def _assert_stable(runs, tag):
    moved = sorted({k for r in runs[1:] for k in r if not torch.equal(r[k], runs[0][k])})
    print(f'{tag}: {len(runs[0])} gradients, bits moved in: {moved}')
    assert 'depth' in runs[0] and any('embed' in k for k in runs[0]), list(runs[0])
    assert not moved, moved


@pytest.mark.parametrize('name,B,levels', [('REF', 2, 1), ('BL2', 1, 4)])
def test_path_step_bit_stable_under_use_deterministic_algorithms(det_state, name, B, levels):
    """torch.use_deterministic_algorithms(True): the step runs, and EVERY gradient (parameters, depth, ctx, pyramid levels,
    embeddings) is bit-identical over three steps on the default route (the one-node encoder layer, the write-once volume)"""
    det_state.set_deterministic(None)
    torch.use_deterministic_algorithms(True)
    runs, default_route = _steps(name, B, levels)
    assert default_route, 'the default training route was not taken'
    _assert_stable(runs, f'[{name} B={B} L={levels}] use_deterministic_algorithms')


def test_path_step_bit_stable_under_cudnn_deterministic(det_state):
    """the reference's --deterministic (torch.backends.cudnn.deterministic = True) alone turns the mode on"""
    det_state.set_deterministic(None)
    torch.use_deterministic_algorithms(False)
    torch.backends.cudnn.deterministic = True
    assert det_state.deterministic_enabled()
    runs, default_route = _steps('REF', 2, 1)
    assert default_route
    _assert_stable(runs, '[REF B=2 L=1] cudnn.deterministic')


def test_mode_on_against_mode_off(det_state):
    """set_deterministic(True) alone (ATen takes the same algorithms on both sides): the gradients that are deterministic without the
    mode keep their bits; `depth` (fixed-point taps instead of fp32 atomics) stays within 1e-5 of its scale"""
    torch.use_deterministic_algorithms(False)
    torch.backends.cudnn.deterministic = False
    det_state.set_deterministic(False)
    off, _ = _steps('REF', 2, 1, n=1)
    det_state.set_deterministic(True)
    on, _ = _steps('REF', 2, 1, n=1)
    # expected to differ: `depth` (fixed-point taps against fp32 atomics) and the embeddings (ATen's reductions, atomically ordered
    # without torch's deterministic flag); every other gradient comes from the same kernels on both sides
    movers = {k for k in off[0] if k == 'depth' or 'embed' in k}
    assert 'depth' in movers
    changed = [k for k in off[0] if k not in movers and not torch.equal(on[0][k], off[0][k])]
    assert not changed, changed
    scale = off[0]['depth'].abs().max().item()
    err = (on[0]['depth'] - off[0]['depth']).abs().max().item()
    print(f'depth gradient: max|on - off| = {err:.3e} on a scale of {scale:.3e} ({err / scale:.2e})')
    assert scale > 0 and err <= 1e-5 * scale


@pytest.mark.parametrize('route', ['ws_grid', 'no_level_hw', 'lds_planes_false'])
def test_da_backward_routes_deterministic(det_state, route):
    """_capi.da_cross_attn_bwd on the routes the training step does not take by default: under the mode bit-stable over 3 calls and
    within 1e-5 of scale of the default (atomic depth taps) result"""
    from da_cases import da_case
    from fb_bev_amd import _capi
    dev = torch.device('cuda:0')
    shapes = ((16, 44), (8, 22))
    args, _ = da_case(7, B=2, N=6, Q=30 * 30, shapes=shapes, E=80, M=8, P=8, DC=40)
    value, ss, ls, pred, ref_cam, mask, qdepth, offsets, attn, d0, dstep = (t.to(dev) if torch.is_tensor(t) else t for t in args)
    Dh = value.shape[-1]
    vp = torch.zeros(value.shape[:-1] + (12,), device=dev); vp[..., :Dh] = value
    g = torch.randn(mask.shape[1], mask.shape[2], 80, generator=torch.Generator().manual_seed(3)).to(dev)
    kw = dict(head_dim=Dh, level_hw=None if route == 'no_level_hw' else [tuple(s) for s in shapes], bev_w=30,
              lds_planes=route != 'lds_planes_false')

    def run():
        outs = [torch.zeros_like(t) for t in (vp, pred, offsets, attn)]
        _capi.da_cross_attn_bwd(vp, ss, ls, pred, ref_cam, mask.view(torch.uint8), qdepth, offsets, attn, g, d0, dstep, 0, *outs, **kw)
        torch.cuda.synchronize()
        return outs

    det_state.set_deterministic(False)
    ref = run()
    det_state.set_deterministic(True)
    runs = [run() for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b)
    for name, a, b in zip(('value', 'depth', 'offsets', 'attn'), runs[0], ref):
        scale = b.abs().max().item()
        err = (a - b).abs().max().item()
        print(f'{route} {name}: max|det - default| = {err:.2e} on a scale of {scale:.3e}')
        assert scale > 0 and err <= 1e-5 * scale, name


@pytest.mark.parametrize('Dh', [10, 32, 12])
def test_msda_boundary_backward_deterministic(det_state, Dh):
    """ms_deform_attn_backward exactly as mmcv calls it (device spatial_shapes, no level_hw; Dh 10 / 32 take the fixed-point
    band-binned route after one host read, Dh 12 the fixed-point global scatter): bit-stable over 3 calls, accumulated into the
    caller's tensors, within 1e-5 of scale of the default form"""
    from fb_bev_amd.ms_deform_attn import ms_deform_attn_backward
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(Dh)
    B, M, L, P, Q = 2, 8, 4, 4, 900
    shapes = torch.tensor([[32, 88], [16, 44], [8, 22], [4, 11]])
    ls = torch.cat([shapes.new_zeros(1), (shapes[:, 0] * shapes[:, 1]).cumsum(0)[:-1]])
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    value = torch.randn(B, S, M, Dh, generator=g).to(dev)
    loc = (torch.rand(B, Q, M, L, P, 2, generator=g) * 1.1 - 0.05).to(dev)
    attn = torch.rand(B, Q, M, L, P, generator=g).softmax(-1).to(dev)
    go = torch.randn(B, Q, M * Dh, generator=g).to(dev)
    init = [torch.randn(t.shape, generator=g).to(dev) for t in (value, loc, attn)]

    def run():
        outs = [t.clone() for t in init]
        ms_deform_attn_backward(value, shapes.to(dev), ls.to(dev), loc, attn, go, *outs)
        torch.cuda.synchronize()
        return outs
    det_state.set_deterministic(False)
    ref = run()
    det_state.set_deterministic(True)
    runs = [run() for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b)
    for name, a, b, i in zip(('value', 'loc', 'attn'), runs[0], ref, init):
        scale = (b - i).abs().max().item()
        err = (a - b).abs().max().item()
        print(f'msda Dh={Dh} {name}: max|det - default| = {err:.2e} on a scale of {scale:.3e}')
        assert scale > 0 and err <= 1e-5 * scale, name


def test_msda_autograd_function_deterministic(det_state):
    from fb_bev_amd.ms_deform_attn import MultiScaleDeformableAttnFunction_fp32 as Fn
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(1)
    B, M, Dh, L, P, Q = 1, 8, 32, 2, 4, 400
    shapes = torch.tensor([[16, 44], [8, 22]], device=dev)
    ls = torch.tensor([0, 16 * 44], device=dev)
    S = 16 * 44 + 8 * 22
    value = torch.randn(B, S, M, Dh, generator=g).to(dev).requires_grad_()
    loc = (torch.rand(B, Q, M, L, P, 2, generator=g)).to(dev).requires_grad_()
    attn = torch.rand(B, Q, M, L, P, generator=g).to(dev).requires_grad_()
    go = torch.randn(B, Q, M * Dh, generator=g).to(dev)
    det_state.set_deterministic(True)
    grads = []
    for _ in range(3):
        for t in (value, loc, attn):
            t.grad = None
        Fn.apply(value, shapes, ls, loc, attn, 64).backward(go)
        grads.append([t.grad.clone() for t in (value, loc, attn)])
    for r in grads[1:]:
        for a, b in zip(r, grads[0]):
            assert torch.equal(a, b)


@pytest.mark.parametrize('cin,k,pad,dims', [(80, 3, 1, (8, 100, 100)), (81, 1, 0, (8, 100, 100))])
def test_conv3d_wgrad_deterministic(det_state, cin, k, pad, dims):
    """the MConv3d training route's weight gradient (fbbev_conv3d_wgrad_ndhwc; 81 input channels padded to 84 as the module does):
    bit-stable over 3 runs, within 1e-4 of scale of torch's convolution weight gradient"""
    from fb_bev_amd import _capi
    import torch.nn.functional as Fn
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(cin)
    cp = (cin + 3) // 4 * 4
    x = torch.zeros(1, *dims, cp)
    x[..., :cin] = torch.randn(1, *dims, cin, generator=g)
    x = x.to(dev)
    dy = torch.randn(1, *dims, 80, generator=g).to(dev)
    det_state.set_deterministic(True)
    runs = [_capi.conv3d_wgrad_ndhwc(x, dy, torch.zeros(k ** 3, 80, cp, device=dev), ksize=k, stride=1, pad=pad) for _ in range(3)]
    torch.cuda.synchronize()
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    xt = x.permute(0, 4, 1, 2, 3).contiguous()
    w = torch.zeros(80, cp, k, k, k, device=dev, requires_grad=True)
    Fn.conv3d(xt, w, padding=pad).backward(dy.permute(0, 4, 1, 2, 3))
    ref = w.grad.permute(2, 3, 4, 0, 1).reshape(k ** 3, 80, cp)
    scale = ref.abs().max().item()
    err = (runs[0] - ref).abs().max().item()
    print(f'conv3d wgrad cin={cin} k={k}: max|det - torch| = {err:.2e} on a scale of {scale:.3e}')
    assert err <= 1e-4 * scale
