"""The exact-fp32 TRAINING route of the row-wise linear layers on the MI355X: fbbev_rows_wgrad_f32 against its arithmetic contract
(include/fbbev.h) -- every element of grad_weight / grad_bias equal to the two-stage host chain of tests/rows_wgrad_f32_ref.py (exact
fp32 fmaf's over each slice's rows in ascending order, slices added in ascending order) up to the backward projection's real size --
and `_RowsLinearF32` (mode f32_mfma under autograd) alone and inside one training step of BackwardProjection.  No tolerance except
in the derived-bound test, whose bound follows from the contract."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _case(dev, R, I, O, seed, strided=False):
    g = torch.Generator().manual_seed(seed)
    gy = torch.randn(R, O + (12 if strided else 0), generator=g).to(dev)
    x = (torch.randn(R, I + (8 if strided else 0), generator=g) * 2).to(dev)
    return gy[:, :O], x[:, :I]


def _check_entry(dev, R, I, O, strided=False, twice=False):
    from fb_bev_amd import _capi
    from rows_wgrad_f32_ref import two_stage_chain
    gy, x = _case(dev, R, I, O, R + I + O, strided)
    L = _capi.rows_wgrad_f32_slice_rows(R, I, O)
    assert L > 0 and L % 4 == 0
    gw, gb = _capi.rows_wgrad_f32(gy, x)
    ew, eb = two_stage_chain(gy, x, L)
    nw, nb = int((gw != ew).sum()), int((gb != eb).sum())
    print(f'[observed] fbbev_rows_wgrad_f32 [{R} rows, {I}->{O}, strided={strided}]: slice {L} rows x {(R + L - 1) // L}; elements that '
          f'differ from the two-stage host chain: grad_weight {nw} of {gw.numel()}, grad_bias {nb} of {gb.numel()}')
    assert torch.equal(gw, ew) and torch.equal(gb, eb)
    gw_only, none = _capi.rows_wgrad_f32(gy, x, bias=False)
    assert none is None and torch.equal(gw_only, gw)
    if twice:
        gw2, gb2 = _capi.rows_wgrad_f32(gy, x)
        assert torch.equal(gw2, gw) and torch.equal(gb2, gb)


@pytest.mark.parametrize('I,O,strided', [(80, 64, False), (80, 160, False), (320, 80, False), (264, 136, False), (80, 512, False),
                                         (80, 160, True)])
def test_entry_equals_the_host_chain_at_two_slices_and_a_tail(dev, I, O, strided):
    from fb_bev_amd import _capi
    L = _capi.rows_wgrad_f32_slice_rows(3, I, O)
    R = 2 * L + 37
    assert _capi.rows_wgrad_f32_slice_rows(R, I, O) == L
    _check_entry(dev, R, I, O, strided, twice=(I, O) == (80, 64))


def test_entry_equals_the_host_chain_at_five_rows(dev):
    _check_entry(dev, 5, 8, 8)


@pytest.fixture(scope='module')
def real_size(dev):
    """160 000 rows, 80 -> 64 (BASELINE configs[2], B = 4): the operands, the entry's result and the slice length, computed once"""
    from fb_bev_amd import _capi
    R, I, O = 160000, 80, 64
    gy, x = _case(dev, R, I, O, 7)
    gw, gb = _capi.rows_wgrad_f32(gy, x)
    return gy, x, gw, gb, _capi.rows_wgrad_f32_slice_rows(R, I, O)


def test_entry_equals_the_host_chain_at_the_real_size(dev, real_size):
    from fb_bev_amd import _capi
    from rows_wgrad_f32_ref import two_stage_chain
    gy, x, gw, gb, L = real_size
    assert L > _capi.rows_wgrad_f32_slice_rows(3, 80, 64)               # not the shortest slice: the length follows the row count
    ew, eb = two_stage_chain(gy, x, L)
    print(f'[observed] fbbev_rows_wgrad_f32 [160000 rows, 80->64]: slice {L} rows x {(gy.shape[0] + L - 1) // L}; elements that differ '
          f'from the two-stage host chain: grad_weight {int((gw != ew).sum())} of {gw.numel()}, grad_bias {int((gb != eb).sum())} of '
          f'{gb.numel()}')
    assert torch.equal(gw, ew) and torch.equal(gb, eb)
    gw2, gb2 = _capi.rows_wgrad_f32(gy, x)                               # the same bits both times
    assert torch.equal(gw2, gw) and torch.equal(gb2, gb)


def test_error_against_float64_is_inside_the_bound_of_the_contract_at_the_real_size(dev, real_size):
    """|gW - gW64| <= 1.06 (L + S) 2^-24 sum_r |gy x| per element: the first-order bound of a length-L fmaf chain (gamma_L on the sum of
    magnitudes) plus S - 1 adds, 1.06 for the higher-order terms ((L + S) 2^-24 < 1e-4); the same bound for gb with |gy|.  Derived
    from the contract, not measured."""
    gy, x, gw, gb, L = real_size
    R = gy.shape[0]
    S = (R + L - 1) // L
    gyd, xd = gy.double(), x.double()
    exact_w, mag_w = gyd.t() @ xd, gyd.abs().t() @ xd.abs()
    exact_b, mag_b = gyd.sum(0), gyd.abs().sum(0)
    k = 1.06 * (L + S) * 2.0 ** -24
    err_w, err_b = (gw.double() - exact_w).abs(), (gb.double() - exact_b).abs()
    print(f'[observed] fbbev_rows_wgrad_f32 [160000 rows, 80->64] vs float64: L = {L}, S = {S}; max abs err grad_weight '
          f'{err_w.max().item():.3e} (scale {exact_w.abs().max().item():.1f}), grad_bias {err_b.max().item():.3e}; smallest bound / error '
          f'margin: grad_weight {(k * mag_w / err_w.clamp_min(1e-300)).min().item():.1f}, grad_bias '
          f'{(k * mag_b / err_b.clamp_min(1e-300)).min().item():.1f}')
    assert (err_w <= k * mag_w).all() and (err_b <= k * mag_b).all()


def _chains(gy, x, w):
    """the three gradients of one layer from the host chains: (gx, gW, gb) for gy (R, O), x (R, I), w (O, I)"""
    from fb_bev_amd import _capi
    import rows_linear_f32_ref as REF
    from rows_wgrad_f32_ref import two_stage_chain
    O, I = w.shape
    gx = REF.host_chain(gy.contiguous(), w.t().contiguous(), _capi.rows_linear_f32_k_order(O))
    gw, gb = two_stage_chain(gy, x, _capi.rows_wgrad_f32_slice_rows(gy.shape[0], I, O))
    return gx, gw, gb


def test_autograd_function_forward_and_three_gradients_bit_for_bit(dev):
    from fb_bev_amd import rows_linear as RL
    R, I, O = 4096, 80, 64
    torch.manual_seed(11)
    lin = RL.Linear(I, O).to(dev)
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(R, I, generator=g) * 2).to(dev).requires_grad_()
    gy = torch.randn(R, O, generator=g).to(dev)
    prev = RL.set_mode('f32_mfma')
    try:
        y = lin(x)
        node = y.grad_fn                                                 # linear_rows reshapes outside the function: a view node on top
        while node is not None and type(node).__name__ != '_RowsLinearF32Backward' and node.next_functions:
            node = node.next_functions[0][0]
        assert type(node).__name__ == '_RowsLinearF32Backward'
        with torch.no_grad():
            y0 = lin(x)
        y.backward(gy)
    finally:
        RL.set_mode(prev)
    assert torch.equal(y.detach(), y0)                                   # the same kernel with and without grad
    gx, gw, gb = _chains(gy, x.detach(), lin.weight.detach())
    assert torch.equal(x.grad, gx)
    assert torch.equal(lin.weight.grad, gw) and torch.equal(lin.bias.grad, gb)


def test_one_training_step_of_the_module_on_the_exact_route(dev, monkeypatch):
    """BackwardProjection, 48 x 48 queries (2 304 rows >= X3_MIN_ROWS), B = 1, one feature level, mode f32_mfma under autograd: every
    Linear of a supported shape runs forward, dgrad and wgrad through _RowsLinearF32 (no row-wise vendor GEMM for such a shape), the
    gradients are finite, two deterministic steps give the same bits, and the (gy, x, w) captured inside the backward of the narrowest
    and the widest layer reproduce what that backward returned from the host chains -- real, partly masked data, no tolerance."""
    import fb_bev_amd
    from fb_bev_amd import _capi, rows_linear as RL
    import test_gpu_backward_projection as T
    m, cfg, cam, feats, depth, lss, gcb = T._setup(dev, B=1, num_levels=1, bev=48, seed=4)
    cam_g = [t.to(dev) for t in cam]
    w_out = torch.randn(1, 80, 48, 48, generator=torch.Generator().manual_seed(9)).to(dev)
    calls = {'fwd': 0, 'dgrad': 0, 'wgrad': 0, 'gemm': []}
    captured = []
    real_f32, real_wgrad, real_bwd = _capi.rows_linear_f32, _capi.rows_wgrad_f32, RL._RowsLinearF32.backward
    in_bwd = [False]

    def f32(x, weight, bias, **kw):
        calls['dgrad' if in_bwd[0] else 'fwd'] += 1
        return real_f32(x, weight, bias, **kw)

    def wgrad(grad_out, x, bias=True):
        calls['wgrad'] += 1
        return real_wgrad(grad_out, x, bias=bias)

    def backward(ctx, gy):
        in_bwd[0] = True
        try:
            out = real_bwd(ctx, gy)
        finally:
            in_bwd[0] = False
        x, w = ctx.saved_tensors
        captured.append((gy.detach().float().clone(), x, w, out))
        return out

    real_linear, real_addmm = F.linear, torch.addmm

    def linear(x, w, b=None):
        if x.is_cuda:
            calls['gemm'].append((x.numel() // max(1, x.shape[-1]), w.shape[1], w.shape[0]))
        return real_linear(x, w, b)

    def addmm(bias, a, bt, **kw):
        if a.is_cuda:
            calls['gemm'].append((a.shape[0], a.shape[1], bt.shape[1]))
        return real_addmm(bias, a, bt, **kw)

    def step():
        m.zero_grad(set_to_none=True)
        f_g = [f.to(dev).requires_grad_() for f in feats]
        d_g, l_g = depth.to(dev).requires_grad_(), lss.to(dev).requires_grad_()
        out = m(f_g, None, lss_bev=l_g, cam_params=cam_g, pred_img_depth=d_g)
        (out * w_out).sum().backward()
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        grads.update({'feats0': f_g[0].grad.clone(), 'depth': d_g.grad.clone(), 'lss': l_g.grad.clone()})
        return grads

    prev = RL.set_mode('f32_mfma')
    fb_bev_amd.set_deterministic(True)
    try:
        monkeypatch.setattr(_capi, 'rows_linear_f32', f32)
        monkeypatch.setattr(_capi, 'rows_wgrad_f32', wgrad)
        monkeypatch.setattr(RL._RowsLinearF32, 'backward', staticmethod(backward))
        monkeypatch.setattr(F, 'linear', linear)
        monkeypatch.setattr(torch, 'addmm', addmm)
        g1 = step()
        monkeypatch.undo()
        first = list(captured)
        g2 = step()
    finally:
        fb_bev_amd.set_deterministic(None)
        RL.set_mode(prev)
    n_lin = sum(isinstance(x, RL.Linear) for x in m.modules())
    print(f'[observed] BackwardProjection training step [bev 48, B=1, L=1] on f32_mfma: {n_lin} Linear modules; _RowsLinearF32 forward '
          f'{calls["fwd"]}, dgrad {calls["dgrad"]}, wgrad {calls["wgrad"]}; vendor GEMM shapes (rows, in, out) {sorted(set(calls["gemm"]))}')
    assert calls['fwd'] + len(calls['gemm']) >= n_lin                    # every Linear was called: on the route, or with a shape it refuses
    assert calls['fwd'] >= 1 and calls['fwd'] == len(first)              # one backward per forward
    assert calls['wgrad'] == calls['fwd'] and 0 < calls['dgrad'] <= calls['fwd']
    for rows, I, O in calls['gemm']:                                     # only shapes the route refuses
        assert rows < RL.X3_MIN_ROWS or I % 8 != 0 or O % 8 != 0, (rows, I, O)
    assert g1.keys() == g2.keys() and len(g1) > n_lin
    for n in g1:
        assert torch.isfinite(g1[n]).all(), n
        assert torch.equal(g1[n], g2[n]), n
    by_width = sorted(first, key=lambda c: c[2].shape[0] * c[2].shape[1])
    for gy, x, w, (gx, gw, gb) in (by_width[0], by_width[-1]):
        ex, ew, eb = _chains(gy, x, w)
        print(f'[observed]   captured layer {w.shape[1]}->{w.shape[0]} at {gy.shape[0]} rows: zero rows of gy '
              f'{int((gy == 0).all(1).sum())}; returned gx {gx is not None}, gW {gw is not None}, gb {gb is not None}')
        assert gw is not None and torch.equal(gw, ew)
        assert gb is None or torch.equal(gb, eb)
        assert gx is None or torch.equal(gx, ex)
