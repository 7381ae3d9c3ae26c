"""Routing of the exact-fp32 TRAINING route of fb_bev_amd.rows_linear (mode f32_mfma under autograd -> _RowsLinearF32), on the CPU:
the `_capi` wrappers are replaced by recorders (they are GPU launches) and the "is this a GPU tensor" predicate by True where the
route depends on it."""
import pytest
import torch
import torch.nn.functional as F

from fb_bev_amd import rows_linear as RL
from fb_bev_amd.backward_projection import LayerNorm

ROWS = RL.X3_MIN_ROWS


@pytest.fixture(autouse=True)
def _restore_mode():
    prev = RL.mode()
    yield
    RL.set_mode(prev)


class _Rec:
    """recorders in place of the wrappers of the route, and counters on the vendor products of rows_linear"""

    def __init__(self, monkeypatch, gpu=True):
        self.fwd, self.wgrad, self.vendor = [], [], []

        def rows_linear_f32(x, weight, bias, relu=False, out=None, addend=None):
            self.fwd.append((x, weight, bias, relu, addend))
            return torch.zeros(x.shape[0], weight.shape[0])

        def rows_wgrad_f32(grad_out, x, bias=True):
            self.wgrad.append((grad_out, x, bias))
            return torch.zeros(grad_out.shape[1], x.shape[1]), (torch.zeros(grad_out.shape[1]) if bias else None)

        monkeypatch.setattr(RL._capi, 'rows_linear_f32', rows_linear_f32)
        monkeypatch.setattr(RL._capi, 'rows_wgrad_f32', rows_wgrad_f32, raising=False)
        if gpu:
            monkeypatch.setattr(RL, '_is_gpu', lambda t: True)

        class _F:                                   # rows_linear's view of torch.nn.functional: linear is counted
            def __getattr__(_, name):
                return getattr(F, name)

            def linear(_, *a, **kw):
                self.vendor.append('linear')
                return F.linear(*a, **kw)
        monkeypatch.setattr(RL, 'F', _F())
        real_bmm = torch.bmm
        monkeypatch.setattr(torch, 'bmm', lambda *a, **kw: self.vendor.append('bmm') or real_bmm(*a, **kw))


def _step(m, x, **kw):
    y = m(x, **kw)
    y.sum().backward()
    return y


def test_a_supported_layer_runs_forward_dgrad_and_wgrad_on_the_new_route(monkeypatch):
    r = _Rec(monkeypatch)
    RL.set_mode('f32_mfma')
    m = RL.Linear(16, 24)
    x = torch.randn(2, ROWS // 2, 16, requires_grad=True)                  # (B, Q, C): reshaped to rows outside the function
    y = _step(m, x)
    assert type(y.grad_fn).__name__ != 'RowsLinearBackward' and y.shape == (2, ROWS // 2, 24)
    assert len(r.fwd) == 2 and len(r.wgrad) == 1 and r.vendor == []
    fx, fw, fb, relu, addend = r.fwd[0]                                    # the forward: bias inside, no ReLU, no addend
    assert fx.shape == (ROWS, 16) and torch.equal(fw, m.weight.detach()) and torch.equal(fb, m.bias.detach()) and not relu and addend is None
    gx_in, wt, no_bias, _, _ = r.fwd[1]                                    # the input gradient: the same entry on W^T
    assert gx_in.shape == (ROWS, 24) and wt.shape == (16, 24) and wt.is_contiguous() and torch.equal(wt, m.weight.detach().t())
    assert no_bias is None
    gy, xs, want_b = r.wgrad[0]
    assert gy.shape == (ROWS, 24) and xs.shape == (ROWS, 16) and want_b is True
    assert x.grad.shape == x.shape and m.weight.grad.shape == (24, 16) and m.bias.grad.shape == (24,)


def test_relu_addend_and_layernorm_stay_separate_steps(monkeypatch):
    r = _Rec(monkeypatch)
    RL.set_mode('f32_mfma')
    m = RL.Linear(16, 8)
    norm = LayerNorm(8)
    x = torch.randn(ROWS, 16, requires_grad=True)
    add = torch.randn(ROWS, 16)
    _step(m, x, relu=True, addend=add)
    assert len(r.fwd) == 2 and torch.equal(r.fwd[0][0], (x + add).detach()) and r.fwd[0][3] is False and r.fwd[0][4] is None
    _step(m, x, ln=(torch.randn(ROWS, 8), norm))
    assert len(r.fwd) == 4 and len(r.wgrad) == 2 and r.vendor == [] and norm.weight.grad is not None


def test_transformed_weights_reach_the_function_differentiably(monkeypatch):
    r = _Rec(monkeypatch)
    RL.set_mode('f32_mfma')
    w, b = torch.nn.Parameter(torch.randn(8, 16)), torch.nn.Parameter(torch.randn(8))
    perm = torch.tensor([7, 6, 5, 4, 3, 2, 1, 0])
    x = torch.randn(ROWS, 16)
    y = RL.linear_rows(x, w, b, cache=RL.X3Weights(), transform=lambda w_, b_: (w_[perm], b_[perm]))
    y.sum().backward()
    assert len(r.fwd) == 1 and len(r.wgrad) == 1 and r.vendor == []        # frozen input: no dgrad call
    assert torch.equal(r.fwd[0][1], w.detach()[perm]) and w.grad is not None and b.grad is not None


@pytest.mark.parametrize('what', ['out_features', 'in_features', 'rows', 'cpu', 'no_grad_needed'])
def test_unsupported_cases_take_todays_path(what, monkeypatch):
    """each case beside the supported layer it differs from in ONE respect, in the same mode and under the same recorders: the
    supported layer reaches the route, the other one does not"""
    r = _Rec(monkeypatch)                                                  # "GPU" tensors
    RL.set_mode('f32_mfma')
    _step(RL.Linear(16, 8), torch.randn(ROWS, 16, requires_grad=True))
    assert len(r.fwd) == 2 and len(r.wgrad) == 1 and r.vendor == []
    r.fwd.clear(), r.wgrad.clear()
    if what == 'cpu':
        monkeypatch.setattr(RL, '_is_gpu', lambda t: t.is_cuda)            # the real predicate: these are CPU tensors
    I, O, R = (12 if what == 'in_features' else 16), (12 if what == 'out_features' else 8), (ROWS - 1 if what == 'rows' else ROWS)
    m = RL.Linear(I, O)
    x = torch.randn(R, I, requires_grad=what != 'no_grad_needed')
    if what == 'no_grad_needed':
        m.requires_grad_(False)
        y = m(x)
        assert y.grad_fn is None
    else:
        y = _step(m, x)
        assert 'RowsLinearF32' not in type(y.grad_fn).__name__
    assert r.fwd == [] and r.wgrad == [] and 'linear' in r.vendor
    assert torch.equal(y, F.linear(x, m.weight, m.bias))


@pytest.mark.parametrize('mode', ['x3', 'f32'])
def test_other_modes_never_reach_the_new_code(mode, monkeypatch):
    r = _Rec(monkeypatch)
    RL.set_mode(mode)
    m = RL.Linear(16, 8)
    x = torch.randn(ROWS, 16, requires_grad=True)
    y = _step(m, x)
    assert r.fwd == [] and r.wgrad == [] and r.vendor == ['linear']
    assert torch.equal(y, F.linear(x, m.weight, m.bias))


def test_frozen_weight_skips_the_wgrad_call_and_frozen_input_the_dgrad_call(monkeypatch):
    r = _Rec(monkeypatch)
    RL.set_mode('f32_mfma')
    m = RL.Linear(16, 8)
    m.requires_grad_(False)
    x = torch.randn(ROWS, 16, requires_grad=True)
    _step(m, x)
    assert len(r.fwd) == 2 and r.wgrad == [] and x.grad is not None        # forward + dgrad
    m.requires_grad_(True)
    r.fwd.clear()
    _step(m, torch.randn(ROWS, 16))
    assert len(r.fwd) == 1 and len(r.wgrad) == 1 and r.wgrad[0][2] is True  # forward + wgrad (with the bias gradient)
    m.bias.requires_grad_(False)
    _step(m, torch.randn(ROWS, 16))
    assert r.wgrad[-1][2] is False and m.weight.grad is not None
    assert r.vendor == []
