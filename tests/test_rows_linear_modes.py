"""The row-wise-layer switch of fb_bev_amd.rows_linear: x3 (default) / f32 (vendor GEMM) / f32_mfma (exact fp32 on the FP32 MFMA).
Routing only, on the CPU: the `_capi` wrappers are replaced by counters (they are GPU launches), tensors are made to look like
GPU tensors where the route depends on it."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import fb_bev_amd
from fb_bev_amd import rows_linear as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _restore_mode():
    prev = RL.mode()
    yield
    RL.set_mode(prev)


def test_set_mode_round_trips_and_rejects_unknown_names():
    assert RL.mode() == 'x3' and RL.X3 is True and RL.F32_MFMA is False          # the suite runs in the default mode
    assert RL.set_mode('f32_mfma') == 'x3'
    assert (RL.X3, RL.F32_MFMA, RL.mode()) == (False, True, 'f32_mfma')
    assert RL.set_mode('f32') == 'f32_mfma'
    assert (RL.X3, RL.F32_MFMA, RL.mode()) == (False, False, 'f32')
    assert fb_bev_amd.set_rows_linear_mode('x3') == 'f32'                         # the package-level name is the same switch
    assert (RL.X3, RL.F32_MFMA, RL.mode()) == (True, False, 'x3')
    for bad in ('fp32', '', None, 'X3'):
        with pytest.raises(ValueError):
            RL.set_mode(bad)
    assert RL.mode() == 'x3'
    RL.X3 = False                              # flipping the flag directly (the benchmark's A/B) is the vendor-GEMM route
    assert RL.mode() == 'f32'
    RL.X3 = True
    RL.set_mode('f32_mfma')
    RL.X3 = True                               # by hand on top of f32_mfma: X3 wins, the x3 route with its fragments -- no fourth state
    assert RL.mode() == 'x3' and not RL.f32_mfma_on()


@pytest.mark.parametrize('env,exp', [(None, (True, False, 'x3')), ('x3', (True, False, 'x3')), ('f32', (False, False, 'f32')),
                                     ('f32_mfma', (False, True, 'f32_mfma'))])
def test_environment_variable_sets_the_initial_mode(env, exp):
    e = {k: v for k, v in os.environ.items() if k != 'FBBEV_ROWS_LINEAR'}
    if env is not None:
        e['FBBEV_ROWS_LINEAR'] = env
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    out = subprocess.run([sys.executable, '-c', 'from fb_bev_amd import rows_linear as R; print(R.X3, R.F32_MFMA, R.mode())'],
                         env=e, capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(exp[0]), str(exp[1]), exp[2]]


class _Counters:
    def __init__(self, monkeypatch):
        self.calls = {n: 0 for n in ('rows_linear_x3_fragments', 'rows_linear_x3', 'rows_linear_x3_ln', 'rows_linear_f32',
                                     'rows_linear_f32_ln')}
        self.last = {}

        def fake(name, out_features):
            def f(x, *a, **kw):
                self.calls[name] += 1
                self.last[name] = (a, kw)
                return torch.zeros(x.shape[0], out_features(x, a, kw))
            return f
        monkeypatch.setattr(RL._capi, 'rows_linear_x3_fragments',
                            lambda w: self.calls.__setitem__('rows_linear_x3_fragments', self.calls['rows_linear_x3_fragments'] + 1) or
                            torch.zeros(16, dtype=torch.uint8))
        monkeypatch.setattr(RL._capi, 'rows_linear_x3', fake('rows_linear_x3', lambda x, a, kw: a[2]))
        monkeypatch.setattr(RL._capi, 'rows_linear_x3_ln', fake('rows_linear_x3_ln', lambda x, a, kw: a[2]))
        monkeypatch.setattr(RL._capi, 'rows_linear_f32', fake('rows_linear_f32', lambda x, a, kw: a[0].shape[0]))
        monkeypatch.setattr(RL._capi, 'rows_linear_f32_ln', fake('rows_linear_f32_ln', lambda x, a, kw: a[0].shape[0]))


def test_default_mode_never_calls_the_f32_wrappers_and_the_new_mode_never_builds_fragments(monkeypatch):
    c = _Counters(monkeypatch)
    monkeypatch.setattr(RL, 'x3_ok', lambda x, i, o: (RL.X3 or RL.F32_MFMA) and not torch.is_grad_enabled())   # "a GPU tensor"
    monkeypatch.setattr(RL, 'ln_fusable', lambda *a: True)
    m = RL.Linear(16, 8)
    norm = torch.nn.LayerNorm(8)
    x = torch.randn(4096, 16)
    with torch.no_grad():
        m(x)
        m(x, relu=True)
        m(x, ln=(torch.randn(4096, 8), norm))
        assert c.calls == {'rows_linear_x3_fragments': 1, 'rows_linear_x3': 2, 'rows_linear_x3_ln': 1, 'rows_linear_f32': 0,
                           'rows_linear_f32_ln': 0}
        assert m._x3.frag is not None
        RL.set_mode('f32_mfma')                                                  # a live cache: the mode is part of its key
        m(x)
        assert m._x3.frag is None and torch.equal(m._x3.w, m.weight.detach()) and m._x3.w.data_ptr() % 16 == 0
        m(x, relu=True)
        assert c.last['rows_linear_f32'][1]['relu'] is True and c.last['rows_linear_f32'][0][0] is m._x3.w
        m(x, ln=(torch.randn(4096, 8), norm))
        assert c.calls == {'rows_linear_x3_fragments': 1, 'rows_linear_x3': 2, 'rows_linear_x3_ln': 1, 'rows_linear_f32': 2,
                           'rows_linear_f32_ln': 1}
        RL.set_mode('x3')                                                        # and back: fragments again
        m(x)
        assert c.calls['rows_linear_x3_fragments'] == 2 and c.calls['rows_linear_x3'] == 3 and m._x3.frag is not None
        RL.set_mode('f32')                                                       # vendor GEMM: none of the wrappers
        before = dict(c.calls)
        y = m(x)
        assert c.calls == before and torch.equal(y, F.linear(x, m.weight, m.bias))
    y = m(x)                                                                     # autograd on: nothing changes in any mode
    assert c.calls == before and y.grad_fn is not None


def test_transform_hook_applies_on_the_new_route(monkeypatch):
    c = _Counters(monkeypatch)
    RL.set_mode('f32_mfma')
    w, b = torch.nn.Parameter(torch.randn(8, 16)), torch.nn.Parameter(torch.randn(8))
    perm = torch.tensor([7, 6, 5, 4, 3, 2, 1, 0])
    cache = RL.X3Weights().get(w, b, lambda w_, b_: (w_[perm], b_[perm]))
    assert cache.frag is None and torch.equal(cache.w, w.detach()[perm]) and torch.equal(cache.b, b.detach()[perm])
    assert c.calls['rows_linear_x3_fragments'] == 0


@pytest.mark.parametrize('mode', ['x3', 'f32', 'f32_mfma'])
def test_cpu_tensors_fall_through_to_f_linear_in_every_mode(mode, monkeypatch):
    c = _Counters(monkeypatch)
    RL.set_mode(mode)
    m = RL.Linear(8, 5)
    ref = torch.nn.Linear(8, 5)
    ref.load_state_dict(m.state_dict())
    x = torch.randn(40000, 8, requires_grad=True)
    y = m(x)
    assert y.grad_fn is not None and 'RowsLinear' not in type(y.grad_fn).__name__     # CPU: autograd's own linear
    assert torch.equal(y, ref(x))
    with torch.no_grad():
        assert torch.equal(m(x), ref(x)) and torch.equal(m(x, relu=True), ref(x).relu())
    assert not any(c.calls.values())



def test_x3_set_by_hand_on_top_of_f32_mfma_builds_fragments(monkeypatch):
    """`rows_linear.X3 = True` while F32_MFMA is still set must not hand `frag = None` to an x3 kernel"""
    c = _Counters(monkeypatch)
    RL.set_mode('f32_mfma')
    monkeypatch.setattr(RL, 'X3', True)
    w = torch.nn.Parameter(torch.randn(8, 16))
    cache = RL.X3Weights().get(w, None)
    assert cache.frag is not None and c.calls['rows_linear_x3_fragments'] == 1
