"""fbbev_rows_linear_f32 / _add / _ln on the MI355X: the exact-fp32 route of the row-wise linear layers against its arithmetic
contract (include/fbbev.h) at the backward projection's real sizes -- EVERY output element equal to a host chain of exact fp32
fmaf's in the order fbbev_rows_linear_f32_k_order returns (tests/rows_linear_f32_ref.py: torch float64 element-wise operations,
run on the device over row chunks; it shares no code with the kernel) -- and the route through the modules (`set_mode`)
against the oracle under the bars of tests/test_gpu_backward_projection.py.  This is the first test that pins the order in which
v_mfma_f32_16x16x4_f32 adds its four products."""
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


def _case(dev, R, I, O, seed, pad_in=8):
    g = torch.Generator().manual_seed(seed)
    xs = (torch.randn(R, I + pad_in, generator=g) * 2).to(dev)
    w = (torch.randn(O, I, generator=g) * 0.2).to(dev)
    b = torch.randn(O, generator=g).to(dev)
    return xs[:, :I], w, b


@pytest.mark.parametrize('R,I,O,relu', [(160000, 80, 64, False), (160000, 80, 128, False), (160000, 80, 512, True),
                                        (160000, 512, 80, False), (20000, 264, 132, False)])
def test_every_element_equals_the_host_chain(dev, R, I, O, relu):
    """plain (strided rows in), `_add` with the 40 000-row positional table, strided `out=` into a wider buffer; no element excluded"""
    from fb_bev_amd import _capi
    import rows_linear_f32_ref as REF
    x, w, b = _case(dev, R, I, O, R + I + O)
    order = _capi.rows_linear_f32_k_order(I)
    assert sorted(order) == list(range(I))
    got = _capi.rows_linear_f32(x, w, b, relu=relu)
    exp = REF.host_chain(x, w, order, b, relu=relu)
    n_diff = int((got != exp).sum())
    print(f'[observed] fbbev_rows_linear_f32 [{R} rows, {I}->{O}, relu={relu}]: elements that differ from the host fmaf chain = '
          f'{n_diff} of {got.numel()}')
    if n_diff:                                           # evidence for the order inside one instruction, should this ever fail
        r, o = [int(v[0]) for v in torch.nonzero(got != exp, as_tuple=True)]
        print(f'  first difference at row {r}, output {o}: kernel {got[r, o].item():.9e}, chain {exp[r, o].item():.9e}')
    assert torch.equal(got, exp)
    P = R // 4
    add = torch.randn(P, I, generator=torch.Generator().manual_seed(P)).to(dev)
    got_a = _capi.rows_linear_f32(x, w, b, relu=relu, addend=add)
    exp_a = REF.host_chain(x, w, order, b, relu=relu, addend=add)
    assert torch.equal(got_a, exp_a)
    assert torch.equal(got_a, _capi.rows_linear_f32((x + add.repeat(4, 1)).contiguous(), w, b, relu=relu))
    wide = torch.full((R, O + 12), float('nan'), device=dev)
    _capi.rows_linear_f32(x, w, b, relu=relu, out=wide[:, 4:4 + O])
    assert torch.equal(wide[:, 4:4 + O], exp) and torch.isnan(wide[:, :4]).all() and torch.isnan(wide[:, 4 + O:]).all()


def test_same_call_twice_and_a_row_block_alone_give_the_same_bits(dev):
    from fb_bev_amd import _capi
    for R, I, O in ((160000, 80, 128), (160000, 512, 80), (20000, 264, 132)):
        x, w, b = _case(dev, R, I, O, 5)
        one, two = _capi.rows_linear_f32(x, w, b, relu=True), _capi.rows_linear_f32(x, w, b, relu=True)
        assert torch.equal(one, two)
        for a, e in ((0, 1), (12345, 12345 + 4097), (R - 700, R), (128 * 7 + 16, 128 * 9)):
            xa = x[a:e] if (a * x.stride(0)) % 4 == 0 else x[a:e].contiguous()
            assert torch.equal(_capi.rows_linear_f32(xa, w, b, relu=True), one[a:e])
    x, w, b = _case(dev, 160000, 80, 80, 6)
    res = torch.randn(160000, 80, device=dev)
    lw, lb = torch.rand(80, device=dev) + 0.5, torch.randn(80, device=dev)
    one = _capi.rows_linear_f32_ln(x, w, b, res, lw, lb, 1e-5)
    assert torch.equal(one, _capi.rows_linear_f32_ln(x, w, b, res, lw, lb, 1e-5))
    assert torch.equal(_capi.rows_linear_f32_ln(x[5000:9001], w, b, res[5000:9001], lw, lb, 1e-5), one[5000:9001])


@pytest.mark.parametrize('R,I,O', [(160000, 80, 80), (160000, 512, 80)])
def test_layernorm_epilogue_against_float64_layer_norm_of_the_host_chain(dev, R, I, O):
    """the bar of the project's own LayerNorm test (atol 2e-6, rtol 1e-5): only the LayerNorm arithmetic is under tolerance"""
    from fb_bev_amd import _capi
    import rows_linear_f32_ref as REF
    g = torch.Generator().manual_seed(R + I)
    x = torch.randn(R, I, generator=g).to(dev)
    w = (torch.randn(O, I, generator=g) / I ** 0.5).to(dev)
    b = (torch.randn(O, generator=g) * 0.3).to(dev)
    res = torch.randn(R, O, generator=g).to(dev)
    lw, lb = (torch.rand(O, generator=g) + 0.5).to(dev), (torch.randn(O, generator=g) * 0.2).to(dev)
    out = _capi.rows_linear_f32_ln(x, w, b, res, lw, lb, 1e-5)
    pre = REF.host_chain(x, w, _capi.rows_linear_f32_k_order(I), b, residual=res)
    ref = F.layer_norm(pre.double(), (O,), lw.double(), lb.double(), 1e-5)
    err = (out.double() - ref).abs().max().item()
    print(f'[observed] fbbev_rows_linear_f32_ln [{R} rows, {I}->{O}, residual=True]: max|err| vs float64 LayerNorm of the host chain = '
          f'{err:.3e} (scale {ref.abs().max().item():.2f})')
    assert torch.allclose(out.double(), ref, atol=2e-6, rtol=1e-5)
    buf = res.clone()                                    # residual == out is allowed
    _capi.rows_linear_f32_ln(x, w, b, buf, lw, lb, 1e-5, out=buf)
    assert torch.equal(buf, out)


def test_absolute_error_at_output_peak_10_is_inside_the_bound_of_the_contract(dev):
    """80 -> 80 at 160 000 rows, inputs scaled so that the output peak is about 10: |got - exact| <= (I + 2) 2^-24 (sum_k |x_k w_k| +
    |b|) element by element (derived from the contract: gamma_K of a K-term fmaf chain on the sum of magnitudes + one rounding of
    the bias add).  The split-operand entry's figure is printed for comparison only."""
    from fb_bev_amd import _capi
    R, I, O = 160000, 80, 80
    g = torch.Generator().manual_seed(16)
    x = (torch.randn(R, I, generator=g) * 2).to(dev)
    w = (torch.randn(O, I, generator=g) * 0.2).to(dev)
    b = torch.randn(O, generator=g).to(dev)
    peak = (x.double() @ w.double().t() + b.double()).abs().max().item()
    x = x * (10.0 / peak) ** 0.5
    w = (w * (10.0 / peak) ** 0.5).contiguous()
    b = b * (10.0 / peak)
    exact = x.double() @ w.double().t() + b.double()
    bound = (I + 2) * 2.0 ** -24 * (x.double().abs() @ w.double().abs().t() + b.double().abs())
    got = _capi.rows_linear_f32(x, w, b)
    got3 = _capi.rows_linear_x3(x, _capi.rows_linear_x3_fragments(w), b, O)
    err, err3 = (got.double() - exact).abs(), (got3.double() - exact).abs()
    print(f'[observed] 80->80 at {R} rows, output peak {exact.abs().max().item():.2f}: max abs err vs float64: fbbev_rows_linear_f32 = '
          f'{err.max().item():.3e}, fbbev_rows_linear_x3 = {err3.max().item():.3e}; smallest bound / error = '
          f'{(bound / err.clamp_min(1e-300)).min().item():.1f}')
    assert (err <= bound).all()


def _count_calls(monkeypatch):
    """counters on every rows_linear wrapper of _capi and on F.linear / torch.addmm (GPU calls only)"""
    from fb_bev_amd import _capi
    calls = {'f32_plain': 0, 'f32_add': 0, 'f32_ln': 0, 'x3': [], 'gemm': []}
    real_f32, real_ln = _capi.rows_linear_f32, _capi.rows_linear_f32_ln

    def f32(x, weight, bias, relu=False, out=None, addend=None):
        calls['f32_add' if addend is not None else 'f32_plain'] += 1
        return real_f32(x, weight, bias, relu=relu, out=out, addend=addend)

    def f32_ln(*a, **kw):
        calls['f32_ln'] += 1
        return real_ln(*a, **kw)

    monkeypatch.setattr(_capi, 'rows_linear_f32', f32)
    monkeypatch.setattr(_capi, 'rows_linear_f32_ln', f32_ln)
    for name in dir(_capi):
        if '_x3' in name and callable(getattr(_capi, name)) and not name.endswith('_supported'):
            real = getattr(_capi, name)
            monkeypatch.setattr(_capi, name, lambda *a, _n=name, _r=real, **kw: (calls['x3'].append(_n), _r(*a, **kw))[1])
    real_linear, real_addmm = F.linear, torch.addmm

    def linear(x, w, b=None):
        if x.is_cuda:
            calls['gemm'].append((x.numel() // max(1, x.shape[-1]), w.shape[1], w.shape[0]))
        return real_linear(x, w, b)

    def addmm(bias, a, bt, **kw):
        if a.is_cuda:
            calls['gemm'].append((a.shape[0], a.shape[1], bt.shape[1]))
        return real_addmm(bias, a, bt, **kw)

    monkeypatch.setattr(F, 'linear', linear)
    monkeypatch.setattr(torch, 'addmm', addmm)
    return calls


def _stats(out, exp):
    err = (out.cpu() - exp).abs()
    bad = (err > 1e-3).any(dim=1).sum().item()
    ok = ~(err > 1e-3).any(dim=1, keepdim=True).expand_as(err)
    return dict(bad=bad, max=err[ok].max().item(), median=err.median().item(), frac4=(err[ok] > 1e-4).float().mean().item())


@pytest.mark.parametrize('setup', ['bev20_L1', 'bev20_L4', 'config2_full'])
def test_module_on_the_new_route_vs_oracle_and_what_it_calls(dev, setup, monkeypatch):
    """BackwardProjection with set_mode('f32_mfma') against oracle/backward_projection_oracle.py under the bars of
    tests/test_gpu_backward_projection.py (bev 20: at most 3 queries beyond 1e-3, median < 1e-5; configs[2] full size, B = 1:
    its BP_FULL_* constants, read from that module), the three modes side by side; on the new route every layer the x3 route would have taken runs the f32 kernel (no
    `*_x3*` wrapper, no vendor GEMM for a shape x3_ok takes); back in the default mode the output equals, bit for bit, the output
    before the mode was ever switched."""
    from fb_bev_amd import rows_linear as RL
    import test_gpu_backward_projection as T
    if setup == 'config2_full':
        bev, L, kw = 200, 4, dict(B=1, num_levels=4, bev=200, shapes=[(16, 44), (32, 88), (8, 22), (4, 11)])
    else:
        bev, L = 20, int(setup[-1])
        kw = dict(num_levels=L, bev=20)
    m, cfg, cam, feats, depth, lss, gcb = T._setup(dev, **kw)
    args = dict(lss_bev=lss.to(dev), cam_params=[t.to(dev) for t in cam], pred_img_depth=depth.to(dev))
    run = lambda: m([f.to(dev) for f in feats], None, **args)  # noqa: E731
    assert RL.mode() == 'x3'
    outs = {}
    try:
        with torch.no_grad():
            outs['x3'] = run()
            RL.set_mode('f32')
            outs['f32'] = run()
            RL.set_mode('f32_mfma')
            calls = _count_calls(monkeypatch)
            outs['f32_mfma'] = run()
            monkeypatch.undo()
            RL.set_mode('x3')
            again = run()
    finally:
        RL.set_mode('x3')
    assert torch.equal(again, outs['x3'])                        # the switch left no stale cache behind
    exp = T._oracle_out(m, cfg, cam, feats, depth, lss, gcb, bev, L)
    st = {k: _stats(v, exp) for k, v in outs.items()}
    for k, s in st.items():
        print(f'[observed] BackwardProjection [{setup}] mode {k:8s} vs oracle: queries beyond 1e-3 = {s["bad"]}, among the rest '
              f'max|err| = {s["max"]:.3e}, median = {s["median"]:.2e}, fraction beyond 1e-4 = {s["frac4"]:.2e}')
    print(f'[observed] BackwardProjection [{setup}] f32_mfma calls: plain {calls["f32_plain"]}, with addend {calls["f32_add"]}, '
          f'with LayerNorm {calls["f32_ln"]}, x3 wrappers {len(calls["x3"])}, vendor GEMMs {calls["gemm"]}')
    s = st['f32_mfma']
    if setup == 'config2_full':
        assert s['bad'] <= T.BP_FULL_BAD_QUERIES, s
        assert s['max'] <= T.BP_FULL_MAX_ERR and s['median'] < 1e-5, s
        assert s['frac4'] <= T.BP_FULL_FRAC_1E4, s
    else:
        assert s['bad'] <= 3 and s['median'] < 1e-5, s
    assert calls['x3'] == []
    for rows, I, O in calls['gemm']:                             # only shapes x3_ok refuses in the default mode as well
        assert rows < RL.X3_MIN_ROWS or I % 8 != 0 or O % 4 != 0, (rows, I, O)
    if setup == 'config2_full':                                  # (at bev 20 a sample has 400 queries: below X3_MIN_ROWS in every mode)
        assert calls['f32_plain'] >= 1 and calls['f32_add'] >= 1 and calls['f32_ln'] >= 1, calls
