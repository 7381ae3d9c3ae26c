"""fbbev_rows_linear_f32 / _add / _ln / _k_order on the CPU emulator: the exact-fp32 route of the row-wise linear layers against
its arithmetic contract (include/fbbev.h) -- every output element is ONE chain of fp32 fmaf's in the order
fbbev_rows_linear_f32_k_order returns, then one add of the bias, one of the residual, ReLU.  The host reference below shares no
code with the kernel: an exact fmaf built from float64 operations (round-to-odd + one final rounding), pinned against libm."""
import ctypes
import os
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))
import emu_capi as E  # noqa: E402


# ------------------------------------------------------------------ host reference
def fmaf32(a, b, c):                       # float32 arrays -> float32, == libm fmaf element-wise
    a, b, c = (t.astype(np.float64) for t in (a, b, c))
    p = a * b                              # exact: 24 + 24 bits
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)          # TwoSum: the exact error of s
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)   # round to odd
    return s.astype(np.float32)            # one final rounding to nearest


def k_order(I):
    buf = (ctypes.c_int * I)()
    assert E.lib().fbbev_rows_linear_f32_k_order(I, ctypes.cast(buf, c_void_p)) == 0
    return list(buf)


def host_chain(x, w, b=None, relu=False, residual=None):
    """steps 1-3 of the contract on float32 tensors x (R, I), w (O, I): (R, O) float32"""
    xn, wn = x.contiguous().numpy(), w.contiguous().numpy()
    acc = np.zeros((xn.shape[0], wn.shape[0]), dtype=np.float32)
    for k in k_order(xn.shape[1]):
        acc = fmaf32(np.ascontiguousarray(np.broadcast_to(wn[None, :, k], acc.shape)),
                     np.ascontiguousarray(np.broadcast_to(xn[:, k, None], acc.shape)), acc)
    y = torch.from_numpy(acc)
    if b is not None:
        y = y + b
    if residual is not None:
        y = y + residual
    return y.relu() if relu else y


def run(x, w, b, relu=False, out=None, addend=None):
    O, I = w.shape
    R = x.shape[0]
    if out is None:
        out = torch.full((R, O), float('nan'))
    bp = E.p(b) if b is not None else None
    if addend is None:
        code = E.lib().fbbev_rows_linear_f32(c_void_p(x.data_ptr()), x.stride(0), E.p(w), bp, R, I, O, 1 if relu else 0,
                                             c_void_p(out.data_ptr()), out.stride(0), None)
    else:
        code = E.lib().fbbev_rows_linear_f32_add(c_void_p(x.data_ptr()), x.stride(0), c_void_p(addend.data_ptr()), addend.stride(0),
                                                 addend.shape[0], E.p(w), bp, R, I, O, 1 if relu else 0, c_void_p(out.data_ptr()),
                                                 out.stride(0), None)
    return code, out


def run_ln(x, w, b, res, lw, lb, eps):
    O, I = w.shape
    R = x.shape[0]
    out = torch.full((R, O), float('nan'))
    code = E.lib().fbbev_rows_linear_f32_ln(c_void_p(x.data_ptr()), x.stride(0), E.p(w), E.p(b) if b is not None else None, R, I, O,
                                            c_void_p(res.data_ptr()) if res is not None else None,
                                            res.stride(0) if res is not None else 0, E.p(lw), E.p(lb), eps,
                                            c_void_p(out.data_ptr()), out.stride(0), None)
    return code, out


SHAPES = [(300, 80, 128, False), (130, 80, 64, False), (257, 80, 96, False), (129, 80, 512, True), (200, 512, 80, False),
          (64, 80, 320, True), (50, 8, 4, False), (1, 264, 132, True)]


def _case(R, I, O):
    g = torch.Generator().manual_seed(R + I + O)
    xs = torch.randn(R, I + 8, generator=g) * 2
    w = torch.randn(O, I, generator=g) * 0.2
    b = torch.randn(O, generator=g) if O != 64 else None
    return xs[:, :I], w, b                                             # row stride I + 8


# ------------------------------------------------------------------ the helper itself
def test_host_fmaf_equals_libm():
    libm = ctypes.CDLL('libm.so.6')
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = np.where(np.arange(4000) % 2 == 0, -(a * b), rng.standard_normal(4000).astype(np.float32)).astype(np.float32)   # cancellation-heavy half
    pinned = [(1 + 2.0 ** -23, 1 - 2.0 ** -23, 2.0 ** 24 + 2), (3.0, 1 / 3, -1.0), (1e-30, 1e-30, 1.0), (16777216.0, 1.0, 1.0),
              (-0.0, 5.0, 0.0), (1.5, 2.0 ** -24, 1.0)]
    a = np.concatenate([a, np.array([t[0] for t in pinned], dtype=np.float32)])
    b = np.concatenate([b, np.array([t[1] for t in pinned], dtype=np.float32)])
    c = np.concatenate([c, np.array([t[2] for t in pinned], dtype=np.float32)])
    exp = np.array([libm.fmaf(float(p), float(q), float(r)) for p, q, r in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(fmaf32(a, b, c), exp)
    # the targeted double-rounding case: the plain float64 form rounds twice and is wrong there
    p, q, r = (np.array([v], dtype=np.float32) for v in pinned[0])
    plain = (p.astype(np.float64) * q.astype(np.float64) + r.astype(np.float64)).astype(np.float32)
    assert plain[0] != exp[4000] and fmaf32(p, q, r)[0] == exp[4000]


def test_torch_form_of_the_host_reference_equals_libm_and_the_numpy_form():
    """tests/rows_linear_f32_ref.py (the form the GPU tests run in float64 on the device) on the CPU"""
    import rows_linear_f32_ref as REF
    libm = ctypes.CDLL('libm.so.6')
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(3000, generator=g), torch.randn(3000, generator=g)
    c = torch.where(torch.arange(3000) % 2 == 0, -(a * b), torch.randn(3000, generator=g))
    pin = torch.tensor([[1 + 2.0 ** -23, 1 - 2.0 ** -23, 2.0 ** 24 + 2], [3.0, 1 / 3, -1.0], [16777216.0, 1.0, 1.0], [1.5, 2.0 ** -24, 1.0]])
    a, b, c = torch.cat([a, pin[:, 0]]), torch.cat([b, pin[:, 1]]), torch.cat([c, pin[:, 2]])
    exp = torch.tensor([libm.fmaf(float(p), float(q), float(r)) for p, q, r in zip(a, b, c)])
    assert torch.equal(REF.fmaf32(a, b, c), exp)
    x, w, bias = _case(257, 80, 96)
    add = torch.randn(257, 80, generator=g)
    assert torch.equal(REF.host_chain(x, w, k_order(80), bias, relu=True, chunk=100), host_chain(x, w, bias, True))
    assert torch.equal(REF.host_chain(x, w, k_order(80), bias, addend=add[:1], chunk=100), host_chain(x + add[:1], w, bias))


# ------------------------------------------------------------------ 1. the order
@pytest.mark.parametrize('I', [8, 16, 80, 264, 320, 512])
def test_k_order_is_a_fixed_permutation(I):
    o1, o2 = k_order(I), k_order(I)
    assert sorted(o1) == list(range(I)) and o1 == o2


def test_k_order_rejects_bad_arguments():
    buf = (ctypes.c_int * 8)()
    assert E.lib().fbbev_rows_linear_f32_k_order(0, ctypes.cast(buf, c_void_p)) == -1
    assert E.lib().fbbev_rows_linear_f32_k_order(-8, ctypes.cast(buf, c_void_p)) == -1
    assert E.lib().fbbev_rows_linear_f32_k_order(8, None) == -1


# ------------------------------------------------------------------ 2. bits == the host chain
@pytest.mark.parametrize('R,I,O,relu', SHAPES)
def test_rows_linear_f32_equals_the_host_chain_exactly(R, I, O, relu):
    x, w, b = _case(R, I, O)
    outs = torch.full((R, O + 4), float('nan'))
    code, got = run(x, w, b, relu=relu, out=outs[:, :O])
    assert code == 0
    assert not torch.isnan(got).any() and torch.isnan(outs[:, O:]).all()          # nothing written beyond the output columns
    exp = host_chain(x, w, b, relu)
    assert torch.equal(got, exp), (got - exp).abs().max()


# ------------------------------------------------------------------ 3. the addend
@pytest.mark.parametrize('R,P,I,O', [(5 * 28, 28, 80, 128), (3 * 100, 100, 512, 80), (90, 45, 80, 64)])
def test_addend_entry_equals_plain_entry_on_the_sum(R, P, I, O):
    """period 28 / 100 / 45: does not divide the 128-row (or the 16-row) tile"""
    x, w, b = _case(R, I, O)
    g = torch.Generator().manual_seed(P)
    add = torch.randn(P, I + 4, generator=g)[:, :I]
    code, got = run(x, w, b, relu=True, addend=add)
    assert code == 0 and not torch.isnan(got).any()
    xs = (x + add.repeat(R // P, 1)).contiguous()
    code, plain = run(xs, w, b, relu=True)
    assert code == 0 and torch.equal(got, plain)
    assert torch.equal(got, host_chain(xs, w, b, True))


# ------------------------------------------------------------------ 4. LayerNorm epilogue
@pytest.mark.parametrize('rows,I,O,with_res', [(200, 80, 80, True), (130, 320, 80, True), (70, 80, 64, False), (33, 16, 20, True)])
def test_layernorm_epilogue_against_float64_layer_norm_of_the_host_chain(rows, I, O, with_res):
    g = torch.Generator().manual_seed(rows + O)
    x = torch.randn(rows, I, generator=g)
    w = torch.randn(O, I, generator=g) / I ** 0.5
    b = torch.randn(O, generator=g) * 0.3
    res = torch.randn(rows, O, generator=g) if with_res else None
    lw, lb = torch.rand(O, generator=g) + 0.5, torch.randn(O, generator=g) * 0.2
    code, out = run_ln(x, w, b, res, lw, lb, 1e-5)
    assert code == 0 and not torch.isnan(out).any()
    pre = host_chain(x, w, b, False, residual=res)                     # only the LayerNorm arithmetic is under tolerance
    ref = F.layer_norm(pre.double(), (O,), lw.double(), lb.double(), 1e-5)
    err = (out.double() - ref).abs().max().item()
    print(f'rows_linear_f32_ln {rows}x{I}->{O}: max abs err vs float64 LayerNorm of the host chain {err:.3e}')
    assert torch.allclose(out.double(), ref, atol=2e-6, rtol=1e-5)
    if with_res:                                                       # residual == out is allowed by the header
        buf = res.clone()
        code = E.lib().fbbev_rows_linear_f32_ln(E.p(x), x.stride(0), E.p(w), E.p(b), rows, I, O, E.p(buf), O, E.p(lw), E.p(lb), 1e-5,
                                                E.p(buf), O, None)
        assert code == 0 and torch.equal(buf, out)
    code, _ = run_ln(x, torch.randn(256, I, generator=g), None, None, torch.ones(256), torch.zeros(256), 1e-5)
    assert code < 0                                                       # wider than one workgroup's output rows: refused


# ------------------------------------------------------------------ 5. position independence, the row-tile knob
def test_bits_do_not_depend_on_where_a_row_sits_or_on_the_row_tile_knob(monkeypatch):
    g = torch.Generator().manual_seed(77)
    x = torch.randn(5 * 128 - 37, 80, generator=g)
    w, b = torch.randn(160, 80, generator=g) * 0.2, torch.randn(160, generator=g)
    code, full = run(x, w, b, relu=True)
    assert code == 0
    for a, e in ((0, 1), (130, 391), (517, 603), (200, 328)):
        code, part = run(x[a:e], w, b, relu=True)
        assert code == 0 and torch.equal(part, full[a:e])
    for rt in ('1', '3', '8'):                                         # row tiles per workgroup (weight staged once)
        monkeypatch.setenv('FBBEV_ROWS_LINEAR_RT', rt)
        code, other = run(x, w, b, relu=True)
        assert code == 0 and torch.equal(other, full)
    lw, lb = torch.rand(80, generator=g) + 0.5, torch.randn(80, generator=g)
    w80, b80, res = w[:80].contiguous(), b[:80].contiguous(), torch.randn(x.shape[0], 80, generator=g)
    monkeypatch.delenv('FBBEV_ROWS_LINEAR_RT')
    code, ln_full = run_ln(x, w80, b80, res, lw, lb, 1e-5)
    monkeypatch.setenv('FBBEV_ROWS_LINEAR_RT', '2')
    code2, ln_rt = run_ln(x, w80, b80, res, lw, lb, 1e-5)
    code3, ln_part = run_ln(x[130:391], w80, b80, res[130:391], lw, lb, 1e-5)
    assert code == 0 and code2 == 0 and code3 == 0
    assert torch.equal(ln_full, ln_rt) and torch.equal(ln_part, ln_full[130:391])


# ------------------------------------------------------------------ 6. argument checks, no launch
def test_invalid_arguments_return_error_codes_without_a_launch():
    L = E.lib()
    x, w, b, out = torch.randn(16, 16), torch.randn(8, 16), torch.randn(8), torch.full((16, 8), float('nan'))
    f = L.fbbev_rows_linear_f32
    P = E.p
    assert f(P(x), 0, P(w), P(b), 16, 12, 8, 0, P(out), 0, None) == -2          # in_features % 8
    assert f(P(x), 0, P(w), P(b), 16, 16, 6, 0, P(out), 0, None) == -2          # out_features % 4
    assert f(P(x), 18, P(w), P(b), 8, 16, 8, 0, P(out), 0, None) == -2          # stride not a multiple of 4
    assert f(P(x), 0, P(w), P(b), 8, 16, 8, 0, P(out), 10, None) == -2
    assert f(c_void_p(x.data_ptr() + 4), 0, P(w), P(b), 8, 16, 8, 0, P(out), 0, None) == -2      # misaligned pointers
    assert f(P(x), 0, c_void_p(w.data_ptr() + 4), P(b), 4, 16, 4, 0, P(out), 0, None) == -2
    assert f(P(x), 0, P(w), c_void_p(b.data_ptr() + 4), 8, 16, 4, 0, P(out), 0, None) == -2
    assert f(P(x), 0, P(w), P(b), 8, 16, 8, 0, c_void_p(out.data_ptr() + 8), 0, None) == -2
    assert f(None, 0, P(w), P(b), 16, 16, 8, 0, P(out), 0, None) == -1          # null pointers with rows > 0
    assert f(P(x), 0, None, P(b), 16, 16, 8, 0, P(out), 0, None) == -1
    assert f(P(x), 0, P(w), P(b), 16, 16, 8, 0, None, 0, None) == -1
    assert f(P(x), 0, P(w), P(b), -1, 16, 8, 0, P(out), 0, None) == -1          # negative sizes
    assert f(P(x), 0, P(w), P(b), 16, -16, 8, 0, P(out), 0, None) == -1
    assert f(P(x), 0, P(w), P(b), 16, 16, -8, 0, P(out), 0, None) == -1
    assert f(P(x), 8, P(w), P(b), 16, 16, 8, 0, P(out), 0, None) == -1          # a row stride shorter than the row
    assert f(None, 0, None, None, 0, 16, 8, 0, None, 0, None) == 0              # rows == 0: nothing to do
    fa = L.fbbev_rows_linear_f32_add
    assert fa(P(x), 0, None, 0, 4, P(w), P(b), 16, 16, 8, 0, P(out), 0, None) == -1
    assert fa(P(x), 0, P(x), 0, 0, P(w), P(b), 16, 16, 8, 0, P(out), 0, None) == -1
    assert fa(P(x), 0, P(x), 18, 4, P(w), P(b), 16, 16, 8, 0, P(out), 0, None) == -2
    assert fa(P(x), 0, c_void_p(x.data_ptr() + 4), 0, 4, P(w), P(b), 8, 16, 8, 0, P(out), 0, None) == -2
    fl = L.fbbev_rows_linear_f32_ln
    assert fl(P(x), 0, P(w), P(b), 16, 16, 8, None, 0, None, P(b), 1e-5, P(out), 0, None) == -1
    assert fl(P(x), 0, P(w), P(b), 16, 16, 8, P(out), 6, P(b), P(b), 1e-5, P(out), 0, None) == -1
    assert fl(P(x), 0, P(w), P(b), 16, 16, 8, None, 0, c_void_p(b.data_ptr() + 4), P(b), 1e-5, P(out), 0, None) == -2
    assert fl(P(x), 0, P(w), P(b), 16, 16, 132, None, 0, P(b), P(b), 1e-5, P(out), 0, None) == -2
    assert torch.isnan(out).all()                                                # nothing ever ran


# ------------------------------------------------------------------ 7. the derived error bound
@pytest.mark.parametrize('R,I,O', [(300, 80, 128), (200, 512, 80), (129, 80, 512), (1, 264, 132)])
def test_error_against_float64_is_inside_the_bound_of_the_contract(R, I, O):
    """|got - exact| <= (I + 2) 2^-24 (sum_k |x_k w_k| + |b|): a K-term fmaf chain has relative error <= gamma_K on the sum of
    magnitudes, the bias add is one more rounding.  Derived, not measured.  The split-operand entry is further away."""
    g = torch.Generator().manual_seed(R + I + O)
    x = (torch.randn(R, I, generator=g) * 2).contiguous()
    w = torch.randn(O, I, generator=g) * 0.2
    b = torch.randn(O, generator=g)
    code, got = run(x, w, b)
    assert code == 0
    exact = x.double() @ w.double().t() + b.double()
    bound = (I + 2) * 2.0 ** -24 * (x.double().abs() @ w.double().abs().t() + b.double().abs())
    err = (got.double() - exact).abs()
    code, got3 = E.rows_linear_x3(x, w, b)
    assert code == 0
    err3 = (got3.double() - exact).abs()
    print(f'{R}x{I}->{O}: max abs err f32 entry {err.max().item():.3e}, x3 entry {err3.max().item():.3e}, '
          f'smallest bound / err margin {(bound / err.clamp_min(1e-300)).min().item():.1f}')
    assert (err <= bound).all()
    assert err3.max() > err.max()
