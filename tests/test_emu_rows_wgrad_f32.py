"""fbbev_rows_wgrad_f32 / _ws_bytes / _slice_rows on the CPU emulator: the exact-fp32 weight and bias gradient of the row-wise linear
layers against its arithmetic contract (include/fbbev.h) -- per slice of L rows one fmaf chain in ascending row order, the slices
added in ascending order -- bit for bit (tests/rows_wgrad_f32_ref.py on tests/rows_linear_f32_ref.py::fmaf32)."""
import os
import sys
from ctypes import c_void_p

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))
import emu_capi as E  # noqa: E402
from rows_wgrad_f32_ref import two_stage_chain  # noqa: E402

BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -3


def slice_rows(R, I, O):
    return E.lib().fbbev_rows_wgrad_f32_slice_rows(R, I, O)


def ws_bytes(R, I, O):
    return E.lib().fbbev_rows_wgrad_f32_ws_bytes(R, I, O)


def run(gy, x, bias=True, ws_floats=None):
    """-> (code, grad_weight, grad_bias, guard words behind the workspace)"""
    R, O = gy.shape
    I = x.shape[1]
    need = ws_bytes(R, I, O)
    n = need // 4 if ws_floats is None else ws_floats
    ws = torch.full((n + 8,), float('nan'))
    gw = torch.full((O, I), float('nan'))
    gb = torch.full((O,), float('nan'))
    code = E.lib().fbbev_rows_wgrad_f32(c_void_p(gy.data_ptr()), gy.stride(0), c_void_p(x.data_ptr()), x.stride(0), R, I, O, E.p(gw),
                                        E.p(gb) if bias else None, E.p(ws), n * 4, None)
    return code, gw, gb, ws[n:]


def _case(R, I, O, strided):
    g = torch.Generator().manual_seed(1000 * R + 10 * I + O)
    gy = torch.randn(R, O + (12 if strided else 0), generator=g)
    x = torch.randn(R, I + (4 if strided else 0), generator=g) * 2
    return gy[:, :O], x[:, :I]                       # strided: views into wider buffers


@pytest.mark.parametrize('I,O', [(8, 8), (24, 40), (16, 136)])
def test_slice_rows_is_a_multiple_of_four_and_stable(I, O):
    for R in (1, 3, 1000, 160000, 10 ** 7):
        L = slice_rows(R, I, O)
        assert L > 0 and L % 4 == 0 and slice_rows(R, I, O) == L
    assert slice_rows(64, I + 4, O) == UNSUPPORTED and slice_rows(64, I, O + 4) == UNSUPPORTED
    assert slice_rows(-1, I, O) == BADARG and slice_rows(64, 0, O) == BADARG


@pytest.mark.parametrize('strided', [False, True])
@pytest.mark.parametrize('I,O', [(8, 8), (24, 40), (16, 136)])
def test_weight_and_bias_gradient_equal_the_two_stage_host_chain_exactly(I, O, strided):
    L0 = slice_rows(3, I, O)
    for R in (3, L0, L0 + 1, 2 * L0 + 37):
        L = slice_rows(R, I, O)
        assert L == L0                               # small row counts share the shortest slice: the row counts above straddle it
        gy, x = _case(R, I, O, strided)
        code, gw, gb, guard = run(gy, x)
        assert code == 0 and torch.isnan(guard).all()
        assert not torch.isnan(gw).any() and not torch.isnan(gb).any()
        ew, eb = two_stage_chain(gy, x, L)
        assert torch.equal(gw, ew), (R, (gw - ew).abs().max())
        assert torch.equal(gb, eb), (R, (gb - eb).abs().max())


def test_null_grad_bias_leaves_the_weight_gradient_unchanged():
    I, O = 24, 40
    R = 2 * slice_rows(3, I, O) + 37
    gy, x = _case(R, I, O, True)
    code, gw, gb, _ = run(gy, x, bias=False)
    assert code == 0 and torch.isnan(gb).all()       # never written
    ew, _ = two_stage_chain(gy, x, slice_rows(R, I, O), bias=False)
    assert torch.equal(gw, ew)
    code2, gw2, _, _ = run(gy, x, bias=True)
    assert code2 == 0 and torch.equal(gw, gw2)


def test_a_longer_slice_is_used_for_many_rows_and_the_chain_follows_it():
    """8 x 8 is one work item per slice and 1024 slices are aimed at: 66 000 rows take slices of 68 rows (not the shortest, 64)"""
    I, O, R = 8, 8, 66000
    L = slice_rows(R, I, O)
    assert L > slice_rows(3, I, O) and L % 4 == 0
    gy, x = _case(R, I, O, False)
    code, gw, gb, guard = run(gy, x)
    assert code == 0 and torch.isnan(guard).all()
    ew, eb = two_stage_chain(gy, x, L)
    assert torch.equal(gw, ew) and torch.equal(gb, eb)


def test_error_codes_without_a_launch():
    f = E.lib().fbbev_rows_wgrad_f32
    P = E.p
    gy, x = torch.randn(16, 16), torch.randn(16, 16)
    gw, gb, ws = torch.full((16, 16), float('nan')), torch.full((16,), float('nan')), torch.full((4096,), float('nan'))
    nb = ws.numel() * 4
    assert ws_bytes(16, 16, 16) <= nb and ws_bytes(16, 16, 16) > 0
    assert f(P(gy), 0, P(x), 0, 16, 12, 16, P(gw), P(gb), P(ws), nb, None) == UNSUPPORTED       # in_features % 8
    assert f(P(gy), 0, P(x), 0, 16, 16, 12, P(gw), P(gb), P(ws), nb, None) == UNSUPPORTED       # out_features % 8
    assert ws_bytes(16, 12, 16) == 0 and ws_bytes(16, 16, 12) == 0
    assert f(c_void_p(gy.data_ptr() + 4), 0, P(x), 0, 8, 16, 16, P(gw), P(gb), P(ws), nb, None) == UNSUPPORTED   # misaligned pointers
    assert f(P(gy), 0, c_void_p(x.data_ptr() + 8), 0, 8, 16, 16, P(gw), P(gb), P(ws), nb, None) == UNSUPPORTED
    assert f(P(gy), 0, P(x), 0, 8, 16, 8, c_void_p(gw.data_ptr() + 4), P(gb), P(ws), nb, None) == UNSUPPORTED
    assert f(P(gy), 0, P(x), 0, 8, 16, 8, P(gw), c_void_p(gb.data_ptr() + 4), P(ws), nb, None) == UNSUPPORTED
    assert f(P(gy), 18, P(x), 0, 8, 16, 16, P(gw), P(gb), P(ws), nb, None) == UNSUPPORTED       # stride not a multiple of 4
    assert f(P(gy), 0, P(x), 0, 16, 16, 16, P(gw), P(gb), P(ws), ws_bytes(16, 16, 16) - 4, None) == WORKSPACE   # short workspace
    assert f(P(gy), 0, P(x), 0, 16, 16, 16, P(gw), P(gb), None, nb, None) == WORKSPACE
    assert f(P(gy), 0, P(x), 0, 16, 16, 16, P(gw), P(gb), c_void_p(ws.data_ptr() + 4), nb - 4, None) == WORKSPACE
    assert f(None, 0, P(x), 0, 16, 16, 16, P(gw), P(gb), P(ws), nb, None) == BADARG             # null pointers
    assert f(P(gy), 0, None, 0, 16, 16, 16, P(gw), P(gb), P(ws), nb, None) == BADARG
    assert f(P(gy), 0, P(x), 0, 16, 16, 16, None, P(gb), P(ws), nb, None) == BADARG
    assert f(P(gy), 0, P(x), 0, -1, 16, 16, P(gw), P(gb), P(ws), nb, None) == BADARG            # negative sizes
    assert f(P(gy), 0, P(x), 0, 16, -16, 16, P(gw), P(gb), P(ws), nb, None) == BADARG
    assert f(P(gy), 0, P(x), 0, 16, 16, 0, P(gw), P(gb), P(ws), nb, None) == BADARG
    assert f(P(gy), 8, P(x), 0, 16, 16, 16, P(gw), P(gb), P(ws), nb, None) == BADARG            # a row stride shorter than the row
    assert torch.isnan(gw).all() and torch.isnan(gb).all() and torch.isnan(ws).all()            # nothing ever ran
    assert f(None, 0, None, 0, 0, 16, 16, P(gw), P(gb), None, 0, None) == 0                     # rows == 0: zero-filled outputs
    assert (gw == 0).all() and (gb == 0).all()
