"""Argument checks of fbbev_depth_loss_fwd / fbbev_depth_loss_grad / fbbev_depth_loss_ws_bytes (include/fbbev.h): every error code is
returned BEFORE any launch, so dummy pointers do and no GPU is needed; the Python wrappers refuse CPU tensors.  (What an empty batch
does to out_f and out_i needs real buffers: tests/test_emu_depth_loss.py::test_empty_batch_zeroes_the_outputs.)"""
import ctypes

import pytest
import torch

from fb_bev_amd import _capi

NULL = ctypes.c_void_p(0)
P = ctypes.c_void_p(0x1000)          # non-null, 16-byte aligned dummy; never dereferenced on these paths
P8 = ctypes.c_void_p(0x1008)
INF, NAN = float('inf'), float('nan')


@pytest.fixture(scope='module')
def lib():
    return _capi.declare(ctypes.CDLL(_capi.LIB_PATH))


def fwd(lib, gt=P, BN=2, H=32, W=64, ds=16, probs=P, D=80, bin0=1.5, step=0.5, labels=P, out_f=P, out_i=P, ws=P, ws_bytes=1 << 30):
    return lib.fbbev_depth_loss_fwd(gt, BN, H, W, ds, probs, D, bin0, step, labels, out_f, out_i, ws, ws_bytes, NULL)


def grad(lib, probs=P, labels=P, out_i=P, grad_loss=P, BN=2, D=80, h=2, w=4, out=P):
    return lib.fbbev_depth_loss_grad(probs, labels, out_i, grad_loss, BN, D, h, w, out, NULL)


def test_bad_arguments(lib):
    for name in ('gt', 'labels', 'out_f', 'out_i', 'ws'):
        assert fwd(lib, **{name: NULL}) == -1, name
    for name in ('probs', 'labels', 'out_i', 'grad_loss', 'out'):
        assert grad(lib, **{name: NULL}) == -1, name
    for dim in ('H', 'W', 'ds', 'D'):
        assert fwd(lib, **{dim: 0}) == -1, dim
        assert fwd(lib, **{dim: -3}) == -1, dim
    for dim in ('D', 'h', 'w'):
        assert grad(lib, **{dim: 0}) == -1, dim
        assert grad(lib, **{dim: -3}) == -1, dim
    assert fwd(lib, BN=-1) == -1 and grad(lib, BN=-1) == -1
    assert fwd(lib, H=33) == -1                             # H % ds
    assert fwd(lib, W=65) == -1                             # W % ds
    for step in (0.0, -0.5, INF, NAN):
        assert fwd(lib, step=step) == -1, step
    for bin0 in (INF, -INF, NAN):
        assert fwd(lib, bin0=bin0) == -1, bin0
    assert fwd(lib, BN=0, gt=NULL) == -1                    # ... also for an empty batch
    assert grad(lib, BN=0, probs=NULL) == -1
    assert fwd(lib, BN=0, step=0.0) == -1


def test_labels_only_call_is_accepted_up_to_the_workspace(lib):
    """probs may be NULL: every check passes, down to the workspace's"""
    assert fwd(lib, probs=NULL, ws_bytes=0) == -3


def test_unsupported(lib):
    assert fwd(lib, D=4097) == -2 and grad(lib, D=4097) == -2
    assert fwd(lib, H=8192, W=8192, ds=8192) == -2                    # a cell wider than a chunk of column minima
    assert fwd(lib, BN=2, H=32768, W=32768, ds=1, D=1) == -2          # BN * h * w = 2^31
    assert grad(lib, BN=2, h=32768, w=32768, D=1) == -2
    assert fwd(lib, BN=1, H=32768, W=32768, ds=1, D=2) == -2          # BN * D * h * w = 2^31
    assert grad(lib, BN=1, h=32768, w=32768, D=2) == -2
    assert grad(lib, BN=2 ** 31 - 1, h=2 ** 31 - 1, w=2 ** 31 - 1, D=4096) == -2       # ... and a product beyond 64 bits
    assert fwd(lib, BN=2, H=128 * 16, W=128 * 16, ds=16, D=128, ws_bytes=0) == -3      # D = 128 is supported


def test_workspace(lib):
    need = lib.fbbev_depth_loss_ws_bytes(2, 2, 4, 80)
    assert fwd(lib, ws_bytes=need - 1) == -3
    assert fwd(lib, ws_bytes=0) == -3
    assert fwd(lib, ws=P8) == -3                            # enough bytes, 8-byte aligned only


def test_order_of_the_checks(lib):
    """a bad argument comes before unsupported, unsupported before the workspace"""
    assert fwd(lib, gt=NULL, D=5000) == -1
    assert fwd(lib, step=0.0, D=5000) == -1
    assert fwd(lib, H=33, D=5000) == -1
    assert fwd(lib, BN=-1, H=32768, W=32768, ds=1) == -1
    assert fwd(lib, D=5000, ws=NULL) == -1
    assert fwd(lib, D=5000, ws_bytes=0) == -2
    assert fwd(lib, D=5000, ws=P8) == -2
    assert fwd(lib, ws=P8, out_f=NULL) == -1
    assert grad(lib, out=NULL, D=5000) == -1
    assert grad(lib, h=0, D=5000) == -1


def test_empty_batch_is_a_no_op_for_the_gradient(lib):
    assert grad(lib, BN=0) == 0
    assert grad(lib, BN=0, D=5000) == 0                     # nothing to do comes before unsupported, as in fbbev_occ_loss_grad


def test_ws_bytes(lib):
    """one float and one int per workgroup, a workgroup per image and cell row, each block rounded up to 16 bytes"""
    rec = lambda BN, h: 2 * ((4 * BN * h + 15) // 16 * 16)  # noqa: E731
    assert lib.fbbev_depth_loss_ws_bytes(1, 3, 5, 4) == rec(1, 3) == 32
    assert lib.fbbev_depth_loss_ws_bytes(2, 2, 44, 80) == rec(2, 2) == 32
    assert lib.fbbev_depth_loss_ws_bytes(24, 16, 44, 80) == rec(24, 16) == 3072          # the shipped shape: 384 workgroups
    assert lib.fbbev_depth_loss_ws_bytes(6, 32, 88, 118) == rec(6, 32)
    assert lib.fbbev_depth_loss_ws_bytes(0, 16, 44, 80) == 0
    assert lib.fbbev_depth_loss_ws_bytes(1, 16, -44, 80) == 0
    assert lib.fbbev_depth_loss_ws_bytes(2, 32768, 32768, 1) == 0                        # unsupported: no size


def test_case_table_sizes(lib):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import depth_loss_cases as DC
    for case in DC.CASES:
        BN, h, w, D = DC.dims(case)
        assert lib.fbbev_depth_loss_ws_bytes(BN, h, w, D) == 2 * ((4 * BN * h + 15) // 16 * 16), case['name']


def test_wrappers_refuse_cpu_tensors():
    gt, probs = torch.zeros(1, 8, 8), torch.full((1, 12, 2, 2), 0.5)
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        _capi.depth_loss_fwd(gt, probs, 4, 12, 1.0, 1.0)
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        _capi.depth_loss_fwd(gt, None, 4, 12, 1.0, 1.0)
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        _capi.depth_loss_grad(probs, torch.zeros(1, 2, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.ones(1))
    from fb_bev_amd.depth_net import depth_loss_fused
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        depth_loss_fused(gt[None], probs[None], 4, [1.0, 13.0, 1.0])
