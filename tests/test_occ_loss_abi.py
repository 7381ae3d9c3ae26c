"""Argument checks of fbbev_occ_loss_stats / fbbev_occ_loss_grad / fbbev_occ_loss_ws_bytes (include/fbbev.h): every error code is
returned BEFORE any launch, so dummy pointers do and no GPU is needed; the Python wrappers refuse CPU tensors.  (What an empty batch
does to the statistics needs real buffers: tests/test_emu_occ_loss.py::test_empty_batch_zeroes_the_statistics.)"""
import ctypes

import pytest
import torch

from fb_bev_amd import _capi

NULL = ctypes.c_void_p(0)
P = ctypes.c_void_p(0x1000)          # non-null, 16-byte aligned dummy; never dereferenced on these paths
P8 = ctypes.c_void_p(0x1008)


@pytest.fixture(scope='module')
def lib():
    return _capi.declare(ctypes.CDLL(_capi.LIB_PATH))


def stats(lib, logits=P, B=1, C=19, H=8, W=8, D=16, labels=P, cw=NULL, plane=NULL, e=18, flags=0, sf=P, si=P, ws=P, ws_bytes=1 << 30):
    return lib.fbbev_occ_loss_stats(logits, 0, 0, 0, 0, 0, B, C, H, W, D, labels, cw, plane, e, flags, 2.0, 0.25, sf, si, ws, ws_bytes, NULL)


def grad(lib, logits=P, B=1, C=19, H=8, W=8, D=16, labels=P, cw=NULL, plane=NULL, e=18, flags=0, gs=P, out=P):
    return lib.fbbev_occ_loss_grad(logits, 0, 0, 0, 0, 0, B, C, H, W, D, labels, cw, plane, e, flags, 2.0, 0.25, gs, out, NULL)


def test_bad_arguments(lib):
    for fn, ptrs in ((stats, ('logits', 'labels', 'sf', 'si', 'ws')), (grad, ('logits', 'labels', 'gs', 'out'))):
        for name in ptrs:
            assert fn(lib, **{name: NULL}) == -1, (fn.__name__, name)
        for dim in ('C', 'H', 'W', 'D'):
            assert fn(lib, **{dim: 0}) == -1, dim
            assert fn(lib, **{dim: -3}) == -1, dim
        assert fn(lib, B=-1) == -1
        assert fn(lib, e=-1) == -1
        assert fn(lib, e=19) == -1                          # empty_idx outside 0..C-1
        assert fn(lib, C=2, e=2) == -1
        assert fn(lib, flags=1) == -1                       # focal without plane_weight
        assert fn(lib, B=0, flags=1) == -1                  # ... also for an empty batch
        assert fn(lib, B=0, logits=NULL) == -1


def test_unsupported(lib):
    for fn in (stats, grad):
        assert fn(lib, C=1, e=0) == -2
        assert fn(lib, C=33, e=0) == -2
        assert fn(lib, B=2, H=1024, W=1024, D=1024) == -2            # B * H * W * D = 2^31
        assert fn(lib, B=1, H=65536, W=65536, D=2) == -2             # ... beyond 64 bits of int arithmetic done in 32
        assert fn(lib, B=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, D=2 ** 31 - 1) == -2    # ... and a product beyond 64 bits


def test_workspace(lib):
    need = lib.fbbev_occ_loss_ws_bytes(1, 19, 8, 8, 16)
    assert stats(lib, ws_bytes=need - 1) == -3
    assert stats(lib, ws_bytes=0) == -3
    assert stats(lib, ws=P8) == -3                          # enough bytes, 8-byte aligned only


def test_order_of_the_checks(lib):
    """a bad argument comes before unsupported, unsupported before the workspace"""
    for fn in (stats, grad):
        assert fn(lib, logits=NULL, C=40, e=0) == -1
        assert fn(lib, C=40, e=40) == -1
        assert fn(lib, C=40, e=0, flags=1) == -1
        assert fn(lib, B=-1, H=65536, W=65536, D=2) == -1
    assert stats(lib, C=40, e=0, ws=NULL) == -1
    assert stats(lib, C=40, e=0, ws_bytes=0) == -2
    assert stats(lib, C=40, e=0, ws=P8) == -2
    assert stats(lib, ws=P8, sf=NULL) == -1


def test_empty_batch_is_a_no_op_for_the_gradient(lib):
    assert grad(lib, B=0) == 0
    assert grad(lib, B=0, C=40, e=0) == 0                   # nothing to do comes before unsupported, as in fbbev_occ_classes


def test_ws_bytes(lib):
    """one record of 3C + 4 floats and C + 1 ints per workgroup, each block rounded up to 16 bytes; workgroups = tiles, at most 1024"""
    rec = lambda n, C: (n * (3 * C + 4) * 4 + 15) // 16 * 16 + (n * (C + 1) * 4 + 15) // 16 * 16  # noqa: E731
    assert lib.fbbev_occ_loss_ws_bytes(2, 19, 5, 7, 3) == rec(2, 19)                 # one 16 x 16 x 3 tile per sample
    assert lib.fbbev_occ_loss_ws_bytes(1, 19, 17, 33, 16) == rec(3 * 5, 19)          # 8 x 8 x 16 tiles
    assert lib.fbbev_occ_loss_ws_bytes(4, 19, 200, 200, 16) == rec(1024, 19)         # the shipped shape: 2500 tiles, 1024 workgroups
    assert lib.fbbev_occ_loss_ws_bytes(0, 19, 8, 8, 16) == 0
    assert lib.fbbev_occ_loss_ws_bytes(1, 19, 8, -8, 16) == 0


def test_wrappers_refuse_cpu_tensors():
    logits, labels = torch.zeros(1, 19, 4, 4, 2), torch.zeros(1, 4, 4, 2, dtype=torch.uint8)
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        _capi.occ_loss_stats(logits, labels, empty_idx=18)
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        _capi.occ_loss_grad(logits, labels, torch.zeros(61), empty_idx=18)
    from fb_bev_amd.occ_loss import voxel_losses_fused
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        voxel_losses_fused(logits, labels, torch.ones(19), empty_idx=18)


def test_case_table_reaches_the_grid_stride(lib):
    """tests/occ_loss_cases.py counts tiles as the launchers do (a record per workgroup, workgroups = min(tiles, 1024)), and its
    table has shapes with more tiles than the statistics kernel's 1024 and the gradient kernel's 2048 workgroups"""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import occ_loss_cases as LC
    rec = lambda n, C: (n * (3 * C + 4) * 4 + 15) // 16 * 16 + (n * (C + 1) * 4 + 15) // 16 * 16  # noqa: E731
    for case in LC.CASES + LC.EXACT_CASES:
        shape = tuple(case[k] for k in ('B', 'C', 'H', 'W', 'D'))
        assert lib.fbbev_occ_loss_ws_bytes(*shape) == rec(min(LC.tiles(case), LC.STATS_BLOCKS), case['C']), case['name']
    assert LC.tiles(LC.by_name('b1_1x8243x16_cl')) == 1031 and LC.tiles(LC.by_name('b1_1x32803x2_cl')) == 2051
    assert LC.tiles(LC.by_name('b1_200x200x2_cl')) == 169
