"""The symbols and the argument checks of fbbev_occ_lovasz_fwd / fbbev_occ_lovasz_grad / fbbev_occ_lovasz_ws_bytes (include/fbbev.h):
every error code is returned BEFORE any launch, so dummy pointers do and no GPU is needed; the Python layers refuse CPU tensors and
carry the switches.  (What an empty batch does to the outputs needs real buffers: tests/test_emu_occ_lovasz.py.)"""
import ctypes
import os

import pytest
import torch

from fb_bev_amd import _capi

NULL = ctypes.c_void_p(0)
P = ctypes.c_void_p(0x1000)          # non-null, 16-byte aligned dummy; never dereferenced on these paths
P8 = ctypes.c_void_p(0x1008)


@pytest.fixture(scope='module')
def lib():
    return _capi.declare(ctypes.CDLL(_capi.LIB_PATH))


def fwd(lib, logits=P, B=1, C=19, H=8, W=8, D=16, labels=P, loss_c=P, fg=P, coef=P, errors=NULL, ws=P, ws_bytes=1 << 40):
    return lib.fbbev_occ_lovasz_fwd(logits, 0, 0, 0, 0, 0, B, C, H, W, D, labels, loss_c, fg, coef, errors, ws, ws_bytes, NULL)


def grad(lib, logits=P, B=1, C=19, H=8, W=8, D=16, labels=P, coef=P, scale=P, out=P):
    return lib.fbbev_occ_lovasz_grad(logits, 0, 0, 0, 0, 0, B, C, H, W, D, labels, coef, scale, out, NULL)


def test_symbols_are_exported_and_declared(lib):
    for name in ('fbbev_occ_lovasz_ws_bytes', 'fbbev_occ_lovasz_fwd', 'fbbev_occ_lovasz_grad'):
        assert getattr(lib, name).argtypes is not None, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fbbev.h')).read()
    for name in ('fbbev_occ_lovasz_ws_bytes(', 'fbbev_occ_lovasz_fwd(', 'fbbev_occ_lovasz_grad('):
        assert name in header
    assert header.count('lovasz_softmax.py:20-33,157-229') >= 2


def test_bad_arguments(lib):
    for fn, ptrs in ((fwd, ('logits', 'labels', 'loss_c', 'fg', 'coef', 'ws')), (grad, ('logits', 'labels', 'coef', 'scale', 'out'))):
        for name in ptrs:
            assert fn(lib, **{name: NULL}) == -1, (fn.__name__, name)
        for dim in ('C', 'H', 'W', 'D'):
            assert fn(lib, **{dim: 0}) == -1, dim
            assert fn(lib, **{dim: -3}) == -1, dim
        assert fn(lib, B=-1) == -1
        assert fn(lib, B=0, logits=NULL) == -1
    assert fwd(lib, B=0, loss_c=NULL) == -1 and fwd(lib, B=0, fg=NULL) == -1
    assert grad(lib, B=0, coef=NULL) == 0                   # an empty batch has no coefficients: 0 and no launch


def test_unsupported(lib):
    for fn in (fwd, grad):
        assert fn(lib, C=1) == -2
        assert fn(lib, C=33) == -2
        assert fn(lib, B=1, H=1024, W=1024, D=64) == -2                     # B * H * W * D = 2^26
        assert fn(lib, B=16, H=2048, W=2048, D=1) == -2
        assert fn(lib, B=1, H=65536, W=65536, D=2) == -2                    # ... beyond 32 bits
        assert fn(lib, B=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, D=2 ** 31 - 1) == -2    # ... and a product beyond 64 bits
    assert lib.fbbev_occ_lovasz_ws_bytes(1, 19, 1024, 1024, 64) == 0
    assert lib.fbbev_occ_lovasz_ws_bytes(1, 33, 8, 8, 16) == 0 and lib.fbbev_occ_lovasz_ws_bytes(0, 19, 8, 8, 16) == 0


def test_workspace(lib):
    need = lib.fbbev_occ_lovasz_ws_bytes(1, 19, 8, 8, 16)
    assert need > 0 and need % 16 == 0
    assert fwd(lib, ws_bytes=need - 1) == -3
    assert fwd(lib, ws_bytes=0) == -3
    assert fwd(lib, ws=P8, ws_bytes=need) == -3             # enough bytes, 8-byte aligned only
    # the classes are sorted in groups: at the shipped grid the workspace stops growing with the batch (16 samples: 10 M voxels)
    at = [lib.fbbev_occ_lovasz_ws_bytes(B, 19, 200, 200, 16) for B in (1, 4, 16)]
    assert max(at) < 320 << 20, at
    assert at[1] < 19 * 4 * 200 * 200 * 16 * 16             # far below two pair buffers over all the classes


def test_python_layers_refuse_cpu_tensors_and_carry_the_switches():
    from fb_bev_amd import occ_loss
    from fb_bev_amd.occ_head import OccHead
    logits, labels = torch.zeros(1, 19, 2, 2, 2), torch.zeros(1, 2, 2, 2, dtype=torch.uint8)
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        _capi.occ_lovasz_fwd(logits, labels)
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        _capi.occ_lovasz_grad(logits, labels, torch.zeros(19, 1, 2, 2, 2), torch.ones(1))
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        occ_loss.lovasz_softmax_fused(logits, labels.long())
    with pytest.raises(ValueError):
        occ_loss.lovasz_softmax_fused(logits, labels.long(), ignore=254)
    tiny = dict(in_channels=[8], out_channel=19, num_level=1, norm_cfg=dict(type='BN3d', requires_grad=True), use_deblock=False)
    assert OccHead(**tiny).fused_lovasz is False and OccHead(**tiny, fused_lovasz=True).fused_lovasz is True
    # the unfused head's Lovasz term is the parent's, operation for operation, on the CPU
    head = OccHead(**tiny)
    g = torch.Generator().manual_seed(0)
    x, t = torch.randn(1, 19, 4, 4, 2, generator=g), torch.randint(0, 19, (1, 4, 4, 2), generator=g)
    want = occ_loss.lovasz_softmax(torch.softmax(x, dim=1), t, ignore=255)
    assert torch.equal(head._lovasz(x, t, True), want) and torch.equal(head._lovasz(x, t, False), want)
