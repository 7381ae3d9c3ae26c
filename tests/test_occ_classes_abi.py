"""Argument checks of fbbev_occ_classes (include/fbbev.h): every error code is returned BEFORE any launch, so dummy pointers do and no GPU
is needed; the Python wrapper refuses CPU tensors."""
import ctypes

import pytest
import torch

from fb_bev_amd import _capi

NULL = ctypes.c_void_p(0)
P = ctypes.c_void_p(0x1000)          # non-null dummy; never dereferenced on these paths


@pytest.fixture(scope='module')
def fn():
    return _capi.declare(ctypes.CDLL(_capi.LIB_PATH)).fbbev_occ_classes


def call(fn, logits=P, strides=(0, 0, 0, 0, 0), B=1, C=19, c0=1, H=8, W=8, D=16, classes=P, gt=NULL, mask=NULL, cm=NULL, hist=NULL):
    return fn(logits, *strides, B, C, c0, H, W, D, classes, gt, mask, cm, hist, NULL)


def test_bad_arguments(fn):
    assert call(fn, logits=NULL) == -1
    assert call(fn, classes=NULL) == -1
    for dim in ('C', 'H', 'W', 'D'):
        assert call(fn, **{dim: 0}) == -1, dim
        assert call(fn, **{dim: -3}) == -1, dim
    assert call(fn, B=-1) == -1
    assert call(fn, c0=-1) == -1
    assert call(fn, mask=P) == -1                   # mask, column_mask or hist without gt
    assert call(fn, cm=P) == -1
    assert call(fn, hist=P) == -1
    assert call(fn, mask=P, cm=P, hist=P) == -1
    assert call(fn, B=0, gt=NULL, hist=P) == -1     # ... also for an empty batch


def test_empty_batch_is_a_no_op(fn):
    assert call(fn, B=0) == 0
    assert call(fn, B=0, gt=P, mask=P, cm=P, hist=P) == 0


def test_unsupported(fn):
    assert call(fn, C=2, c0=1) == -2                # n = 1
    assert call(fn, C=19, c0=19) == -2              # n = 0
    assert call(fn, C=5, c0=9) == -2                # n < 0
    assert call(fn, C=34, c0=1) == -2               # n = 33
    assert call(fn, C=33, c0=0) == -2
    assert call(fn, B=2, H=1024, W=1024, D=1024) == -2            # B * H * W * D = 2^31
    assert call(fn, B=1, H=65536, W=65536, D=2) == -2             # ... beyond 64 bits of int arithmetic done in 32
    assert call(fn, B=4, gt=P, hist=P, H=1024, W=1024, D=1024) == -2


def test_bad_argument_comes_before_unsupported(fn):
    assert call(fn, logits=NULL, C=40, c0=1) == -1
    assert call(fn, C=40, c0=1, hist=P) == -1


def test_wrapper_refuses_cpu_tensors():
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        _capi.occ_classes(torch.zeros(1, 19, 4, 4, 2), c0=1)
