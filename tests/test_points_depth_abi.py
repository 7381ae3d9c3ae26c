"""fbbev_points_to_depth in the three places that must agree: the built library exports the symbol, include/fbbev.h declares it with
the arguments of the issue (plus max_points, which sizes the grid without a host read of offsets), and fb_bev_amd._capi's ctypes
table has the same types in the same order.  The return codes are taken before any launch, so dummy pointers do and no GPU is
needed; the Python wrapper refuses CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from fb_bev_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = ctypes.c_void_p(0)
P = ctypes.c_void_p(0x1000)          # non-null dummy; never dereferenced on these paths

ARGS = [('const float*', 'points'), ('int', 'point_stride'), ('const int32_t*', 'offsets'), ('int', 'max_points'), ('int', 'B'),
        ('int', 'N'), ('const float*', 'lidar2img'), ('const float*', 'post_rots'), ('const float*', 'post_trans'), ('int', 'H'),
        ('int', 'W'), ('int', 'downsample'), ('float', 'depth_lo'), ('float', 'depth_hi'), ('float*', 'out'),
        ('fbbev_stream_t', 'stream')]
CTYPES = {'int': ctypes.c_int, 'float': ctypes.c_float}


@pytest.fixture(scope='module')
def lib():
    return _capi.declare(ctypes.CDLL(_capi.LIB_PATH))


def test_symbol_is_exported(lib):
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), 'fbbev_points_to_depth')


def test_header_declares_it_with_these_arguments():
    with open(os.path.join(ROOT, 'include', 'fbbev.h')) as f:
        text = f.read()
    m = re.search(r'\nint fbbev_points_to_depth\(([^;]*)\);', text)
    assert m, 'no declaration in include/fbbev.h'
    got = []
    for arg in re.sub(r'\s+', ' ', m.group(1)).split(','):
        typ, name = arg.strip().rsplit(' ', 1)
        got.append((typ, name))
    assert got == ARGS
    assert 'loading.py:876-966' in text                              # the reference lines it replaces
    assert re.search(r'#define FBBEV_E_DEPTH_RANGE \(-4\)', text) and re.search(r'#define FBBEV_E_MAP_SIZE \(-5\)', text)


def test_ctypes_table_matches_the_header():
    res, args = _capi.SIGNATURES['fbbev_points_to_depth']
    assert res is ctypes.c_int
    assert args == [CTYPES.get(t, ctypes.c_void_p) for t, _ in ARGS]


def call(lib, **kw):
    a = dict(points=P, point_stride=5, offsets=P, max_points=100, B=2, N=6, lidar2img=P, post_rots=P, post_trans=P, H=256, W=704,
             downsample=1, depth_lo=1.0, depth_hi=45.0, out=P)
    a.update(kw)
    return lib.fbbev_points_to_depth(*[a[name] for _, name in ARGS[:-1]], NULL)


def test_return_codes_before_any_launch(lib):
    for name in ('points', 'offsets', 'lidar2img', 'post_rots', 'post_trans', 'out'):
        assert call(lib, **{name: NULL}) == -1, name
    assert call(lib, point_stride=2) == -1 and call(lib, downsample=0) == -1 and call(lib, max_points=-1) == -1
    assert call(lib, depth_lo=0.0) == -1 and call(lib, depth_lo=float('nan')) == -1 and call(lib, depth_hi=float('nan')) == -1
    assert call(lib, H=3, downsample=4) == 0 and call(lib, W=0) == 0 and call(lib, B=0) == 0 and call(lib, N=0) == 0
    assert call(lib, depth_hi=100.0) == -4
    assert call(lib, H=4096, W=4096) == -5 and call(lib, H=8192, W=8192, downsample=2) == -5
    assert call(lib, B=4096, N=4096) == -2
    assert call(lib, out=NULL, depth_hi=100.0) == -1 and call(lib, depth_hi=100.0, H=4096, W=4096) == -4
    assert call(lib, B=0, depth_hi=100.0) == 0                       # nothing to do comes before the refusals


def test_wrapper_refuses_cpu_tensors():
    pts, off = torch.zeros(4, 3), torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(_capi.FbbevError, match='GPU tensor'):
        _capi.points_to_depth(pts, off, 4, torch.eye(4).view(1, 1, 4, 4), torch.eye(3).view(1, 1, 3, 3), torch.zeros(1, 1, 3), 4, 4, 1, 1.0, 45.0)
