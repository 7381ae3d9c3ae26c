"""fbbev_bev_pool_v2_dense_fwd_rows at the ABI boundary, without a GPU: the symbol is exported with the signature the binding
declares, and every invalid call is answered by the argument checks (include/fbbev.h error convention) BEFORE any launch."""
import ctypes
import os
import re

from fb_bev_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'fbbev_bev_pool_v2_dense_fwd_rows'
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
BF16, F16, CPL8 = 0x800000, 0x1000000, 0x4


def _lib():
    return _capi.declare(ctypes.CDLL(_capi.LIB_PATH))


def test_symbol_is_exported_and_declared_as_the_header_spells_it():
    lib = _lib()
    assert hasattr(lib, NAME)
    restype, argtypes = _capi.SIGNATURES[NAME]
    assert restype is ctypes.c_int
    src = open(os.path.join(ROOT, 'include', 'fbbev.h')).read()
    m = re.search(r'int\s+' + NAME + r'\s*\(([^;]*)\)\s*;', src)
    assert m, 'prototype missing from include/fbbev.h'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    assert len(params) == len(argtypes) == 21

    def ctype(p):
        if '*' in p or 'fbbev_stream_t' in p:
            return ctypes.c_void_p
        if p.startswith('long long'):
            return ctypes.c_int64
        if p.startswith('size_t'):
            return ctypes.c_size_t
        assert p.startswith('int '), p
        return ctypes.c_int
    assert [ctype(p) for p in params] == list(argtypes)
    assert callable(_capi.bev_pool_v2_dense_fwd_rows)


def test_invalid_arguments_return_error_codes_without_touching_the_gpu():
    fn = getattr(_lib(), NAME)
    NULL = ctypes.c_void_p(0)
    P, P8 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)      # 16-byte aligned / not; never dereferenced on these paths
    BIG = 1 << 30

    def call(depth=P, feat=P, rd=P, rf=P, ir=P, st=P, ln=P, B=2, C=80, Z=4, Y=16, X=16, out=P, stride_b=0, addend=NULL,
             addend_stride=0, ws=P, ws_bytes=BIG, tv=128, flags=F16):
        return fn(depth, feat, rd, rf, ir, st, ln, B, C, Z, Y, X, out, stride_b, addend, addend_stride, ws, ws_bytes, tv, flags, NULL)

    n = 4 * 16 * 16 * 80
    # FBBEV_E_BADARG
    for name in ('depth', 'feat', 'rd', 'rf', 'ir', 'st', 'ln', 'out', 'ws'):
        assert call(**{name: NULL}) == BADARG, name                 # null pointers
    for name in 'BCZYX':
        assert call(**{name: 0}) == BADARG and call(**{name: -3}) == BADARG, name     # non-positive sizes
    assert call(flags=BF16 | F16) == BADARG                         # both storage flags
    assert call(stride_b=n - 8) == BADARG                           # batch stride below Z*Y*X*C
    assert call(addend=P, addend_stride=72) == BADARG               # addend row stride below C
    # FBBEV_E_UNSUPPORTED
    assert call(C=84, flags=F16) == UNSUPPORTED                     # C % 8, 16-bit rows
    assert call(C=84, flags=BF16) == UNSUPPORTED
    assert call(C=82, flags=0) == UNSUPPORTED                       # C % 4, fp32 rows
    assert call(C=264) == UNSUPPORTED                               # C > 256
    assert call(stride_b=n + 4, flags=F16) == UNSUPPORTED           # batch stride % 8 elements (16-bit)
    assert call(stride_b=n + 2, flags=0) == UNSUPPORTED             # ... % 4 elements (fp32)
    assert call(addend=P, addend_stride=82) == UNSUPPORTED          # addend row stride % 4 floats
    assert call(out=P8) == UNSUPPORTED                              # pointers off 16 bytes
    assert call(feat=P8) == UNSUPPORTED
    assert call(addend=P8) == UNSUPPORTED
    for tv in (8, 16, 32):
        assert call(tv=tv) == UNSUPPORTED, tv                       # the small-tile kernel keeps its contiguous fp32 form
    assert call(B=1 << 12, Z=1 << 6, Y=1 << 7, X=1 << 7) == UNSUPPORTED   # B*Z*Y*X >= 2^31
    # FBBEV_E_WORKSPACE: 2 * 4*16*16 voxels in 128-voxel tiles = 16 tiles -> 17 table entries of 8 bytes
    assert call(ws_bytes=17 * 8 - 1) == WORKSPACE
    assert call(ws_bytes=0) == WORKSPACE
    # the stride checks accept the padded strides a ring slot has: nothing left to reject but the (too small) workspace
    assert call(stride_b=3 * n, addend=P, addend_stride=96, ws_bytes=8) == WORKSPACE
    assert call(stride_b=3 * n, flags=CPL8, ws_bytes=8) == WORKSPACE
