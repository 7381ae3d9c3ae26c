"""fbbev_image_prep's return codes on the built library (include/fbbev.h states each): every row returns before any launch, so this
runs without a GPU; `out` and `canvas` sit between guard bands of a pattern that must survive.  Also the three places that must
agree on the limits: the library, the planner, the header's text."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_prep_cases as C  # noqa: E402
from fb_bev_amd import _capi, image_prep as IP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    assert os.path.exists(_capi.LIB_PATH), 'run `python -m fb_bev_amd.build` (or __graft_entry__.build())'
    return _capi.declare(ctypes.CDLL(_capi.LIB_PATH))


def _call(lib, **kw):
    """host buffers stand in for device memory: no row reaches a launch"""
    a = dict(frames=torch.zeros(4 * 4 * 3 + 16, dtype=torch.uint8), stride=48, n=1, Hs=4, Ws=4, fH=2, fW=2, plan=torch.zeros(64, dtype=torch.int32),
             need=[4, 2, 2, 4, 4], mean=[0.0] * 3, inv=[1.0] * 3, flags=0, out_offset=0, canvas=True)
    a.update(kw)
    buf = torch.full((C.GUARD + 12 + C.GUARD,), C.PATTERN)
    cbuf = torch.full((C.GUARD + 12 + C.GUARD,), C.PATTERN_U8, dtype=torch.uint8)
    assert buf.data_ptr() % 16 == 0
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    arr = lambda ty, v: None if v is None else ctypes.cast((ty * len(v))(*v), ctypes.c_void_p)  # noqa: E731
    out = None if a['out_offset'] is None else ctypes.c_void_p(buf.data_ptr() + 4 * C.GUARD + a['out_offset'])
    code = lib.fbbev_image_prep(p(a['frames']), a['stride'], a['n'], a['Hs'], a['Ws'], a['fH'], a['fW'], p(a['plan']),
                                arr(ctypes.c_int, a['need']), arr(ctypes.c_float, a['mean']), arr(ctypes.c_float, a['inv']), a['flags'],
                                out, ctypes.c_void_p(cbuf.data_ptr() + C.GUARD) if a['canvas'] else None, None)
    assert bool((buf == C.PATTERN).all()) and bool((cbuf == C.PATTERN_U8).all()), f'{kw}: written to before the decline'
    return code


def test_return_codes(lib):
    L = IP.limits()
    for kw in (dict(frames=None), dict(plan=None), dict(need=None), dict(mean=None), dict(inv=None), dict(out_offset=None),
               dict(n=-1), dict(Hs=0), dict(Ws=0), dict(fH=0), dict(fW=-3), dict(flags=4), dict(flags=-1), dict(stride=47),
               dict(need=[4, 2, -1, 4, 4])):
        assert _call(lib, **kw) == -1, kw
    for kw in (dict(n=0), dict(n=0, need=[99, 999, 999, 999, 999]), dict(n=0, out_offset=4)):      # nothing to do comes before the declines
        assert _call(lib, **kw) == 0, kw
    for i, key in enumerate(('max_taps', 'max_box_w', 'max_box_h', 'max_src_rows', 'max_src_cols')):
        need = [4, 2, 2, 4, 4]
        need[i] = L[key] + 1
        assert _call(lib, need=need) == -2, key
    for kw in (dict(out_offset=4), dict(out_offset=8), dict(fH=16384), dict(fW=16384), dict(canvas=False, out_offset=12)):
        assert _call(lib, **kw) == -2, kw
    odd = torch.zeros(80, dtype=torch.uint8)
    assert _call(lib, frames=odd[1:]) == -2                                                          # frames at an odd address
    assert _call(lib, stride=47, out_offset=4) == -1 and _call(lib, need=[99, 2, 2, 4, 4], fH=0) == -1   # the order of the checks
    assert _call(lib, n=1 << 20, fH=16000, fW=16000, stride=48) == -2                                # 2^31 tiles or more


def test_limits_agree(lib):
    got = C.limits_of(type('A', (), dict(lib=lib)))
    assert got == IP.limits() == _capi.image_prep_limits()
    assert (C.TW, C.TH) == (got['tile_w'], got['tile_h'])
    assert lib.fbbev_image_prep_limits(*([None] * 7)) == -1
    text = open(os.path.join(ROOT, 'include', 'fbbev.h')).read()
    doc = text[text.index('Camera frames to network input'):text.index('int fbbev_image_prep(')]
    for key, pattern in (('max_taps', r'count > (\d+)'), ('max_box_w', r'box above (\d+) x'), ('max_box_h', r'box above \d+ x (\d+)'),
                         ('max_src_rows', r'more than (\d+) source rows'), ('max_src_cols', r'or\s+(\d+) source columns')):
        assert int(re.search(pattern, doc).group(1)) == got[key], key


def test_wrapper_refuses_cpu_tensors():
    case = C.by_name('mini_test_pipeline')
    with pytest.raises(_capi.FbbevError):
        IP.prepare_images(torch.from_numpy(C.frames_of(case)), case['augs'])
    with pytest.raises(_capi.FbbevError):
        _capi.image_prep(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32), [0] * 5, 2, 2, [0] * 3, [1] * 3)
