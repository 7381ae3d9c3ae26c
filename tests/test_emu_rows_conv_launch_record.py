"""Which kernel a call of the row-wise linear layers and of the convolutions launches, on the CPU emulator (the product's capi.hip
compiled against tests/emu/rt.h, which logs every launch and every opt-in to dynamic LDS): entry, shape and knobs -> [return code,
(kernel instantiation, grid, block, dynamic LDS bytes) | ('lds opt-in', kernel, bytes), ...] in the order the runtime calls were made.
The persistent, training, LayerNorm and plain row kernels give the same bits, and so do the MT = 4 / 2 / 1 tilings of a convolution:
a launcher that takes another route or forms another grid passes every numerical test and only costs speed; this table is what sees
it.  The table (tests/golden/rows_conv_launch_record.json) was recorded on the launchers before they shared their operand records.

FBBEV_ROWS_LINEAR_NT is read once per process in every build, so its cases run in one fresh child interpreter."""
import ast
import ctypes
import json
import os
import subprocess
import sys
from ctypes import c_void_p

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'emu'))
import emu_capi as E  # noqa: E402

KNOBS = ('FBBEV_ROWS_LINEAR_P', 'FBBEV_ROWS_LINEAR_RT', 'FBBEV_ROWS_LINEAR_SLOTS', 'FBBEV_FFN_HC')
DET = 1                                                          # FBBEV_FLAG_DETERMINISTIC


def _records(reader, width):
    read = getattr(E.lib(), reader)                              # emulator build only (tests/emu/rt.h): not in include/fbbev.h
    read.restype, read.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_longlong)]
    name, nums = ctypes.c_char_p(), (ctypes.c_longlong * width)()
    out = []
    for i in range(read(-1, ctypes.byref(name), nums)):
        read(i, ctypes.byref(name), nums)
        out.append((name.value.decode(), *nums[:]))
    return out


def _log():
    launches = [(text[text.index('K = ') + 4:text.rindex(']')], g, b, lds) for text, g, b, lds in _records('fbbev_emu_launch_log_read', 3)]
    optins = _records('fbbev_emu_lds_optin_log_read', 2)
    out = []
    for i in range(len(launches) + 1):
        out += [('lds opt-in', kernel, nbytes) for kernel, nbytes, before in optins if before == i]
        out += launches[i:i + 1]
    return out


def _clear():
    clear = E.lib().fbbev_emu_launch_log_clear
    clear.restype, clear.argtypes = None, []
    clear()


def _log_only(on):
    switch = E.lib().fbbev_emu_launch_log_only
    switch.restype, switch.argtypes = None, [ctypes.c_int]
    switch(on)


def _ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


def _fragments(O, I):
    return E._fragments(torch.zeros(O, I))                       # (the buffer, the aligned pointer into it)


def run_rows(entry, I, O, R=300, addend=False, residual=False, mask=False, ln=False, elem=0, hidden=0, tokens=100):
    """one call of a row entry on R rows of ones and zero weights -> its return code; the log then holds what it launched"""
    lib = E.lib()
    x, out = torch.ones(R, I), torch.zeros(R, max(O, 1))
    add = torch.ones(tokens, I) if addend else None
    res = torch.ones(R, O) if residual else None
    msk = torch.ones(R, O) if mask else None
    ln_w, ln_b, bias = torch.ones(O), torch.zeros(O), torch.zeros(O)
    f32 = entry.startswith('f32')
    keep = torch.zeros(O, I)                                     # f32: the weight itself; x3: its fragments
    keep, w = (keep, _ptr(keep)) if f32 else _fragments(O, I)
    fam = 'fbbev_rows_linear_' + ('f32' if f32 else 'x3')
    _clear()
    if entry in ('x3', 'f32'):
        return getattr(lib, fam)(_ptr(x), 0, w, _ptr(bias), R, I, O, 1, _ptr(out), 0, None)
    if entry in ('x3_add', 'f32_add'):
        return getattr(lib, fam + '_add')(_ptr(x), 0, _ptr(add), 0, tokens, w, _ptr(bias), R, I, O, 0, _ptr(out), 0, None)
    if entry in ('x3_ln', 'f32_ln'):
        return getattr(lib, fam + '_ln')(_ptr(x), 0, w, _ptr(bias), R, I, O, _ptr(res), 0, _ptr(ln_w), _ptr(ln_b), 1e-5, _ptr(out), 0, None)
    if entry == 'x3_train':
        return lib.fbbev_rows_linear_x3_train(_ptr(x), 0, _ptr(add), 0, tokens if addend else 0, w, _ptr(bias), R, I, O, 1, _ptr(res), 0,
                                              _ptr(msk), 0, _ptr(out), 0, None)
    head_dim = 10 if O % 10 == 0 else 16
    if entry == 'x3_planes':
        return lib.fbbev_rows_linear_x3_planes(_ptr(x), 0, w, _ptr(bias), R, I, O, tokens, head_dim, _ptr(out), None)
    if entry == 'x3_planes_e':
        return lib.fbbev_rows_linear_x3_planes_e(_ptr(x), 0, w, _ptr(bias), R, I, O, tokens, head_dim, elem, _ptr(out), None)
    k1, w1 = _fragments(hidden, I)
    k2, w2 = _fragments(O, hidden)
    b1 = torch.zeros(hidden)
    _clear()
    if entry == 'ffn':
        return lib.fbbev_rows_ffn_x3(_ptr(x), 0, w1, _ptr(b1), w2, _ptr(bias), R, I, hidden, O, _ptr(res), 0, _ptr(ln_w) if ln else None,
                                     _ptr(ln_b) if ln else None, 1e-5, _ptr(out), 0, None)
    head = (_ptr(x), 0, w, _ptr(bias), _ptr(res), 0, _ptr(ln_w), _ptr(ln_b), 1e-5, w1, _ptr(b1), w2, _ptr(bias), R, I, hidden,
            _ptr(ln_w), _ptr(ln_b), 1e-5)
    if entry == 'tail':
        return lib.fbbev_rows_tail_ffn_x3(*head, _ptr(out), 0, None)
    if entry == 'tail_planes':
        return lib.fbbev_rows_tail_ffn_x3_planes(*head, tokens, _ptr(out), None)
    raise KeyError(entry)


def _out_dim(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def run_conv(entry, vol, Cin, Cout, k=3, s=1, p=1, transposed=False, planar=False, flags=0):
    """one call of a convolution entry on a volume of ones and zero weights -> its return code"""
    lib = E.lib()
    B, D, H, W = vol
    Do, Ho, Wo = (D, H, W) if transposed else [_out_dim(n, k, s, p) for n in (D, H, W)]
    if planar or entry == 'conv2d':
        assert D == 1
        Do = 1
    up = 2 if transposed else 1
    pad16 = lambda c: (c + 15) // 16 * 16                        # noqa: E731
    x, out = torch.ones(B, D, H, W, Cin), torch.zeros(B, up * Do, up * Ho, up * Wo, Cout)
    bf16 = entry in ('bf16', 'tiled')
    wf = torch.zeros(27 * pad16(Cin) * pad16(Cout) + 64, dtype=torch.bfloat16 if bf16 else torch.float32)
    bias = torch.zeros(pad16(max(Cin, Cout)) + 16)
    _clear()
    if entry == 'conv3d':
        return lib.fbbev_conv3d_ndhwc(_ptr(x), _ptr(wf), _ptr(bias), None, B, D, H, W, Cin, Do, Ho, Wo, Cout, k, s, p, 1,
                                      1 if transposed else 0, _ptr(out), None)
    if entry == 'conv2d':
        return lib.fbbev_conv2d_nhwc(_ptr(x), _ptr(wf), _ptr(bias), None, B, H, W, Cin, Ho, Wo, Cout, k, s, p, 1, _ptr(out), None)
    if entry == 'bf16':
        return lib.fbbev_conv3d_ndhwc_bf16(_ptr(x), _ptr(wf), _ptr(bias), None, B, D, H, W, Cin, Do, Ho, Wo, Cout, k, s, p, 1,
                                           1 if transposed else 0, 1 if planar else 0, _ptr(out), None)
    if entry == 'tiled':
        return lib.fbbev_conv3d_k3s1_tiled_bf16(_ptr(x), _ptr(wf), _ptr(bias), None, B, D, H, W, Cin, Cout, 1, _ptr(out), None)
    dy = torch.ones(B, Do, Ho, Wo, Cout)
    if entry == 'dgrad':
        dx = torch.zeros(B, D, H, W, Cin)
        return lib.fbbev_conv3d_dgrad_ndhwc(_ptr(dy), _ptr(wf), _ptr(bias), B, Do, Ho, Wo, Cout, D, H, W, Cin, k, s, p, _ptr(dx), None)
    dw = torch.zeros(k ** 3, Cout, Cin)
    dims = (B, D, H, W, Cin, Do, Ho, Wo, Cout, k, s, p)
    if entry == 'wgrad':
        return lib.fbbev_conv3d_wgrad_ndhwc(_ptr(x), _ptr(dy), *dims, _ptr(dw), None)
    if entry == 'wgrad_ex':
        need = lib.fbbev_conv3d_wgrad_ws_bytes(B, Do, Ho, Wo, Cin, Cout, k, flags)
        ws = torch.zeros(need // 4 + 4)
        return lib.fbbev_conv3d_wgrad_ndhwc_ex(_ptr(x), _ptr(dy), *dims, _ptr(dw), flags, _ptr(ws), need, None)
    raise KeyError(entry)


def run(family, entry, *shape, env=None, **kw):
    """-> [return code, runtime call, runtime call, ...] of the one call under test (fragments are built before the log is cleared)"""
    for name in KNOBS:
        os.environ.pop(name, None)
    os.environ.update(env or {})
    _log_only(1)                                                 # what is launched, not what it computes: no kernel runs
    try:
        code = (run_rows if family == 'rows' else run_conv)(entry, *shape, **kw)
        return [code] + _log()
    finally:
        _log_only(0)
        for name in KNOBS:
            os.environ.pop(name, None)


# 300 rows: three 128-row tiles, the last one partial (five 64-row tiles at 16 rows per wave).  In -> out features: 80 -> 80 the
# persistent <5, 3>, 128 -> 80 <5, 4>, 80 -> 128 <8, 3>, 128 -> 128 <8, 4> (under the training epilogue the old kernel), 256 -> 80 two K
# chunks (never persistent, one row tile per workgroup), 80 -> 256 two output chunks (the grid doubles; the LayerNorm entries refuse
# it behind the launch geometry), 80 -> 40 three output tiles
SHAPES = ((80, 80), (128, 80), (80, 128), (128, 128), (256, 80), (80, 256), (80, 40))
V1, V2 = (1, 5, 6, 7), (2, 9, 9, 9)                             # 210 voxels: one 256-voxel block; 1 458: six


def _row_cases(nt1=False):
    t = {}

    def add(name, entry, *shape, **kw):
        assert name not in t, name
        t[name] = ('rows', entry, shape, kw)
    off = {'FBBEV_ROWS_LINEAR_P': '0'}
    for I, O in SHAPES:
        s = f'{I}->{O}'
        add(f'x3 {s}', 'x3', I, O)
        add(f'x3 {s} addend', 'x3_add', I, O, addend=True)
        add(f'x3 {s} ln', 'x3_ln', I, O)
        add(f'x3 {s} train', 'x3_train', I, O)
        add(f'x3 {s} planes', 'x3_planes', I, O)
        if nt1:
            continue
        add(f'x3 {s} persistent off', 'x3', I, O, env=off)
        add(f'f32 {s}', 'f32', I, O)
        add(f'x3 {s} ln residual', 'x3_ln', I, O, residual=True)
        add(f'x3 {s} train addend', 'x3_train', I, O, addend=True)
        add(f'x3 {s} train residual mask', 'x3_train', I, O, residual=True, mask=True)
        add(f'x3 {s} train addend residual mask', 'x3_train', I, O, addend=True, residual=True, mask=True)
        for e in (0, 1, 2):
            add(f'x3 {s} planes elem {e}', 'x3_planes_e', I, O, elem=e)
        for rt in ('1', '3'):
            add(f'x3 {s} persistent off rt {rt}', 'x3', I, O, env=dict(off, FBBEV_ROWS_LINEAR_RT=rt))
        add(f'x3 {s} addend rt 3', 'x3_add', I, O, addend=True, env={'FBBEV_ROWS_LINEAR_RT': '3'})
        for n in ('1', '2'):
            add(f'x3 {s} slots {n}', 'x3', I, O, env={'FBBEV_ROWS_LINEAR_SLOTS': n})
        add(f'x3 {s} train slots 2', 'x3_train', I, O, mask=True, env={'FBBEV_ROWS_LINEAR_SLOTS': '2'})
        add(f'f32 {s} addend', 'f32_add', I, O, addend=True)
        add(f'f32 {s} ln', 'f32_ln', I, O)
        add(f'f32 {s} ln residual', 'f32_ln', I, O, residual=True)
        add(f'f32 {s} rt 3', 'f32', I, O, env={'FBBEV_ROWS_LINEAR_RT': '3'})
    if nt1:
        return t
    for I, H, O in ((80, 320, 80), (16, 64, 16)):
        for hc in ('32', '64'):
            for ln in (False, True):
                add(f'ffn {I}->{H}->{O} hc {hc} ln {ln}', 'ffn', I, O, hidden=H, ln=ln, residual=ln, env={'FBBEV_FFN_HC': hc})
        add(f'ffn {I}->{H}->{O} ln without residual', 'ffn', I, O, hidden=H, ln=True)
    add('ffn 80->96->80 hidden % 64', 'ffn', 80, 80, hidden=96)
    for E_, H in ((16, 64), (80, 320), (16, 320), (80, 64)):
        for entry in ('tail', 'tail_planes'):
            add(f'{entry} {E_} hidden {H}', entry, E_, E_, hidden=H, residual=E_ == 80)
    add('tail 80 hidden 320 hc 64 is ignored', 'tail', 80, 80, hidden=320, env={'FBBEV_FFN_HC': '64'})
    add('tail 96 refused', 'tail', 96, 96, hidden=64)
    return t


def _conv_cases():
    t = {}

    def add(name, entry, *shape, **kw):
        assert name not in t, name
        t[name] = ('conv', entry, shape, kw)
    vols = (('v1', V1), ('v2', V2))
    for v, vol in vols:
        for k in (1, 2, 3):
            for s in (1, 2):
                for p in (0, 1):
                    add(f'conv3d {v} 16->16 k{k} s{s} p{p}', 'conv3d', vol, 16, 16, k=k, s=s, p=p)
        for Cin in (16, 32):
            for Cout in (16, 32, 48, 64):                        # MT 1, 2, 1 (three tiles: gy = 3), 4
                add(f'conv3d {v} {Cin}->{Cout} k3', 'conv3d', vol, Cin, Cout)
        for Cout in (16, 32, 48, 64):
            add(f'conv3d {v} 16->{Cout} k1', 'conv3d', vol, 16, Cout, k=1, p=0)
            add(f'conv3d {v} 32->{Cout} k2 s2', 'conv3d', vol, 32, Cout, k=2, s=2, p=0)
            add(f'conv3d {v} 16->{Cout} transposed', 'conv3d', vol, 16, Cout, transposed=True)
            add(f'bf16 {v} 32->{Cout} k3', 'bf16', vol, 32, Cout)
            add(f'bf16 {v} 32->{Cout} transposed', 'bf16', vol, 32, Cout, transposed=True)
        add(f'conv3d {v} 24->16 refused', 'conv3d', vol, 24, 16)
        add(f'bf16 {v} 32->32 k1 s2', 'bf16', vol, 32, 32, k=1, s=2, p=0)
        add(f'bf16 {v} 32->16 k3 s2', 'bf16', vol, 32, 16, s=2)
        add(f'bf16 {v} 16->16 refused', 'bf16', vol, 16, 16)
        add(f'dgrad {v} 16->48 k3', 'dgrad', vol, 16, 48)       # the kernel's input is dy (48 channels), its output dx (16: one tile)
        add(f'dgrad {v} 48->16 k3', 'dgrad', vol, 48, 16)
        add(f'dgrad {v} 32->64 k3 s2', 'dgrad', vol, 32, 64, s=2)
        add(f'dgrad {v} 64->32 k2 s2', 'dgrad', vol, 64, 32, k=2, s=2, p=0)
        add(f'dgrad {v} 32->16 k1', 'dgrad', vol, 32, 16, k=1, p=0)
        for k, p in ((1, 0), (2, 0), (3, 1)):
            add(f'wgrad {v} 16->32 k{k}', 'wgrad', vol, 16, 32, k=k, p=p)
            add(f'wgrad_ex {v} 16->32 k{k} deterministic', 'wgrad_ex', vol, 16, 32, k=k, p=p, flags=DET)
        add(f'wgrad_ex {v} 80->72 k3 s2 atomic', 'wgrad_ex', vol, 80, 72, s=2, flags=0)
        add(f'wgrad_ex {v} 80->72 k3 s2 deterministic', 'wgrad_ex', vol, 80, 72, s=2, flags=DET)
    for v, img in (('6x7', (1, 1, 6, 7)), ('37x37', (1, 1, 37, 37))):
        for k, p in ((1, 0), (3, 1)):
            for s in (1, 2):
                add(f'conv2d {v} 16->16 k{k} s{s}', 'conv2d', img, 16, 16, k=k, s=s, p=p)
        for Cout in (32, 48, 64):
            add(f'conv2d {v} 32->{Cout} k3', 'conv2d', img, 32, Cout)
            add(f'bf16 planar {v} 32->{Cout} k3', 'bf16', img, 32, Cout, planar=True)
        add(f'bf16 planar {v} 32->16 k1', 'bf16', img, 32, 16, k=1, p=0, planar=True)
        add(f'bf16 one plane not planar {v} 32->16 k3', 'bf16', img, 32, 16)
    for v, vol in (('5x9x9', (1, 5, 9, 9)), ('4x8x17', (1, 4, 8, 17)), ('2 of 4x8x8', (2, 4, 8, 8))):   # 8 tiles; 3, rounded up to 8; 2
        for Cout in (16, 32, 48, 64):
            add(f'tiled {v} 32->{Cout}', 'tiled', vol, 32, Cout)
        add(f'tiled {v} 16->16 refused', 'tiled', vol, 16, 16)
    return t


CASES = dict(_row_cases(), **_conv_cases())
NT1_CASES = _row_cases(nt1=True)


def run_case(case):
    family, entry, shape, kw = case
    return run(family, entry, *shape, **kw)


@pytest.mark.parametrize('name', list(CASES))
def test_entry_launches_what_it_launched(name):
    assert run_case(CASES[name]) == LAUNCHES[name]


def test_16_rows_per_wave_in_a_child_process():
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_emu_rows_conv_launch_record as T\n'
            'print({name: T.run_case(case) for name, case in T.NT1_CASES.items()})\n') % (ROOT, HERE)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, FBBEV_ROWS_LINEAR_NT='1'), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ast.literal_eval(r.stdout.strip().splitlines()[-1])
    assert got == NT1_LAUNCHES, [(name, got.get(name), want) for name, want in NT1_LAUNCHES.items() if got.get(name) != want]


def test_the_tables_have_every_case_and_every_kind_of_row():
    assert set(LAUNCHES) == set(CASES) and set(NT1_LAUNCHES) == set(NT1_CASES)
    rows = list(LAUNCHES.values())
    assert any(v == [-2] for v in rows) and any(len(v) == 3 and v[1][0] != 'lds opt-in' for v in rows)   # a refusal; two launches
    kernels = {call[0] for v in list(LAUNCHES.values()) + list(NT1_LAUNCHES.values()) for call in v[1:] if call[0] != 'lds opt-in'}
    for text in ('k_rows_linear_x3p<5, 3, 0>', 'k_rows_linear_x3p<8, 4, 0>', 'k_rows_linear_x3p<8, 3, 1>', 'k_rows_linear_x3<2, false, 1>',
                 'k_rows_linear_x3<2, true>', 'k_rows_linear_x3<1, false>', 'k_rows_linear_x3<2, false>', 'k_rows_linear_f32<true>',
                 'k_conv3d_ndhwc<1, 3, 4>', 'k_conv3d_ndhwc<2, 2, 2>', 'k_conv3d_ndhwc_bf16<1, 3, 1>', 'k_conv3d_k3_tile_bf16<4>',
                 'k_conv3d_wgrad_ndhwc<3, true>', 'k_sum_chunks_add'):
        assert text in kernels, text


# name -> [return code, runtime call, ...]: a launch as [kernel instantiation, grid, block, dynamic LDS bytes], an opt-in to dynamic LDS
# as ['lds opt-in', kernel, bytes]; 'nt1': the same under FBBEV_ROWS_LINEAR_NT=1.  Recorded results, kept as data.
with open(os.path.join(HERE, 'golden', 'rows_conv_launch_record.json')) as _f:
    _RECORD = json.load(_f)
LAUNCHES = {name: [v[0]] + [tuple(call) for call in v[1:]] for name, v in _RECORD['launches'].items()}
NT1_LAUNCHES = {name: [v[0]] + [tuple(call) for call in v[1:]] for name, v in _RECORD['nt1'].items()}
