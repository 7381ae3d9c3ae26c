"""Which kernel a call of the pooling family launches, on the CPU emulator (the product's capi.hip compiled against tests/emu/rt.h,
whose FBBEV_LAUNCH logs every launch): entry, shape, flags word and knobs -> [return code, (kernel instantiation, grid, block,
dynamic LDS bytes), ...].  Store policy, channels per lane, workgroup size, XCD order and the experimental routes all give the same
bits, so a mis-decoded flag passes every numerical test and only costs speed; this table is what sees it.  The literals at the end
were recorded on the launchers before they shared their operand records."""
import ctypes
import os
import sys
from ctypes import c_void_p

import pytest
import torch

from fb_bev_amd import synthetic as S
from oracle import oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import emu_capi as E  # noqa: E402

ST_NT, ST_2, CPL8, WG128, WG_2, SWIZZLE, SC1_NT = 0x1, 0x2, 0x4, 0x100, 0x200, 0x400, 0x20000
CHANNELS_LAST, OUT_BF16, OUT_F16, SPLIT_LONG, PIPE, GATHER8 = 0x100000, 0x800000, 0x1000000, 0x2000000, 0x4000000, 0x8000000
CSPLIT = lambda n: n << 4            # noqa: E731
CHUNK = lambda lg: lg << 12          # noqa: E731

# one camera of 2 x 4 pixels and 2 depth bins into a 12 x 12 x 3 grid, two samples: Y * X = 144 is a multiple of 8 and gives 3 / 2 / 1
# tiles per plane at 64 / 128 / 256 voxels (the last one partial), so the rounding of a swizzled grid shows
B, N, D, H, W, Z, Y, X = 2, 1, 2, 2, 4, 3, 12, 12
GRID = {'x': [-6.0, 6.0, 1.0], 'y': [-6.0, 6.0, 1.0], 'z': [-1.0, 2.0, 1.0], 'depth': [1.0, 3.0, 1.0]}
KNOBS = ('FBBEV_POOL_PIPE_TPW', 'FBBEV_ZMEAN_COL')


def _f3(v):
    return ctypes.cast((ctypes.c_float * 3)(*v), c_void_p)


@pytest.fixture(scope='module')
def inputs():
    made = {}

    def get(C):
        if C not in made:
            cfg = S.PathConfig('LAUNCH', (16, 32), 8, GRID, C, n_cams=N)
            assert (cfg.D, cfg.feat_hw, cfg.grid_xyz) == (D, (H, W), (X, Y, Z))
            vt = O.ViewTransformerOracle(cfg.grid_config, cfg.input_size, cfg.downsample)
            cam = S.camera_rig(cfg, B, seed=0, bda_aug=True)
            depth, ctx = S.depth_and_context(cfg, B, seed=0)
            fr = vt.frustum
            axes = (fr[0, 0, :, 0].contiguous(), fr[0, :, 0, 1].contiguous(), fr[:, 0, 0, 2].contiguous())
            grid3 = (vt.grid_lower_bound.tolist(), vt.grid_interval.tolist(), vt.grid_size.tolist())
            rb, rd, rf, st, ln, ir, counts = E.lift_rank_build(*axes, cam, *grid3)
            assert counts[0] > 0
            made[C] = dict(cam=cam, depth=depth, ctx=ctx, feat=E.nchw_to_nhwc(ctx), axes=axes, grid3=grid3, rd=rd, rf=rf, st=st, ln=ln,
                           ir=ir, counts=counts)
        return made[C]
    return get


def _log():
    read = E.lib().fbbev_emu_launch_log_read                    # emulator build only (tests/emu/rt.h): not in include/fbbev.h
    read.restype, read.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_longlong)]
    name, nums = ctypes.c_char_p(), (ctypes.c_longlong * 3)()
    out = []
    for i in range(read(-1, ctypes.byref(name), nums)):
        read(i, ctypes.byref(name), nums)
        text = name.value.decode()
        out.append((text[text.index('K = ') + 4:text.rindex(']')], nums[0], nums[1], nums[2]))
    return out


def _clear():
    clear = E.lib().fbbev_emu_launch_log_clear
    clear.restype, clear.argtypes = None, []
    clear()


def _tile_table(c, tv, flags, cached=False, state=None):
    lib, p = E.lib(), E.p
    ws = torch.zeros(lib.fbbev_pool_dense_workspace_bytes(B, Z, Y, X), dtype=torch.uint8)
    head = (p(c['ir']), p(c['st']), p(c['counts']), c['ir'].numel(), B, Z, Y, X, tv, flags, p(ws), ws.numel())
    if cached:
        gate = torch.full((2,), -1, dtype=torch.int32)
        return lib.fbbev_pool_tile_index_cached(*head, p(state), p(gate), None), ws
    return lib.fbbev_pool_tile_index(*head, None), ws


def _gather(c):
    p = E.p
    return (p(c['depth']), p(c['feat']), p(c['rd']), p(c['rf']), p(c['ir']), p(c['st']), p(c['ln']))


def run(inputs, entry, C=16, tv=128, flags=0, env=None, **kw):
    """-> [return code, launch, launch, ...] of the one call under test (the tile table a forward needs is built before the log is cleared)"""
    lib, p, c = E.lib(), E.p, inputs(C)
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env or {})
    try:
        if entry in ('tile_index', 'tile_index_cached'):
            _clear()
            code, _ = _tile_table(c, tv, flags, entry == 'tile_index_cached', torch.tensor([kw.get('hit', 0), 1], dtype=torch.int32))
        elif entry == 'fwd':
            dt = torch.bfloat16 if flags & OUT_BF16 else torch.float16 if flags & OUT_F16 else torch.float32
            out = torch.zeros((B, Z, Y, X, C) if flags & CHANNELS_LAST else (B, C, Z, Y, X), dtype=dt)
            ws = _tile_table(c, tv, flags)[1]
            _clear()
            tail = (B, C, Z, Y, X, p(out), 0, 0, p(ws), ws.numel(), tv, flags)
            if kw.get('addend'):
                code = lib.fbbev_bev_pool_v2_dense_fwd_add(*_gather(c), *tail, p(torch.ones(B, C, Y, X)), None)
            else:
                code = lib.fbbev_bev_pool_v2_dense_fwd(*_gather(c), *tail, None)
        elif entry == 'rows':
            dt = torch.bfloat16 if flags & OUT_BF16 else torch.float16 if flags & OUT_F16 else torch.float32
            out = torch.zeros(B, Z * Y * X, C, dtype=dt)
            add = torch.ones(B, Y * X, C) if kw.get('addend') else None
            ws = _tile_table(c, tv, flags | CHANNELS_LAST)[1]
            _clear()
            code = lib.fbbev_bev_pool_v2_dense_fwd_rows(*_gather(c), B, C, Z, Y, X, p(out), 0, None if add is None else p(add), 0, p(ws),
                                                        ws.numel(), tv, flags, None)
        elif entry == 'diag':
            out = torch.zeros(B, C, Z, Y, X, dtype=torch.bfloat16 if flags & OUT_BF16 else torch.float32)
            ws = _tile_table(c, tv, flags)[1]
            _clear()
            code = lib.fbbev_diag_pool_store_floor(*_gather(c), B, C, Z, Y, X, p(out), p(ws), ws.numel(), tv, flags, kw['mode'], None)
        elif entry in ('zmean', 'zmean_split', 'zmean_rows'):
            out = torch.zeros(B, C, Y, X)
            ws = _tile_table(c, tv, flags)[1]
            _clear()
            tail = (B, C, Z, Y, X, p(out), p(ws), ws.numel(), tv, flags)
            if entry == 'zmean':
                code = lib.fbbev_pool_zmean(*_gather(c), *tail, None)
            elif entry == 'zmean_split':
                partial = torch.zeros(kw['z_groups'] * out.numel() + 4)
                at = partial.data_ptr() + (-partial.data_ptr()) % 16
                code = lib.fbbev_pool_zmean_split(*_gather(c), *tail, kw['z_groups'], c_void_p(at), kw['z_groups'] * out.numel() * 4, None)
            else:
                bias = torch.ones(Y * X, C) if kw.get('bias') else None
                code = lib.fbbev_pool_zmean_rows(*_gather(c), B, C, Z, Y, X, None if bias is None else p(bias), *tail[5:], None)
        elif entry == 'lift_splat':
            need = lib.fbbev_lift_splat_fused_ws_bytes(B, N, D, H, W, C, Z, Y, X)
            ws = torch.zeros(need, dtype=torch.uint8)
            out = torch.zeros(B, C, Z, Y, X, dtype=torch.bfloat16 if flags & OUT_BF16 else torch.float32)
            key = torch.full((lib.fbbev_cam_key_words(B, N),), -1, dtype=torch.int32) if kw.get('cache') else None
            state = torch.tensor([0, 0, -1, -1], dtype=torch.int32) if kw.get('cache') else None
            args = (None, *[p(t) for t in c['axes']], *[p(t) for t in c['cam']], p(c['depth']), p(c['ctx']), B, N, D, H, W, C,
                    *[_f3(v) for v in c['grid3']], Z, Y, X, p(out), 0, 0, tv, flags, p(ws), need,
                    None if key is None else p(key), None if state is None else p(state), None)
            if kw.get('cache') == 'hit':
                E.ok(lib.fbbev_lift_splat_fused(*args))
            _clear()
            code = lib.fbbev_lift_splat_fused(*args)
        elif entry == 'bwd':
            og = torch.ones(B, C, Z, Y, X)
            dg, fg = torch.zeros_like(c['depth']), torch.zeros_like(c['feat'])
            ws = torch.zeros(lib.fbbev_pool_dense_bwd_workspace_bytes(B, N, D, H, W, C, Z, Y, X), dtype=torch.uint8)
            mid = (p(c['depth']), p(c['feat']), p(c['rd']), p(c['ir']), p(c['st']), p(c['counts']), c['ir'].numel(), B, N, D, H, W, C, Z, Y, X,
                   p(dg), p(fg), p(ws), ws.numel(), None)
            _clear()
            if kw.get('zgrad'):
                code = lib.fbbev_bev_pool_v2_dense_bwd_z(p(og), 0, 0, p(torch.ones(B, C, Y, X)), 0.5, *mid)
            else:
                code = lib.fbbev_bev_pool_v2_dense_bwd(p(og), 0, 0, *mid)
        else:
            raise KeyError(entry)
        return [code] + _log()
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)


def _cases():
    t = {}

    def add(name, entry, **kw):
        assert name not in t, name
        t[name] = (entry, kw)
    # ---- the planar forward: store policy x channels per lane, channel split, workgroup size, XCD order, tile size, element type
    for st, s in ((0, 'st0'), (ST_NT, 'st1'), (ST_2, 'st2'), (SC1_NT, 'sc1nt')):
        add(f'fwd {s}', 'fwd', flags=st)
        add(f'fwd {s} cpl8', 'fwd', flags=st | CPL8)
    for n in (1, 2, 3, 0xF):
        add(f'fwd csplit {n}', 'fwd', flags=SC1_NT | CPL8 | CSPLIT(n))
    add('fwd C24 csplit 2 refuses cpl8', 'fwd', C=24, flags=SC1_NT | CPL8 | CSPLIT(2))
    add('fwd C80 csplit 0xF is 20', 'fwd', C=80, flags=SC1_NT | CPL8 | CSPLIT(0xF))
    add('fwd 128 threads', 'fwd', flags=SC1_NT | CPL8 | WG128)
    add('fwd workgroup field 2 is 256 threads', 'fwd', flags=SC1_NT | CPL8 | WG_2)
    add('fwd 128 threads st0 cpl4', 'fwd', flags=WG128)
    for tv in (64, 128, 256):
        add(f'fwd swizzle tv{tv}', 'fwd', tv=tv, flags=SC1_NT | CPL8 | SWIZZLE)
        add(f'fwd swizzle chunk 3 tv{tv}', 'fwd', tv=tv, flags=SC1_NT | CPL8 | SWIZZLE | CHUNK(3))
    add('fwd swizzle chunk 1 csplit 2', 'fwd', tv=64, flags=SC1_NT | SWIZZLE | CHUNK(1) | CSPLIT(2))
    add('fwd chunk field without the swizzle flag', 'fwd', flags=SC1_NT | CHUNK(3))
    for tv in (64, 256, 512, 1024, 100, 8):
        add(f'fwd tv{tv}', 'fwd', tv=tv, flags=SC1_NT | CPL8)
        add(f'fwd tv{tv} cpl4 st1', 'fwd', tv=tv, flags=ST_NT)
    for ot, s in ((OUT_BF16, 'bf16'), (OUT_F16, 'f16')):
        add(f'fwd {s}', 'fwd', flags=SC1_NT | CPL8 | ot)
        add(f'fwd {s} addend', 'fwd', flags=SC1_NT | CPL8 | ot, addend=True)
        add(f'fwd {s} 128 threads', 'fwd', flags=SC1_NT | CPL8 | ot | WG128)
        add(f'fwd {s} 128 threads addend', 'fwd', flags=SC1_NT | CPL8 | ot | WG128, addend=True)
        add(f'fwd {s} st0 cpl4 tv64 swizzle', 'fwd', tv=64, flags=ot | SWIZZLE)
        add(f'fwd {s} channels last', 'fwd', flags=SC1_NT | ot | CHANNELS_LAST)
    add('fwd both 16-bit types', 'fwd', flags=SC1_NT | OUT_BF16 | OUT_F16)
    add('fwd addend', 'fwd', flags=SC1_NT | CPL8, addend=True)
    add('fwd addend st0 tv256', 'fwd', tv=256, flags=0, addend=True)
    add('fwd addend channels last', 'fwd', flags=SC1_NT | CHANNELS_LAST, addend=True)
    # ---- the experimental routes of the planar forward
    for tv in (64, 128, 256, 512):
        add(f'fwd pipe tv{tv}', 'fwd', tv=tv, flags=SC1_NT | CPL8 | PIPE)
    add('fwd pipe cpl4 st2 swizzle addend', 'fwd', tv=64, flags=ST_2 | PIPE | SWIZZLE, addend=True)
    add('fwd pipe tpw 2', 'fwd', tv=64, flags=SC1_NT | CPL8 | PIPE | CSPLIT(2), env={'FBBEV_POOL_PIPE_TPW': '2'})
    add('fwd pipe tpw 100', 'fwd', tv=64, flags=SC1_NT | CPL8 | PIPE, env={'FBBEV_POOL_PIPE_TPW': '100'})
    add('fwd pipe tpw 2 tv256', 'fwd', tv=256, flags=SC1_NT | PIPE, env={'FBBEV_POOL_PIPE_TPW': '2'})
    add('fwd pipe st1 is the plain route', 'fwd', flags=ST_NT | CPL8 | PIPE)
    add('fwd pipe 128 threads is the plain route', 'fwd', flags=SC1_NT | CPL8 | PIPE | WG128)
    add('fwd pipe bf16 is the plain route', 'fwd', flags=SC1_NT | CPL8 | PIPE | OUT_BF16)
    add('fwd pipe gather8 is the pipe', 'fwd', flags=SC1_NT | CPL8 | PIPE | GATHER8)
    add('fwd pipe split-long is split-long', 'fwd', flags=SC1_NT | CPL8 | PIPE | SPLIT_LONG)
    for route, s in ((SPLIT_LONG, 'split-long'), (GATHER8, 'gather8'), (SPLIT_LONG | GATHER8, 'gather8 with split-long')):
        add(f'fwd {s} tv64', 'fwd', tv=64, flags=SC1_NT | route)
        add(f'fwd {s} tv128 cpl8 swizzle', 'fwd', flags=SC1_NT | CPL8 | SWIZZLE | route)
        add(f'fwd {s} st2 addend', 'fwd', flags=ST_2 | CPL8 | route, addend=True)
        add(f'fwd {s} 128 threads', 'fwd', flags=SC1_NT | CPL8 | WG128 | route)
        add(f'fwd {s} bf16', 'fwd', flags=SC1_NT | CPL8 | OUT_BF16 | route)
        add(f'fwd {s} st0', 'fwd', flags=CPL8 | route)
        add(f'fwd {s} st1', 'fwd', flags=ST_NT | CPL8 | route)
        add(f'fwd {s} tv256', 'fwd', tv=256, flags=SC1_NT | CPL8 | route)
    # ---- channels-last: 8 / 16 / 32-voxel tiles (plain round-robin at chunk 0), then the flat 64..1024-voxel tiles
    for tv in (8, 16, 32):
        for st, s in ((0, 'st0'), (ST_NT, 'st1'), (ST_2, 'st2'), (SC1_NT, 'sc1nt')):
            add(f'cl tv{tv} {s}', 'fwd', tv=tv, flags=CHANNELS_LAST | st)
        add(f'cl tv{tv} swizzle', 'fwd', tv=tv, flags=CHANNELS_LAST | SC1_NT | SWIZZLE)
        add(f'cl tv{tv} swizzle chunk 3', 'fwd', tv=tv, flags=CHANNELS_LAST | SC1_NT | SWIZZLE | CHUNK(3))
    add('cl tv32 C136 takes more than 1024 threads', 'fwd', C=136, tv=32, flags=CHANNELS_LAST | SC1_NT)
    for tv in (64, 128, 256, 512, 1024, 100):
        add(f'cl tv{tv}', 'fwd', tv=tv, flags=CHANNELS_LAST | SC1_NT)
        add(f'cl tv{tv} cpl8 swizzle', 'fwd', tv=tv, flags=CHANNELS_LAST | SC1_NT | CPL8 | SWIZZLE)
    for st, s in ((0, 'st0'), (ST_NT, 'st1'), (ST_2, 'st2')):
        add(f'cl tv128 {s} cpl8 swizzle chunk 3', 'fwd', flags=CHANNELS_LAST | st | CPL8 | SWIZZLE | CHUNK(3))
    add('cl tv128 ignores split, workgroup size and the experimental routes', 'fwd',
        flags=CHANNELS_LAST | SC1_NT | CSPLIT(2) | WG128 | PIPE | SPLIT_LONG | GATHER8)
    add('cl C20 refuses cpl8', 'fwd', C=20, flags=CHANNELS_LAST | SC1_NT | CPL8)
    # ---- rows of a strided slot
    for ot, s in ((0, 'f32'), (OUT_BF16, 'bf16'), (OUT_F16, 'f16')):
        for tv in (64, 128):
            add(f'rows {s} tv{tv}', 'rows', tv=tv, flags=SC1_NT | ot)
            add(f'rows {s} tv{tv} cpl8 swizzle addend', 'rows', tv=tv, flags=SC1_NT | CPL8 | SWIZZLE | ot, addend=True)
        add(f'rows {s} st0 swizzle chunk 3', 'rows', flags=ot | SWIZZLE | CHUNK(3))
        add(f'rows {s} st1 cpl8', 'rows', flags=ST_NT | CPL8 | ot)
    for tv in (256, 512, 1024, 100, 16):
        add(f'rows f32 tv{tv}', 'rows', tv=tv, flags=SC1_NT | CPL8)
    add('rows C20 f32 refuses cpl8', 'rows', C=20, flags=SC1_NT | CPL8)
    add('rows f32 ignores split, workgroup size and the experimental routes', 'rows', flags=SC1_NT | CSPLIT(2) | WG128 | PIPE | SPLIT_LONG | GATHER8)
    # ---- the store-floor diagnostic
    for ot, s in ((0, 'f32'), (OUT_BF16, 'bf16')):
        for mode in (1, 2, 3):
            add(f'diag {s} mode {mode}', 'diag', flags=SC1_NT | CPL8 | ot, mode=mode)
        add(f'diag {s} st2 swizzle csplit 2', 'diag', flags=ST_2 | CPL8 | SWIZZLE | CSPLIT(2) | ot, mode=1)
        add(f'diag {s} swizzle chunk 3', 'diag', flags=SC1_NT | CPL8 | SWIZZLE | CHUNK(3) | ot, mode=2)
    add('diag cpl4', 'diag', flags=SC1_NT, mode=1)
    add('diag st1', 'diag', flags=ST_NT | CPL8, mode=1)
    add('diag 128 threads', 'diag', flags=SC1_NT | CPL8 | WG128, mode=1)
    add('diag tv64', 'diag', tv=64, flags=SC1_NT | CPL8, mode=1)
    add('diag C24 csplit 2', 'diag', C=24, flags=SC1_NT | CPL8 | CSPLIT(2), mode=1)
    # ---- the Z-mean
    col = {'FBBEV_ZMEAN_COL': '1'}
    for tv in (64, 128, 256):
        add(f'zmean tv{tv}', 'zmean', tv=tv, flags=SC1_NT)
        add(f'zmean tv{tv} cpl8 column', 'zmean', tv=tv, flags=SC1_NT | CPL8, env=col)
    add('zmean cpl8 csplit 2', 'zmean', flags=CPL8 | CSPLIT(2))
    add('zmean column cpl4 csplit 2', 'zmean', flags=CSPLIT(2), env=col)
    add('zmean C24 csplit 2 refuses cpl8', 'zmean', C=24, flags=CPL8 | CSPLIT(2))
    add('zmean ignores store policy, workgroup size, swizzle and the experimental routes', 'zmean',
        flags=ST_NT | CPL8 | WG128 | SWIZZLE | CHUNK(3) | PIPE | SPLIT_LONG | GATHER8 | OUT_BF16)
    add('zmean tv512', 'zmean', tv=512, flags=SC1_NT)
    add('zmean tv100', 'zmean', tv=100, flags=SC1_NT)
    add('zmean channels last', 'zmean', flags=SC1_NT | CHANNELS_LAST)
    for g in (1, 2, 5):
        add(f'zmean {g} groups', 'zmean_split', flags=SC1_NT | CPL8, z_groups=g)
        add(f'zmean {g} groups column', 'zmean_split', flags=SC1_NT | CPL8, z_groups=g, env=col)
    add('zmean 2 groups tv64 cpl4 csplit 2', 'zmean_split', tv=64, flags=CSPLIT(2), z_groups=2)
    for bias in (False, True):
        add(f'zmean rows bias {bias}', 'zmean_rows', flags=SC1_NT | CPL8, bias=bias)
        add(f'zmean rows bias {bias} column', 'zmean_rows', tv=64, flags=SC1_NT, bias=bias, env=col)
    # ---- the tile index
    for entry in ('tile_index', 'tile_index_cached'):
        for tv in (64, 128, 256, 1024, 100):
            add(f'{entry} planar tv{tv}', entry, tv=tv, flags=SC1_NT | CPL8)
        for tv in (64, 128, 100):
            add(f'{entry} flat tv{tv}', entry, tv=tv, flags=CHANNELS_LAST)
        for tv in (8, 16, 32):
            add(f'{entry} small tv{tv}', entry, tv=tv, flags=CHANNELS_LAST)
            add(f'{entry} tv{tv} without channels last', entry, tv=tv, flags=0)
    add('tile_index_cached planar hit', 'tile_index_cached', flags=0, hit=1)
    # ---- the one-entry lift-splat
    for cache in (None, 'miss', 'hit'):
        add(f'lift_splat cache {cache}', 'lift_splat', flags=SC1_NT | CPL8 | SWIZZLE, cache=cache)
        add(f'lift_splat cache {cache} bf16 tv64', 'lift_splat', tv=64, flags=SC1_NT | OUT_BF16, cache=cache)
    add('lift_splat channels last small tiles', 'lift_splat', tv=16, flags=SC1_NT | CHANNELS_LAST)
    add('lift_splat channels last small tiles cached', 'lift_splat', tv=16, flags=SC1_NT | CHANNELS_LAST, cache='miss')
    add('lift_splat pipe', 'lift_splat', tv=64, flags=SC1_NT | CPL8 | PIPE)
    # ---- the fused backward
    for C in (16, 24, 136):
        add(f'bwd C{C}', 'bwd', C=C)
        add(f'bwd C{C} zgrad', 'bwd', C=C, zgrad=True)
    add('bwd C132 refused behind three launches', 'bwd', C=132)
    return t


CASES = _cases()


@pytest.mark.parametrize('name', list(CASES))
def test_pool_entry_launches_what_it_launched(inputs, name):
    entry, kw = CASES[name]
    assert run(inputs, entry, **kw) == LAUNCHES[name]


def test_the_table_has_every_case_and_both_kinds_of_rows():
    assert set(LAUNCHES) == set(CASES)
    assert any(v == [-2] for v in LAUNCHES.values()) and any(v[0] == 0 and len(v) > 3 for v in LAUNCHES.values())


# name -> [return code, (kernel instantiation, grid, block, dynamic LDS bytes), ...]
LAUNCHES = {
    'fwd st0': [0,
        ('k_pool_fwd_dense2<128, 4, 0, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd st0 cpl8': [0,
        ('k_pool_fwd_dense2<128, 8, 0, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd st1': [0,
        ('k_pool_fwd_dense2<128, 4, 1, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd st1 cpl8': [0,
        ('k_pool_fwd_dense2<128, 8, 1, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd st2': [0,
        ('k_pool_fwd_dense2<128, 4, 4, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd st2 cpl8': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd sc1nt': [0,
        ('k_pool_fwd_dense2<128, 4, 4, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd sc1nt cpl8': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd csplit 1': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd csplit 2': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 24, 256, 9856)],
    'fwd csplit 3': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd csplit 15': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd C24 csplit 2 refuses cpl8': [0,
        ('k_pool_fwd_dense2<128, 4, 4, 256, 0, false, 0, 0, 4>', 24, 256, 11968)],
    'fwd C80 csplit 0xF is 20': [0,
        ('k_pool_fwd_dense2<128, 4, 4, 256, 0, false, 0, 0, 4>', 240, 256, 7744)],
    'fwd 128 threads': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 128, 0, false, 0, 0, 4>', 12, 128, 14080)],
    'fwd workgroup field 2 is 256 threads': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd 128 threads st0 cpl4': [0,
        ('k_pool_fwd_dense2<128, 4, 0, 128, 0, false, 0, 0, 4>', 12, 128, 14080)],
    'fwd swizzle tv64': [0,
        ('k_pool_fwd_dense2<64, 8, 4, 256, 0, false, 0, 0, 4>', 512, 256, 9216)],
    'fwd swizzle chunk 3 tv64': [0,
        ('k_pool_fwd_dense2<64, 8, 4, 256, 0, false, 0, 0, 4>', 64, 256, 9216)],
    'fwd swizzle tv128': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 512, 256, 14080)],
    'fwd swizzle chunk 3 tv128': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 64, 256, 14080)],
    'fwd swizzle tv256': [0,
        ('k_pool_fwd_dense2<256, 8, 4, 256, 0, false, 0, 0, 4>', 512, 256, 23808)],
    'fwd swizzle chunk 3 tv256': [0,
        ('k_pool_fwd_dense2<256, 8, 4, 256, 0, false, 0, 0, 4>', 64, 256, 23808)],
    'fwd swizzle chunk 1 csplit 2': [0,
        ('k_pool_fwd_dense2<64, 4, 4, 256, 0, false, 0, 0, 4>', 48, 256, 7040)],
    'fwd chunk field without the swizzle flag': [0,
        ('k_pool_fwd_dense2<128, 4, 4, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd tv64': [0,
        ('k_pool_fwd_dense2<64, 8, 4, 256, 0, false, 0, 0, 4>', 18, 256, 9216)],
    'fwd tv64 cpl4 st1': [0,
        ('k_pool_fwd_dense2<64, 4, 1, 256, 0, false, 0, 0, 4>', 18, 256, 9216)],
    'fwd tv256': [0,
        ('k_pool_fwd_dense2<256, 8, 4, 256, 0, false, 0, 0, 4>', 6, 256, 23808)],
    'fwd tv256 cpl4 st1': [0,
        ('k_pool_fwd_dense2<256, 4, 1, 256, 0, false, 0, 0, 4>', 6, 256, 23808)],
    'fwd tv512': [0,
        ('k_pool_fwd_dense2<512, 8, 4, 256, 0, false, 0, 0, 4>', 6, 256, 43264)],
    'fwd tv512 cpl4 st1': [0,
        ('k_pool_fwd_dense2<512, 4, 1, 256, 0, false, 0, 0, 4>', 6, 256, 43264)],
    'fwd tv1024': [0,
        ('k_pool_fwd_dense2<1024, 8, 4, 256, 0, false, 0, 0, 4>', 6, 256, 82176)],
    'fwd tv1024 cpl4 st1': [0,
        ('k_pool_fwd_dense2<1024, 4, 1, 256, 0, false, 0, 0, 4>', 6, 256, 82176)],
    'fwd tv100': [0,
        ('k_pool_fwd_dense2<64, 8, 4, 256, 0, false, 0, 0, 4>', 18, 256, 9216)],
    'fwd tv100 cpl4 st1': [0,
        ('k_pool_fwd_dense2<64, 4, 1, 256, 0, false, 0, 0, 4>', 18, 256, 9216)],
    'fwd tv8': [0,
        ('k_pool_fwd_dense2<64, 8, 4, 256, 0, false, 0, 0, 4>', 18, 256, 9216)],
    'fwd tv8 cpl4 st1': [0,
        ('k_pool_fwd_dense2<64, 4, 1, 256, 0, false, 0, 0, 4>', 18, 256, 9216)],
    'fwd bf16': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 1, true, 0, 0, 4>', 12, 256, 9984)],
    'fwd bf16 addend': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 1, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd bf16 128 threads': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 128, 1, false, 0, 0, 4>', 12, 128, 14080)],
    'fwd bf16 128 threads addend': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 128, 1, false, 0, 0, 4>', 12, 128, 14080)],
    'fwd bf16 st0 cpl4 tv64 swizzle': [0,
        ('k_pool_fwd_dense2<64, 4, 4, 256, 1, true, 0, 0, 4>', 512, 256, 7168)],
    'fwd bf16 channels last': [-2],
    'fwd f16': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 2, true, 0, 0, 4>', 12, 256, 9984)],
    'fwd f16 addend': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 2, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd f16 128 threads': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 128, 2, false, 0, 0, 4>', 12, 128, 14080)],
    'fwd f16 128 threads addend': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 128, 2, false, 0, 0, 4>', 12, 128, 14080)],
    'fwd f16 st0 cpl4 tv64 swizzle': [0,
        ('k_pool_fwd_dense2<64, 4, 4, 256, 2, true, 0, 0, 4>', 512, 256, 7168)],
    'fwd f16 channels last': [-2],
    'fwd both 16-bit types': [-1],
    'fwd addend': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd addend st0 tv256': [0,
        ('k_pool_fwd_dense2<256, 4, 0, 256, 0, false, 0, 0, 4>', 6, 256, 23808)],
    'fwd addend channels last': [-2],
    'fwd pipe tv64': [0,
        ('k_pool_fwd_dense_pipe<64, 8, 4, 256>', 18, 256, 14080)],
    'fwd pipe tv128': [0,
        ('k_pool_fwd_dense_pipe<128, 8, 4, 256>', 12, 256, 19712)],
    'fwd pipe tv256': [0,
        ('k_pool_fwd_dense_pipe<256, 8, 4, 256>', 6, 256, 30976)],
    'fwd pipe tv512': [0,
        ('k_pool_fwd_dense2<512, 8, 4, 256, 0, false, 0, 0, 4>', 6, 256, 43264)],
    'fwd pipe cpl4 st2 swizzle addend': [0,
        ('k_pool_fwd_dense_pipe<64, 4, 4, 256>', 512, 256, 14080)],
    'fwd pipe tpw 2': [0,
        ('k_pool_fwd_dense_pipe<64, 8, 4, 256>', 18, 256, 11904)],
    'fwd pipe tpw 100': [0,
        ('k_pool_fwd_dense_pipe<64, 8, 4, 256>', 1, 256, 14080)],
    'fwd pipe tpw 2 tv256': [0,
        ('k_pool_fwd_dense_pipe<256, 4, 4, 256>', 3, 256, 30976)],
    'fwd pipe st1 is the plain route': [0,
        ('k_pool_fwd_dense2<128, 8, 1, 256, 0, false, 0, 0, 4>', 12, 256, 14080)],
    'fwd pipe 128 threads is the plain route': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 128, 0, false, 0, 0, 4>', 12, 128, 14080)],
    'fwd pipe bf16 is the plain route': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 1, true, 0, 0, 4>', 12, 256, 9984)],
    'fwd pipe gather8 is the pipe': [0,
        ('k_pool_fwd_dense_pipe<128, 8, 4, 256>', 12, 256, 19712)],
    'fwd pipe split-long is split-long': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 32, 4>', 12, 256, 16656)],
    'fwd split-long tv64': [0,
        ('k_pool_fwd_dense2<64, 4, 4, 256, 0, false, 0, 32, 4>', 18, 256, 11536)],
    'fwd split-long tv128 cpl8 swizzle': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 32, 4>', 512, 256, 16656)],
    'fwd split-long st2 addend': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 32, 4>', 12, 256, 16656)],
    'fwd split-long 128 threads': [-2],
    'fwd split-long bf16': [-2],
    'fwd split-long st0': [-2],
    'fwd split-long st1': [-2],
    'fwd split-long tv256': [-2],
    'fwd gather8 tv64': [0,
        ('k_pool_fwd_dense2<64, 4, 4, 256, 0, false, 0, 0, 8>', 18, 256, 9216)],
    'fwd gather8 tv128 cpl8 swizzle': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 8>', 512, 256, 14080)],
    'fwd gather8 st2 addend': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 8>', 12, 256, 14080)],
    'fwd gather8 128 threads': [-2],
    'fwd gather8 bf16': [-2],
    'fwd gather8 st0': [-2],
    'fwd gather8 st1': [-2],
    'fwd gather8 tv256': [-2],
    'fwd gather8 with split-long tv64': [0,
        ('k_pool_fwd_dense2<64, 4, 4, 256, 0, false, 0, 32, 4>', 18, 256, 11536)],
    'fwd gather8 with split-long tv128 cpl8 swizzle': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 32, 4>', 512, 256, 16656)],
    'fwd gather8 with split-long st2 addend': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 32, 4>', 12, 256, 16656)],
    'fwd gather8 with split-long 128 threads': [-2],
    'fwd gather8 with split-long bf16': [-2],
    'fwd gather8 with split-long st0': [-2],
    'fwd gather8 with split-long st1': [-2],
    'fwd gather8 with split-long tv256': [-2],
    'cl tv8 st0': [0,
        ('k_pool_fwd_cl_small<0>', 108, 64, 0)],
    'cl tv8 st1': [0,
        ('k_pool_fwd_cl_small<1>', 108, 64, 0)],
    'cl tv8 st2': [0,
        ('k_pool_fwd_cl_small<4>', 108, 64, 0)],
    'cl tv8 sc1nt': [0,
        ('k_pool_fwd_cl_small<4>', 108, 64, 0)],
    'cl tv8 swizzle': [0,
        ('k_pool_fwd_cl_small<4>', 112, 64, 0)],
    'cl tv8 swizzle chunk 3': [0,
        ('k_pool_fwd_cl_small<4>', 128, 64, 0)],
    'cl tv16 st0': [0,
        ('k_pool_fwd_cl_small<0>', 54, 64, 0)],
    'cl tv16 st1': [0,
        ('k_pool_fwd_cl_small<1>', 54, 64, 0)],
    'cl tv16 st2': [0,
        ('k_pool_fwd_cl_small<4>', 54, 64, 0)],
    'cl tv16 sc1nt': [0,
        ('k_pool_fwd_cl_small<4>', 54, 64, 0)],
    'cl tv16 swizzle': [0,
        ('k_pool_fwd_cl_small<4>', 56, 64, 0)],
    'cl tv16 swizzle chunk 3': [0,
        ('k_pool_fwd_cl_small<4>', 64, 64, 0)],
    'cl tv32 st0': [0,
        ('k_pool_fwd_cl_small<0>', 27, 128, 0)],
    'cl tv32 st1': [0,
        ('k_pool_fwd_cl_small<1>', 27, 128, 0)],
    'cl tv32 st2': [0,
        ('k_pool_fwd_cl_small<4>', 27, 128, 0)],
    'cl tv32 sc1nt': [0,
        ('k_pool_fwd_cl_small<4>', 27, 128, 0)],
    'cl tv32 swizzle': [0,
        ('k_pool_fwd_cl_small<4>', 32, 128, 0)],
    'cl tv32 swizzle chunk 3': [0,
        ('k_pool_fwd_cl_small<4>', 64, 128, 0)],
    'cl tv32 C136 takes more than 1024 threads': [-2],
    'cl tv64': [0,
        ('k_pool_fwd_dense_cl<64, 4, 4, 256>', 14, 256, 4864)],
    'cl tv64 cpl8 swizzle': [0,
        ('k_pool_fwd_dense_cl<64, 8, 4, 256>', 128, 256, 4864)],
    'cl tv128': [0,
        ('k_pool_fwd_dense_cl<128, 4, 4, 256>', 7, 256, 5632)],
    'cl tv128 cpl8 swizzle': [0,
        ('k_pool_fwd_dense_cl<128, 8, 4, 256>', 128, 256, 5632)],
    'cl tv256': [0,
        ('k_pool_fwd_dense_cl<256, 4, 4, 256>', 4, 256, 7168)],
    'cl tv256 cpl8 swizzle': [0,
        ('k_pool_fwd_dense_cl<256, 8, 4, 256>', 128, 256, 7168)],
    'cl tv512': [0,
        ('k_pool_fwd_dense_cl<512, 4, 4, 256>', 2, 256, 10240)],
    'cl tv512 cpl8 swizzle': [0,
        ('k_pool_fwd_dense_cl<512, 8, 4, 256>', 128, 256, 10240)],
    'cl tv1024': [0,
        ('k_pool_fwd_dense_cl<1024, 4, 4, 256>', 1, 256, 16384)],
    'cl tv1024 cpl8 swizzle': [0,
        ('k_pool_fwd_dense_cl<1024, 8, 4, 256>', 128, 256, 16384)],
    'cl tv100': [0,
        ('k_pool_fwd_dense_cl<64, 4, 4, 256>', 14, 256, 4864)],
    'cl tv100 cpl8 swizzle': [0,
        ('k_pool_fwd_dense_cl<64, 8, 4, 256>', 128, 256, 4864)],
    'cl tv128 st0 cpl8 swizzle chunk 3': [0,
        ('k_pool_fwd_dense_cl<128, 8, 0, 256>', 64, 256, 5632)],
    'cl tv128 st1 cpl8 swizzle chunk 3': [0,
        ('k_pool_fwd_dense_cl<128, 8, 1, 256>', 64, 256, 5632)],
    'cl tv128 st2 cpl8 swizzle chunk 3': [0,
        ('k_pool_fwd_dense_cl<128, 8, 4, 256>', 64, 256, 5632)],
    'cl tv128 ignores split, workgroup size and the experimental routes': [0,
        ('k_pool_fwd_dense_cl<128, 4, 4, 256>', 7, 256, 5632)],
    'cl C20 refuses cpl8': [0,
        ('k_pool_fwd_dense_cl<128, 4, 4, 256>', 7, 256, 5632)],
    'rows f32 tv64': [0,
        ('k_pool_fwd_dense_rows<64, 4, 4, 256, 0>', 14, 256, 4864)],
    'rows f32 tv64 cpl8 swizzle addend': [0,
        ('k_pool_fwd_dense_rows<64, 8, 4, 256, 0>', 128, 256, 4864)],
    'rows f32 tv128': [0,
        ('k_pool_fwd_dense_rows<128, 4, 4, 256, 0>', 7, 256, 5632)],
    'rows f32 tv128 cpl8 swizzle addend': [0,
        ('k_pool_fwd_dense_rows<128, 8, 4, 256, 0>', 128, 256, 5632)],
    'rows f32 st0 swizzle chunk 3': [0,
        ('k_pool_fwd_dense_rows<128, 4, 0, 256, 0>', 64, 256, 5632)],
    'rows f32 st1 cpl8': [0,
        ('k_pool_fwd_dense_rows<128, 8, 1, 256, 0>', 7, 256, 5632)],
    'rows bf16 tv64': [0,
        ('k_pool_fwd_dense_rows<64, 8, 4, 256, 1>', 14, 256, 4864)],
    'rows bf16 tv64 cpl8 swizzle addend': [0,
        ('k_pool_fwd_dense_rows<64, 8, 4, 256, 1>', 128, 256, 4864)],
    'rows bf16 tv128': [0,
        ('k_pool_fwd_dense_rows<128, 8, 4, 256, 1>', 7, 256, 5632)],
    'rows bf16 tv128 cpl8 swizzle addend': [0,
        ('k_pool_fwd_dense_rows<128, 8, 4, 256, 1>', 128, 256, 5632)],
    'rows bf16 st0 swizzle chunk 3': [0,
        ('k_pool_fwd_dense_rows<128, 8, 4, 256, 1>', 64, 256, 5632)],
    'rows bf16 st1 cpl8': [0,
        ('k_pool_fwd_dense_rows<128, 8, 4, 256, 1>', 7, 256, 5632)],
    'rows f16 tv64': [0,
        ('k_pool_fwd_dense_rows<64, 8, 4, 256, 2>', 14, 256, 4864)],
    'rows f16 tv64 cpl8 swizzle addend': [0,
        ('k_pool_fwd_dense_rows<64, 8, 4, 256, 2>', 128, 256, 4864)],
    'rows f16 tv128': [0,
        ('k_pool_fwd_dense_rows<128, 8, 4, 256, 2>', 7, 256, 5632)],
    'rows f16 tv128 cpl8 swizzle addend': [0,
        ('k_pool_fwd_dense_rows<128, 8, 4, 256, 2>', 128, 256, 5632)],
    'rows f16 st0 swizzle chunk 3': [0,
        ('k_pool_fwd_dense_rows<128, 8, 4, 256, 2>', 64, 256, 5632)],
    'rows f16 st1 cpl8': [0,
        ('k_pool_fwd_dense_rows<128, 8, 4, 256, 2>', 7, 256, 5632)],
    'rows f32 tv256': [0,
        ('k_pool_fwd_dense_rows<256, 8, 4, 256, 0>', 4, 256, 7168)],
    'rows f32 tv512': [0,
        ('k_pool_fwd_dense_rows<512, 8, 4, 256, 0>', 2, 256, 10240)],
    'rows f32 tv1024': [0,
        ('k_pool_fwd_dense_rows<1024, 8, 4, 256, 0>', 1, 256, 16384)],
    'rows f32 tv100': [0,
        ('k_pool_fwd_dense_rows<64, 8, 4, 256, 0>', 14, 256, 4864)],
    'rows f32 tv16': [-2],
    'rows C20 f32 refuses cpl8': [0,
        ('k_pool_fwd_dense_rows<128, 4, 4, 256, 0>', 7, 256, 5632)],
    'rows f32 ignores split, workgroup size and the experimental routes': [0,
        ('k_pool_fwd_dense_rows<128, 4, 4, 256, 0>', 7, 256, 5632)],
    'diag f32 mode 1': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 1>', 12, 256, 14080)],
    'diag f32 mode 2': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 2>', 12, 256, 14080)],
    'diag f32 mode 3': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 3>', 12, 256, 14080)],
    'diag f32 st2 swizzle csplit 2': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 1>', 512, 256, 9856)],
    'diag f32 swizzle chunk 3': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 2>', 64, 256, 14080)],
    'diag bf16 mode 1': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 1, true, 1>', 12, 256, 9984)],
    'diag bf16 mode 2': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 1, true, 2>', 12, 256, 9984)],
    'diag bf16 mode 3': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 1, true, 3>', 12, 256, 9984)],
    'diag bf16 st2 swizzle csplit 2': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 1, true, 1>', 512, 256, 7808)],
    'diag bf16 swizzle chunk 3': [0,
        ('k_pool_fwd_dense2<128, 8, 4, 256, 1, true, 2>', 64, 256, 9984)],
    'diag cpl4': [-2],
    'diag st1': [-2],
    'diag 128 threads': [-2],
    'diag tv64': [-2],
    'diag C24 csplit 2': [-2],
    'zmean tv64': [0,
        ('k_pool_zmean<64, 4, 256>', 6, 256, 9216)],
    'zmean tv64 cpl8 column': [0,
        ('k_pool_zmean_col<64, 8, 256>', 6, 256, 14176)],
    'zmean tv128': [0,
        ('k_pool_zmean<128, 4, 256>', 4, 256, 14080)],
    'zmean tv128 cpl8 column': [0,
        ('k_pool_zmean_col<128, 8, 256>', 4, 256, 19808)],
    'zmean tv256': [0,
        ('k_pool_zmean<256, 4, 256>', 2, 256, 23808)],
    'zmean tv256 cpl8 column': [0,
        ('k_pool_zmean_col<256, 8, 256>', 2, 256, 31072)],
    'zmean cpl8 csplit 2': [0,
        ('k_pool_zmean<128, 8, 256>', 8, 256, 9856)],
    'zmean column cpl4 csplit 2': [0,
        ('k_pool_zmean_col<128, 4, 256>', 8, 256, 15584)],
    'zmean C24 csplit 2 refuses cpl8': [0,
        ('k_pool_zmean<128, 4, 256>', 8, 256, 11968)],
    'zmean ignores store policy, workgroup size, swizzle and the experimental routes': [0,
        ('k_pool_zmean<128, 8, 256>', 4, 256, 14080)],
    'zmean tv512': [-2],
    'zmean tv100': [0,
        ('k_pool_zmean<64, 4, 256>', 6, 256, 9216)],
    'zmean channels last': [-2],
    'zmean 1 groups': [0,
        ('k_pool_zmean<128, 8, 256>', 4, 256, 14080)],
    'zmean 1 groups column': [0,
        ('k_pool_zmean_col<128, 8, 256>', 4, 256, 19808)],
    'zmean 2 groups': [0,
        ('k_pool_zmean<128, 8, 256>', 8, 256, 14080),
        ('k_pool_zmean_reduce', 5, 256, 0)],
    'zmean 2 groups column': [0,
        ('k_pool_zmean<128, 8, 256>', 8, 256, 14080),
        ('k_pool_zmean_reduce', 5, 256, 0)],
    'zmean 5 groups': [0,
        ('k_pool_zmean<128, 8, 256>', 12, 256, 14080),
        ('k_pool_zmean_reduce', 5, 256, 0)],
    'zmean 5 groups column': [0,
        ('k_pool_zmean<128, 8, 256>', 12, 256, 14080),
        ('k_pool_zmean_reduce', 5, 256, 0)],
    'zmean 2 groups tv64 cpl4 csplit 2': [0,
        ('k_pool_zmean<64, 4, 256>', 24, 256, 7040),
        ('k_pool_zmean_reduce', 5, 256, 0)],
    'zmean rows bias False': [0,
        ('k_pool_zmean<128, 8, 256>', 4, 256, 14080)],
    'zmean rows bias False column': [0,
        ('k_pool_zmean<64, 4, 256>', 6, 256, 9216)],
    'zmean rows bias True': [0,
        ('k_pool_zmean<128, 8, 256>', 4, 256, 14080)],
    'zmean rows bias True column': [0,
        ('k_pool_zmean<64, 4, 256>', 6, 256, 9216)],
    'tile_index planar tv64': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index planar tv128': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index planar tv256': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index planar tv1024': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index planar tv100': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index flat tv64': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index flat tv128': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index flat tv100': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index small tv8': [0,
        ('k_tile_scatter', 1, 256, 0)],
    'tile_index tv8 without channels last': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index small tv16': [0,
        ('k_tile_scatter', 1, 256, 0)],
    'tile_index tv16 without channels last': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index small tv32': [0,
        ('k_tile_scatter', 1, 256, 0)],
    'tile_index tv32 without channels last': [0,
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached planar tv64': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached planar tv128': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached planar tv256': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached planar tv1024': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached planar tv100': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached flat tv64': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached flat tv128': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached flat tv100': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached small tv8': [-2],
    'tile_index_cached tv8 without channels last': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached small tv16': [-2],
    'tile_index_cached tv16 without channels last': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached small tv32': [-2],
    'tile_index_cached tv32 without channels last': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'tile_index_cached planar hit': [0,
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0)],
    'lift_splat cache None': [0,
        ('k_keys_hist_geom<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_sort_hist<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_interval_count<4, 4>', 1, 256, 0),
        ('k_interval_write<4, 4>', 1, 256, 8192),
        ('k_nchw_to_nhwc', 2, 256, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 512, 256, 14080)],
    'lift_splat cache None bf16 tv64': [0,
        ('k_keys_hist_geom<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_sort_hist<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_interval_count<4, 4>', 1, 256, 0),
        ('k_interval_write<4, 4>', 1, 256, 8192),
        ('k_nchw_to_nhwc', 2, 256, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_fwd_dense2<64, 4, 4, 256, 1, true, 0, 0, 4>', 18, 256, 7168)],
    'lift_splat cache miss': [0,
        ('k_cam_key', 1, 256, 0),
        ('k_keys_hist_geom<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_sort_hist<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_interval_count<4, 4>', 1, 256, 0),
        ('k_interval_write<4, 4>', 1, 256, 8192),
        ('k_nchw_to_nhwc', 2, 256, 0),
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 512, 256, 14080)],
    'lift_splat cache miss bf16 tv64': [0,
        ('k_cam_key', 1, 256, 0),
        ('k_keys_hist_geom<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_sort_hist<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_interval_count<4, 4>', 1, 256, 0),
        ('k_interval_write<4, 4>', 1, 256, 8192),
        ('k_nchw_to_nhwc', 2, 256, 0),
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_fwd_dense2<64, 4, 4, 256, 1, true, 0, 0, 4>', 18, 256, 7168)],
    'lift_splat cache hit': [0,
        ('k_cam_key', 1, 256, 0),
        ('k_keys_hist_geom<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_sort_hist<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_interval_count<4, 4>', 1, 256, 0),
        ('k_interval_write<4, 4>', 1, 256, 8192),
        ('k_nchw_to_nhwc', 2, 256, 0),
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_fwd_dense2<128, 8, 4, 256, 0, false, 0, 0, 4>', 512, 256, 14080)],
    'lift_splat cache hit bf16 tv64': [0,
        ('k_cam_key', 1, 256, 0),
        ('k_keys_hist_geom<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_sort_hist<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_interval_count<4, 4>', 1, 256, 0),
        ('k_interval_write<4, 4>', 1, 256, 8192),
        ('k_nchw_to_nhwc', 2, 256, 0),
        ('k_tile_table_gate', 1, 1, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_fwd_dense2<64, 4, 4, 256, 1, true, 0, 0, 4>', 18, 256, 7168)],
    'lift_splat channels last small tiles': [0,
        ('k_keys_hist_geom<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_sort_hist<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_interval_count<4, 4>', 1, 256, 0),
        ('k_interval_write<4, 4>', 1, 256, 8192),
        ('k_nchw_to_nhwc', 2, 256, 0),
        ('k_tile_scatter', 1, 256, 0),
        ('k_pool_fwd_cl_small<4>', 54, 64, 0)],
    'lift_splat channels last small tiles cached': [-2,
        ('k_cam_key', 1, 256, 0),
        ('k_keys_hist_geom<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_sort_hist<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_interval_count<4, 4>', 1, 256, 0),
        ('k_interval_write<4, 4>', 1, 256, 8192),
        ('k_nchw_to_nhwc', 2, 256, 0)],
    'lift_splat pipe': [0,
        ('k_keys_hist_geom<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_sort_hist<256, 8>', 1, 256, 0),
        ('k_sort_scatter<4, 8>', 1, 256, 0),
        ('k_interval_count<4, 4>', 1, 256, 0),
        ('k_interval_write<4, 4>', 1, 256, 8192),
        ('k_nchw_to_nhwc', 2, 256, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_fwd_dense_pipe<64, 8, 4, 256>', 18, 256, 14080)],
    'bwd C16': [0,
        ('k_point_row_table', 1, 256, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_bwd_rows<128>', 12, 256, 8448),
        ('k_pool_bwd_pixel<4>', 2, 256, 0)],
    'bwd C16 zgrad': [0,
        ('k_point_row_table', 1, 256, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_bwd_rows<128>', 12, 256, 8448),
        ('k_pool_bwd_pixel<4>', 2, 256, 0)],
    'bwd C24': [0,
        ('k_point_row_table', 1, 256, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_bwd_rows<128>', 12, 256, 12672),
        ('k_pool_bwd_pixel<4>', 2, 256, 0)],
    'bwd C24 zgrad': [0,
        ('k_point_row_table', 1, 256, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_bwd_rows<128>', 12, 256, 12672),
        ('k_pool_bwd_pixel<4>', 2, 256, 0)],
    'bwd C136': [0,
        ('k_point_row_table', 1, 256, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_bwd_rows<128>', 12, 256, 71808),
        ('k_pool_bwd_pixel<8>', 2, 256, 0)],
    'bwd C136 zgrad': [0,
        ('k_point_row_table', 1, 256, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_bwd_rows<128>', 12, 256, 71808),
        ('k_pool_bwd_pixel<8>', 2, 256, 0)],
    'bwd C132 refused behind three launches': [-2,
        ('k_point_row_table', 1, 256, 0),
        ('k_tile_lower_bound2', 1, 256, 0),
        ('k_pool_bwd_rows<128>', 12, 256, 69696)],
}
