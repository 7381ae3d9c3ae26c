"""fbbev_bev_pool_v2_dense_fwd_rows on the CPU emulator (the product's capi.hip + kernel headers compiled against tests/emu/rt.h):
the pooled volume written once as slot 0 of a voxel-major ring == today's composite -- fbbev_bev_pool_v2_dense_fwd[_add] into an fp32
(B,C,Z,Y,X) volume, then fbbev_history_frame_vm into the slot -- word for word, and == the loop-exact oracle cast by torch."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'emu'))
import emu_capi as E  # noqa: E402
import pool_rows_cases as K  # noqa: E402

CPL8, SWIZZLE, SC1_NT = 0x4, 0x400, 0x20000
CHANNELS_LAST, OUT_BF16, OUT_F16 = 0x100000, 0x800000, 0x1000000


def pool_dense_rows(depth, feat, rd, rf, ir, st, ln, counts, n_max, B, C, Z, Y, X, tile_voxels, out_rows, flags=0, addend_rows=None):
    """Emulator binding of fbbev_bev_pool_v2_dense_fwd_rows: out_rows (B, Z*Y*X, C) f32 / bf16 / f16 with any batch stride (slot 0 of
    a (B, T+1, N, C) ring), the storage flag follows its dtype; addend_rows (B, Y*X, C) f32 or None.  -> return code"""
    from ctypes import c_void_p
    lib, p = E.lib(), E.p
    fl = (flags & ~(OUT_BF16 | OUT_F16)) | {torch.float32: 0, torch.bfloat16: OUT_BF16, torch.float16: OUT_F16}[out_rows.dtype]
    ws = torch.zeros(lib.fbbev_pool_dense_workspace_bytes(B, Z, Y, X), dtype=torch.uint8)
    E.ok(lib.fbbev_pool_tile_index(p(ir), p(st), p(counts), n_max, B, Z, Y, X, tile_voxels, flags | CHANNELS_LAST, p(ws), ws.numel(), None))
    assert out_rows.stride()[1:] == (C, 1) and not out_rows.is_cuda
    return lib.fbbev_bev_pool_v2_dense_fwd_rows(p(depth), p(feat), p(rd), p(rf), p(ir), p(st), p(ln), B, C, Z, Y, X,
                                                c_void_p(out_rows.data_ptr()), out_rows.stride(0) if B > 1 else 0,
                                                None if addend_rows is None else c_void_p(addend_rows.data_ptr()),
                                                0 if addend_rows is None else addend_rows.stride(1), p(ws), ws.numel(),
                                                tile_voxels, fl, None)
PATTERN = {torch.float32: 12345.0, torch.bfloat16: 3.0, torch.float16: 5.0}


@pytest.fixture(scope='module')
def cases():
    return {C: K.build(C) for C in K.CHANNELS}


def _idx(c):
    return (c['depth'], c['feat'], c['ranks_depth'], c['ranks_feat'], c['interval_rank'], c['interval_starts'], c['interval_lengths'],
            c['counts'], c['n_max'])


@pytest.mark.parametrize('with_addend', [False, True])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize('tv', K.TILES)
@pytest.mark.parametrize('C', K.CHANNELS)
def test_rows_entry_equals_composite_and_oracle(cases, C, tv, dtype, with_addend):
    c = cases[C]
    B, Z, Y, X, N, T = K.B, K.Z, K.Y, K.X, K.ZYX, K.T_RING
    add_rows = c['addend_rows'] if with_addend else None
    # today's composite: fp32 planes (+ the planar addend), then the transposing, rounding copy into slot 0
    add_planes = add_rows.transpose(1, 2).reshape(B, C, Y, X).contiguous() if with_addend else None
    code, vol = E.pool_dense(*_idx(c), B, C, Z, Y, X, tv, CPL8 | SC1_NT, addend=add_planes)
    assert code == 0 and not torch.isnan(vol).any()
    ring0 = torch.full((B, T + 1, N, C), PATTERN[dtype], dtype=dtype)
    E.history_frame_vm(vol.view(B, C, N), dtype, out=ring0[:, 0])
    # the new entry, straight into slot 0 of a second ring
    ring1 = torch.full((B, T + 1, N, C), PATTERN[dtype], dtype=dtype)
    flags = (CPL8 | SC1_NT | SWIZZLE) if tv == 128 else SC1_NT          # both lane-group shapes of the fp32 rows, with / without the XCD order
    assert pool_dense_rows(*_idx(c), B, C, Z, Y, X, tv, ring1[:, 0], flags=flags, addend_rows=add_rows) == 0
    assert torch.equal(K.words(ring1), K.words(ring0))                  # slot 0 bit for bit, slots 1..T untouched
    assert (ring1[:, 1:] == PATTERN[dtype]).all()
    assert torch.equal(K.words(ring1[:, 0]), K.words(K.expected_rows(c, C, dtype, with_addend)))


def test_rows_entry_padded_addend_rows_and_contiguous_output(cases):
    """addend rows with a stride (a column block of a wider buffer) and a contiguous (B, N, C) destination (stride 0 = default)."""
    C, tv = 16, 64
    c = cases[C]
    B, Z, Y, X, N = K.B, K.Z, K.Y, K.X, K.ZYX
    wide = torch.full((B, K.YX, C + 8), float('nan'))
    wide[..., :C] = c['addend_rows']
    out = torch.full((B, N, C), float('nan'), dtype=torch.float16)
    assert pool_dense_rows(*_idx(c), B, C, Z, Y, X, tv, out, flags=SC1_NT, addend_rows=wide[..., :C]) == 0
    assert torch.equal(K.words(out), K.words(K.expected_rows(c, C, torch.float16, True)))
