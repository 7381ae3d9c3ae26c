"""The high-digit-first rank build (FBBEV_RANK_FINISH=1: one scatter by the high 10 key bits, k_bucket_finish, k_bucket_intervals)
on the CPU emulator against the two-pass segmented route (=0) and against ViewTransformerOracle.voxel_pooling_prepare_v2: all index
tensors and counts with torch.equal, on the edge cases of tests/rank_finish_cases.py.  Every build gets a workspace filled with
0xA5 and outputs filled with -7: nothing may rely on cleared memory."""
import ctypes
import os
import sys
from ctypes import c_void_p

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import emu_capi as E  # noqa: E402
import rank_finish_cases as T  # noqa: E402


def _build(dims, coor, ws=None, depth=None, thr=0.01):
    B, N, D, H, W, _ = coor.shape
    n = B * N * D * H * W
    out = [torch.full((n,), -7, dtype=torch.int32) for _ in range(6)]
    counts = torch.full((2,), -1, dtype=torch.int32)
    need = E.lib().fbbev_rank_workspace_bytes(n)
    if ws is None:
        ws = torch.full((need,), 0xA5, dtype=torch.uint8)
    assert ws.numel() >= need
    arr = ctypes.c_float * 3
    lo, it, gs = arr(0.0, 0.0, 0.0), arr(1.0, 1.0, 1.0), arr(*[float(d) for d in dims])
    tail = (B, N, D, H, W, ctypes.cast(lo, c_void_p), ctypes.cast(it, c_void_p), ctypes.cast(gs, c_void_p), *[E.p(t) for t in out],
            E.p(counts), E.p(ws), ws.numel(), None)
    if depth is None:
        E.ok(E.lib().fbbev_rank_build(E.p(coor), *tail))
    else:
        E.ok(E.lib().fbbev_rank_build_depth(E.p(coor), E.p(depth), thr, *tail))
    return (*out, counts)


def _both_routes(monkeypatch, dims, coor, **kw):
    """route 1 and route 0 (both on the two-pass segmented plan) -> the new route's build, checked against the old one"""
    monkeypatch.setenv('FBBEV_RANK_SEG', '2')
    monkeypatch.setenv('FBBEV_RANK_FINISH', '0')
    old = _build(dims, coor, **kw)
    monkeypatch.setenv('FBBEV_RANK_FINISH', '1')
    new = _build(dims, coor, **kw)
    assert torch.equal(new[6], old[6])
    T.assert_index(new, T.exact(old), 'route 1 vs route 0')
    return new


@pytest.mark.parametrize('name', T.CASES)
def test_finish_route_equals_two_pass_route_and_oracle_emulated(name, monkeypatch):
    dims, coor = T.case(name)
    new = _both_routes(monkeypatch, dims, coor)
    exp = T.oracle_index(dims, coor)
    T.assert_index(new, exp, name)
    if name == 'empty_B2':
        assert new[6].tolist() == [0, 0]
    if name == 'one_voxel_B1':
        assert new[6].tolist() == [9000, 1] and new[4][0].item() == 9000
    if name == 'low4_B3':                                     # the buckets the case was built for are really there
        rb = new[0][:new[6][0]].long()
        per_bucket = torch.bincount(rb[rb < 15990] >> 4, minlength=1000)
        assert per_bucket[5] == 64 and per_bucket[7] == 65 and per_bucket[9] == 3000 and per_bucket[999] >= 23
        assert (per_bucket == 0).sum() > 300
        assert len({int((rb >= b * 15990).sum() - (rb >= (b + 1) * 15990).sum()) for b in range(3)}) == 3


def test_finish_route_depth_threshold_entry_emulated(monkeypatch):
    dims, coor = T.case('low4_B3')
    d = T.depth_for(coor)
    new = _both_routes(monkeypatch, dims, coor, depth=d)
    T.assert_index(new, T.oracle_index(dims, coor, d), 'depth')
    assert 0 < new[6][0] < T.oracle_index(dims, coor)[0].numel()


def test_finish_route_two_builds_on_one_workspace_emulated(monkeypatch):
    """the second build finds the first one's bucket offsets, head counts and pairs in the workspace and must not read them"""
    monkeypatch.setenv('FBBEV_RANK_SEG', '2')
    monkeypatch.setenv('FBBEV_RANK_FINISH', '1')
    dims, coor = T.case('low4_B3')
    _, coor2 = T.case('low4_B3', seed=1)
    n = coor.numel() // 3
    ws = torch.full((E.lib().fbbev_rank_workspace_bytes(n),), 0xA5, dtype=torch.uint8)
    first = _build(dims, coor, ws=ws)
    T.assert_index(first, T.oracle_index(dims, coor), 'first')
    second = _build(dims, coor2, ws=ws)
    T.assert_index(second, T.oracle_index(dims, coor2), 'second')
    assert not torch.equal(first[1], second[1])
    _, coor3 = T.case('one_voxel_B1')                         # a smaller build (one sample) in the same, larger buffer
    T.assert_index(_build(dims, coor3, ws=ws), T.oracle_index(dims, coor3), 'third')


def test_finish_route_leaves_one_digit_plans_and_the_global_sort_alone_emulated(monkeypatch):
    """FBBEV_RANK_FINISH=1 means "wherever legal": a sample of at most 2^10 voxels (one digit) and the global sort keep their routes"""
    monkeypatch.setenv('FBBEV_RANK_FINISH', '1')
    dims = (8, 8, 4)
    import numpy as np
    coor = T._coor(dims, [np.arange(256).repeat(3), np.arange(100)], 1200, 0)
    for seg in ('2', '0'):
        monkeypatch.setenv('FBBEV_RANK_SEG', seg)
        T.assert_index(_build(dims, coor), T.oracle_index(dims, coor), 'seg ' + seg)
