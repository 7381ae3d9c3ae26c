"""The view transformation writes its volume once, as slot 0 of the voxel-major history ring (fbbev_bev_pool_v2_dense_fwd_rows):
(a) the kernel against today's composite and the CPU oracle, word for word; (b) the direct-slot route of FBViewTransform +
TemporalHistoryFusion against today's route over a three-frame sequence with a restart; (c) the cases that must fall back."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pool_rows_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
PATTERN = {torch.float32: 12345.0, torch.bfloat16: 3.0, torch.float16: 5.0}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cases(dev):
    """per channel count: the host case (kept unchanged: the oracle reads it) and its device copy"""
    out = {}
    for C in K.CHANNELS:
        c = K.build(C)
        out[C] = (c, {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()})
    return out


# ------------------------------------------------------------------------------------------------ (a) kernel
@pytest.mark.parametrize('with_addend', [False, True])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize('tv', K.TILES)
@pytest.mark.parametrize('C', K.CHANNELS)
def test_rows_kernel_equals_composite_and_oracle(dev, cases, C, tv, dtype, with_addend):
    from fb_bev_amd import _capi
    host, c = cases[C]
    B, Z, Y, X, N, T = K.B, K.Z, K.Y, K.X, K.ZYX, K.T_RING
    idx = (c['depth'], c['feat'], c['ranks_depth'], c['ranks_feat'], c['interval_rank'], c['interval_starts'], c['interval_lengths'])
    ws_bytes = _capi.pool_dense_workspace_bytes(B, Z, Y, X)
    flags = _capi.pool_flags(csplit=1)
    # addend rows with a PADDED row stride (pattern in the padding): a column block of a wider buffer
    wide = torch.full((B, K.YX, C + 8), 777.0, device=dev)
    wide[..., :C] = c['addend_rows']
    add_rows = wide[..., :C] if with_addend else None
    # today's composite: fp32 planes (+ planar addend) -> transposing, rounding copy into slot 0 of a ring
    ws0 = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    _capi.pool_tile_index(c['interval_rank'], c['interval_starts'], c['counts'], c['n_max'], B, Z, Y, X, ws0, tv)
    vol = torch.full((B, C, Z, Y, X), float('nan'), device=dev)
    add_planes = c['addend_rows'].transpose(1, 2).reshape(B, C, Y, X).contiguous() if with_addend else None
    _capi.bev_pool_v2_dense_fwd(*idx, B, C, Z, Y, X, vol, ws0, tv, flags, addend=add_planes)
    ring0 = torch.full((B, T + 1, N, C), PATTERN[dtype], dtype=dtype, device=dev)
    _capi.history_frame_vm(vol.view(B, C, N), ring0[:, 0])
    # the new entry, straight into slot 0 of a second ring (batch stride (T + 1) * N * C)
    ws1 = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    _capi.pool_tile_index(c['interval_rank'], c['interval_starts'], c['counts'], c['n_max'], B, Z, Y, X, ws1, tv,
                          flags=_capi.POOL_CHANNELS_LAST)
    ring1 = torch.full((B, T + 1, N, C), PATTERN[dtype], dtype=dtype, device=dev)
    rows_flags = flags if tv == 128 else (flags & ~_capi.POOL_CPL8)      # both lane-group shapes of the fp32 rows
    ret = _capi.bev_pool_v2_dense_fwd_rows(*idx, B, C, Z, Y, X, ring1[:, 0], ws1, tv, rows_flags, addend_rows=add_rows)
    torch.cuda.synchronize()
    assert ret.data_ptr() == ring1.data_ptr() and ring1[:, 0].stride(0) == (T + 1) * N * C
    assert torch.equal(K.words(ring1), K.words(ring0))                   # slot 0 word for word; slots 1..T as they were
    assert (ring1[:, 1:] == PATTERN[dtype]).all()
    assert (wide[..., C:] == 777.0).all() and torch.equal(wide[..., :C], c['addend_rows'])
    # the CPU oracle's pooled volume (+ addend), cast by torch: the equality test_gpu_parity.py holds the planar kernel to
    assert torch.equal(K.words(ring1[:, 0]).cpu(), K.words(K.expected_rows(host, C, dtype, with_addend)))


# ------------------------------------------------------------------------------------------------ (b), (c) modules
def _modules(dev, history_dtype, fp_extra=None, ring_layout='voxel_major'):
    from fb_bev_amd import configs, synthetic as S
    from fb_bev_amd.fb_view_transform import FBViewTransform
    from fb_bev_amd.history_fusion import TemporalHistoryFusion
    pc = S.CONFIGS['REF']
    X, Y, Z = pc.grid_xyz
    gcb = {'x': pc.grid_config['x'], 'y': pc.grid_config['y'], 'z': [-1, 5.4, 1.6]}
    cfg = configs.fbocc_r50(bev_h=Y, bev_w=X, numC_Trans=pc.channels, input_size=pc.input_size, grid_config=pc.grid_config,
                            grid_config_bevformer=gcb, depth_bound=tuple(pc.grid_config['depth']), downsample=pc.downsample)
    fp = dict(cfg['forward_projection'], **(fp_extra or {}))
    torch.manual_seed(0)
    m = FBViewTransform(fp, cfg['backward_projection'])
    with torch.no_grad():
        for n_, p_ in m.named_parameters():
            if 'sampling_offsets.weight' in n_ or 'attention_weights.weight' in n_:
                p_.normal_(0, 0.05)
    dx = [pc.grid_config[a][2] for a in 'xyz']
    bx = [pc.grid_config[a][0] + pc.grid_config[a][2] / 2 for a in 'xyz']
    hist = TemporalHistoryFusion(dx, bx, single_bev_num_channels=pc.channels, history_cat_num=2, history_dtype=history_dtype,
                                 ring_layout=ring_layout)
    return pc, m.to(dev).eval(), hist.to(dev).eval()


@pytest.fixture(scope='module')
def frames(dev):
    """three frames of B = 2 (shared, never modified): camera rig, context, depth, metas -- a sequence start at frame 0, sample 1
    restarts at frame 2, ego motion in between"""
    from fb_bev_amd import synthetic as S
    pc = S.CONFIGS['REF']
    ego = torch.eye(4); ego[0, 3] = 1.5; ego[1, 3] = -0.7
    out = []
    for i in range(3):
        cam = [t.to(dev) for t in S.camera_rig(pc, 2, seed=i, bda_aug=True)]
        depth, ctx = (t.to(dev) for t in S.depth_and_context(pc, 2, seed=i))
        metas = [dict(sequence_group_idx=b, start_of_sequence=(i == 0 or (i == 2 and b == 1)), curr_to_prev_ego_rt=ego) for b in range(2)]
        out.append((cam, ctx, depth, metas))
    return out


def _run(m, hist, frames, direct, dev, between=None):
    """-> per frame (output, history_bev, history_sweep_time, went through the slot)"""
    res = []
    with torch.no_grad():
        for cam, ctx, depth, metas in frames:
            slot = m.history_slot(hist, ctx.shape[0], dev) if direct else None
            bev = m(cam, ctx, depth, out_slot=slot)
            in_slot = slot is not None and bev is slot
            if between is not None:
                between(hist)
            out = hist.fuse_history(bev, metas, cam[5], in_slot=in_slot)
            res.append((out.clone(), hist.history_bev.clone(), hist.history_sweep_time.clone(), in_slot))
    torch.cuda.synchronize()
    return res


class _Calls:
    """counts the calls of the two _capi functions the routes differ in"""

    def __init__(self, monkeypatch):
        from fb_bev_amd import _capi
        self.n = {'rows': 0, 'frame': 0}
        rows, frame = _capi.bev_pool_v2_dense_fwd_rows, _capi.history_frame_vm

        def w_rows(*a, **k):
            self.n['rows'] += 1
            return rows(*a, **k)

        def w_frame(*a, **k):
            self.n['frame'] += 1
            return frame(*a, **k)
        monkeypatch.setattr(_capi, 'bev_pool_v2_dense_fwd_rows', w_rows)
        monkeypatch.setattr(_capi, 'history_frame_vm', w_frame)

    def take(self):
        n, self.n = self.n, {'rows': 0, 'frame': 0}
        return n


def _same(a, b):
    for (o0, h0, s0, _), (o1, h1, s1, _) in zip(a, b):
        assert o0.shape == o1.shape and torch.equal(o0, o1)
        assert h0.dtype == h1.dtype and h0.shape == h1.shape and torch.equal(K.words(h0), K.words(h1))
        assert torch.equal(s0, s1)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_direct_slot_route_equals_todays_route(dev, frames, monkeypatch, dtype):
    calls = _Calls(monkeypatch)
    pc, m0, h0 = _modules(dev, dtype)
    ref = _run(m0, h0, frames, False, dev)
    assert calls.take() == {'rows': 0, 'frame': 3} and not any(r[3] for r in ref)
    pc, m1, h1 = _modules(dev, dtype)
    got = _run(m1, h1, frames, True, dev)
    assert calls.take() == {'rows': 3, 'frame': 0} and all(r[3] for r in got)
    X, Y, Z = pc.grid_xyz
    assert got[0][0].shape == (2, pc.channels, Y, X, Z) and got[0][1].shape == (2, 2, Z * Y * X, pc.channels) and got[0][1].dtype == dtype
    _same(ref, got)
    assert torch.equal(got[2][2], torch.tensor([[0., 1.], [0., 0.]]))    # sample 1 restarted at frame 2


def test_direct_slot_through_the_detector_switch(dev, monkeypatch):
    """FBOCC(execution=dict(history_direct_slot=True)) wires begin_frame -> forward(out_slot) -> fuse_history(in_slot)"""
    from test_gpu_full_model import _inputs, _small_model
    calls = _Calls(monkeypatch)
    ex = dict(history_dtype='f16', history_ring='voxel_major')
    base = _small_model(dev, dict(ex, history_direct_slot=False)).eval()
    m = _small_model(dev, dict(ex, history_direct_slot=True)).eval()
    m.load_state_dict(base.state_dict())
    img_inputs, metas, _, _ = _inputs(dev, 2)
    def feats(model, first):
        r = model.extract_feat(None, img_inputs, metas(first))
        f = r['img_bev_feat_ndhwc'] if 'img_bev_feat_ndhwc' in r else r['img_bev_feat']
        return list(f) if isinstance(f, (list, tuple)) else [f]
    assert m.history_direct_slot and not base.history_direct_slot
    with torch.no_grad():
        for i in range(2):
            a = feats(base, i == 0)
            assert calls.take() == {'rows': 0, 'frame': 1}
            b = feats(m, i == 0)
            assert calls.take() == {'rows': 1, 'frame': 0}
            assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
            assert torch.equal(K.words(base.history.history_bev), K.words(m.history.history_bev))


@pytest.mark.parametrize('case', ['training', 'planar', 'extra_relu', 'volume_dtype'])
def test_fallbacks_hand_over_the_volume_as_before(dev, frames, monkeypatch, case):
    calls = _Calls(monkeypatch)
    kw = {'planar': dict(ring_layout='planar'), 'extra_relu': dict(fp_extra=dict(extra_relu=True)),
          'volume_dtype': dict(fp_extra=dict(out_dtype=torch.bfloat16))}.get(case, {})
    two = frames[:2]
    runs = []
    for direct in (False, True):
        pc, m, h = _modules(dev, torch.float16, **kw)
        if case == 'training':
            h.train()
        X, Y, Z = pc.grid_xyz
        with torch.no_grad():
            assert m.history_slot(h, 2, dev) is None
            if case in ('training', 'planar'):
                assert h.begin_frame(2, (Z, Y, X), dev) is None
            if case == 'volume_dtype':
                assert h.begin_frame(2, (Z, Y, X), dev, volume_dtype=torch.bfloat16) is None
        runs.append(_run(m, h, two, direct, dev))
        assert calls.take()['rows'] == 0 and not any(r[3] for r in runs[-1])
    _same(*runs)


def test_begin_frame_needs_eval_mode_without_gradients(dev):
    pc, m, h = _modules(dev, torch.float16)
    X, Y, Z = pc.grid_xyz
    assert h.begin_frame(2, (Z, Y, X), dev) is None                       # gradients enabled
    with torch.no_grad():
        slot = h.begin_frame(2, (Z, Y, X), dev)
        assert slot is not None and tuple(slot.shape) == (2, Z * Y * X, pc.channels) and slot.dtype == torch.float16
        assert slot.stride() == (3 * Z * Y * X * pc.channels, pc.channels, 1)
        assert h.begin_frame(2, (Z, Y, X), torch.device('cpu')) is None


def test_route_change_between_begin_frame_and_fuse_history_falls_back(dev, frames, monkeypatch):
    """the ring's storage type changes after the slot was written: fuse_history does not guess -- it rebuilds the volume the rows stand
    for and takes today's path (the transposing copy runs), result = today's path fed with that volume"""
    calls = _Calls(monkeypatch)
    pc, m, h = _modules(dev, torch.float16)
    X, Y, Z = pc.grid_xyz
    cam, ctx, depth, metas = frames[0]
    with torch.no_grad():
        slot = m.history_slot(h, 2, dev)
        bev = m(cam, ctx, depth, out_slot=slot)
        assert bev is slot
        vol = slot.float().transpose(1, 2).reshape(2, pc.channels, Z, Y, X).permute(0, 1, 3, 4, 2).clone()
        h.history_dtype = torch.bfloat16
        out = h.fuse_history(bev, metas, cam[5], in_slot=True)
        assert calls.take() == {'rows': 1, 'frame': 1} and h.history_bev.dtype == torch.bfloat16
        pc, m2, h2 = _modules(dev, torch.bfloat16)
        exp = h2.fuse_history(vol, metas, cam[5])
        assert torch.equal(out, exp) and torch.equal(K.words(h.history_bev), K.words(h2.history_bev))
        with pytest.raises(ValueError):
            h.fuse_history(slot, metas, cam[5], in_slot=True)             # no begin_frame before it
