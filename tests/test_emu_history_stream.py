"""CPU emulator: the two device pieces of the history fusion's device-resident sequence state (stream mode), driven through the
C ABI of the emulated library -- the SAME capi.hip and kernel headers as the product.

  fbbev_history_stream_prologue : everything fuse_history computes between reading img_metas and the warp (fbocc.py:220-261,
                                  279-281, 313-314), against the host recurrence of history_fusion.py, fbbev_history_flow and torch.
  fbbev_history_warp_vm_src     : fbbev_history_warp_vm with a per-sample source select, against today's sequence -- fill the started
                                  sample's T frames with the current rows, then fbbev_history_warp_vm.
Every comparison is bit equality."""
import ctypes
import math
import os
import sys
from ctypes import c_void_p

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import emu_capi as E  # noqa: E402

DX, LOWER, FREQ = (0.8, 0.8, 0.8), (-40.0, -40.0, -1.0), 0.5
ET = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _f3(v):
    return ctypes.cast((ctypes.c_float * 3)(*v), c_void_p)


def _rigid(g, B):
    """(B,4,4) ego motions: a yaw, a small pitch and a translation."""
    m = torch.eye(4).repeat(B, 1, 1)
    for b in range(B):
        a, p = (torch.rand(2, generator=g) - 0.5).tolist()
        rz = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        ry = torch.tensor([[math.cos(0.1 * p), 0.0, math.sin(0.1 * p)], [0.0, 1.0, 0.0], [-math.sin(0.1 * p), 0.0, math.cos(0.1 * p)]])
        m[b, :3, :3] = rz @ ry
        m[b, :3, 3] = (torch.rand(3, generator=g) - 0.5) * torch.tensor([4.0, 4.0, 0.5])
    return m.contiguous()


def _bda(g, B, flip=None):
    """(B,3,3) BEV augmentations: rotation about z times a scale; sample `flip` has its y axis flipped."""
    m = torch.zeros(B, 3, 3)
    for b in range(B):
        a = float(torch.rand(1, generator=g) - 0.5)
        s = 1.0 + 0.1 * float(torch.rand(1, generator=g) - 0.5)
        m[b] = s * torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        if b == flip:
            m[b, 1] = -m[b, 1]
    return m.contiguous()


def _fwd(bda):
    m = torch.zeros(bda.shape[0], 4, 4)
    m[:, :3, :3] = bda
    m[:, 3, 3] = 1.0
    return m


def _prologue(flags, ego, bda, b1, wt, augs, sweep, T, C):
    B = flags.numel()
    used, flow = torch.full((B, 4, 4), float('nan')), torch.full((B, 4, 4), float('nan'))
    bias1 = torch.full((B * (T + 1), C), float('nan'))
    E.ok(E.lib().fbbev_history_stream_prologue(E.p(flags), E.p(ego), E.p(bda), E.p(b1), E.p(wt), _f3(DX), _f3(LOWER), FREQ, B, T, C,
                                               E.p(augs), E.p(sweep), E.p(used), E.p(flow), E.p(bias1), None))
    return flow, bias1, used


def test_stream_prologue_follows_the_host_recurrence():
    g = torch.Generator().manual_seed(5)
    B, T, C = 3, 3, 16
    b1, wt = torch.randn(C, generator=g), torch.randn(C, generator=g)
    # the state a running stream holds: the forward augmentations of the frame before, sweep times of a few frames
    augs_h = _fwd(_bda(g, B))
    sweep_h = torch.tensor([[0.0, 1.0, 2.0], [0.0, 1.0, 1.0], [0.0, 3.0, 4.0]])
    augs_d, sweep_d = augs_h.clone(), sweep_h.clone()
    for i, fl in enumerate(([1, 0, 0], [0, 0, 0], [0, 1, 0], [3, 3, 3])):
        flags = torch.tensor(fl, dtype=torch.int32)
        ego, bda = _rigid(g, B), _bda(g, B, flip=i % B)
        fwd = _fwd(bda)
        # history_fusion.py's host logic (fbocc.py:227-261), in its order
        empty, start = (flags & 2) != 0, (flags & 1) != 0
        augs_h[empty], sweep_h[empty] = fwd[empty], 0.0
        sweep_h = sweep_h + 1
        sweep_h[start], augs_h[start] = 0.0, fwd[start]
        augs_used = augs_h.clone()
        flow_exp = E.history_flow(augs_used, ego, bda, DX, LOWER)
        sw = torch.cat([torch.zeros(B, 1), sweep_h], dim=1)                        # :279-281
        bias_exp = b1[None, :] + (sw * FREQ).reshape(B * (T + 1), 1) * wt[None, :]
        sweep_h, augs_h = sw[:, :-1].contiguous(), fwd.clone()                     # :313-314
        flow, bias1, used = _prologue(flags, ego, bda, b1, wt, augs_d, sweep_d, T, C)
        assert torch.equal(used, augs_used) and torch.equal(flow, flow_exp), i
        assert torch.equal(bias1, bias_exp), i
        assert torch.equal(sweep_d, sweep_h) and torch.equal(augs_d, augs_h), i
    assert torch.equal(sweep_d, torch.zeros(B, T))                                 # the last frame started every sample


def test_stream_prologue_first_frame_without_a_start_ends_with_sweep_one():
    """Bit 1 alone (an empty history, start_of_sequence clear): the old state -- NaN here -- is not read, the sweep times end at 1
    like the reference's (zeros at :238, + 1 at :252), the augmentations at fwd."""
    g = torch.Generator().manual_seed(6)
    B, T, C = 3, 3, 16
    b1, wt = torch.randn(C, generator=g), torch.randn(C, generator=g)
    augs, sweep = torch.full((B, 4, 4), float('nan')), torch.full((B, T), float('nan'))
    ego, bda = _rigid(g, B), _bda(g, B, flip=1)
    flow, bias1, _ = _prologue(torch.full((B,), 2, dtype=torch.int32), ego, bda, b1, wt, augs, sweep, T, C)
    assert torch.equal(sweep, torch.tensor([[0.0, 1.0, 1.0]]).repeat(B, 1))
    assert torch.equal(augs, _fwd(bda))
    assert torch.equal(flow, E.history_flow(_fwd(bda), ego, bda, DX, LOWER))
    tau = torch.tensor([0.0, 1.0, 1.0, 1.0]).repeat(B) * FREQ
    assert torch.equal(bias1, b1[None, :] + tau[:, None] * wt[None, :])


@pytest.mark.parametrize('dt,T,C,grid', [(torch.float32, 3, 16, (4, 10, 12)),       # an odd frame tail
                                         (torch.float16, 16, 80, (2, 6, 30)),       # ten 16-byte groups per voxel, a ragged last x chunk, the four-frame unroll
                                         (torch.bfloat16, 3, 80, (4, 10, 12))])     # bf16 storage
def test_warp_vm_src_equals_ring_fill_then_warp(dt, T, C, grid):
    g = torch.Generator().manual_seed(7)
    B, (Z, Y, X) = 2, grid
    N = Z * Y * X
    bits = torch.int32 if dt == torch.float32 else torch.int16
    flow = torch.eye(4).repeat(B, 1, 1)
    flow[0, :3, 3] = torch.tensor([1.25, -0.5, 0.25])
    flow[1, :3, :3] = torch.tensor([[0.9, -0.4, 0.0], [0.4, 0.9, 0.0], [0.0, 0.0, 1.0]])
    flow[1, :3, 3] = torch.tensor([-0.75, 1.5, 0.0])
    flow = flow.contiguous()
    old = (torch.randn(B, T, N, C, generator=g) * 2).to(dt)
    curr = torch.randn(B, C, N, generator=g)
    # today's sequence: slot 0 = the current frame, the started sample's T frames filled with its rows, then the warp
    ref = torch.full((B, T + 2, N, C), float('nan'), dtype=dt)                      # slot T + 1: padding between the samples
    E.history_frame_vm(curr, dt, out=ref[:, 0])
    filled = old.clone()
    filled[1] = ref[1, 0].unsqueeze(0).expand(T, N, C)
    E.history_warp_vm(filled, flow, (Z, Y, X), out=ref[:, 1:T + 1])
    # the source select: the started sample's old ring is never read
    got = torch.full((B, T + 2, N, C), float('nan'), dtype=dt)
    E.history_frame_vm(curr, dt, out=got[:, 0])
    poisoned = old.clone()
    poisoned[1] = float('nan')
    flags = torch.tensor([0, 1], dtype=torch.int32)
    dst = got[:, 1:T + 1]
    E.ok(E.lib().fbbev_history_warp_vm_src(E.p(poisoned), poisoned.stride(0), c_void_p(got.data_ptr()), got.stride(0), E.p(flags),
                                           E.p(flow), B, T, C, Z, Y, X, c_void_p(dst.data_ptr()), dst.stride(0), ET[dt], None))
    assert torch.equal(got.view(bits), ref.view(bits))                              # output bytes AND the NaN padding around them
    assert torch.isnan(got[:, T + 1].float()).all()
    assert torch.isfinite(got[:, :T + 1].float()).all()                             # nothing of the poisoned ring got in
    # flags = 0 everywhere: fbbev_history_warp_vm itself
    none = torch.zeros(B, dtype=torch.int32)
    E.ok(E.lib().fbbev_history_warp_vm_src(E.p(old), old.stride(0), c_void_p(got.data_ptr()), got.stride(0),
                                           E.p(none), E.p(flow), B, T, C, Z, Y, X,
                                           c_void_p(dst.data_ptr()), dst.stride(0), ET[dt], None))
    assert torch.equal(dst.contiguous().view(bits), E.history_warp_vm(old, flow, (Z, Y, X)).view(bits))


def test_argument_errors_of_both_entries():
    """-1 invalid argument, -2 unsupported layout, 0 for an empty batch: rejected before any launch, so dummy pointers do."""
    lib = E.lib()
    NULL, P16, P8 = c_void_p(0), c_void_p(0x1000), c_void_p(0x1008)
    dx, lo, bad_dx = _f3(DX), _f3(LOWER), _f3((0.8, 0.0, 0.8))
    pro = lib.fbbev_history_stream_prologue
    assert pro(NULL, P16, P16, P16, P16, dx, lo, 0.5, 2, 16, 80, P16, P16, P16, P16, P16, None) == -1     # null flags
    assert pro(P16, P16, P16, P16, P16, dx, lo, 0.5, 2, 16, 80, NULL, P16, P16, P16, P16, None) == -1     # null state
    assert pro(P16, P16, P16, P16, P16, dx, lo, 0.5, 2, 16, 80, P16, P16, P16, P16, NULL, None) == -1     # null bias1
    assert pro(P16, P16, P16, P16, P16, NULL, lo, 0.5, 2, 16, 80, P16, P16, P16, P16, P16, None) == -1    # null dx3
    assert pro(P16, P16, P16, P16, P16, bad_dx, lo, 0.5, 2, 16, 80, P16, P16, P16, P16, P16, None) == -1  # voxel size 0
    assert pro(P16, P16, P16, P16, P16, dx, lo, 0.5, -1, 16, 80, P16, P16, P16, P16, P16, None) == -1     # B < 0
    assert pro(P16, P16, P16, P16, P16, dx, lo, 0.5, 2, 16, 0, P16, P16, P16, P16, P16, None) == -1       # C <= 0
    assert pro(NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0.5, 0, 16, 80, NULL, NULL, NULL, NULL, NULL, None) == 0   # empty batch: no-op
    src = lib.fbbev_history_warp_vm_src
    assert src(P16, 0, P16, 0, P16, P16, 1, 16, 80, 8, 8, 8, P16, 0, 3, None) == -1                  # elem_type
    assert src(P16, 0, P16, 0, P16, P16, 1, 16, 84, 8, 8, 8, P16, 0, 2, None) == -2                  # C % 8 (16-bit row pieces)
    assert src(P16, 0, P16, 0, P16, P16, 1, 16, 80, 8, 8, 8, P8, 0, 2, None) == -2                   # out not 16-byte aligned
    assert src(P16, 0, P8, 0, P16, P16, 1, 16, 80, 8, 8, 8, P16, 0, 2, None) == -2                   # curr not 16-byte aligned
    assert src(P16, 100, P16, 0, P16, P16, 1, 16, 80, 8, 8, 8, P16, 0, 2, None) == -1                # batch stride < T*N*C
    assert src(P16, 0, P16, 100, P16, P16, 1, 16, 80, 8, 8, 8, P16, 0, 2, None) == -1                # curr stride < N*C
    assert src(P16, 0, P16, 8 * 8 * 8 * 80 + 4, P16, P16, 1, 16, 80, 8, 8, 8, P16, 0, 2, None) == -2  # curr stride % 8
    assert src(P16, 0, NULL, 0, P16, P16, 1, 16, 80, 8, 8, 8, P16, 0, 2, None) == -1                 # null curr
    assert src(P16, 0, P16, 0, NULL, P16, 1, 16, 80, 8, 8, 8, P16, 0, 2, None) == -1                 # null flags
    assert src(NULL, 0, P16, 0, P16, P16, 1, 16, 80, 8, 8, 8, P16, 0, 2, None) == -1                 # null history
    assert src(P16, 0, P16, 0, P16, P16, 1, 16, 80, 1, 8, 8, P16, 0, 2, None) == -1                  # Z < 2
    assert src(P16, 0, P16, 0, P16, P16, 1, 0, 80, 8, 8, 8, P16, 0, 2, None) == 0                    # no frames: no-op
    assert src(NULL, 0, NULL, 0, NULL, NULL, 0, 16, 80, 8, 8, 8, NULL, 0, 2, None) == 0              # empty batch: no-op


def test_workgroup_limit_of_the_one_kernel_step_behind_its_weight_launch():
    """fbbev_history_fused_vm counts its workgroups after it has laid the weight fragments out: 2^29 samples of a 2 x 2 x 2 grid
    are 2^31 workgroups, -2, with the fragments written and neither ring touched (dummy pointers do for them)."""
    lib = E.lib()
    P16 = c_void_p(0x1000)
    T, C = 1, 80
    w1, w2 = torch.randn(C, C), torch.randn(C, (T + 1) * C)
    need = (1 + T + 1) * 5 * 3 * 64 * 8 * 2                                                     # W1 and T + 1 W2 as bf16 fragments
    ws = torch.zeros(need // 2 + 8, dtype=torch.int16)
    args = lambda B, nbytes: (P16, 0, P16, 0, P16, c_void_p(w1.data_ptr()), P16, c_void_p(w2.data_ptr()), P16, B, T, C, C,   # noqa: E731
                              2, 2, 2, P16, c_void_p(ws.data_ptr()), nbytes, 2, None)
    assert lib.fbbev_history_fused_vm(*args(1 << 29, need - 1)) == -3 and not ws.any()          # the workspace comes first
    assert lib.fbbev_history_fused_vm(*args(1 << 29, need)) == -2
    assert ws[:need // 2].any() and not ws[need // 2:].any()


@pytest.mark.parametrize('dt', [torch.float32, torch.float16])
def test_module_stream_state_on_emulated_kernels_equals_the_default_route(monkeypatch, dt):
    """fb_bev_amd.history_fusion's host code for stream_state=True driving the emulated kernels, against the same module on the
    default route: output, ring, sweep times, forward augmentations and sequence ids after every frame of a stream with restarts,
    a detour through the default route (frames 3-4: the mirrors carry the state both ways) and a reset (frame 6 starts nothing:
    sweep 1).  Pinned memory and the copy events are stood in for: there is no device here."""
    from fb_bev_amd import _capi
    from fb_bev_amd.history_fusion import TemporalHistoryFusion
    import numpy as np

    def conv_stub(feats, w1, bias1, w2, bias2, out, compute=torch.float32, voxel_major=False):
        out.copy_(E.history_conv(feats, w1.contiguous(), bias1.contiguous(), w2.contiguous(), bias2.contiguous(),
                                 voxel_major=voxel_major, x3=compute == 'bf16x3'))
        return out

    def prologue_stub(flags, ego, bda, b1, wt, dx3, lower3, freq, augs, sweep, used, flow, bias1):
        B, T = sweep.shape
        E.ok(E.lib().fbbev_history_stream_prologue(E.p(flags), E.p(ego), E.p(bda), E.p(b1), E.p(wt), _f3(dx3), _f3(lower3), float(freq),
                                                   B, T, b1.shape[0], E.p(augs), E.p(sweep), E.p(used), E.p(flow), E.p(bias1), None))
        return flow, bias1

    def warp_src_stub(history, curr, flags, flow, out, grid_zyx):
        B, T, N, C = history.shape
        E.ok(E.lib().fbbev_history_warp_vm_src(c_void_p(history.data_ptr()), history.stride(0), c_void_p(curr.data_ptr()),
                                               curr.stride(0), E.p(flags), E.p(flow), B, T, C, *grid_zyx, c_void_p(out.data_ptr()),
                                               out.stride(0), ET[history.dtype], None))
        return out

    class Event:
        def query(self): return True
        def synchronize(self): pass
        def record(self): pass
    for name, fn in (('history_flow', lambda a, e, b, d, lo: E.history_flow(a.contiguous(), e, b, d, lo)),
                     ('history_warp_vm', lambda h, f, o, g: E.history_warp_vm(h, f, g, out=o)),
                     ('history_frame_vm', lambda c, o, inner=1: E.history_frame_vm(c, o.dtype, out=o, inner=inner)),
                     ('history_conv', conv_stub), ('history_stream_prologue', prologue_stub), ('history_warp_vm_src', warp_src_stub),
                     ('require_gpu', lambda t, n: None)):
        monkeypatch.setattr(_capi, name, fn)
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    monkeypatch.setattr(torch.cuda, 'Event', Event)
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'history_fusion_seq4.npz'))
    T, C, (Z, Y, X) = 3, 16, (4, 10, 12)
    torch.manual_seed(0)
    eager, stream = (TemporalHistoryFusion([0.8] * 3, [-X * 0.4 + 0.4, -Y * 0.4 + 0.4, -Z * 0.4 + 0.4], single_bev_num_channels=C,
                                           history_cat_num=T, history_dtype=dt).eval() for _ in range(2))
    with torch.no_grad():
        for seq in (eager.history_keyframe_time_conv, eager.history_keyframe_cat_conv):
            seq[1].running_mean.normal_(0, 0.1)
            seq[1].running_var.uniform_(0.5, 1.5)
    stream.load_state_dict(eager.state_dict())
    assert stream._voxel_major()
    starts = [[True, False], [False, False], [False, True], [False, False], [False, False], [True, True], [False, False], [False, False]]
    sid, g = [0, 1], torch.Generator().manual_seed(1)
    for i, st in enumerate(starts):
        stream.stream_state = i not in (3, 4)
        if i == 6:
            eager.reset()
            stream.reset()
        sid = [s + 10 if st[b] else s for b, s in enumerate(sid)]
        metas = [dict(sequence_group_idx=sid[b], start_of_sequence=st[b], curr_to_prev_ego_rt=z[f'f{i % 4}.ego'][b]) for b in range(2)]
        curr, bda = torch.randn(2, C, Y, X, Z, generator=g), torch.from_numpy(z[f'f{i % 4}.bda'])
        with torch.no_grad():
            exp, out = eager.fuse_history(curr, metas, bda), stream.fuse_history(curr, metas, bda)
        assert torch.equal(out, exp), i
        assert torch.equal(stream.history_as_reference(), eager.history_as_reference()), i
        assert torch.equal(stream.history_sweep_time, eager.history_sweep_time), i
        assert torch.equal(stream.history_forward_augs, eager.history_forward_augs), i
        assert torch.equal(stream.history_seq_ids, eager.history_seq_ids), i
        assert stream._st_ok == stream.stream_state and eager._st is None, i
    assert torch.equal(stream.history_sweep_time, torch.tensor([[0.0, 1.0, 2.0]]).repeat(2, 1))
    stream.pipelined_step = True
    with pytest.raises(ValueError, match='stream_state'):
        stream.fuse_history(curr, metas, bda)
