"""Deterministic mode (include/fbbev.h FBBEV_FLAG_DETERMINISTIC) on the CPU device emulator: the fixed-point depth taps of the DA
backward (csrc/det_kernels.h) against a host restatement of the same integer arithmetic summed in a shuffled order, the
flags-word entries of the two LDS-plane DA backward routes against their plain entries, and the Python switch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'emu'))
sys.path.insert(0, os.path.dirname(__file__))
import emu_capi as E  # noqa: E402
from da_cases import da_case  # noqa: E402
from fb_bev_amd import _capi  # noqa: E402

FLAG_DET = _capi.FLAG_DETERMINISTIC


def test_switch_follows_torch_flags_and_override():
    import fb_bev_amd as F
    saved = (torch.are_deterministic_algorithms_enabled(), torch.backends.cudnn.deterministic, F._deterministic_override)
    try:
        F.set_deterministic(None)
        torch.use_deterministic_algorithms(False)
        torch.backends.cudnn.deterministic = False
        assert F.deterministic_enabled() is False
        torch.use_deterministic_algorithms(True)
        assert F.deterministic_enabled() is True
        torch.use_deterministic_algorithms(False)
        torch.backends.cudnn.deterministic = True                    # the reference's tools/train.py --deterministic
        assert F.deterministic_enabled() is True
        F.set_deterministic(False)
        assert F.deterministic_enabled() is False
        torch.backends.cudnn.deterministic = False
        F.set_deterministic(True)
        assert F.deterministic_enabled() is True
        assert not torch.are_deterministic_algorithms_enabled() and not torch.backends.cudnn.deterministic   # torch left alone
        F.set_deterministic(None)
        assert F.deterministic_enabled() is False
        with pytest.raises(TypeError):
            F.set_deterministic(1)
    finally:
        torch.use_deterministic_algorithms(saved[0])
        torch.backends.cudnn.deterministic = saved[1]
        F._deterministic_override = saved[2]
    assert (torch.are_deterministic_algorithms_enabled(), torch.backends.cudnn.deterministic, F._deterministic_override) == saved


def _corners(x, y, H, W):
    """fbbev_daf_plane_corners in float32 numpy (the same operation order)"""
    f = np.float32
    h_im, w_im = f(y) * f(H) - f(0.5), f(x) * f(W) - f(0.5)
    live = h_im > -1 and w_im > -1 and h_im < H and w_im < W
    h, w = (h_im, w_im) if live else (f(0), f(0))
    h_low, w_low = int(np.floor(h)), int(np.floor(w))
    lh, lw = f(h - f(h_low)), f(w - f(w_low))
    hh, hw = f(f(1) - lh), f(f(1) - lw)
    left, right, top, bottom = w_low < 0, w_low >= W - 1, h_low < 0, h_low >= H - 1
    xa, xb = (0 if left else w_low), (w_low if right else w_low + 1)
    ya, yb = (0 if top else h_low), (h_low if bottom else h_low + 1)
    s = f(1) if live else f(0)
    off = [ya * W + xa, ya * W + xb, yb * W + xa, yb * W + xb]
    wgt = [f(0) if (top or left) else f(f(s * hh) * hw), f(0) if (top or right) else f(f(s * hh) * lw),
           f(0) if (bottom or left) else f(f(s * lh) * hw), f(0) if (bottom or right) else f(f(s * lh) * lw)]
    return off, wgt


def _taps_restated(dsum, ref_cam, qdepth, B, Ncam, Q, Za, DC, H0, W0, d0, dstep, order):
    """the fixed-point sum of det_kernels.h restated on the host, contributions added in `order`; also the fp64 sum of the same
    fp32 contributions and their fp32 sum in that order (what the float-atomic form computes for that arrival order)"""
    f = np.float32
    n_out = B * Ncam * DC * H0 * W0
    gmax = np.abs(dsum).max()
    kq = int(np.ceil(np.log2(Q * Za)))
    ex = int(np.frombuffer(np.float32(gmax).tobytes(), dtype=np.uint32)[0] >> 23)
    s = 61 - (ex - 126 if ex else -126) - kq
    acc = np.zeros(n_out, dtype=np.int64)
    ref64, atom = np.zeros(n_out), np.zeros(n_out, dtype=np.float32)
    contrib = []
    for i in range(dsum.size):
        d = dsum.flat[i]
        if d == 0:
            continue
        cam, rem = divmod(i, B * Q * Za)
        b = rem // (Q * Za)
        fb = np.floor(f(f(qdepth.flat[i] - f(d0)) / f(dstep)))
        fb = int(min(max(fb, 0), DC - 1))
        off, wgt = _corners(ref_cam.flat[2 * i], ref_cam.flat[2 * i + 1], H0, W0)
        base = ((b * Ncam + cam) * DC + fb) * H0 * W0
        for k in range(4):
            if wgt[k] != 0:
                contrib.append((base + off[k], f(wgt[k] * f(d))))
    for j in order(len(contrib)):
        o, v = contrib[j]
        acc[o] += int(np.rint(np.float64(v) * 2.0 ** s))
        ref64[o] += np.float64(v)
        atom[o] = f(atom[o] + v)
    out = (acc.astype(np.float64) * 2.0 ** -s).astype(np.float32)
    return out, ref64, atom


@pytest.mark.parametrize('seed,B,Ncam,Q,Za,DC,H0,W0', [(0, 1, 2, 40, 4, 5, 4, 6), (1, 2, 3, 64, 4, 7, 5, 3), (2, 1, 1, 9, 2, 3, 1, 2)])
def test_depth_taps_fixed_point_equals_host_restatement(seed, B, Ncam, Q, Za, DC, H0, W0):
    g = torch.Generator().manual_seed(seed)
    dsum = torch.randn(Ncam, B, Q, Za, generator=g) * torch.logspace(-6, 2, Q * Za).view(Q, Za)[None, None]
    dsum[torch.rand(dsum.shape, generator=g) < 0.3] = 0.0
    ref_cam = torch.rand(Ncam, B, Q, Za, 2, generator=g) * 1.3 - 0.15
    qdepth = torch.rand(Ncam, B, Q, Za, generator=g) * (DC + 4.0)
    d0, dstep = 2.0, 1.0
    init = torch.randn(B, Ncam, DC, H0, W0, generator=g)            # accumulated into
    gd = init.clone()
    need = E.lib().fbbev_da_depth_taps_det_ws_bytes(B, Ncam, DC, H0, W0)
    ws = torch.full((need // 4,), float('nan'))                      # garbage: the entry clears its own state
    E.ok(E.lib().fbbev_da_depth_taps_det(E.p(dsum), E.p(ref_cam), E.p(qdepth), B, Ncam, Q, Za, DC, H0, W0, d0, dstep, E.p(gd),
                                         E.p(ws), need, None))
    args = (dsum.numpy(), ref_cam.numpy(), qdepth.numpy(), B, Ncam, Q, Za, DC, H0, W0, d0, dstep)
    rng = np.random.default_rng(seed)
    fwd, ref64, atom = _taps_restated(*args, order=lambda n: range(n))
    shuf, _, atom_shuf = _taps_restated(*args, order=lambda n: rng.permutation(n))
    assert np.array_equal(fwd, shuf)                                  # the integer sum does not depend on the order
    exp = (init.numpy().ravel() + fwd).reshape(gd.shape)
    assert torch.equal(gd, torch.from_numpy(exp))
    scale = np.abs(ref64).max()
    err_det, err_atom = np.abs(fwd - ref64).max() / scale, np.abs(atom - ref64).max() / scale
    print(f'depth taps: max|fixed point - fp64| = {err_det:.2e}, max|fp32 sum - fp64| = {err_atom:.2e} of the scale '
          f'(fp32 sums in two orders differ by {np.abs(atom - atom_shuf).max() / scale:.2e})')
    assert err_det <= max(err_atom, 2.0 ** -24)


def test_depth_taps_all_zero_and_non_finite():
    B, Ncam, Q, Za, DC, H0, W0 = 1, 1, 8, 4, 3, 2, 3
    ref_cam = torch.full((Ncam, B, Q, Za, 2), 0.5)
    qdepth = torch.full((Ncam, B, Q, Za), 3.0)
    need = E.lib().fbbev_da_depth_taps_det_ws_bytes(B, Ncam, DC, H0, W0)
    ws = torch.zeros(need // 4)
    for fill, check in ((0.0, lambda gd: torch.equal(gd, torch.ones_like(gd))), (float('inf'), lambda gd: torch.isnan(gd).all())):
        dsum = torch.zeros(Ncam, B, Q, Za)
        dsum[0, 0, 3, 1] = fill
        gd = torch.ones(B, Ncam, DC, H0, W0)
        E.ok(E.lib().fbbev_da_depth_taps_det(E.p(dsum), E.p(ref_cam), E.p(qdepth), B, Ncam, Q, Za, DC, H0, W0, 2.0, 1.0, E.p(gd),
                                             E.p(ws), need, None))
        assert check(gd), fill
    assert E.lib().fbbev_da_depth_taps_det(E.p(dsum), E.p(ref_cam), E.p(qdepth), B, Ncam, Q, Za, DC, H0, W0, 2.0, 1.0, E.p(gd),
                                           E.p(ws), need - 8, None) == -3


def _da_bwd_ex(value, ss, ls, pred, ref_cam, mask, qdepth, offsets, attn, d0, dstep, grad_slots, shapes, bev_w, flags, Dh, planes=None):
    """fbbev_da_cross_attn_bwd_ws_grid_ex (planes None) / fbbev_da_cross_attn_bwd_planes_ex on the emulator"""
    code, gv, gd, go, ga = E.da_cross_attn_bwd_entry('planes' if planes is not None else 'ws_grid', planes if planes is not None else value,
                                                     ss, ls, pred, ref_cam, mask, qdepth, offsets, attn, d0, dstep, grad_slots, Dh,
                                                     value.shape[-1], level_hw=shapes, bev_w=bev_w, flags=flags)
    E.ok(code)
    return gv, gd, go, ga


@pytest.mark.parametrize('route', ['ws_grid_unit', 'ws_grid_unit_planes', 'planes'])
def test_da_backward_deterministic_mode_against_plain_entry(route, monkeypatch):
    """the flags-word entries (both unit-gradient kernels: k_da_cross_attn_bwd_unit, k_da_bwd_unit_planes): without the flag the plain
    entry's bits; with it every gradient but the depth distribution's is unchanged (same kernels), the depth distribution's within
    fp32 re-association of the atomic form and the same bits from call to call"""
    monkeypatch.setenv('FBBEV_DA_BWD_OWNED', '1')
    monkeypatch.setenv('FBBEV_DA_BWD_UNIT_PLANES', '0' if route == 'ws_grid_unit' else '1')
    shapes = ((16, 44), (8, 22))
    args, _ = da_case(31, B=2, Q=5 * 11, shapes=shapes, E=80, M=8, P=8, DC=20)
    value, ss, ls, pred, ref_cam, mask, qdepth, offsets, attn, d0, dstep = args
    Dh = value.shape[-1]
    vp = torch.zeros(value.shape[:-1] + (12,)); vp[..., :Dh] = value
    g = torch.randn(mask.shape[1], mask.shape[2], 80, generator=torch.Generator().manual_seed(5))
    planes = value.permute(0, 2, 1, 3).contiguous() if route == 'planes' else None
    run = lambda flags: _da_bwd_ex(vp, ss, ls, pred, ref_cam, mask, qdepth, offsets, attn, d0, dstep, g, shapes, 11, flags, Dh, planes)  # noqa: E731
    off, on, on2 = run(0), run(FLAG_DET), run(FLAG_DET)
    for a, b in zip(on, on2):
        assert torch.equal(a, b)
    for name, a, b in zip(('value', 'offsets', 'attn'), (on[0], on[2], on[3]), (off[0], off[2], off[3])):
        assert torch.equal(a, b), name
    scale = off[1].abs().max().item()
    err = (on[1] - off[1]).abs().max().item()
    print(f'{route}: depth gradient max|det - atomic| = {err:.2e} on a scale of {scale:.3e}')
    assert scale > 0 and err <= 2e-6 * scale
    if planes is None:                                                # the plain entry on the same inputs: the same bits as flags 0
        ref = E.da_cross_attn_bwd(vp, ss, ls, pred, ref_cam, mask, qdepth, offsets, attn, d0, dstep, g, head_dim=Dh, lds_planes=True,
                                  level_hw=[tuple(x) for x in shapes], bev_w=11)
        for a, b in zip(off, ref):
            assert torch.equal(a, b)


def test_conv3d_wgrad_chunk_partials_equal_fixed_order_sum():
    """k_conv3d_wgrad_ndhwc<., true> + k_sum_chunks_add: the stored chunk partials added in chunk order, into what dw held"""
    from fb_bev_amd import mfma_conv3d  # noqa: F401  (the layouts below are the module's)
    g = torch.Generator().manual_seed(4)
    B, D, H, W, Cin, Cout, k = 1, 6, 9, 8, 8, 12, 3
    x = torch.randn(B, D, H, W, Cin, generator=g)
    dy = torch.randn(B, D, H, W, Cout, generator=g)
    plain = torch.zeros(k ** 3, Cout, Cin)
    E.ok(E.lib().fbbev_conv3d_wgrad_ndhwc(E.p(x), E.p(dy), B, D, H, W, Cin, D, H, W, Cout, k, 1, 1, E.p(plain), None))
    init = torch.randn(k ** 3, Cout, Cin, generator=g)
    det = init.clone()
    need = E.lib().fbbev_conv3d_wgrad_ws_bytes(B, D, H, W, Cin, Cout, k, FLAG_DET)
    ws = torch.full((need // 4,), float('nan'))
    E.ok(E.lib().fbbev_conv3d_wgrad_ndhwc_ex(E.p(x), E.p(dy), B, D, H, W, Cin, D, H, W, Cout, k, 1, 1, E.p(det), FLAG_DET, E.p(ws), need,
                                             None))
    n_chunks = need // (4 * k ** 3 * Cout * Cin)
    part = ws.view(n_chunks, k ** 3, Cout, Cin)
    s = torch.zeros_like(init)
    for c in range(n_chunks):                                         # the host restatement: chunk order
        s = s + part[c]
    assert torch.equal(det, init + s)
    assert torch.allclose(det - init, plain, atol=1e-4, rtol=1e-5)
    assert E.lib().fbbev_conv3d_wgrad_ndhwc_ex(E.p(x), E.p(dy), B, D, H, W, Cin, D, H, W, Cout, k, 1, 1, E.p(det), FLAG_DET, E.p(ws),
                                               need - 4, None) == -3


@pytest.mark.parametrize('Dh', [12, 10])
def test_msda_backward_fixed_point_scatter(Dh):
    """fbbev_msda_bwd_ex: the value gradient as fixed point ADDED to grad_value, the other two gradients as fbbev_msda_bwd; the
    value gradient within fp32 re-association of the atomic form and equal to the restated fixed-point sum"""
    g = torch.Generator().manual_seed(Dh)
    B, M, L, P, Q = 2, 2, 2, 3, 11
    shapes = torch.tensor([[5, 7], [3, 4]])
    ls = torch.tensor([0, 35])
    S = 47
    value = torch.randn(B, S, M, Dh, generator=g)
    loc = torch.rand(B, Q, M, L, P, 2, generator=g) * 1.2 - 0.1
    attn = torch.rand(B, Q, M, L, P, generator=g)
    go = torch.randn(B, Q, M * Dh, generator=g)
    outs = {}
    for flags in (0, FLAG_DET):
        gv = torch.ones(B, S, M, Dh)
        gl, ga = torch.zeros_like(loc), torch.zeros_like(attn)
        need = E.lib().fbbev_msda_bwd_det_ws_bytes(B, S, M, Dh)
        ws = torch.full((need // 4,), float('nan'))
        E.ok(E.lib().fbbev_msda_bwd_ex(E.p(value), E.p(shapes), E.p(ls), E.p(loc), E.p(attn), E.p(go), B, S, M, Dh, L, Q, P, E.p(gv),
                                       E.p(gl), E.p(ga), flags, E.p(ws), need, None))
        outs[flags] = (gv, gl, ga, ws)
    (gv0, gl0, ga0, _), (gv1, gl1, ga1, ws) = outs[0], outs[FLAG_DET]
    assert torch.equal(gl0, gl1) and torch.equal(ga0, ga1)
    hdr = ws[:64].view(torch.int32)
    s = int(hdr[3])
    acc = ws[64:64 + 2 * B * S * M * Dh].view(torch.int64).reshape(B, S, M, Dh)
    assert torch.equal(gv1, 1.0 + (acc.double() * 2.0 ** -s).float())
    scale = (gv0 - 1).abs().max().item()
    print(f'msda Dh={Dh}: max|fixed point - atomic| = {(gv1 - gv0).abs().max().item():.2e} on a scale of {scale:.3e}')
    assert (gv1 - gv0).abs().max().item() <= 2e-6 * scale


def test_da_backward_global_kernel_fixed_point():
    """fbbev_da_cross_attn_bwd_ex: the global kernel with fixed-point value words and the fixed-point depth taps, against the plain
    global-atomic entry (M = 6: a head count no LDS-plane route takes in the deterministic mode)"""
    shapes = ((6, 9), (3, 5))
    args, _ = da_case(12, B=1, N=3, Q=20, shapes=shapes, E=36, M=6, P=4, DC=6)
    value, ss, ls, pred, ref_cam, mask, qdepth, offsets, attn, d0, dstep = args
    Ncam, B, Q, Za = mask.shape
    _, S, M, Dh = value.shape
    L, P = attn.shape[3], attn.shape[4]
    DC = pred.shape[1]
    g = torch.randn(B, Q, M * Dh, generator=torch.Generator().manual_seed(2))
    m8 = mask.to(torch.uint8).contiguous()
    res = {}
    for flags in (0, FLAG_DET, FLAG_DET):
        outs = [torch.zeros_like(t) for t in (value, pred, offsets, attn)]
        need = E.lib().fbbev_da_cross_attn_bwd_det_ws_bytes(B, Ncam, S, M, Dh, Q, Za, DC, *shapes[0])
        ws = torch.full(((need + 15) // 16 * 4,), float('nan'))
        E.ok(E.lib().fbbev_da_cross_attn_bwd_ex(E.p(value), E.p(ss), E.p(ls), E.p(pred), E.p(ref_cam), E.p(m8), E.p(qdepth), E.p(offsets),
                                                E.p(attn), E.p(g), B, Ncam, S, M, Dh, L, Q, P, Za, DC, d0, dstep, 0, Dh,
                                                *(E.p(t) for t in outs), shapes[0][0], shapes[0][1], flags, E.p(ws), need, None))
        res.setdefault(flags, []).append(outs)
    off, (on, on2) = res[0][0], res[FLAG_DET]
    for a, b in zip(on, on2):
        assert torch.equal(a, b)
    for name, a, b in zip(('value', 'depth', 'offsets', 'attn'), on, off):
        scale = b.abs().max().item()
        err = (a - b).abs().max().item()
        print(f'global DA {name}: max|fixed point - atomic| = {err:.2e} on a scale of {scale:.3e}')
        assert scale > 0 and err <= 2e-6 * scale, name
