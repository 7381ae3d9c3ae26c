"""Case table, float64 reference, input builders, bounds and adapters for the depth-aware (DA) cross-attention kernels, shared by the
GPU test (tests/test_gpu_da_kernels.py, through fb_bev_amd._capi) and the emulator test (tests/test_emu_da_kernels.py, through
tests/emu/emu_capi.py): fbbev_da_cross_attn_fwd / _fwd_e / _fwd_zt / _fwd_planes / _fused / _fused_e and fbbev_da_cross_attn_bwd /
_bwd_ws / _bwd_ws_grid / _bwd_planes with their _ex forms, at the smallest shapes at which each of their code paths exists.

The reference (`reference`) is written from the contract in the header of fb_bev_amd/csrc/da_kernels.h, not from the kernels: a
camera is hit if any anchor bit of the query is set; every anchor of a hit camera is sampled; sample p uses anchor p % Za; the depth
weight is ONE bilinear sample of the plane of bin clip(floor((d - d0) / dstep), 0, DC - 1) of the level-0 sized depth distribution;
a sample is valid for -1 < h_im < H and -1 < w_im < W, corners outside the level are zero; the camera sum is divided by
max(hit count, 1).  It is vectorised float64 torch, differentiable, and also returns S: the same sum on absolute values.

Layer A, exact dyadic inputs (`dyadic_case`).  Level heights are powers of two and so is level 0's width; value is an integer in
[-4, 4], pred_depth k/8 in [0, 1], ref_cam a quarter pixel of level 0 between one pixel outside and one pixel outside, offsets half
pixels (x offsets of a level whose width is no power of two: 0, +-w/2, +-w, so that offset / w is still exact), the attention
weights k/16 summing to 1 per unit, dstep a power of two, qdepth on bin edges and bin centres from below d0 to beyond the last
bin, grad_slots an integer in [-3, 3], and every query is seen by 0, 1, 2 or 4 cameras.  Every product and every partial sum is then a
multiple of a quantum 2^-k that stays below 2^24 quanta (`check_representable` asserts it from S), so fp32 arithmetic is exact in
ANY order and the result must equal the float64 reference bit for bit: slots, and in the backward grad_value, grad_pred_depth,
grad_offsets and grad_attn against float64 autograd of the same reference.  No tolerance.  A wrong or misplaced sample, a wrong
count, a lost corner or an argument that arrives in another's place changes a dyadic number.  The builder plants samples exactly at
h_im = -1, h_im = H, w_im = -1 and w_im = W and asserts them, samples exactly on grid points, depths exactly on bin edges and queries
that no camera sees.

Layer B, real values with full mantissas at level sizes that are no powers of two (`real_case`).  Forward entries, componentwise
against float64:  |got - exact| <= c * S + T.
  c, in units of u = 2^-24, from the expressions of k_da_cross_attn_fwd (the other forward kernels evaluate the same expressions; an
  fma where the compiler contracts one only removes a rounding).  The builder keeps every fractional pixel coordinate in [1/8, 7/8]:
    lh = h_im - floor(h_im)          exact for h_im >= 0; for h_im in (-1, 0) at most u relative (lh >= 1/2 there or exact)
    hh = 1 - lh                      at most u relative for lh < 1/2, exact else; with lh's error over hh >= 1/8: at most 4 u
    w  = hh * hw                     4 + 4 + 1 = 9 u for the worst corner weight
    w * v, three adds                1 + 3 u of sum |w v|
    weight = attn * dw, * weight     1 + 1 u
    dw (one bilinear sample of pred_depth >= 0)   9 + 1 + 3 = 13 u
  = 28 u per sample; the planes kernels' extra live-flag product in the weight adds 1: 30 u with the second-order terms rounded up.
  Accumulation: L * P adds into the camera's column, at most Ncam camera adds, one division:
      c = (30 + L * P + Ncam + 1) * 2^-24.
  T, the position term: a pixel coordinate computed in fp32 as (ref + off / size) * size - 0.5 is off by at most
      delta = u * (|off| + 2 |loc * size| + |im|) * (1 + 2^-10)      (division, addition, product, subtraction)
  (the depth sample's ref * size - 0.5: u * (|ref * size| + |im|)), and T = sum over the samples of |d out / d im| * delta, the
  derivative taken by float64 autograd of the reference's bilinear sample with respect to the pixel coordinates (`position_term`).
  Because no coordinate is within 1/8 pixel of a kink the one-sided derivative is the derivative.  The pipelined kernel divides the
  offset by the size like every other kernel (an earlier form multiplied by the reciprocal): it takes the same count.
  The entries that project in the kernel (fused, fused_e) add the bf16 split's 4 * 2^-16 per product of both projections, through the
  same position term for the offsets and through the softmax for the weights, and must be at least 30 times closer to the exact result
  than the same computation on plain bf16-rounded query and weights (`fused_real_case`, `check_fused_real`).
  The LDS-plane backward routes (chunked scatter, owned planes, bwd_planes) have a bound per gradient, with half a fixed-point quantum
  per addend of grad_value, the addends counted by the reference (`backward_bounds`, `check_bwd_real`).
  No layer B: the 16-bit rows of fwd_e, the fused softmax of the pipelined kernel's logits flag, the global-atomic backward (not an
  LDS-plane route; its cases are layer A only in the table) and the deterministic entries (the same kernels with fixed-point taps).

Plain Python and CPU torch only; the adapters import their library on first use.
"""
import math
import os
import sys

import torch

U24 = 2.0 ** -24
F32, F64 = torch.float32, torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))


def observed(text):
    print(f'[observed] {text}')


# ------------------------------------------------------------------------------------------------------------------ reference
def _bilinear(src, H, W, h_im, w_im, base=None, mode='val'):
    """src (..., N, C), h_im / w_im (..., K) [, base (..., K): token offset] -> (..., K, C): the MSDA bilinear sample.  mode (for the
    bounds, on |src|): 'dh' / 'dw' weigh the corners by |d weight / d h_im| / |d weight / d w_im|, 'one' by 1"""
    valid = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
    hl, wl = torch.floor(h_im.detach()), torch.floor(w_im.detach())
    lh, lw = h_im - hl, w_im - wl
    hh, hw = 1 - lh, 1 - lw
    C = src.shape[-1]
    src = src.expand(*h_im.shape[:-1], *src.shape[-2:])
    out = 0
    one = torch.ones_like(hh)
    weights = {'val': (hh * hw, hh * lw, lh * hw, lh * lw), 'dh': (hw, lw, hw, lw), 'dw': (hh, hh, lh, lh), 'one': (one, one, one, one)}[mode]
    for (dy, dx), wgt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), weights):
        y, x = hl + dy, wl + dx
        inb = valid & (y >= 0) & (y < H) & (x >= 0) & (x < W)
        idx = (y.clamp(0, H - 1) * W + x.clamp(0, W - 1)).long()
        if base is not None:
            idx = idx + base
        v = torch.gather(src, -2, idx.unsqueeze(-1).expand(*idx.shape, C))
        out = out + v * torch.where(inb, wgt, torch.zeros_like(wgt)).unsqueeze(-1)
    return out


def pixel_coords(ss, ref_cam, offsets, Za):
    """-> per level (h_im, w_im) of shape (Ncam, B, Q, M, P), and the depth sample's (h_im, w_im) of shape (Ncam, B, Q, Za); float64"""
    shapes = [(int(h), int(w)) for h, w in ss.tolist()]
    ref_cam, offsets = ref_cam.double(), offsets.double()
    P = offsets.shape[4]
    z = torch.arange(P) % Za
    rc = ref_cam[:, :, :, z]                                          # (Ncam, B, Q, P, 2)
    out = []
    for l, (h, w) in enumerate(shapes):
        w_im = (rc[..., 0].unsqueeze(3) + offsets[None, :, :, :, l, :, 0] / w) * w - 0.5
        h_im = (rc[..., 1].unsqueeze(3) + offsets[None, :, :, :, l, :, 1] / h) * h - 0.5
        out.append((h_im, w_im))
    H0, W0 = shapes[0]
    return out, (ref_cam[..., 1] * H0 - 0.5, ref_cam[..., 0] * W0 - 0.5)


def _parts(value, ss, ls, pred_depth, ref_cam, mask, qdepth, offsets, attn, d0, dstep, pix=None):
    """the pieces of the reference: per level the bilinear samples (Ncam, B, M, Q, P, Dh), the depth weights (Ncam, B, Q, Za)"""
    Ncam, B, Q, Za = mask.shape
    BN, S, M, Dh = value.shape
    L, P = attn.shape[3], attn.shape[4]
    DC = pred_depth.shape[1]
    shapes = [(int(h), int(w)) for h, w in ss.tolist()]
    starts = [int(x) for x in ls.tolist()]
    H0, W0 = shapes[0]
    if pix is None:
        pix = pixel_coords(ss, ref_cam, offsets, Za)
    lv, (dh, dw) = pix
    bins = torch.floor((qdepth.double() - d0) / dstep).clamp(0, DC - 1).long()
    planes = pred_depth.reshape(B, Ncam, DC * H0 * W0).permute(1, 0, 2).unsqueeze(-1)       # (Ncam, B, DC*H0*W0, 1)
    depth_w = _bilinear(planes, H0, W0, dh.reshape(Ncam, B, Q * Za), dw.reshape(Ncam, B, Q * Za),
                        base=bins.reshape(Ncam, B, Q * Za) * (H0 * W0))[..., 0].reshape(Ncam, B, Q, Za)
    v = value.reshape(B, Ncam, S, M, Dh).permute(1, 0, 3, 2, 4)                              # (Ncam, B, M, S, Dh)
    bil = []
    for l, (h, w) in enumerate(shapes):
        h_im, w_im = lv[l]
        hi = h_im.permute(0, 1, 3, 2, 4).reshape(Ncam, B, M, Q * P)
        wi = w_im.permute(0, 1, 3, 2, 4).reshape(Ncam, B, M, Q * P)
        bil.append(_bilinear(v[:, :, :, starts[l]:starts[l] + h * w], h, w, hi, wi).reshape(Ncam, B, M, Q, P, Dh))
    return bil, depth_w


def _combine(bil, depth_w, attn, mask):
    Ncam, B, Q, Za = mask.shape
    L, P = attn.shape[3], attn.shape[4]
    z = torch.arange(P) % Za
    dwp = depth_w[..., z].unsqueeze(2)                                                     # (Ncam, B, 1, Q, P)
    total = 0
    for l in range(L):
        wt = attn[:, :, :, l, :].permute(0, 2, 1, 3).unsqueeze(0) * dwp                      # (Ncam, B, M, Q, P)
        total = total + (bil[l] * wt.unsqueeze(-1)).sum(4)                                 # (Ncam, B, M, Q, Dh)
    hit = mask.bool().any(-1)                                                              # (Ncam, B, Q)
    count = hit.sum(0).clamp(min=1).to(total.dtype)                                        # (B, Q)
    acc = (total * hit[:, :, None, :, None].to(total.dtype)).sum(0)                        # (B, M, Q, Dh)
    out = acc / count[:, None, :, None]
    return out.permute(0, 2, 1, 3).reshape(B, Q, -1)


def reference(value, ss, ls, pred_depth, ref_cam, mask, qdepth, offsets, attn, d0, dstep):
    """value (B*Ncam, S, M, Dh), pred_depth (B*Ncam, DC, H0, W0), ref_cam (Ncam, B, Q, Za, 2), mask (Ncam, B, Q, Za), qdepth
    (Ncam, B, Q, Za), offsets (B, Q, M, L, P, 2), attn (B, Q, M, L, P) -> slots (B, Q, M*Dh) in float64 (differentiable in value,
    pred_depth, offsets and attn) and S, the same sum on absolute values."""
    value, pred_depth, offsets, attn = (t if t.dtype == F64 else t.double() for t in (value, pred_depth, offsets, attn))
    geo = (ss, ls)
    bil, dw = _parts(value, *geo, pred_depth, ref_cam, mask, qdepth, offsets, attn, d0, dstep)
    slots = _combine(bil, dw, attn, mask)
    with torch.no_grad():
        bil_a, dw_a = _parts(value.detach().abs(), *geo, pred_depth.detach().abs(), ref_cam, mask, qdepth, offsets.detach(), attn, d0, dstep)
        S = _combine(bil_a, dw_a, attn.detach().abs(), mask)
    return slots, S


def reference_backward(case, grad_slots):
    """float64 autograd of `reference`: (grad_value, grad_pred_depth, grad_offsets, grad_attn) in the logical layouts"""
    leaves = [case[k].double().requires_grad_() for k in ('value', 'pred_depth', 'offsets', 'attn')]
    slots, _ = reference(leaves[0], case['ss'], case['ls'], leaves[1], case['ref_cam'], case['mask'], case['qdepth'], leaves[2], leaves[3],
                         case['d0'], case['dstep'])
    return torch.autograd.grad(slots, leaves, grad_slots.double())


def position_term(case, doff=None):
    """T of layer B: sum over the samples of |d slots / d pixel coordinate| * (fp32 rounding bound of that coordinate); (B, Q, M*Dh).
    doff (B, Q, M, L, P, 2): a bound on the error of the offsets themselves (projected in the kernel), added to that of the coordinate"""
    c = case
    mask, Za = c['mask'], c['mask'].shape[-1]
    Ncam, B, Q, _ = mask.shape
    value, pred, offsets, attn = (c[k].double() for k in ('value', 'pred_depth', 'offsets', 'attn'))
    ref = c['ref_cam'].double()
    L, P = attn.shape[3], attn.shape[4]
    Dh = value.shape[-1]
    shapes = [(int(h), int(w)) for h, w in c['ss'].tolist()]
    lv, (dh, dw) = pixel_coords(c['ss'], ref, offsets, Za)
    lv = [(h.clone().requires_grad_(), w.clone().requires_grad_()) for h, w in lv]
    dh, dw = dh.clone().requires_grad_(), dw.clone().requires_grad_()
    bil, depth_w = _parts(value, c['ss'], c['ls'], pred, ref, mask, c['qdepth'], offsets, attn, c['d0'], c['dstep'], pix=(lv, (dh, dw)))
    up = U24 * (1 + 2.0 ** -10)
    z = torch.arange(P) % Za
    rc = ref[:, :, :, z]
    gdh, gdw = torch.autograd.grad(depth_w.sum(), (dh, dw), retain_graph=True)
    H0, W0 = shapes[0]
    d_depth = (gdh.abs() * up * ((ref[..., 1] * H0).abs() + dh.detach().abs()) +
               gdw.abs() * up * ((ref[..., 0] * W0).abs() + dw.detach().abs()))             # (Ncam, B, Q, Za): bound on |delta dw|
    dwp = depth_w.detach().abs()[..., z].unsqueeze(2)                                      # (Ncam, B, 1, Q, P)
    ddp = d_depth[..., z].unsqueeze(2)
    total = 0
    for l, (h, w) in enumerate(shapes):
        h_im, w_im = lv[l]
        loc_h = (rc[..., 1].unsqueeze(3) + offsets[None, :, :, :, l, :, 1] / h)
        loc_w = (rc[..., 0].unsqueeze(3) + offsets[None, :, :, :, l, :, 0] / w)
        del_h = up * (offsets[None, :, :, :, l, :, 1].abs() + 2 * (loc_h * h).abs() + h_im.detach().abs())   # (Ncam, B, Q, M, P)
        del_w = up * (offsets[None, :, :, :, l, :, 0].abs() + 2 * (loc_w * w).abs() + w_im.detach().abs())
        if doff is not None:
            del_h, del_w = del_h + doff[None, :, :, :, l, :, 1], del_w + doff[None, :, :, :, l, :, 0]
        a = attn[:, :, :, l, :].permute(0, 2, 1, 3).unsqueeze(0).abs()                      # (1, B, M, Q, P)
        per_c = []
        for ch in range(Dh):
            gh, gw = torch.autograd.grad(bil[l][..., ch].sum(), (h_im, w_im), retain_graph=True)
            mv = (gh.abs() * del_h + gw.abs() * del_w).permute(0, 1, 3, 2, 4)              # (Ncam, B, M, Q, P)
            per_c.append(((mv * a * dwp) + bil[l][..., ch].detach().abs() * a * ddp).sum(4))
        total = total + torch.stack(per_c, -1)                                             # (Ncam, B, M, Q, Dh)
    hit = mask.bool().any(-1)
    count = hit.sum(0).clamp(min=1).double()
    acc = (total * hit[:, :, None, :, None].double()).sum(0) / count[:, None, :, None]
    return acc.permute(0, 2, 1, 3).reshape(B, Q, -1)


def backward_bounds(case, route, q_per_chunk):
    """Layer B of the LDS-plane backward routes: per gradient a componentwise bound  c * S + T [+ n * q / 2].
    S: the gradient's sum on absolute values (|grad_slots|, |value|, |attn|; corner weights and pred_depth are >= 0).
    T: the position term -- every addend's derivative with respect to a pixel coordinate, in absolute value (bilinear weights:
       |d w_k / d h| = hw or lw; a gradient with respect to an offset: the mixed second derivative, at most the sum of the four
       |corners|; the pure ones vanish), times the fp32 rounding bound of that coordinate (`position_term`).
    c, in u = 2^-24, from k_da_cross_attn_bwd_unit / k_da_bwd_unit_planes / the scatter kernels:
       g = grad_slots / count 1; corner weight 9; bilinear value 9 + 1 + 3 = 13; depth weight 13; weight = attn * dw 1
       grad_attn    = sum_cam dw * <g, bil>             13 + Dh (dot) + 1 + 13 + 1 + Ncam   <= (29 + Dh + Ncam) u
       grad_offsets = sum_cam weight * <g, d bil / d im>  the same count (derivative weights are hw, lw: 4 u at most)
       grad_value addend g * weight * w_k               1 + 14 + 9 + 2 = 26, one conversion back from fixed point, n_chunks
                                                        partial planes added in fp32: (27 + n_chunks) u,
                    + half a quantum per addend: the planes count in q = 2^-30 of the power of two above max |grad_slots| of what
                      the plane's workgroup scatters (da_kernels.h) -- owned planes: of the SAMPLE b (k_da_bwd_scatter_owned,
                      gmax_bits[b]); chunked scatter: of head m's slots of the chunk's q_per_chunk queries of sample b
                      (k_da_cross_attn_bwd_scatter).  The term is sum over the addends of the word of q(addend) / 2: every
                      (sample, corner) pair of a hit camera is counted here with the quantum of its own sample / (head, chunk)
       grad_pred_depth addend ddw * corner weight, ddw = sum over the L*P/Za samples of the anchor and (atomically) the M heads of
                    attn * <g, bil>:  13 + Dh + 2 + L*P/Za + 9 + 1, then n_d * M fp32 atomic adds on the word:
                                                        (25 + Dh + L*P/Za + M * n_d) u
    Every sample of a hit camera is at least 1/8 pixel from a kink (`real_case` asserts it), so no addend changes its cell."""
    c = case
    mask, Za = c['mask'], c['mask'].shape[-1]
    Ncam, B, Q, _ = mask.shape
    V = c['value'].double().abs().requires_grad_()
    Pd = c['pred_depth'].double().abs().requires_grad_()
    A, offsets, ref = c['attn'].double().abs(), c['offsets'].double(), c['ref_cam'].double()
    BN, S, M, Dh = V.shape
    L, P = A.shape[3], A.shape[4]
    DC = Pd.shape[1]
    shapes = [(int(h), int(w)) for h, w in c['ss'].tolist()]
    starts = [int(x) for x in c['ls'].tolist()]
    H0, W0 = shapes[0]
    lv, (dh, dw) = pixel_coords(c['ss'], ref, offsets, Za)
    up = U24 * (1 + 2.0 ** -10)
    hit = mask.bool().any(-1)
    count = hit.sum(0).clamp(min=1).double()
    hw_ = (hit.double() / count[None])[:, :, None, :, None]                              # (Ncam, B, 1, Q, 1)
    hitf = hit.double()[:, :, None, :, None]
    g = c['grad_slots'].double().abs().view(B, Q, M, Dh).permute(0, 2, 1, 3)[None, :, :, :, None, :]   # (1, B, M, Q, 1, Dh)
    z = torch.arange(P) % Za
    rc = ref[:, :, :, z]
    bins = torch.floor((c['qdepth'].double() - c['d0']) / c['dstep']).clamp(0, DC - 1).long().reshape(Ncam, B, Q * Za) * (H0 * W0)
    planes = Pd.reshape(B, Ncam, DC * H0 * W0).permute(1, 0, 2).unsqueeze(-1)

    def depth(mode):
        return _bilinear(planes, H0, W0, dh.reshape(Ncam, B, Q * Za), dw.reshape(Ncam, B, Q * Za), base=bins, mode=mode)[..., 0].reshape(Ncam, B, Q, Za)

    d_val, d_dh, d_dw, d_one = depth('val'), depth('dh'), depth('dw'), depth('one')
    del_dh = up * ((ref[..., 1] * H0).abs() + dh.abs())
    del_dw = up * ((ref[..., 0] * W0).abs() + dw.abs())
    d_depth = (d_dh * del_dh + d_dw * del_dw).detach()                                   # bound on |delta dw|, (Ncam, B, Q, Za)
    dwp = d_val.detach()[..., z].unsqueeze(2)                                            # (Ncam, B, 1, Q, P)
    ddp = d_depth[..., z].unsqueeze(2)
    v = V.reshape(B, Ncam, S, M, Dh).permute(1, 0, 3, 2, 4)
    # half a quantum of the plane an addend of (sample b, head m, query q) goes to: (1, B, M, Q, 1)
    gs = c['grad_slots'].double().abs().view(B, Q, M, Dh)
    if route == 'owned':
        gm = gs.amax((1, 2, 3)).view(B, 1, 1).expand(B, M, Q)
    else:
        n_chunks = -(-Q // q_per_chunk)
        pad = torch.zeros(B, n_chunks * q_per_chunk, M, Dh, dtype=F64)
        pad[:, :Q] = gs
        gm = pad.view(B, n_chunks, q_per_chunk, M, Dh).amax((2, 4)).repeat_interleave(q_per_chunk, 1)[:, :Q].permute(0, 2, 1)
    n_chunks = -(-Q // q_per_chunk)
    half_q = torch.where(gm > 0, 2.0 ** (torch.floor(torch.log2(gm.clamp(min=1e-300))) + 1 - 30), torch.zeros_like(gm)) / 2
    half_q = half_q[None, :, :, :, None]
    F_S = F_T = F_n = 0
    S_a, T_a, S_o, T_o = [], [], [], []
    ddw_abs = torch.zeros(Ncam, B, Q, Za, dtype=F64)
    a_pos = torch.zeros(Ncam, B, Q, Za, dtype=F64)
    for l, (h, w) in enumerate(shapes):
        h_im, w_im = lv[l]
        hi = h_im.permute(0, 1, 3, 2, 4).reshape(Ncam, B, M, Q * P)
        wi = w_im.permute(0, 1, 3, 2, 4).reshape(Ncam, B, M, Q * P)
        src = v[:, :, :, starts[l]:starts[l] + h * w]
        bv, bh, bw, b1 = (_bilinear(src, h, w, hi, wi, mode=m_).reshape(Ncam, B, M, Q, P, Dh) for m_ in ('val', 'dh', 'dw', 'one'))
        gb, gh, gw, g1 = ((g * t).sum(-1) for t in (bv, bh, bw, b1))                      # (Ncam, B, M, Q, P)
        loc_h = rc[..., 1].unsqueeze(3) + offsets[None, :, :, :, l, :, 1] / h
        loc_w = rc[..., 0].unsqueeze(3) + offsets[None, :, :, :, l, :, 0] / w
        del_h = (up * (offsets[None, :, :, :, l, :, 1].abs() + 2 * (loc_h * h).abs() + h_im.abs())).permute(0, 1, 3, 2, 4)
        del_w = (up * (offsets[None, :, :, :, l, :, 0].abs() + 2 * (loc_w * w).abs() + w_im.abs())).permute(0, 1, 3, 2, 4)
        a_l = A[:, :, :, l, :].permute(0, 2, 1, 3).unsqueeze(0)                            # (1, B, M, Q, P)
        move = gh * del_h + gw * del_w
        F_S = F_S + (hw_ * a_l * dwp * gb).sum()
        F_T = F_T + (hw_ * a_l * (dwp * move + ddp * gb)).sum()
        F_n = F_n + (hitf * half_q * b1.sum(-1)).sum()
        with torch.no_grad():
            S_a.append((hw_ * dwp * gb).sum(0))
            T_a.append((hw_ * (dwp * move + ddp * gb)).sum(0))
            S_o.append(torch.stack([(hw_ * a_l * dwp * gw).sum(0), (hw_ * a_l * dwp * gh).sum(0)], -1))
            T_o.append(torch.stack([(hw_ * a_l * (dwp * g1 * del_h + ddp * gw)).sum(0), (hw_ * a_l * (dwp * g1 * del_w + ddp * gh)).sum(0)], -1))
            per_z = lambda t: (hw_ * a_l * t).sum(2).reshape(Ncam, B, Q, P // Za, Za).sum(3)  # noqa: E731
            ddw_abs += per_z(gb)
            a_pos += per_z(move)
    S_v, = torch.autograd.grad(F_S, V, retain_graph=True)
    T_v, = torch.autograd.grad(F_T, V, retain_graph=True)
    quantum, = torch.autograd.grad(F_n, V)
    S_d, = torch.autograd.grad((ddw_abs * d_val).sum(), Pd, retain_graph=True)
    T_d, = torch.autograd.grad((a_pos * d_val + ddw_abs * (d_dh * del_dh + d_dw * del_dw)).sum(), Pd, retain_graph=True)
    n_d, = torch.autograd.grad((hit.double()[..., None] * d_one).sum(), Pd)
    lay = lambda ts: torch.stack(ts, 3).permute(0, 2, 1, 3, 4) if ts[0].dim() == 4 else torch.stack(ts, 3).permute(0, 2, 1, 3, 4, 5)  # noqa: E731
    cu = (29 + Dh + Ncam) * U24
    return dict(grad_value=(27 + n_chunks) * U24 * S_v + T_v + quantum,
                grad_pred_depth=(25 + Dh + L * P // Za + M * n_d) * U24 * S_d + T_d,
                grad_offsets=cu * lay(S_o) + lay(T_o), grad_attn=cu * lay(S_a) + lay(T_a))


def forward_c(L, P, Ncam):
    """c of layer B (see the module docstring)"""
    return (30 + L * P + Ncam + 1) * U24


# ------------------------------------------------------------------------------------------------------------------ input builders
def _geometry(shapes):
    ss = torch.tensor(shapes, dtype=torch.int64)
    n = ss[:, 0] * ss[:, 1]
    ls = torch.cat([ss.new_zeros(1), n.cumsum(0)[:-1]])
    return ss, ls, int(n.sum())


def _pow2(n):
    return n & (n - 1) == 0


def _masks(g, Ncam, B, Q, Za, counts, forced=None):
    """every (b, q) is seen by a number of cameras drawn from `counts`; a seen camera has a random non-empty set of anchor bits"""
    cnt = torch.tensor(counts)[torch.randint(0, len(counts), (B, Q), generator=g)]
    if forced is not None:
        for (b, q), n in forced.items():
            cnt[b, q] = n
    rank = torch.rand(Ncam, B, Q, generator=g).argsort(0).argsort(0)
    hit = rank < cnt[None]
    bits = torch.rand(Ncam, B, Q, Za, generator=g) < 0.5
    bits.scatter_(3, torch.randint(0, Za, (Ncam, B, Q, 1), generator=g), True)
    return hit[..., None] & bits, cnt


def dyadic_case(seed, B, Ncam, Q, M, Dh, shapes, P, Za, DC, counts=(0, 1, 2, 4), attn_uniform=False):
    """Layer A inputs (module docstring); asserts what the construction promises.  attn_uniform: the weights of a unit are 1/k on k in
    {1, 2, 4, 8} of its L*P samples and 0 elsewhere, with `logits` (0 on the survivors, -200 elsewhere) whose softmax they are."""
    g = torch.Generator().manual_seed(seed)
    ss, ls, S = _geometry(shapes)
    L = len(shapes)
    H0, W0 = shapes[0]
    assert all(_pow2(h) for h, _ in shapes), 'layer A: level heights are powers of two'
    wide0 = not _pow2(W0)          # level 0's width is no power of two (one level only): x in eighths of the image, no x border plants
    assert not wide0 or L == 1
    counts = tuple(n for n in counts if n <= Ncam)
    low = min(n for n in counts if n > 0)
    forced = {(0, q): low for q in range(min(4, Q))}
    if Q > 4 and 0 in counts:
        forced[(0, 4)] = 0
    mask, cnt = _masks(g, Ncam, B, Q, Za, counts, forced)
    value = torch.randint(-4, 5, (B * Ncam, S, M, Dh), generator=g).float()
    pred = torch.randint(0, 9, (B * Ncam, DC, H0, W0), generator=g).float() / 8
    ux = torch.randint(-4, 4 * W0 + 5, (Ncam, B, Q, Za), generator=g).float() / 4
    uy = torch.randint(-4, 4 * H0 + 5, (Ncam, B, Q, Za), generator=g).float() / 4
    ref_cam = torch.stack([ux / W0, uy / H0], -1)
    if wide0:
        ref_cam[..., 0] = torch.randint(-1, 10, (Ncam, B, Q, Za), generator=g).float() / 8
    offsets = torch.randint(-4, 5, (B, Q, M, L, P, 2), generator=g).float() / 2
    for l, (h, w) in enumerate(shapes):
        if not _pow2(w):          # offset / w must be exact: 0, +-1/2 or +-1 of the width
            offsets[:, :, :, l, :, 0] = torch.randint(-2, 3, (B, Q, M, P), generator=g).float() * (w / 2)
    LP = L * P
    logits = None
    if attn_uniform:
        k = 2 ** torch.randint(0, 4, (B, Q, M, 1), generator=g)
        keep = torch.rand(B, Q, M, LP, generator=g).argsort(-1).argsort(-1) < k
        attn = (keep.float() / k).view(B, Q, M, L, P)
        logits = torch.where(keep, 0.0, -200.0).view(B, Q, M, L, P)
    else:
        pick = torch.randint(0, LP, (B, Q, M, 16), generator=g)
        attn = (torch.zeros(B, Q, M, LP).scatter_add_(3, pick, torch.ones(pick.shape)) / 16).view(B, Q, M, L, P)
    d0, dstep = 2.0, 0.5
    qdepth = d0 + dstep * torch.randint(-3, 2 * DC + 4, (Ncam, B, Q, Za), generator=g).float() / 2
    # plants: the first four queries of sample 0 put anchor 0 / head 0 / level 0 / point 0 of their first camera exactly on a border
    hit = mask.any(-1)
    for q, (rx, ry) in enumerate(((1.0 / W0, -0.5 / H0), (1.0 / W0, (H0 + 0.5) / H0), (-0.5 / W0, 1.0 / H0), ((W0 + 0.5) / W0, 1.0 / H0))):
        if q >= Q or (wide0 and q >= 2):
            break
        if wide0:
            rx = 0.25
        cam = int(hit[:, 0, q].nonzero()[0])
        ref_cam[cam, 0, q, 0, 0], ref_cam[cam, 0, q, 0, 1] = rx, ry
        offsets[0, q, 0, 0, 0] = 0.0
    grad_slots = torch.randint(-3, 4, (B, Q, M * Dh), generator=g).float()
    case = dict(value=value, ss=ss, ls=ls, pred_depth=pred, ref_cam=ref_cam, mask=mask, qdepth=qdepth, offsets=offsets, attn=attn,
                d0=d0, dstep=dstep, grad_slots=grad_slots, shapes=tuple(shapes), logits=logits, Za=Za, DC=DC, counts=cnt)
    # what the construction promises, on the samples of hit cameras
    lv, _ = pixel_coords(ss, ref_cam, offsets, Za)
    h0, w0 = lv[0]
    hm = hit[:, :, :, None, None].expand_as(h0)
    if Q >= 4:
        assert ((h0 == -1) & hm).any() and ((h0 == H0) & hm).any()
        assert wide0 or (((w0 == -1) & hm).any() and ((w0 == W0) & hm).any())
    on_grid = (h0 == h0.floor()) & (wide0 | (w0 == w0.floor())) & (h0 >= 0) & (h0 < H0) & (w0 >= 0) & (w0 < W0) & hm
    assert on_grid.any(), 'no sample exactly on a grid point (a grid row where level 0 is 88 wide)'
    rel = (qdepth.double() - d0) / dstep
    assert ((rel == rel.floor()) & hit[..., None]).any() and (rel < 0).any() and (rel > DC).any()
    if 0 in counts and Q > 4:
        assert (cnt == 0).any()
    assert set(hit.sum(0).unique().tolist()) <= set(counts)
    return case


def check_representable(case, S):
    """Layer A: every partial sum of the forward is a multiple of a quantum q and at most S * count, which must stay below 2^24 q"""
    H0, W0 = case['shapes'][0]
    bits = 0
    for h, w in case['shapes']:
        # fractional pixel coordinates of level l: multiples of min(1/2, size / (4 * size0)) (x of a width that is no power of two:
        # ref * w is a multiple of 1 / (4 * W0))
        fy = max(1, int(math.log2(4 * H0 / h))) if h < 2 * H0 else 1
        if not _pow2(W0):
            fx = 1
        else:
            fx = int(math.log2(4 * W0)) if not _pow2(w) else (max(1, int(math.log2(4 * W0 / w))) if w < 2 * W0 else 1)
        bits = max(bits, fx + fy)
    q = 2.0 ** -(bits + 4 + 3 + 4)          # corner weights, attn k/16 (1/8 when uniform), pred k/8 times level-0 weights in 1/16
    count = case['mask'].any(-1).sum(0).clamp(min=1).double()
    top = (S * count[..., None]).max().item()
    assert top / q < 2 ** 24, (top, q)


def real_case(seed, B, Ncam, Q, M, Dh, shapes, P, Za, DC, counts=(0, 1, 2, 3, 4, 5, 6), phase=None, offsets=None):
    """Layer B inputs: full-mantissa values, and every pixel coordinate that a hit camera samples -- the depth samples included -- has
    its fractional part in [1/8, 7/8] (asserted in float64 on the fp32 inputs, 100 % of them), a share of them in (-1, 0) and
    (size - 1, size); qdepth stays a quarter bin from every bin edge.  phase / offsets (the entries that project in the kernel, see
    `fused_real_operands`): every reference point sits `phase` into a coarsest-level pixel and the offsets are the caller's."""
    g = torch.Generator().manual_seed(seed)
    ss, ls, S = _geometry(shapes)
    L = len(shapes)
    H0, W0 = shapes[0]
    counts = tuple(n for n in counts if n <= Ncam)
    mask, cnt = _masks(g, Ncam, B, Q, Za, counts)
    hit = mask.any(-1)
    value = torch.randn(B * Ncam, S, M, Dh, generator=g)
    pred = torch.rand(B * Ncam, DC, H0, W0, generator=g).softmax(1).contiguous()

    # The offsets are shared by the cameras of a query, so the cameras' reference points of one (query, anchor) differ by whole pixels
    # of the COARSEST level (nested pyramid: whole pixels of every level) plus a jitter of 0.02 pixel: one draw of an offset then
    # clears every hit camera at once.
    hc, wc = min(h for h, _ in shapes), min(w for _, w in shapes)
    assert all(H0 % h == 0 and W0 % w == 0 for h, w in shapes), 'layer B: a nested pyramid'
    Rh, Rw = H0 // hc, W0 // wc

    def ref_pix(R, size_c):      # level-0 pixel coordinates from R pixels outside to R pixels outside, fractional part in [0.2, 0.8]
        common = torch.randint(0, R, (1, B, Q, Za), generator=g).double() + 0.22 + 0.56 * torch.rand((1, B, Q, Za), generator=g, dtype=F64)
        if phase is not None:
            common = torch.full((1, B, Q, Za), float(phase), dtype=F64)
        k = torch.randint(-1, size_c + 1, (Ncam, B, Q, Za), generator=g).double()
        return k * R + common + 0.04 * (torch.rand((Ncam, B, Q, Za), generator=g, dtype=F64) - 0.5)

    ref_cam = torch.stack([(ref_pix(Rw, wc) + 0.5) / W0, (ref_pix(Rh, hc) + 0.5) / H0], -1).float()
    # offsets are shared by the cameras of a query: redraw the samples that are within 1/8 pixel of a kink for some hit camera
    given = offsets is not None
    offsets = offsets if given else torch.zeros(B, Q, M, L, P, 2)
    todo = torch.ones(B, Q, M, L, P, dtype=torch.bool) & (not given)
    for _ in range(400):
        if not todo.any():
            break
        new = torch.stack([(torch.rand(B, Q, M, L, P, generator=g) * 2 - 1) * 2.5, (torch.rand(B, Q, M, L, P, generator=g) * 2 - 1) * 2.5], -1)
        offsets = torch.where(todo[..., None], new, offsets)
        lv, _ = pixel_coords(ss, ref_cam, offsets, Za)
        bad = torch.zeros_like(todo)
        for l in range(L):
            for t in lv[l]:
                f = t - t.floor()
                b_ = ((f < 0.15) | (f > 0.85)) & hit[:, :, :, None, None]
                bad[:, :, :, l, :] |= b_.any(0)
        todo = bad
    assert not todo.any(), 'no kink-free offsets found'
    k = torch.randint(0, DC + 2, (Ncam, B, Q, Za), generator=g).float() - 1          # from below d0 to beyond the last bin
    d0, dstep = 2.0, 0.75
    qdepth = d0 + dstep * (k + 0.25 + 0.5 * torch.rand(Ncam, B, Q, Za, generator=g))
    attn = torch.randn(B, Q, M, L * P, generator=g).softmax(-1).view(B, Q, M, L, P).contiguous()
    grad_slots = torch.randn(B, Q, M * Dh, generator=g)
    case = dict(value=value, ss=ss, ls=ls, pred_depth=pred, ref_cam=ref_cam, mask=mask, qdepth=qdepth, offsets=offsets, attn=attn,
                d0=d0, dstep=dstep, grad_slots=grad_slots, shapes=tuple(shapes), logits=None, Za=Za, DC=DC, counts=cnt)
    # the condition, in float64, on 100 % of the samples of hit cameras
    lv, dep = pixel_coords(ss, ref_cam, offsets, Za)
    border = 0
    for l, (h, w) in enumerate(shapes):
        for t, size in zip(lv[l], (h, w)):
            f = t - t.floor()
            hm = hit[:, :, :, None, None].expand_as(t)
            assert (((f >= 0.125) & (f <= 0.875)) | ~hm).all()
            border += int((((t > -1) & (t < 0)) | ((t > size - 1) & (t < size)))[hm].sum())
    assert border > 0
    for t in dep:
        f = t - t.floor()
        assert (((f >= 0.125) & (f <= 0.875)) | ~hit[..., None]).all()
    rel = (qdepth.double() - d0) / dstep
    f = rel - rel.floor()
    assert ((f >= 0.25) & (f <= 0.75)).all()
    if Ncam >= 6:
        assert {3, 5, 6} <= set(hit.sum(0).unique().tolist())
    return case


def fused_operands(case, seed, M, Dh, row_pad=0, period=None):
    """Layer A operands of the entries that project in the kernel: integer query rows (+ an integer addend table), sampling_offsets
    weights in {-1/2, 0, 1/2} (two per row) with a half-integer bias, a zero attention_weights weight and a bias in {0, -200} with 1,
    2, 4 or 8 survivors per head.  Rewrites case['offsets'] / case['attn'] with what those operands produce (exact in float64)."""
    g = torch.Generator().manual_seed(seed)
    B, Q = case['offsets'].shape[:2]
    L, P = case['attn'].shape[3], case['attn'].shape[4]
    E = M * Dh
    buf = torch.full((B, Q, E + row_pad), float('nan'))
    buf[..., :E] = torch.randint(-2, 3, (B, Q, E), generator=g).float()
    query = buf[..., :E]
    addend = None
    if period:
        assert (B * Q) % period == 0
        addend = torch.randint(-1, 2, (period, E), generator=g).float()
    n_so = M * L * P * 2
    w_so = torch.zeros(n_so, E)
    cols = torch.randint(0, E, (n_so, 2), generator=g)
    w_so.scatter_(1, cols, (torch.randint(0, 2, (n_so, 2), generator=g).float() - 0.5))
    b_so = torch.randint(-3, 4, (n_so,), generator=g).float() / 2
    so_w = w_so.view(M, L, P, 2, E)
    so_b = b_so.view(M, L, P, 2)
    for l, (h, w) in enumerate(case['shapes']):
        if not _pow2(w):          # x offsets of this level: 0, +-w/2 or +-w from the bias alone
            so_w[:, l, :, 0] = 0.0
            so_b[:, l, :, 0] = torch.randint(-2, 3, (M, P), generator=g).float() * (w / 2)
    w_aw = torch.zeros(M * L * P, E)
    k = 2 ** torch.randint(0, 4, (M, 1), generator=g)
    keep = torch.rand(M, L * P, generator=g).argsort(-1).argsort(-1) < k
    b_aw = torch.where(keep, 0.0, -200.0).reshape(-1)
    x = query.double().reshape(B * Q, E)
    if addend is not None:
        x = x + addend.double().repeat(B * Q // period, 1)
    off = (x @ w_so.double().t() + b_so.double()).view(B, Q, M, L, P, 2)
    assert torch.equal(off, off.float().double())
    case = dict(case)
    case['offsets'] = off.float()
    case['attn'] = (keep.float() / k).view(1, 1, M, L, P).expand(B, Q, M, L, P).contiguous()
    case['logits'] = None
    return case, dict(query=query, addend=addend, w_so=w_so, b_so=b_so, w_aw=w_aw, b_aw=b_aw)


SPLIT = 4 * 2.0 ** -16          # the bf16 split's cost per product (tests/rows_train_cases.py derives it)


def fused_real_case(seed, B, Ncam, Q, M, Dh, shapes, P, Za, DC, row_pad=0, period=None):
    """Layer B of the entries that project in the kernel.  Full-mantissa query rows in [-1, 1] (+ an addend table), four weights
    of at most 0.075 per sampling_offsets row (the projection moves a sample by at most 0.3 pixel), a bias that puts the sample 1/2
    into a pixel of its level for reference points that sit `phase` into a coarsest-level pixel, dense attention_weights.  The exact
    offsets and softmaxed weights are float64.  Returns the case, the operands and the two terms the projections add to the bound:
      doff: |delta offset| <= (4 * 2^-16 + (E + 2) * 2^-24) * (|x| |W|^T + |b|)  (split products, fp32 accumulation, bias add),
            which moves the pixel coordinate by the same amount (d im / d offset = 1): it joins the position term;
      rho:  the logits carry the same kind of error eps; a softmax weight a_i = e^(l_i) / sum_j e^(l_j) then changes by at most
            |delta l_i| + sum_j a_j |delta l_j| <= 2 max eps relatively, and the kernel's own softmax costs the exponent's product
            with log2(e) (|l - max| u), v_exp_f32 (1 u) and its share again in the sum, L*P adds, a reciprocal (2 u) and a product:
            rho = 2 max eps + (2 (R + 2) + L*P + 3) u  with R the unit's logit range; slots are linear in the weights: rho * S."""
    g = torch.Generator().manual_seed(seed)
    L = len(shapes)
    E = M * Dh
    H0, W0 = shapes[0]
    phase = 0.5
    buf = torch.full((B, Q, E + row_pad), float('nan'))
    buf[..., :E] = torch.rand(B, Q, E, generator=g) * 2 - 1
    query = buf[..., :E]
    addend = (torch.rand(period, E, generator=g) - 0.5) if period else None
    x = query.double().reshape(B * Q, E)
    if addend is not None:
        x = x + addend.double().repeat(B * Q // period, 1)
    n_so = M * L * P * 2
    w_so = torch.zeros(n_so, E)
    w_so.scatter_(1, torch.rand(n_so, E, generator=g).argsort(1)[:, :4], (torch.rand(n_so, 4, generator=g) * 2 - 1) * (0.075 / 1.5))
    b_so = torch.randint(-2, 3, (M, L, P, 2), generator=g).double()
    for l, (h, w) in enumerate(shapes):
        for xy, (size, size0) in enumerate(((w, W0), (h, H0))):
            base = (phase + 0.5) * size / size0 - 0.5                      # the reference point's pixel coordinate of this level, mod 1
            b_so[:, l, :, xy] += 0.5 - (base - math.floor(base))
    b_so = b_so.reshape(-1).float()
    w_aw = (torch.randn(M * L * P, E, generator=g) * (1.0 / E ** 0.5))
    b_aw = torch.randn(M * L * P, generator=g) * 0.5
    off = (x @ w_so.double().t() + b_so.double()).view(B, Q, M, L, P, 2)
    logits = (x @ w_aw.double().t() + b_aw.double()).view(B, Q, M, L * P)
    case = real_case(seed, B, Ncam, Q, M, Dh, shapes, P, Za, DC, phase=phase, offsets=off)
    case['attn'] = logits.softmax(-1).view(B, Q, M, L, P)
    ce = SPLIT + (E + 2) * U24
    doff = ce * (x.abs() @ w_so.double().abs().t() + b_so.double().abs()).view(B, Q, M, L, P, 2)
    eps = ce * (x.abs() @ w_aw.double().abs().t() + b_aw.double().abs()).view(B, Q, M, L * P)
    R = logits.max(-1).values - logits.min(-1).values
    rho = 2 * eps.max(-1).values + (2 * (R + 2) + L * P + 3) * U24                     # (B, Q, M)
    # the same projections on plain bf16-rounded operands: what a kernel without the lo terms would compute
    xb, wsb, wab = x.float().bfloat16().double(), w_so.bfloat16().double(), w_aw.bfloat16().double()
    plain = dict(offsets=(xb @ wsb.t() + b_so.double()).view(B, Q, M, L, P, 2),
                 attn=(xb @ wab.t() + b_aw.double()).view(B, Q, M, L * P).softmax(-1).view(B, Q, M, L, P))
    return case, dict(query=query, addend=addend, w_so=w_so, b_so=b_so, w_aw=w_aw, b_aw=b_aw), doff, rho, plain


# ------------------------------------------------------------------------------------------------------------------ layouts
def pack_rows(value, HS, chunk_major=False, dtype=F32, pad=float('nan')):
    """(BN, S, M, Dh) -> the (BN, S, M, HS) token rows the entries read: head-major [head][HS] with `pad` in the HS - Dh padding
    elements, or chunk-major [chunk][head][4 floats | 8 16-bit elements] (head_minor bit 2)"""
    BN, S, M, Dh = value.shape
    rows = torch.full((BN, S, M, HS), pad, dtype=dtype)
    rows[..., :Dh] = value.to(dtype)
    if chunk_major:
        ce = 4 if dtype == F32 else 8
        assert HS % ce == 0
        rows = rows.view(BN, S, M, HS // ce, ce).permute(0, 1, 3, 2, 4).contiguous().view(BN, S, M, HS)
    return rows


def unpack_rows(rows, Dh, chunk_major=False):
    """inverse of pack_rows for fp32 rows: (logical (BN, S, M, Dh), the padding elements)"""
    BN, S, M, HS = rows.shape
    if chunk_major:
        rows = rows.view(BN, S, HS // 4, M, 4).permute(0, 1, 3, 2, 4).reshape(BN, S, M, HS)
    return rows[..., :Dh], rows[..., Dh:]


def to_layout(t, head_minor_bit, pair):
    """(B, Q, M, L, P[, 2]) -> (B, Q, L, P, M[, 2]) when the bit is set"""
    if not head_minor_bit:
        return t.contiguous()
    return (t.permute(0, 1, 3, 4, 2, 5) if pair else t.permute(0, 1, 3, 4, 2)).contiguous()


def from_layout(t, head_minor_bit, pair):
    if not head_minor_bit:
        return t
    return (t.permute(0, 1, 4, 2, 3, 5) if pair else t.permute(0, 1, 4, 2, 3)).contiguous()


def at_float_offset(t, floats):
    """the same values as a contiguous view that starts `floats` 4-byte elements into a 64-byte aligned buffer"""
    buf = torch.full((t.numel() + floats + 16,), float('nan'), dtype=t.dtype)
    assert buf.data_ptr() % 64 == 0
    v = buf[floats:floats + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------------------------------------ adapters
class GpuApi:
    """fb_bev_amd._capi on cuda:0"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi
        self.c = _capi
        self.device = torch.device('cuda:0')

    def to(self, t):
        """CPU tensor or CPU view of a 1-D buffer -> the same values at the same element offset of a device buffer"""
        if t is None:
            return None
        base = t._base if t._base is not None else t
        d = base.to(self.device)
        return d if t._base is None else d.as_strided(t.shape, t.stride(), t.storage_offset())

    def _geo(self, c):
        return [self.to(c[k]) for k in ('ss', 'ls', 'pred_depth', 'ref_cam', 'mask', 'qdepth')]

    def fwd(self, c, rows, offsets, attn, Dh, head_minor=0, misalign=False, zero_token=None, bev_w=0):
        B, Q = c['mask'].shape[1:3]
        M = rows.shape[2]
        slots = at_float_offset(torch.full((B, Q, M * Dh), float('nan')), 1 if misalign else 0)
        slots = self.to(slots)
        if zero_token is not None:
            buf, v = self.c.da_value_buffer(rows.shape[0] * rows.shape[1], M * rows.shape[3], self.device)
            v.copy_(rows.view(v.shape))
            buf[-1].fill_(zero_token)
            rows_d = v.view(rows.shape)
        else:
            rows_d = self.to(rows)
        ss, ls, pred, ref, mask, qd = self._geo(c)
        self.c.da_cross_attn_fwd(rows_d, ss, ls, pred, ref, mask, qd, self.to(offsets), self.to(attn), c['d0'], c['dstep'], slots,
                                 head_minor=head_minor, head_dim=Dh, zero_token=zero_token is not None, bev_w=bev_w)
        torch.cuda.synchronize()
        return slots.cpu().contiguous()

    def fuses_softmax(self, *a):
        return self.c.da_fuses_softmax(*a)

    def planes_of(self, rows, Dh, chunk_major=False):
        p = self.c.value_rows_to_head_planes(self.to(rows), head_dim=Dh, interleaved=chunk_major)
        torch.cuda.synchronize()
        return p.cpu()

    def fwd_planes_supported(self, *a):
        return self.c.da_cross_attn_fwd_planes_supported(*a)

    def fwd_planes(self, c, planes, offsets, attn, head_minor=0, bev_w=0):
        B, Q = c['mask'].shape[1:3]
        BN, M, S, Dh = planes.shape
        slots = torch.full((B, Q, M * Dh), float('nan'), device=self.device)
        ss, ls, pred, ref, mask, qd = self._geo(c)
        self.c.da_cross_attn_fwd_planes(self.to(planes), ss, ls, pred, ref, mask, qd, self.to(offsets), self.to(attn), c['d0'], c['dstep'],
                                        slots, head_minor=head_minor, bev_w=bev_w, min_level_width=min(w for _, w in c['shapes']))
        torch.cuda.synchronize()
        return slots.cpu()

    def fused_supported(self, *a):
        return self.c.da_cross_attn_fused_supported(*a)

    def fused(self, c, planes, ops, P, bev_w):
        B, Q = c['mask'].shape[1:3]
        BN, M, S, Dh = planes.shape
        slots = torch.full((B, Q, M * Dh), float('nan'), device=self.device)
        ss, ls, pred, ref, mask, qd = self._geo(c)
        f_so = self.c.rows_linear_x3_fragments(self.to(ops['w_so']))
        f_aw = self.c.rows_linear_x3_fragments(self.to(ops['w_aw']))
        self.c.da_cross_attn_fused(self.to(planes), ss, ls, pred, ref, mask, qd, self.to(ops['query']), self.to(ops['addend']), f_so,
                                   self.to(ops['b_so']), f_aw, self.to(ops['b_aw']), P, c['d0'], c['dstep'], bev_w,
                                   min(w for _, w in c['shapes']), slots)
        torch.cuda.synchronize()
        return slots.cpu()

    def ws_bytes(self, B, Ncam, S, M, Dh, Q, HS, L, P, level_hw, Za=None):
        return self.c.da_cross_attn_bwd_ws_bytes(B, Ncam, S, M, Dh, Q, HS, L, P, level_hw, Za)

    def bwd_planes_supported(self, *a):
        return self.c.da_cross_attn_bwd_planes_supported(*a)

    def bwd(self, entry, c, src, offsets, attn, Dh, HS, head_minor=0, bev_w=0, det=False, prefill=None):
        """entry 'bwd' | 'ws' | 'ws_grid' | 'planes'; det: the _ex entry with the deterministic flag; -> (gv rows, gd, go, ga)"""
        import fb_bev_amd
        prefill = prefill or {}
        if entry == 'planes':
            BN, M, S, _ = src.shape
        else:
            BN, S, M, _ = src.shape
        dev = self.device
        gv = torch.full((BN, S, M, HS), float(prefill.get('gv', 0.0)), device=dev)
        gd = torch.full(c['pred_depth'].shape, float(prefill.get('gd', 0.0)), device=dev)
        go = torch.full(offsets.shape, float(prefill.get('go', 0.0)), device=dev)
        ga = torch.full(attn.shape, float(prefill.get('ga', 0.0)), device=dev)
        ss, ls, pred, ref, mask, qd = self._geo(c)
        level_hw = [tuple(x) for x in c['shapes']]
        fb_bev_amd.set_deterministic(True if det else False)
        try:
            if entry == 'planes':
                self.c.da_cross_attn_bwd_planes(self.to(src), ss, ls, pred, ref, mask, qd, self.to(offsets), self.to(attn),
                                                self.to(c['grad_slots']), c['d0'], c['dstep'], head_minor, HS, gv, gd, go, ga, level_hw, bev_w)
            else:
                self.c.da_cross_attn_bwd(self.to(src), ss, ls, pred, ref, mask, qd, self.to(offsets), self.to(attn), self.to(c['grad_slots']),
                                         c['d0'], c['dstep'], head_minor, gv, gd, go, ga, head_dim=Dh, lds_planes=entry != 'bwd',
                                         level_hw=level_hw, bev_w=bev_w, grid_entry=entry != 'ws')
        finally:
            fb_bev_amd.set_deterministic(None)
        torch.cuda.synchronize()
        return gv.cpu(), gd.cpu(), go.cpu(), ga.cpu()


class EmuApi:
    """tests/emu/emu_capi.py: the same launchers and kernels compiled for the CPU"""
    name = 'emu'

    def __init__(self):
        sys.path.insert(0, os.path.join(HERE, 'emu'))
        import emu_capi
        self.E = emu_capi
        self.device = torch.device('cpu')

    def _geo(self, c):
        return c['ss'], c['ls'], c['pred_depth'], c['ref_cam'], c['mask'], c['qdepth']

    def fwd(self, c, rows, offsets, attn, Dh, head_minor=0, misalign=False, zero_token=None, bev_w=0):
        return self.E.da_cross_attn_fwd(rows, *self._geo(c), offsets, attn, c['d0'], c['dstep'], misalign=misalign, head_minor=head_minor,
                                        head_dim=Dh, zero_token=zero_token, bev_w=bev_w)

    def fuses_softmax(self, *a):
        return bool(self.E.lib().fbbev_da_cross_attn_fwd_zt_fuses_softmax(*a))

    def planes_of(self, rows, Dh, chunk_major=False):
        return self.E.value_rows_to_head_planes(rows, Dh, chunk_major)

    def fwd_planes_supported(self, *a):
        return bool(self.E.lib().fbbev_da_cross_attn_fwd_planes_supported(*a))

    def fwd_planes(self, c, planes, offsets, attn, head_minor=0, bev_w=0):
        code, slots = self.E.da_cross_attn_fwd_planes_on(planes, *self._geo(c), offsets, attn, c['d0'], c['dstep'], head_minor=head_minor,
                                                         bev_w=bev_w, min_level_width=min(w for _, w in c['shapes']))
        assert code == 0, code
        return slots

    def fused_supported(self, *a):
        return bool(self.E.lib().fbbev_da_cross_attn_fused_supported(*a))

    def fused(self, c, planes, ops, P, bev_w):
        code, slots = self.E.da_cross_attn_fused(planes, *self._geo(c), ops['query'], ops['addend'], ops['w_so'], ops['b_so'], ops['w_aw'],
                                                 ops['b_aw'], P, c['d0'], c['dstep'], bev_w)
        assert code == 0, code
        return slots

    def ws_bytes(self, B, Ncam, S, M, Dh, Q, HS, L, P, level_hw, Za=None):
        arr = self.E._capi._level_hw(level_hw, L)
        if Za is not None:
            return self.E.lib().fbbev_da_cross_attn_bwd_ws_bytes_za(B, Ncam, S, M, Dh, Q, HS, L, P, int(Za), arr)
        return self.E.lib().fbbev_da_cross_attn_bwd_ws_bytes(B, Ncam, S, M, Dh, Q, HS, L, P, arr)

    def bwd_planes_supported(self, B, Ncam, S, M, Dh, L, Q, P, Za, HS, level_hw, bev_w):
        return bool(self.E.lib().fbbev_da_cross_attn_bwd_planes_supported(B, Ncam, S, M, Dh, L, Q, P, Za, HS,
                                                                           self.E._capi._level_hw(level_hw, L), int(bev_w)))

    def bwd(self, entry, c, src, offsets, attn, Dh, HS, head_minor=0, bev_w=0, det=False, prefill=None):
        level_hw = [tuple(x) for x in c['shapes']]
        code, gv, gd, go, ga = self.E.da_cross_attn_bwd_entry(
            entry, src, *self._geo(c), offsets, attn, c['d0'], c['dstep'], c['grad_slots'], Dh, HS, head_minor=head_minor,
            level_hw=level_hw, bev_w=bev_w, flags={True: self.E._capi.FLAG_DETERMINISTIC, 'flag_off': 0}.get(det), prefill=prefill)
        assert code == 0, code
        return gv, gd, go, ga


# ------------------------------------------------------------------------------------------------------------------ case table
def _fw(Dh, M=4, B=2, Ncam=4, Q=33, shapes=((4, 8), (2, 4)), P=4, Za=2, DC=5, HS=None, layout='head', head_minor=0, misalign=False,
        attn_off=0, real=False, route='unit', dtype=F32, seed=0):
    """one forward case of fbbev_da_cross_attn_fwd / _fwd_e; route: the kernel the table believes the launcher picks"""
    return dict(Dh=Dh, M=M, B=B, Ncam=Ncam, Q=Q, shapes=shapes, P=P, Za=Za, DC=DC, HS=Dh if HS is None else HS, layout=layout,
                head_minor=head_minor, misalign=misalign, attn_off=attn_off, real=real, route=route, dtype=dtype, seed=seed)


REAL_SHAPES = ((16, 44), (8, 22), (4, 11))      # the shipped pyramid: layer B's level sizes (a case takes its first L levels)

FWD_CASES = {
    # ---- channel-per-lane kernel
    'chan_dh4_m2_za2_p4': _fw(4, M=2, route='chan'),
    'chan_dh6': _fw(6, route='chan'),
    'chan_dh10_slots_at_4_bytes': _fw(10, misalign=True, route='chan'),
    'chan_dh10_odd_hs': _fw(10, HS=11, route='chan'),
    'chan_dh6_head_minor_7': _fw(6, HS=8, layout='chunk', head_minor=7, route='chan'),
}
for _dh, (_narrow, _wide) in {8: (10, 12), 10: (10, 12), 16: (18, 20), 32: (34, 36)}.items():
    # ---- unit kernel: three row layouts each (the WIDE ones with NaN in the padding floats); 264 units = two workgroups
    FWD_CASES[f'unit_dh{_dh}_narrow'] = _fw(_dh, HS=_narrow, real=True)
    FWD_CASES[f'unit_dh{_dh}_wide'] = _fw(_dh, HS=_wide, real=True)
    FWD_CASES[f'unit_dh{_dh}_chunk'] = _fw(_dh, HS=_wide, layout='chunk', head_minor=4, real=True)
for _hm in range(8):
    FWD_CASES[f'unit_dh10_head_minor_{_hm}'] = _fw(10, HS=12, layout='chunk' if _hm & 4 else 'head', head_minor=_hm, seed=10 + _hm)
FWD_CASES.update({
    # ---- unstaged attention weights
    'unit_unstaged_lp40': _fw(10, HS=12, shapes=((4, 8), (2, 4), (4, 8), (2, 4), (4, 8)), P=8, Za=4, Q=17),
    'unit_unstaged_p6_za3': _fw(10, HS=12, shapes=((4, 8),), P=6, Za=3),
    'unit_unstaged_attn_at_4_bytes': _fw(10, HS=12, attn_off=1),
    'unit_staged_lp36': _fw(8, HS=8, shapes=((4, 8), (2, 4)) * 4 + ((4, 8),), P=4, Za=4, Q=17),
    # ---- anchors
    'unit_za1': _fw(8, P=8, Za=1), 'unit_za2': _fw(8, P=8, Za=2), 'unit_za4': _fw(8, P=8, Za=4), 'unit_za8': _fw(8, P=8, Za=8, Q=17),
    # ---- unit counts
    'unit_count_160': _fw(10, HS=12, B=1, Q=20, M=8),
    'unit_count_592': _fw(10, HS=12, B=2, Q=37, M=8),
    'unit_count_2400_padding_workgroups': _fw(8, HS=8, B=1, Q=300, M=8, shapes=((4, 8),), Ncam=2),
})
for _dt, _tag in ((torch.bfloat16, 'bf16'), (torch.float16, 'fp16')):
    for _dh, _hs in {8: 16, 10: 16, 16: 24, 32: 40}.items():
        FWD_CASES[f'e_{_tag}_dh{_dh}'] = _fw(_dh, HS=_hs, layout='chunk', head_minor=4, dtype=_dt, seed=3)


def _zt(Dh, L, P, Q, bev_w, logits, B=1, Ncam=4, M=8, real=False, seed=0, Za=4, head_minor=5, pipe=True):
    shapes = (((4, 8), (2, 4)) * 5)[:L]
    return dict(Dh=Dh, M=M, B=B, Ncam=Ncam, Q=Q, shapes=shapes, P=P, Za=Za, DC=5, HS=(Dh + 3) // 4 * 4, bev_w=bev_w, logits=logits, real=real,
                seed=seed, head_minor=head_minor, pipe=pipe)


ZT_CASES = {
    'zt_dh8_lp8_linear': _zt(8, 1, 8, 37, 0, False, real=True),
    'zt_dh10_lp8_linear_logits': _zt(10, 1, 8, 37, 0, True),
    'zt_dh10_lp16_grid5x7': _zt(10, 2, 8, 35, 7, False, real=True),
    'zt_dh8_lp16_grid5x7_logits': _zt(8, 2, 8, 35, 7, True),
    'zt_dh8_lp32_grid8x16': _zt(8, 4, 8, 128, 16, False),
    'zt_dh10_lp32_grid8x16_logits': _zt(10, 4, 8, 128, 16, True),
    'zt_dh10_lp36_grid12x25': _zt(10, 9, 4, 300, 25, False, Ncam=2),
    'zt_dh8_lp36_linear_logits': _zt(8, 9, 4, 37, 0, True),
    'zt_dh10_m4_linear': _zt(10, 2, 8, 70, 0, False, M=4),
    # outside the preconditions (two anchors): the row kernels on the same buffer
    'zt_fallback_za2': _zt(10, 2, 8, 37, 0, False, Za=2, pipe=False),
}


def _pl(Dh, Q, bev_w, shapes=((4, 8), (2, 4)), B=2, Ncam=4, real=False, seed=0, head_minor=0):
    return dict(Dh=Dh, M=8, B=B, Ncam=Ncam, Q=Q, shapes=shapes, P=8, Za=4, DC=5, bev_w=bev_w, real=real, seed=seed, head_minor=head_minor)


PLANES_CASES = {
    'planes_dh8_list_q70': _pl(8, 70, 0, real=True),
    'planes_dh10_list_q70_three_levels': _pl(10, 70, 0, shapes=((4, 8), (2, 4), (2, 2)), real=True),
    'planes_dh8_grid5x11': _pl(8, 55, 11),
    'planes_dh10_grid5x11_head_minor_3': _pl(10, 55, 11, head_minor=3),
}


def _fu(Dh, shapes, bh, bw, B=1, Ncam=4, period=None, row_pad=0, seed=0):
    return dict(Dh=Dh, M=8, B=B, Ncam=Ncam, Q=bh * bw, shapes=shapes, P=8, Za=4, DC=5, bev_w=bw, period=period, row_pad=row_pad, seed=seed)


FUSED_CASES = {
    'fused_dh8_l1_grid5x7': _fu(8, ((4, 8),), 5, 7),
    'fused_dh10_l2_grid9x8': _fu(10, ((4, 8), (2, 4)), 9, 8, B=2, period=72),
    'fused_dh8_l3_grid16x16': _fu(8, ((8, 8), (4, 8), (2, 4)), 16, 16),
    'fused_dh10_l4_grid5x7_row_stride': _fu(10, ((4, 8), (2, 4), (4, 8), (2, 4)), 5, 7, B=2, row_pad=4, period=35),
    # the LDS staging boundary at Dh = 10: 176 tokens = 1 760 floats are staged, 184 are not
    'fused_dh10_coarse_8x22_staged': _fu(10, ((16, 32), (8, 22)), 5, 7, Ncam=2),
    'fused_dh10_coarse_8x23_not_staged': _fu(10, ((16, 32), (8, 23)), 5, 7, Ncam=2),
}


def _bw(entry, Dh, M=4, B=2, Ncam=4, Q=33, shapes=((4, 8), (2, 4)), P=4, Za=2, DC=5, HS=None, head_minor=0, bev_w=0, det=False,
        route=None, seed=0, planes=False, real_params=None):
    return dict(entry=entry, Dh=Dh, M=M, B=B, Ncam=Ncam, Q=Q, shapes=shapes, P=P, Za=Za, DC=DC, HS=Dh if HS is None else HS,
                head_minor=head_minor, bev_w=bev_w, det=det, route=route, seed=seed, planes=planes, real_params=real_params)


OWNED = dict(B=2, Ncam=6, M=8, P=8, Za=4, shapes=((4, 8), (2, 4), (2, 2)), Q=40)          # 3 regions * 2 * 6 * 8 = 288 planes >= 256
BWD_CASES = {}
for _dh, _hs in ((4, 4), (8, 10), (10, 10), (16, 18)):
    BWD_CASES[f'atomic16_dh{_dh}'] = _bw('bwd', _dh, HS=_hs, route='atomic')
for _dh in (20, 32):
    BWD_CASES[f'atomic32_dh{_dh}'] = _bw('bwd', _dh, HS=_dh + 2, route='atomic', Q=17)
for _hm in range(8):
    BWD_CASES[f'atomic16_dh10_head_minor_{_hm}'] = _bw('bwd', 10, HS=12, head_minor=_hm, route='atomic', seed=20 + _hm)
for _dh, _hs in ((4, 4), (8, 8), (10, 12), (16, 16)):
    BWD_CASES[f'chunked_dh{_dh}_one_region'] = _bw('ws', _dh, HS=_hs, route='chunked')
BWD_CASES.update({
    'chunked_q300_two_chunks': _bw('ws', 8, HS=8, B=1, M=8, Q=300, Ncam=2, shapes=((4, 8),), route='chunked'),
    # 717 tokens fit a 68 KB plane at HS = 12: two bands of 22 and 10 rows of the 32 x 32 level, then the 4 x 8 level; with the pre-pass
    'chunked_regions_prepass': _bw('ws_grid', 10, HS=12, route='chunked', shapes=((32, 32), (4, 8)), P=4, Za=4,
                                   real_params=dict(shapes=((36, 30), (4, 6)))),         # layer B: bands of 23 and 13 rows, then the 4 x 6 level
    'chunked_za8_owned_declines': _bw('ws_grid', 8, HS=8, P=8, Za=8, route='chunked', Q=17, **{k: OWNED[k] for k in ('B', 'Ncam', 'M', 'shapes')}),
    'chunked_head_minor_7': _bw('ws', 10, HS=12, head_minor=7, route='chunked'),
    # ---- owned planes: 288 planes, the default switch-over
    'owned_dh10_list': _bw('ws', 10, HS=12, route='owned', **OWNED),
    'owned_dh8_grid5x8': _bw('ws_grid', 8, HS=8, bev_w=8, route='owned', **OWNED),
    'owned_dh10_grid5x8_chunk_rows': _bw('ws_grid', 10, HS=12, head_minor=5, bev_w=8, route='owned', **OWNED),
    'owned_level_one_token_wide': _bw('ws_grid', 10, HS=12, bev_w=8, route='owned_rows', real_params=dict(shapes=((16, 44), (8, 22), (4, 1))),
                                       **dict(OWNED, shapes=((4, 8), (2, 4), (4, 1)))),
    # 1 442 tokens fit a 136 KB plane at HS = 12: two bands of 16 rows; 2 * 2 * 8 * 8 = 256 planes
    'owned_level_32x88_bands': _bw('ws_grid', 10, HS=12, bev_w=5, route='owned', B=2, Ncam=8, M=8, P=8, Za=4, Q=20, shapes=((32, 88),), seed=5,
                                    real_params=dict(shapes=((32, 88),), Ncam=8)),
    # ---- the same owned shapes on the forward's head planes
    'planes_dh10_grid5x8': _bw('planes', 10, HS=12, bev_w=8, route='owned', planes=True, **OWNED),
    'planes_dh8_grid5x8': _bw('planes', 8, HS=8, bev_w=8, route='owned', planes=True, **OWNED),
    # ---- the flags-word entries, deterministic
    'det_atomic_dh20': _bw('bwd', 20, HS=22, det=True, route='atomic', Q=17),
    'det_atomic_m6_dh6': _bw('bwd', 6, M=6, HS=6, det=True, route='atomic'),
    'det_ws_grid_chunked': _bw('ws_grid', 10, HS=12, det=True, route='chunked'),
    'det_ws_grid_owned': _bw('ws_grid', 10, HS=12, bev_w=8, det=True, route='owned', **OWNED),
    'det_planes': _bw('planes', 10, HS=12, bev_w=8, det=True, route='owned', planes=True, **OWNED),
})


# ------------------------------------------------------------------------------------------------------------------ checks
_CACHE = {}


def _case_for(kind, p, real):
    """inputs + float64 reference of a table entry, built once per process and shared (never modified by the checks)"""
    key = (kind, real, p['seed'], p['B'], p['Ncam'], p['Q'], p['M'], p['Dh'], p['shapes'], p['P'], p['Za'], p['DC'], kind == 'zt')
    if key not in _CACHE:
        if real:
            c = real_case(100 + p['seed'], p['B'], p['Ncam'], p['Q'], p['M'], p['Dh'], p['shapes'], p['P'], p['Za'], p['DC'])
        else:
            c = dyadic_case(p['seed'], p['B'], p['Ncam'], p['Q'], p['M'], p['Dh'], p['shapes'], p['P'], p['Za'], p['DC'],
                            attn_uniform=kind == 'zt')
        _CACHE[key] = c
    return _CACHE[key]


def _ref(c):
    if 'ref' not in c:
        with torch.no_grad():
            c['ref'] = reference(c['value'], c['ss'], c['ls'], c['pred_depth'], c['ref_cam'], c['mask'], c['qdepth'], c['offsets'], c['attn'],
                                 c['d0'], c['dstep'])
    return c['ref']


def _assert_exact(tag, got, c):
    exp, S = _ref(c)
    check_representable(c, S)
    assert not torch.isnan(got).any(), tag
    bad = (got.double() != exp).sum().item()
    assert bad == 0, f'{tag}: {bad} of {exp.numel()} slots differ from the float64 reference, max|diff| = {(got.double() - exp).abs().max().item():.3e}'
    observed(f'{tag}: layer A, {exp.numel()} slots bit-equal')


def _assert_bound(tag, got, c):
    exp, S = _ref(c)
    if 'T' not in c:
        c['T'] = position_term(c)
    L, P = c['attn'].shape[3], c['attn'].shape[4]
    bound = forward_c(L, P, c['mask'].shape[0]) * S + c['T']
    err = (got.double() - exp).abs()
    assert not torch.isnan(got).any(), tag
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    observed(f'{tag}: layer B max err/bound = {ratio:.3f} (max|err| = {err.max().item():.3e}, c = {forward_c(L, P, c["mask"].shape[0]) / U24:.0f} u, '
             f'T share of the bound at the worst component = {(c["T"] / bound.clamp(min=1e-300)).flatten()[(err / bound.clamp(min=1e-300)).argmax()].item():.2f})')
    assert (err <= bound).all(), f'{tag}: err/bound = {ratio:.3f}'
    return ratio


def fwd_route(p):
    """The kernel the table expects da_fwd_rows to pick, restated from its documented conditions.  The library reports nothing about
    its forward row kernels (nor about staged against unstaged weights), so this only keeps the table consistent with itself: it is
    NOT a route assertion.  Both kernels compute the same bits, so a unit case sent to the channel kernel would stay green here; the
    forward groups whose route the library does report are fwd_zt (_fuses_softmax) and the _supported probes."""
    if p['dtype'] != F32:
        return 'unit'
    al8 = not p['misalign']
    return 'unit' if al8 and p['HS'] % 2 == 0 and p['Dh'] in (8, 10, 16, 32) else 'chan'


def check_fwd(api, name, real=False):
    p = FWD_CASES[name]
    assert fwd_route(p) == p['route'], name
    c = _case_for('fwd', _real_params(p) if real else p, real)
    rows = pack_rows(c['value'], p['HS'], chunk_major=p['layout'] == 'chunk', dtype=p['dtype'])
    offsets = to_layout(c['offsets'], p['head_minor'] & 1, True)
    attn = to_layout(c['attn'], p['head_minor'] & 2, False)
    if p['attn_off']:
        attn = at_float_offset(attn, p['attn_off'])
    got = api.fwd(c, rows, offsets, attn, p['Dh'], head_minor=p['head_minor'], misalign=p['misalign'])
    tag = f'fwd{"_e" if p["dtype"] != F32 else ""} {name} [{api.name}]'
    return _assert_bound(tag, got, c) if real else _assert_exact(tag, got, c)


def check_zt(api, name, real=False):
    p = _real_params(ZT_CASES[name]) if real else ZT_CASES[name]
    c = _case_for('zt', p, real)
    L = len(c['shapes'])
    S = int(c['value'].shape[1])
    fuses = api.fuses_softmax(p['B'], c['mask'].shape[0], S, p['M'], p['Dh'], L, p['Q'], p['P'], p['Za'], p['head_minor'], p['HS'])
    assert fuses == p['pipe'], name
    rows = pack_rows(c['value'], p['HS'], chunk_major=bool(p['head_minor'] & 4))
    offsets = to_layout(c['offsets'], p['head_minor'] & 1, True)
    attn = c['logits'] if p['logits'] else c['attn']
    hm = p['head_minor'] | (0x10 if p['logits'] else 0)
    got = api.fwd(c, rows, offsets, attn, p['Dh'], head_minor=hm, zero_token=0.0, bev_w=p['bev_w'])
    tag = f'fwd_zt {name} [{api.name}]'
    if real:
        return _assert_bound(tag, got, c)
    _assert_exact(tag, got, c)
    if not p['pipe']:          # the fallback: the same bits as the row entry on the same operands
        assert torch.equal(got, api.fwd(c, rows, offsets, attn, p['Dh'], head_minor=hm)), name
    elif not p['logits']:      # padded corners and out-of-image samples really read the zero token
        poisoned = api.fwd(c, rows, offsets, attn, p['Dh'], head_minor=hm, zero_token=1.0, bev_w=p['bev_w'])
        assert not torch.equal(poisoned, got), f'{name}: a poisoned zero token changes nothing'


def check_fwd_planes(api, name, real=False):
    p = _real_params(PLANES_CASES[name]) if real else PLANES_CASES[name]
    c = _case_for('planes', p, real)
    S = int(c['value'].shape[1])
    assert api.fwd_planes_supported(p['B'], c['mask'].shape[0], S, p['M'], p['Dh'], len(c['shapes']), p['Q'], p['P'], p['Za'])
    planes = api.planes_of(pack_rows(c['value'], (p['Dh'] + 3) // 4 * 4), p['Dh'])
    assert torch.equal(planes, c['value'].permute(0, 2, 1, 3))
    offsets = to_layout(c['offsets'], p['head_minor'] & 1, True)
    attn = to_layout(c['attn'], p['head_minor'] & 2, False)
    got = api.fwd_planes(c, planes, offsets, attn, head_minor=p['head_minor'], bev_w=p['bev_w'])
    tag = f'fwd_planes {name} [{api.name}]'
    return _assert_bound(tag, got, c) if real else _assert_exact(tag, got, c)


def check_fused(api, name, dtype=F32):
    p = FUSED_CASES[name]
    base = _case_for('fused', p, False)
    key = ('ops', name)
    if key not in _CACHE:
        _CACHE[key] = fused_operands({k: v for k, v in base.items() if k not in ('ref', 'T')}, p['seed'] + 7, p['M'], p['Dh'],
                                     row_pad=p['row_pad'], period=p['period'])
    c, ops = _CACHE[key]
    S = int(c['value'].shape[1])
    assert api.fused_supported(p['B'], c['mask'].shape[0], S, p['M'], p['Dh'], len(c['shapes']), p['Q'], p['P'], p['Za'], p['bev_w'])
    planes = c['value'].permute(0, 2, 1, 3).contiguous().to(dtype)
    assert torch.equal(planes.float(), c['value'].permute(0, 2, 1, 3))              # 16-bit planes hold the same integers
    got = api.fused(c, planes, ops, p['P'], p['bev_w'])
    _assert_exact(f'fused{"_e " + str(dtype)[6:] if dtype != F32 else ""} {name} [{api.name}]', got, c)


FUSED_REAL = ['fused_dh8_l1_grid5x7', 'fused_dh10_l2_grid9x8', 'fused_dh8_l3_grid16x16']


def check_fused_real(api, name, dtype=F32):
    """layer B of one fused case: inside (c + rho) * S + T, and at least 30 times closer to the exact result than the same
    computation on plain bf16-rounded query and weights (the project's bar for split-operand kernels).  16-bit planes: the tokens
    are rounded to the type first, the reference samples those."""
    p = _real_params(FUSED_CASES[name])
    key = ('fused_real', name, dtype)
    if key not in _CACHE:
        c, ops, doff, rho, plain = fused_real_case(200 + p['seed'], p['B'], p['Ncam'], p['Q'], p['M'], p['Dh'], p['shapes'], p['P'], p['Za'],
                                                   p['DC'], row_pad=p['row_pad'], period=p['period'])
        c['value'] = c['value'].to(dtype).float()
        exp, S = _ref(c)
        T = position_term(c, doff=doff)
        L = len(p['shapes'])
        bound = (forward_c(L, p['P'], p['Ncam']) + rho.repeat_interleave(p['Dh'], -1)) * S + T
        with torch.no_grad():
            low, _ = reference(c['value'], c['ss'], c['ls'], c['pred_depth'], c['ref_cam'], c['mask'], c['qdepth'], plain['offsets'],
                               plain['attn'], c['d0'], c['dstep'])
        _CACHE[key] = (c, ops, bound, (low - exp).abs().max().item())
    c, ops, bound, err_bf16 = _CACHE[key]
    exp, S = _ref(c)
    assert api.fused_supported(p['B'], p['Ncam'], int(c['value'].shape[1]), p['M'], p['Dh'], len(p['shapes']), p['Q'], p['P'], p['Za'], p['bev_w'])
    planes = c['value'].permute(0, 2, 1, 3).contiguous().to(dtype)
    got = api.fused(c, planes, ops, p['P'], p['bev_w'])
    assert not torch.isnan(got).any()
    err = (got.double() - exp).abs()
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    gain = err_bf16 / max(err.max().item(), 1e-300)
    observed(f'fused{"_e " + str(dtype)[6:] if dtype != F32 else ""} {name} [{api.name}]: layer B max err/bound = {ratio:.3f}, max|err| = '
             f'{err.max().item():.3e}, bf16-operand error / error = {gain:.0f}')
    assert ratio <= 1.0, ratio
    assert gain >= 30, gain
    return ratio, gain


def bwd_route(api, p, S):
    """'atomic' | 'chunked' | 'owned' from what the library reports: the workspace of the route a launch with Za anchors takes
    against the maximum over both LDS-plane routes (0: no LDS-plane route)"""
    L = len(p['shapes'])
    hw = [tuple(x) for x in p['shapes']]
    za = api.ws_bytes(p['B'], p['Ncam'], S, p['M'], p['Dh'], p['Q'], p['HS'], L, p['P'], hw, Za=p['Za'])
    if za == 0:
        return 'atomic'
    # the owned plan's workspace starts with B * Ncam * Q hit records of 64 bytes; the chunked plan's with partial planes
    # B * M * chunks * Ncam * S * HS floats: told apart through the probe of the other anchor count (the owned plan needs Za <= 4)
    za8 = api.ws_bytes(p['B'], p['Ncam'], S, p['M'], p['Dh'], p['Q'], p['HS'], L, p['P'], hw, Za=8)
    if p['Za'] <= 4 and za != za8:
        return 'owned'
    return 'chunked'


BWD_REAL = [f'chunked_dh{d}_one_region' for d in (4, 8, 10, 16)] + [
    'chunked_q300_two_chunks', 'owned_dh10_list', 'owned_dh8_grid5x8', 'owned_dh10_grid5x8_chunk_rows', 'planes_dh10_grid5x8',
    'planes_dh8_grid5x8', 'chunked_regions_prepass', 'chunked_za8_owned_declines', 'owned_level_one_token_wide', 'owned_level_32x88_bands']


def _real_params(p):
    """layer B runs a table entry at the shipped level sizes, six cameras (hit counts 0-6) and seven depth bins; a case whose own
    level sizes (or camera count) are its point names them in its 'real_params' field"""
    d = dict(p, Ncam=6, DC=7, shapes=REAL_SHAPES[:len(p['shapes'])])
    d.update(p.get('real_params') or {})
    return d


def chunk_queries(api, p, S):
    """queries per chunk of the chunked scatter, restated from da_bwd_tile_plan under the default knobs (two workgroups per CU in one
    round, a whole number of 256- or 512-thread passes) and checked against the workspace the library reports: B * M * chunks
    partial planes of Ncam * S * HS floats, plus the pre-pass records (8 floats per (sample, camera, query)) with several regions"""
    B, M, Q = p['B'], p['M'], p['Q']
    want = min(max(-(-512 // (B * M)), 1), 256)
    qpc = -(-Q // want)
    threads = 512 if qpc >= 512 else 256
    qpc = -(-qpc // threads) * threads
    chunks = -(-Q // qpc)
    part = -(-(B * M * chunks * p['Ncam'] * S * p['HS'] * 4) // 256) * 256
    ws = api.ws_bytes(B, p['Ncam'], S, M, p['Dh'], Q, p['HS'], len(p['shapes']), p['P'], [tuple(x) for x in p['shapes']], Za=p['Za'])
    assert ws in (part, part + B * p['Ncam'] * Q * 8 * 4), (ws, part, chunks)
    return qpc


def _run_bwd(api, name, p, c, expect_route):
    """one backward case on the adapter -> (tag, route, the four gradients in the logical layouts, grad_value's padding channels)"""
    S = int(c['value'].shape[1])
    qi = bool(p['head_minor'] & 4)
    entry = p['entry']
    hw = [tuple(x) for x in p['shapes']]
    route = 'atomic' if entry == 'bwd' else bwd_route(api, p, S)
    if entry == 'bwd' and p['det']:
        # the wrapper's deterministic mode takes an LDS-plane route wherever one plans the shape: fbbev_da_cross_attn_bwd_ex is
        # reached only where the library reports none
        assert api.ws_bytes(p['B'], p['Ncam'], S, p['M'], p['Dh'], p['Q'], p['HS'], len(hw), p['P'], hw, Za=p['Za']) == 0, name
    assert route == (expect_route or p['route'].split('_')[0]), (name, route)
    if route == 'owned' and p['M'] == 8 and p['Za'] == 4 and p['bev_w']:
        # the unit gradients: k_da_bwd_unit_planes unless a level is one token wide ('owned_rows': k_da_cross_attn_bwd_unit)
        planes_unit = api.bwd_planes_supported(p['B'], p['Ncam'], S, p['M'], p['Dh'], len(hw), p['Q'], p['P'], p['Za'], p['HS'], hw, p['bev_w'])
        assert planes_unit == (p['route'] != 'owned_rows'), (name, planes_unit)
    if entry == 'planes':
        assert p['route'] == 'owned'
    offsets = to_layout(c['offsets'], p['head_minor'] & 1, True)
    attn = to_layout(c['attn'], p['head_minor'] & 2, False)
    if entry == 'planes':
        src = c['value'].permute(0, 2, 1, 3).contiguous()
        prefill = dict(gv=float('nan'), go=float('nan'), ga=float('nan'))
    else:
        src = pack_rows(c['value'], p['HS'], chunk_major=qi, pad=0.0)
        prefill = dict(gv=float('nan')) if route != 'atomic' else {}
    gv, gd, go, ga = api.bwd(entry, c, src, offsets, attn, p['Dh'], p['HS'], head_minor=p['head_minor'], bev_w=p['bev_w'], det=p['det'],
                             prefill=prefill)
    gv_l, gv_pad = unpack_rows(gv, p['Dh'], chunk_major=qi)
    tag = f'{ {"bwd": "bwd", "ws": "bwd_ws", "ws_grid": "bwd_ws_grid", "planes": "bwd_planes"}[entry]}{"_ex" if p["det"] else ""} {name} [{api.name}]'
    grads = dict(grad_value=gv_l, grad_pred_depth=gd, grad_offsets=from_layout(go, p['head_minor'] & 1, True),
                 grad_attn=from_layout(ga, p['head_minor'] & 2, False))
    for what, got in grads.items():
        assert not torch.isnan(got).any(), f'{tag}: NaN left in {what}'
    if gv_pad.numel():
        assert (gv_pad == 0).all(), f'{tag}: padding channels of grad_value are not zero'
    return tag, route, grads


def check_bwd(api, name, expect_route=None, det=None):
    """layer A of one backward case: the four gradients against float64 autograd of the reference, bit for bit.  expect_route: the
    route under a knob, where it differs from the table's.  det='flag_off' (emulator adapter only): the _ex entry without its flag."""
    p = BWD_CASES[name]
    p = p if det is None else dict(p, det=det)
    c = _case_for('bwd', p, False)
    tag, route, grads = _run_bwd(api, name, p, c, expect_route)
    if 'grads' not in c:
        c['grads'] = reference_backward(c, c['grad_slots'])
    for (what, got), exp in zip(grads.items(), c['grads']):
        bad = (got.double() != exp).sum().item()
        assert bad == 0, f'{tag}: {bad} of {exp.numel()} words of {what} differ, max|diff| = {(got.double() - exp).abs().max().item():.3e}'
    observed(f'{tag}: layer A, four gradients bit-equal ({route})')


def check_bwd_real(api, name):
    """layer B of one LDS-plane backward case: the four gradients inside the bounds of `backward_bounds`"""
    p = _real_params(BWD_CASES[name])
    c = _case_for('bwd', p, True)
    tag, route, grads = _run_bwd(api, name, p, c, None)
    if 'grads' not in c:
        c['grads'] = reference_backward(c, c['grad_slots'])
        c['gbounds'] = backward_bounds(c, route, chunk_queries(api, p, int(c['value'].shape[1])) if route == 'chunked' else p['Q'])
    worst = {}
    for (what, got), exp in zip(grads.items(), c['grads']):
        err, bound = (got.double() - exp).abs(), c['gbounds'][what]
        assert bound.shape == exp.shape, (what, bound.shape, exp.shape)
        worst[what] = (err / bound.clamp(min=1e-300)).max().item()
    observed(f'{tag}: layer B max err/bound ' + ', '.join(f'{k[5:]} = {v:.4f}' for k, v in worst.items()) + f' ({route})')
    for what, r in worst.items():
        assert r <= 1.0, f'{tag}: {what} err/bound = {r:.3f}'
    return worst


# ------------------------------------------------------------------------------------------------------------------ knobs
# Knobs the product build reads once per process: each setting runs the layer-A cases it bears on (the GPU test starts one child
# process per setting, the emulator build re-reads the knobs on every call)
_ONE_REGION = [f'chunked_dh{d}_one_region' for d in (4, 8, 10, 16)]
KNOB_RUNS = {
    'fused_hw8': ({'FBBEV_DA_FUSED_HW': '8'}, [('fused', n, None) for n in FUSED_CASES]),
    'pipe_wps3': ({'FBBEV_DA_PIPE_WPS': '3'}, [('zt', n, None) for n in ZT_CASES]),
    # the owned plan wherever the shape allows it, whatever the number of planes (M = 4: the row kernel's unit gradients)
    'bwd_owned1': ({'FBBEV_DA_BWD_OWNED': '1'}, [('bwd', n, 'owned') for n in _ONE_REGION + ['chunked_q300_two_chunks']] +
                   [('bwd', 'chunked_za8_owned_declines', 'chunked')]),
    # never the owned plan: the 288-plane shapes through the chunked scatter
    'bwd_owned0': ({'FBBEV_DA_BWD_OWNED': '0'}, [('bwd', n, 'chunked') for n in ('owned_dh10_list', 'owned_dh8_grid5x8',
                                                                                 'owned_dh10_grid5x8_chunk_rows', 'owned_level_one_token_wide')]),
    # 16 tokens per plane: the 4 x 8 level in two bands of two rows, on both routes
    'bwd_tokens16': ({'FBBEV_DA_BWD_TOKENS': '16'}, [('bwd', n, None) for n in _ONE_REGION + ['owned_dh10_list', 'owned_dh8_grid5x8',
                                                                                             'planes_dh10_grid5x8']]),
}


def run_knob(api, key):
    """the cases of one knob setting; the caller has set the environment"""
    env, runs = KNOB_RUNS[key]
    for k, v in env.items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    for kind, name, route in runs:
        if kind == 'fused':
            check_fused(api, name)
        elif kind == 'zt':
            check_zt(api, name)
        else:
            check_bwd(api, name, expect_route=route)
    return len(runs)
