"""Case table, input generators, references and checks for fbbev_occ_loss_stats / fbbev_occ_loss_grad (fb_bev_amd/csrc/occ_loss_kernels.h),
shared by the emulator test (tests/test_emu_occ_loss.py, through tests/emu/emu_capi.py's library) and the GPU test
(tests/test_gpu_occ_loss.py, through fb_bev_amd._capi.occ_loss_stats / occ_loss_grad).

Logits are N(0, 3) from a seeded generator with planted voxels: a NaN, a +inf and a -inf among the classes, a row of NaN only, a row
whose classes are all equal, and a row with one class 40 above the rest (p saturates).  Label sets: 'uniform' (every class, 4 % set
to 255), 'absent' (only the last classes occur), 'single' (one class in exactly one voxel), 'skewed' (95 % empty_idx), 'all255'.

Layers of every check:
  1. counts: stats_i equals a numpy bincount bit for bit.
  2. exact floats (EXACT_CASES: C = 16 and 32, a voxel's logits constant over its classes): p = 1/C exactly, so P, N, Q and G must
     equal count / C resp. count (C - 1) / C bit for bit.
  3. real floats: every statistic against its float64 restatement at 2e-5 |ref| + 1e-6 (the bar of tests/test_occ_modules.py for
     these losses; all terms are non-negative, so a relative bar is meaningful).
  4. gradient: for a seeded random grad_stats with entries of both signs, |got - ref64| <= RHO * A elementwise, A = the float64 sum
     of the absolute values of the element's contributions (softmax part and CLS part); where A == 0 (a voxel labelled 255, a
     non-finite input) the gradient must be exactly 0.
     RHO is measured, not derived (the device's expf / logf error is not documented): the parent of the kernel is fp32 torch
     autograd of the same formula on the CPU; `python tests/occ_loss_cases.py` evaluates it on this table's inputs and prints its
     worst err / A against float64, per mode.  Observed: 1.921e-06 (cross entropy; b2_8x8x16_padded, uniform labels) and 5.787e-05
     (focal; the same case: at a logit of +-9 and beyond, 1 - sigmoid(x) in fp32 keeps three digits, and the term it scales is
     all of that element's A).  RHO = 4 x the mode's worst: 7.684e-06 and 2.315e-04, both above the floor 2^-20 = 9.54e-07; the
     margin covers another summation order and a device libm a few ulp off the host's.  These figures were taken on the table
     before the four grid-stride cases joined it and RHO has stayed where they put it: with those cases the parent's own worst is
     1.921e-06 and 3.142e-04 (the focal tail grows with the number of voxels drawn), which would have set a wider focal bound.
     The kernels' own worst err / A over the whole table: 1.921e-06 (cross entropy) and 1.415e-05 (focal), the same on the MI355X
     and on the emulator; their worst statistic sits at 0.012 of layer 3's bar (profiles/r15_occ_loss_observed.txt).
  5. guard words around grad_logits, stats_f, stats_i and the workspace come back intact; logits and labels come back unwritten.

Plain Python, numpy and CPU torch only; the adapters import their library on first use.
"""
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # `python tests/occ_loss_cases.py` finds the package

GUARD = 16                       # guard words in front of and behind every output
PATTERN = 7.5
IPATTERN = -1234567
RHO = {False: 4 * 1.921e-06, True: 4 * 5.787e-05}      # by mode (focal?), see the header; never below 2 ** -20
assert min(RHO.values()) >= 2.0 ** -20
GAMMA, ALPHA = 2.0, 0.25


def observed(text):
    print(f'[observed] {text}')


def _case(name, B, C, H, W, D, layout, e=None, padded=False):
    return dict(name=name, B=B, C=C, H=H, W=W, D=D, layout=layout, e=C - 1 if e is None else e, padded=padded)


def _both(name, *shape, **kw):
    return [_case(f'{name}_cl', *shape, 'cl', **kw), _case(f'{name}_planes', *shape, 'planes', **kw)]


# tile of the kernels: 8 x 8 columns x the whole depth at D >= 16 (16 x 16 below, depth chunks of 64), 256 voxels per step
CASES = (
    _both('b2_5x7x3', 2, 19, 5, 7, 3) +                         # nothing a multiple of a tile, a wave or 4
    _both('b1_16x16x16', 1, 19, 16, 16, 16) +                   # the shipped depth with whole tiles
    _both('b1_17x33x16', 1, 19, 17, 33, 16) +                   # one row and one column over
    _both('b2_8x8x16_padded', 2, 19, 8, 8, 16, padded=True) +   # padded batch stride and a non-zero storage offset
    [_case('b1_6x4x5_permuted', 1, 19, 6, 4, 5, 'permuted')] +  # a view of (B, D, C, W, H) memory: the slow stride path
    _both('n2', 1, 2, 6, 6, 4, e=1) + _both('n32', 1, 32, 6, 6, 4, e=0) +       # C at its bounds
    _both('c18', 1, 18, 9, 9, 4, e=17) +                        # sem_scal's begin = 0 branch
    _both('b1_3x9x70', 1, 19, 3, 9, 70) +                       # depth above a chunk
    [_case('b1_200x200x2_cl', 1, 19, 200, 200, 2, 'cl')] +      # the focal plane's hard-coded grid (13 x 13 tiles of 16 x 16 x 2)
    # more tiles than one pass of the grid, so that a workgroup carries its sums from tile to tile and reuses its LDS rows:
    # 1031 tiles of 8 x 8 x 16 (the last one 3 columns wide) over the statistics kernel's 1024 workgroups, and 2051 tiles of
    # 16 x 16 x 2 over the gradient kernel's 2048 (the statistics kernel walks them in three passes)
    _both('b1_1x8243x16', 1, 19, 1, 8243, 16) + _both('b1_1x32803x2', 1, 19, 1, 32803, 2)
)
CASE_IDS = [c['name'] for c in CASES]
EXACT_CASES = (_both('exact16_9x7x5', 1, 16, 9, 7, 5) + _both('exact32_b2_5x6x3', 2, 32, 5, 6, 3) +
               [_case('exact16_40x40x16_cl', 1, 16, 40, 40, 16, 'cl')] +
               _both('exact16_1x8243x16', 1, 16, 1, 8243, 16) + _both('exact32_1x32803x2', 1, 32, 1, 32803, 2))      # grid-stride, as above
STATS_BLOCKS, GRAD_BLOCKS = 1024, 2048            # the launchers' grid caps (capi.hip)


def tiles(case):
    """the launchers' tile count: 8 x 8 columns x min(D, 64) at D >= 16, 16 x 16 below"""
    TD = min(case['D'], 64)
    T = 8 if TD >= 16 else 16
    return case['B'] * -(-case['H'] // T) * -(-case['W'] // T) * -(-case['D'] // TD)


assert sum(tiles(c) > STATS_BLOCKS for c in CASES) >= 4 and sum(tiles(c) > GRAD_BLOCKS for c in CASES) >= 2
assert sum(tiles(c) > STATS_BLOCKS for c in EXACT_CASES) >= 4 and sum(tiles(c) > GRAD_BLOCKS for c in EXACT_CASES) >= 2
EXACT_IDS = [c['name'] for c in EXACT_CASES]
LABEL_KINDS = ['uniform', 'absent', 'single', 'skewed', 'all255']
REPEAT_IDS = ['b1_17x33x16_cl', 'b1_17x33x16_planes', 'b2_5x7x3_cl', 'b1_1x8243x16_cl', 'b1_1x32803x2_planes']


def by_name(name):
    return (CASES + EXACT_CASES)[(CASE_IDS + EXACT_IDS).index(name)]


def _seed(case, extra=0):
    return case['B'] * 7 + case['H'] * 131 + case['W'] * 17 + case['D'] * 3 + case['C'] * 1009 + extra


# ------------------------------------------------------------------------------------------------------------------ inputs
def logical_logits(case, exact=False):
    """(B, C, H, W, D) contiguous f32"""
    g = torch.Generator().manual_seed(_seed(case))
    B, C, H, W, D = (case[k] for k in ('B', 'C', 'H', 'W', 'D'))
    nv = B * H * W * D
    if exact:                                                        # a different multiple of 0.25 per voxel, constant over its classes
        V = (torch.randint(-40, 41, (nv, 1), generator=g).float() / 4).expand(nv, C).clone()
    else:
        V = torch.randn((nv, C), generator=g) * 3
        rows = torch.randperm(nv, generator=g)[:6].tolist()
        cls = torch.randint(0, C, (6,), generator=g).tolist()
        V[rows[0], cls[0]] = float('nan')
        V[rows[1], cls[1]] = float('inf')
        V[rows[2], cls[2]] = float('-inf')
        V[rows[3], :] = float('nan')
        V[rows[4], :] = 1.25
        V[rows[5], cls[5]] = V[rows[5]].max() + 40.0
    return V.view(B, H, W, D, C).permute(0, 4, 1, 2, 3).contiguous()


def labels(case, kind):
    """(B, H, W, D) uint8"""
    g = torch.Generator().manual_seed(_seed(case, 1))
    B, C, H, W, D, e = (case[k] for k in ('B', 'C', 'H', 'W', 'D', 'e'))
    nv = B * H * W * D
    order = torch.randperm(nv, generator=g)
    if kind == 'all255':
        return torch.full((B, H, W, D), 255, dtype=torch.uint8)
    if kind == 'absent':
        lo = max(C - 6, C // 2)
        t = torch.randint(lo, C, (nv,), generator=g, dtype=torch.uint8)
    elif kind == 'skewed':
        t = torch.randint(0, C, (nv,), generator=g, dtype=torch.uint8)
        t[order[:int(nv * 0.95)]] = e
    else:
        t = torch.randint(0, C, (nv,), generator=g, dtype=torch.uint8)
    if kind == 'single':
        one = (e + 1) % C if C > 2 else 1 - e
        t[t == one] = e
        t[order[-1]] = one
    k = max(int(nv * 0.04), 1)
    t[order[:k]] = 255                                               # (never order[-1])
    return t.view(B, H, W, D)


def lay_out(case, L, fill=PATTERN):
    """-> (storage 1-D f32, size, stride, offset): L in the case's memory layout.  'cl': the NCDHW view of channels-last memory;
    'planes': contiguous class planes; 'permuted': a view of (B, D, C, W, H) memory; padded: a slice of a bigger buffer (batch
    stride + 37, offset 5).  GUARD words of `fill` in front and behind."""
    B, C, H, W, D = L.shape
    per = C * H * W * D
    sb, off = (per + 37, GUARD + 5) if case['padded'] else (per, GUARD)
    storage = torch.full((off + B * sb + GUARD,), fill)
    if case['layout'] == 'cl':
        stride = (sb, 1, W * D * C, D * C, C)
        src = L.permute(0, 2, 3, 4, 1)
    elif case['layout'] == 'planes':
        stride = (sb, H * W * D, W * D, D, 1)
        src = L
    else:
        stride = (sb, W * H, 1, H, C * W * H)
        src = L.permute(0, 4, 1, 3, 2)
    for b in range(B):
        storage[off + b * sb: off + b * sb + per] = src[b].reshape(-1)
    return storage, tuple(L.shape), stride, off


def plane_weight(case):
    """the radial plane of CustomFocalLoss on the case's (H, W)"""
    from fb_bev_amd.occ_loss import CustomFocalLoss
    return CustomFocalLoss(bev_hw=(case['H'], case['W'])).c.float().contiguous()


def class_weight(case):
    C = case['C']
    w = 0.05 + torch.rand(C, generator=torch.Generator().manual_seed(_seed(case, 2)))
    if C == 19:
        w[0] = 0.0                                                   # occ_loss.class_weights(19): the void class weighs nothing
    return w.float()


def grad_stats(case):
    g = torch.randn(3 * case['C'] + 4, generator=torch.Generator().manual_seed(_seed(case, 3)))
    assert (g > 0).any() and (g < 0).any() and torch.isfinite(g).all()
    return g.float()


# ------------------------------------------------------------------------------------------------------------------ references
def stats_torch(L, lab, cw, plane, e, focal, dtype):
    """the statistics in plain torch at `dtype`, differentiable in L -> (stats_f (3C + 4,), stats_i (C + 1,) int64)"""
    C = L.shape[1]
    x = torch.nan_to_num(L.to(dtype), nan=0.0, posinf=0.0, neginf=0.0)
    p = F.softmax(x, dim=1)
    m = lab != 255
    mf = m.to(dtype)[:, None]
    oh = ((lab[:, None] == torch.arange(C)[None, :, None, None, None]) & m[:, None]).to(dtype)
    dims = (0, 2, 3, 4)
    P, N, Q = (p * mf).sum(dims), (p * oh).sum(dims), ((1 - p) * (mf - oh)).sum(dims)
    G = ((1 - p[:, e]) * mf[:, 0]).sum()
    w = cw.to(dtype)[None, :, None, None, None]
    if focal:                                                        # CustomFocalLoss.forward's operations
        s = x.sigmoid()
        pt = (1 - s) * oh + s * (1 - oh)
        fw = (ALPHA * oh + (1 - ALPHA) * (1 - oh)) * pt.pow(GAMMA)
        loss = F.binary_cross_entropy_with_logits(x, oh, reduction='none') * fw * w
        CLS = (loss.sum(1) * plane.to(dtype)[None, :, :, None] * mf[:, 0]).sum()
    else:
        CLS = -((w * oh).sum(1) * (F.log_softmax(x, dim=1) * oh).sum(1)).sum()
    stats_f = torch.cat([P, N, Q, G[None], CLS[None], torch.zeros(2, dtype=dtype)])
    stats_i = torch.cat([oh.sum(dims), mf.sum()[None]]).round().to(torch.int64)
    return stats_f, stats_i


def grad_ref64(L, lab, cw, plane, e, focal, gS):
    """the backward formula in float64 -> (grad (B, C, H, W, D), A: the sum of the absolute values of every element's contributions)"""
    C = L.shape[1]
    dt = torch.float64
    fin = torch.isfinite(L)
    x = torch.nan_to_num(L.to(dt), nan=0.0, posinf=0.0, neginf=0.0)
    p = F.softmax(x, dim=1)
    m = lab != 255
    mf = m.to(dt)[:, None]
    oh = ((lab[:, None] == torch.arange(C)[None, :, None, None, None]) & m[:, None]).to(dt)
    v = lambda t: t.to(dt)[None, :, None, None, None]  # noqa: E731
    gS = gS.to(dt)
    gP, gN, gQ, gG, gCLS = gS[:C], gS[C:2 * C], gS[2 * C:3 * C], gS[3 * C], gS[3 * C + 1]
    g = mf * v(gP) + oh * v(gN) - (mf - oh) * v(gQ)
    g[:, e] -= mf[:, 0] * gG
    ga = mf * v(gP).abs() + oh * v(gN).abs() + (mf - oh) * v(gQ).abs()
    ga[:, e] += mf[:, 0] * gG.abs()
    soft = p * (g - (g * p).sum(1, keepdim=True))
    a_soft = p * (ga + (ga * p).sum(1, keepdim=True))
    if focal:
        s = x.sigmoid()
        pos = -ALPHA * (1 - s) ** GAMMA * (GAMMA * s * F.softplus(-x) + (1 - s))
        neg = (1 - ALPHA) * s ** GAMMA * (GAMMA * (1 - s) * F.softplus(x) + s)
        cls = gCLS * mf * plane.to(dt)[None, None, :, :, None] * v(cw) * torch.where(oh > 0, pos, neg)
        a_cls = cls.abs()
    else:
        wt = (v(cw) * oh).sum(1, keepdim=True)
        cls = gCLS * wt * (p * mf - oh)
        a_cls = gCLS.abs() * wt * (p * mf + oh)
    zero = torch.zeros_like(x)
    return torch.where(fin, soft + cls, zero), torch.where(fin, a_soft + a_cls, zero)


_REF = {}


def reference(case, kind, focal, exact=False):
    """(L, labels, class weights, plane, grad_stats, stats_f64, stats_i, grad64, A), computed once and shared; callers leave them
    unchanged"""
    key = (case['name'], kind, focal, exact)
    if key not in _REF:
        L, lab = logical_logits(case, exact), labels(case, kind)
        cw, plane, gS = class_weight(case), plane_weight(case), grad_stats(case)
        sf, si = stats_torch(L, lab, cw, plane, case['e'], focal, torch.float64)
        grad, A = grad_ref64(L, lab, cw, plane, case['e'], focal, gS)
        ref = (L, lab, cw, plane, gS, sf, si, grad, A)
        if L.numel() > 1 << 20:                                      # a large case has one user per (label set, mode): not kept
            return ref
        _REF[key] = ref
    return _REF[key]


def parent_ratio(case, kind, focal):
    """worst err / A of the parent -- fp32 torch autograd of the same formula on the CPU -- against float64"""
    L, lab, cw, plane, gS, _, _, grad, A = reference(case, kind, focal)
    x = L.clone().requires_grad_()
    sf, _ = stats_torch(x, lab, cw, plane, case['e'], focal, torch.float32)
    (sf * gS).sum().backward()
    err = (x.grad.double() - grad).abs()
    ok = A > 0
    assert (err[~ok] == 0).all()
    return float((err[ok] / A[ok]).max()) if ok.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------ adapters
class EmuApi:
    """the C entries of the CPU-emulated library, CPU tensors"""
    name = 'emu'

    def __init__(self):
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
        import emu_capi
        self.lib = emu_capi.lib()

    def dev(self, t):
        return None if t is None else t.clone()

    def cpu(self, t):
        return t

    def ws_bytes(self, B, C, H, W, D):
        return self.lib.fbbev_occ_loss_ws_bytes(B, C, H, W, D)

    def _args(self, view, lab, cw, plane, e, focal):
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        B, C, H, W, D = view.shape
        return (p(view), *view.stride(), B, C, H, W, D, p(lab), p(cw), p(plane), e, 1 if focal else 0, GAMMA, ALPHA)

    def stats(self, view, lab, cw, plane, e, focal, stats_f, stats_i, ws):
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        return self.lib.fbbev_occ_loss_stats(*self._args(view, lab, cw, plane, e, focal), p(stats_f), p(stats_i), p(ws), ws.numel(), None)

    def grad(self, view, lab, cw, plane, e, focal, gS, out):
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        return self.lib.fbbev_occ_loss_grad(*self._args(view, lab, cw, plane, e, focal), p(gS), p(out), None)


class GpuApi:
    """fb_bev_amd._capi.occ_loss_stats / occ_loss_grad on cuda:0"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi
        self.c = _capi
        self.device = torch.device('cuda:0')

    def dev(self, t):
        return None if t is None else t.to(self.device)

    def cpu(self, t):
        return t.cpu()

    def ws_bytes(self, B, C, H, W, D):
        return self.c.lib().fbbev_occ_loss_ws_bytes(B, C, H, W, D)

    def stats(self, view, lab, cw, plane, e, focal, stats_f, stats_i, ws):
        self.c.occ_loss_stats(view, lab, cw, plane, e, focal, GAMMA, ALPHA, stats_f=stats_f, stats_i=stats_i, ws=ws)
        return 0

    def grad(self, view, lab, cw, plane, e, focal, gS, out):
        got = self.c.occ_loss_grad(view, lab, gS, cw, plane, e, focal, GAMMA, ALPHA, out=out)
        assert got is out
        return 0


def run(api, case, L, lab, cw, plane, focal, gS):
    """one forward and one backward call -> (stats_f, stats_i, grad (B, C, H, W, D) contiguous) on the CPU.  Every output is a slice
    of a larger patterned buffer whose other words must come back intact; the inputs must come back unchanged."""
    storage, size, stride, off = lay_out(case, L)
    B, C, H, W, D = size
    nf, ni = 3 * C + 4, C + 1
    d_storage = api.dev(storage)
    view = d_storage.as_strided(size, stride, off)
    d_lab, d_cw, d_plane, d_gS = api.dev(lab), api.dev(cw), api.dev(plane if focal else None), api.dev(gS)
    need = api.ws_bytes(B, C, H, W, D)
    assert need > 0 and need % 16 == 0
    bf = api.dev(torch.full((GUARD + nf + GUARD,), PATTERN))
    bi = api.dev(torch.full((GUARD + ni + GUARD,), IPATTERN, dtype=torch.int32))
    bw = api.dev(torch.full((64 + need + 64,), 0xA5, dtype=torch.uint8))
    assert api.stats(view, d_lab, d_cw, d_plane, case['e'], focal, bf[GUARD:GUARD + nf], bi[GUARD:GUARD + ni], bw[64:64 + need]) == 0
    g_storage = api.dev(torch.full_like(storage, PATTERN))
    g_view = g_storage.as_strided(size, stride, off)
    assert api.grad(view, d_lab, d_cw, d_plane, case['e'], focal, d_gS, g_view) == 0
    bf, bi, bw, g_back = api.cpu(bf), api.cpu(bi), api.cpu(bw), api.cpu(g_storage)
    assert (bf[:GUARD] == PATTERN).all() and (bf[GUARD + nf:] == PATTERN).all(), 'guard words of stats_f overwritten'
    assert (bi[:GUARD] == IPATTERN).all() and (bi[GUARD + ni:] == IPATTERN).all(), 'guard words of stats_i overwritten'
    assert (bw[:64] == 0xA5).all() and (bw[64 + need:] == 0xA5).all(), 'guard bytes of the workspace overwritten'
    inside = torch.zeros(storage.numel(), dtype=torch.bool)
    inside.as_strided(size, stride, off).fill_(True)
    assert int(inside.sum()) == L.numel()
    assert (g_back[~inside] == PATTERN).all(), 'grad_logits written outside the view'
    nn = lambda t: torch.nan_to_num(t, 1e9, 2e9, -2e9)  # noqa: E731
    assert torch.equal(nn(api.cpu(d_storage)), nn(storage)), 'the logits were written to'
    assert torch.equal(api.cpu(d_lab), lab), 'the labels were written to'
    return bf[GUARD:GUARD + nf].clone(), bi[GUARD:GUARD + ni].clone(), g_back.as_strided(size, stride, off).contiguous()


# ------------------------------------------------------------------------------------------------------------------ checks
def _names(C):
    return [f'P[{c}]' for c in range(C)] + [f'N[{c}]' for c in range(C)] + [f'Q[{c}]' for c in range(C)] + ['G', 'CLS', 'spare', 'spare']


def check(api, case, kind, focal):
    """layers 1, 3, 4 and 5 (and the all-255 rule) on one case, label set and mode"""
    L, lab, cw, plane, gS, sf, si, grad, A = reference(case, kind, focal)
    C = case['C']
    tag = f'{api.name} {case["name"]} {kind} {"focal" if focal else "ce"}'
    got_f, got_i, got_g = run(api, case, L, lab, cw, plane, focal, gS)
    # 1: counts
    t = lab.numpy().reshape(-1)
    want_i = np.append(np.bincount(t[t != 255], minlength=C)[:C], (t != 255).sum()).astype(np.int32)
    assert np.array_equal(si.numpy().astype(np.int32), want_i)
    assert np.array_equal(got_i.numpy(), want_i), (got_i.numpy(), want_i)
    if kind == 'single':
        assert (want_i[:C] == 1).sum() >= 1
    if kind == 'absent':
        assert (want_i[:C] == 0).sum() >= C // 2 - 1
    # 3: floats
    err = (got_f.double() - sf).abs()
    bar = 2e-5 * sf.abs() + 1e-6
    ratio = err / bar
    worst = {k: float(ratio[s].max()) for k, s in (('P', slice(0, C)), ('N', slice(C, 2 * C)), ('Q', slice(2 * C, 3 * C)),
                                                   ('G', slice(3 * C, 3 * C + 1)), ('CLS', slice(3 * C + 1, 3 * C + 2)))}
    observed(f'{tag}: worst err / (2e-5 |ref| + 1e-6) per statistic: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert (sf >= 0).all() and float(got_f[3 * C + 2]) == 0.0 and float(got_f[3 * C + 3]) == 0.0
    assert (err <= bar).all(), [(n, float(g), float(w)) for n, g, w, bad in zip(_names(C), got_f, sf, err > bar) if bad][:5]
    # 4: gradient
    gerr = (got_g.double() - grad).abs()
    live = A > 0
    assert (got_g[~live] == 0).all(), 'a gradient where nothing contributes (a voxel labelled 255 or a non-finite logit)'
    assert torch.isfinite(got_g).all()
    r = float((gerr[live] / A[live]).max()) if live.any() else 0.0
    observed(f'{tag}: gradient worst err / A = {r:.3e} (RHO = {RHO[focal]:.3e}), largest |grad| = {float(grad.abs().max()):.3e}')
    assert (gerr <= RHO[focal] * A).all(), r
    if kind == 'all255':
        assert (got_f == 0).all() and (got_i == 0).all() and (got_g == 0).all() and not live.any()
    else:
        assert live.any() and float(grad.abs().max()) > 0
    return got_f, got_i, got_g


def check_exact(api, case):
    """layer 2: p = 1/C exactly, every sum a multiple of 1/C below 2^24 / C"""
    C, e = case['C'], case['e']
    for kind in ('uniform', 'skewed'):
        L, lab, cw, plane, gS, sf, si, _, _ = reference(case, kind, False, exact=True)
        got_f, got_i, _ = run(api, case, L, lab, cw, plane, False, gS)
        cnt, nv = si[:C].double(), si[C].double()
        want = torch.cat([nv.expand(C) / C, cnt / C, (nv - cnt) * (C - 1) / C, (nv * (C - 1) / C)[None]]).float()
        assert torch.equal(got_i.long(), si)
        bad = int((got_f[:3 * C + 1] != want).sum())
        observed(f'{api.name} {case["name"]} {kind}: statistics that differ from count / C = {bad} of {3 * C + 1}')
        assert torch.equal(got_f[:3 * C + 1], want), (got_f[:3 * C + 1], want)


def check_repeat(api, case):
    """layer 5 of the issue: two runs, identical bytes"""
    for focal in (False, True):
        L, lab, cw, plane, gS = reference(case, 'uniform', focal)[:5]
        a, b = (run(api, case, L, lab, cw, plane, focal, gS) for _ in range(2))
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


if __name__ == '__main__':                                           # the measurement behind RHO
    worst = {False: 0.0, True: 0.0}
    for case in CASES:
        for kind in LABEL_KINDS[:4] if case['H'] < 200 else ['uniform']:
            for focal in (False, True):
                r = parent_ratio(case, kind, focal)
                worst[focal] = max(worst[focal], r)
                observed(f'parent (fp32 torch autograd, CPU) {case["name"]} {kind} {"focal" if focal else "ce"}: worst err / A = {r:.3e}')
    observed(f'parent worst err / A: ce {worst[False]:.3e}, focal {worst[True]:.3e}; 4 x worst = {4 * max(worst.values()):.3e}; '
             f'floor 2^-20 = {2.0 ** -20:.3e}')
