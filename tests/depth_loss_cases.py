"""Case table, input generators, references and checks for fbbev_depth_loss_fwd / fbbev_depth_loss_grad (fb_bev_amd/csrc/depth_loss_kernels.h),
shared by the emulator test (tests/test_emu_depth_loss.py, through tests/emu/emu_capi.py's library) and the GPU test
(tests/test_gpu_depth_loss.py, through fb_bev_amd._capi.depth_loss_fwd / depth_loss_grad).

gt is seeded: 60 % of the entries are zero, the rest uniform in [0, hi + 5]; then every third cell is made sparse (all but one or two
of its entries zeroed, as a projected lidar sweep looks: without them a cell of 16 x 16 random depths has its minimum below the first
bin and nothing would be foreground); then entries are planted, one cell each, as far as the case has cells: the exact edges
bin0 + k step for k in {1, D + 1, 0, D} and the float just below each, a -0.0, a negative value, a NaN, a +inf, a cell whose only
non-zero is out of range, and a cell whose minimum falls below bin 1 while its other entries are in range (the reference makes that
cell background).  The case step04 (a non-dyadic step) places every depth at (k + 0.5 +- 0.25) bins and plants no edges; the module
asserts at import that the fp32 division, the fp32 reciprocal-multiply and a float64 evaluation give the same bin for every cell of
it, so the case is exact by construction whichever of them a reference uses.
probs is softmax(3 N(0, 1)) over D with planted foreground cells: p = 0 at the label's bin, p = 1 at the label's bin with zeros
elsewhere, p = 1 at a wrong bin, p = 1e-9 at the label's bin.

Checks per case, the same on the emulator and on the GPU:
  1. labels and count equal CM_DepthNet.get_downsampled_gt_depth on the CPU bit for bit (argmax where the one-hot row has a one, -1
     elsewhere), for every cell of every case; the labels-only call (probs = NULL) gives the same.
  2. exact floats: a variant in which every foreground cell's probabilities are 0 or 1, so that every term is 0 or exactly 100:
     bce_sum == 100 k and loss == float32(100 k) / float32(count) bit for bit.
  3. real floats: |loss - ref64| <= RHO_F ref64, ref64 evaluated in float64 from the fp32 inputs (all terms are non-negative).
     RHO_F is measured, not derived (the device's logf / log1pf error is not documented): the parent is fp32 torch get_depth_loss on
     the CPU; `python tests/depth_loss_cases.py` evaluates it on this table and prints its worst relative error against float64.
     Observed: 1.057e-07 (chunks_scalar; 7.862e-08 at shipped_rows).  RHO_F = 4 x that, never below 2^-20 and never above the 1e-4
     of tests/test_depth_net.py: the floor 2^-20 = 9.537e-07 holds.  The factor 4 covers another summation order and a device libm
     a few ulp from the host's.  The kernels' own figures are in profiles/r21_depth_loss_observed.txt (worst on the MI355X:
     1.136e-07 for the loss, 1.921e-07 for the gradient).
  4. gradient: elementwise |got - ref64| <= 2^-20 |ref64| for grad_loss = 0.37 and -3.0 (derived: no transcendental, at most ten
     correctly rounded fp32 operations per element; 2^-20 is 16 ulp), exactly 0 where the label is -1.
  5. guard words around labels, out_f, out_i, grad_probs and the workspace come back intact; gt and probs come back unwritten.
  6. two runs give identical bits in every output.

The launchers do not cap their grids (a workgroup per image and cell row; a thread per gradient element), so the table has no
over-the-cap case; `chunks_v4` and `chunks_scalar` cross the one size at which the forward kernel takes another path, a cell row of
more than 4096 columns, which it walks in chunks (4096 / ds cells, rounded down to a multiple of 4).

Plain Python, numpy and CPU torch only; the adapters import their library on first use.
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # `python tests/depth_loss_cases.py` finds the package

GUARD = 16                       # guard words in front of and behind every output
PATTERN = 7.5
IPATTERN = -1234567
PARENT_WORST = 1.057e-07         # see the header
RHO_F = min(max(4 * PARENT_WORST, 2.0 ** -20), 1e-4)
RHO_G = 2.0 ** -20
GRAD_LOSSES = (0.37, -3.0)
CHUNK_COLS = 4096                # FBBEV_DL_COLS of depth_loss_kernels.h


def observed(text):
    print(f'[observed] {text}')


def _case(name, BN, H, W, ds, D, cfg, offset=0):
    return dict(name=name, BN=BN, H=H, W=W, ds=ds, D=D, cfg=cfg, offset=offset)


CASES = [
    _case('px', 1, 3, 5, 1, 4, [1, 5, 1]),                         # cell = pixel, nothing a multiple of 4
    _case('odd3', 2, 9, 21, 3, 7, [1, 8, 1], offset=1),            # odd cell, scalar loads, gt 4-byte aligned only
    _case('ds4_w65', 1, 8, 260, 4, 12, [1, 13, 1]),                # one cell over a wave per row
    _case('shipped_rows', 2, 32, 704, 16, 80, [2, 42, 0.5]),       # the shipped geometry, two cell rows
    _case('ds32', 1, 64, 96, 32, 59, [1, 60, 1]),                  # 1024 pixels per cell, more than a workgroup
    _case('ds8_d118', 1, 16, 64, 8, 118, [1, 60, 0.5]),            # widest D of the reference
    _case('d1', 1, 8, 8, 4, 1, [1, 2, 1]),                         # a single bin
    _case('step04', 1, 16, 48, 4, 20, [1, 9, 0.4]),                # non-dyadic step
    _case('allzero', 1, 8, 16, 4, 12, [1, 13, 1]),                 # no foreground
    _case('chunks_v4', 1, 2, 4104, 2, 3, [1, 4, 1]),               # 2052 cells in a row: chunks of 2048 + 4, 16-byte loads
    _case('chunks_scalar', 1, 3, 4101, 3, 3, [1, 4, 1]),           # 1367 cells in a row: chunks of 1364 + 3, scalar loads
]
CASE_IDS = [c['name'] for c in CASES]
for _c in CASES:                                                     # the chunk cases are beyond a chunk, the others within one
    _cc = CHUNK_COLS // _c['ds']
    _cc = _cc & ~3 if _cc >= 4 else _cc
    assert (_c['W'] // _c['ds'] > _cc) == _c['name'].startswith('chunks'), _c['name']


def by_name(name):
    return CASES[CASE_IDS.index(name)]


def dims(case):
    return case['BN'], case['H'] // case['ds'], case['W'] // case['ds'], case['D']


def bin0_of(case):
    lo, _, step = case['cfg']
    return np.float32(lo - step)


def _seed(case, extra=0):
    return case['BN'] * 7 + case['H'] * 131 + case['W'] * 17 + case['ds'] * 3 + case['D'] * 1009 + extra


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_gt(case):
    """(BN, H, W) f32"""
    g = torch.Generator().manual_seed(_seed(case))
    BN, H, W, ds, D = (case[k] for k in ('BN', 'H', 'W', 'ds', 'D'))
    lo, hi, step = case['cfg']
    h, w = H // ds, W // ds
    if case['name'] == 'allzero':
        return torch.zeros(BN, H, W)
    b0, st = bin0_of(case), np.float32(step)
    if case['name'] == 'step04':
        k = torch.randint(-1, D + 3, (BN, H, W), generator=g).float()
        quarter = torch.where(torch.rand((BN, H, W), generator=g) < 0.5, 0.25, 0.75)
        gt = (float(b0) + (k + quarter).double() * float(st)).float()
    else:
        gt = torch.rand((BN, H, W), generator=g) * (hi + 5)
    gt = torch.where(torch.rand((BN, H, W), generator=g) < 0.6, torch.zeros(()), gt)
    cells = gt.view(BN, h, ds, w, ds).permute(0, 1, 3, 2, 4).reshape(-1, ds * ds).clone()
    nc, px = cells.shape
    # every third cell sparse: one or two entries survive
    for c in torch.randperm(nc, generator=g)[: nc // 3].tolist():
        keep = torch.randperm(px, generator=g)[: 1 + (c & 1)]
        row = torch.zeros(px)
        row[keep] = cells[c, keep]
        cells[c] = row
    edge = lambda k: np.float32(b0 + np.float32(k) * st)  # noqa: E731  (fp32 arithmetic)
    below = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))  # noqa: E731
    alone = lambda v: ('alone', float(v))  # noqa: E731
    plants = []
    if case['name'] != 'step04':
        for k in (1, D + 1, 0, D):
            plants += [alone(edge(k)), alone(below(edge(k)))]
    plants += [('one', -0.0), ('one', -3.0), ('one', float('nan')), ('one', float('inf')), alone(hi + 100.0),
               ('low', float(b0 + np.float32(0.5) * st))]
    order = torch.randperm(nc, generator=g).tolist()
    for c, (kind, v) in zip(order[: max(nc - 1, 0)], plants):
        at = int(torch.randint(0, px, (1,), generator=g))
        if kind == 'alone':
            cells[c] = 0.0
        elif kind == 'low':                                          # the other entries in range
            cells[c] = float(lo) + 0.5 * float(step) * torch.arange(px).clamp(max=D - 1).float()
        cells[c, at] = v
    return cells.view(BN, h, w, ds, ds).permute(0, 1, 3, 2, 4).reshape(BN, H, W).contiguous()


def _net(case):
    from fb_bev_amd.depth_net import CM_DepthNet
    return CM_DepthNet(in_channels=8, context_channels=4, depth_channels=case['D'], mid_channels=8, use_dcn=False, use_aspp=False,
                       downsample=case['ds'], grid_config=dict(depth=list(case['cfg'])), loss_depth_weight=1.0)


def ref_labels(case, gt):
    """(BN, h, w) int32 from the CPU CM_DepthNet.get_downsampled_gt_depth: argmax where the row has a one, -1 elsewhere"""
    onehot = _net(case).get_downsampled_gt_depth(gt[None])
    BN, h, w, D = dims(case)
    assert onehot.shape == (BN * h * w, D) and ((onehot == 0) | (onehot == 1)).all() and (onehot.sum(1) <= 1).all()
    lab = torch.where(onehot.sum(1) > 0, onehot.argmax(1), torch.full((), -1)).to(torch.int32)
    return lab.view(BN, h, w)


def make_probs(case, labels, exact=False):
    """(BN, D, h, w) f32"""
    g = torch.Generator().manual_seed(_seed(case, 1))
    BN, h, w, D = dims(case)
    P = torch.softmax(3 * torch.randn((BN * h * w, D), generator=g), dim=1)
    lab = labels.reshape(-1).long()
    fg = torch.nonzero(lab >= 0).reshape(-1)
    fg = fg[torch.randperm(fg.numel(), generator=g)].tolist()
    if exact:                                                        # every foreground row 0 / 1: no one, the label's bin, any bin, several
        for i, c in enumerate(fg):
            row = torch.zeros(D)
            kind = i % 4
            if kind == 1:
                row[lab[c]] = 1.0
            elif kind == 2:
                row[int(torch.randint(0, D, (1,), generator=g))] = 1.0
            elif kind == 3:
                row[torch.rand(D, generator=g) < 0.5] = 1.0
            P[c] = row
    else:
        for i, c in enumerate(fg[:4]):
            if i == 0:
                P[c, lab[c]] = 0.0
            elif i == 1:
                P[c] = 0.0
                P[c, lab[c]] = 1.0
            elif i == 2:
                P[c, (lab[c] + 1) % D] = 1.0                         # (D == 1: the label's own bin)
            else:
                P[c, lab[c]] = 1e-9
    return P.view(BN, h, w, D).permute(0, 3, 1, 2).contiguous()


def exact_k(probs, labels):
    """number of terms that are exactly 100 in the 0 / 1 variant: p = 0 at the label's bin, p = 1 at another"""
    BN, D, h, w = probs.shape
    P = probs.permute(0, 2, 3, 1).reshape(-1, D)
    lab = labels.reshape(-1).long()
    fg = lab >= 0
    assert ((P[fg] == 0) | (P[fg] == 1)).all()
    onehot = torch.zeros_like(P)
    onehot[fg, lab[fg]] = 1.0
    return int((P[fg] != onehot[fg]).sum())


def ref64(probs, labels):
    """(bce_sum, loss, count) in float64 from the fp32 inputs"""
    BN, D, h, w = probs.shape
    P = probs.permute(0, 2, 3, 1).reshape(-1, D).double()
    lab = labels.reshape(-1).long()
    fg = lab >= 0
    onehot = torch.zeros_like(P)
    onehot[fg, lab[fg]] = 1.0
    term = -torch.where(onehot > 0, torch.log(P), torch.log1p(-P)).clamp(min=-100.0)
    s = float(term[fg].sum())
    count = int(fg.sum())
    return s, s / max(count, 1), count


def grad_ref64(probs, labels, grad_loss):
    """(BN, D, h, w) float64: torch's binary_cross_entropy backward with its fp32 epsilon, times grad_loss / max(count, 1)"""
    BN, D, h, w = probs.shape
    p = probs.double()
    lab = labels.long()[:, None]                                     # (BN, 1, h, w)
    fg = lab >= 0
    tgt = (torch.arange(D).view(1, D, 1, 1) == lab).double()
    scale = float(np.float32(grad_loss)) / max(int(fg.sum()), 1)
    den = ((1 - p) * p).clamp(min=float(np.float32(1e-12)))
    return torch.where(fg, scale * (p - tgt) / den, torch.zeros((), dtype=torch.float64))


_REF = {}


def reference(case, exact=False):
    """(gt, labels, probs), computed once and shared; callers leave them unchanged"""
    key = (case['name'], exact)
    if key not in _REF:
        gt = _REF[(case['name'], not exact)][0] if (case['name'], not exact) in _REF else make_gt(case)
        lab = ref_labels(case, gt)
        _REF[key] = (gt, lab, make_probs(case, lab, exact))
    return _REF[key]


def parent_error(case):
    """relative error of the parent -- fp32 torch get_depth_loss on the CPU -- against float64"""
    gt, lab, probs = reference(case)
    loss = float(_net(case).get_depth_loss(gt[None], probs[None])['loss_depth'])
    _, want, _ = ref64(probs, lab)
    return abs(loss - want) / want if want > 0 else abs(loss)


# step04: the three ways to a bin agree on every cell
def _assert_step04_is_exact():
    case = by_name('step04')
    gt = make_gt(case)
    ds = case['ds']
    BN, h, w, D = dims(case)
    cells = gt.view(BN, h, ds, w, ds).permute(0, 1, 3, 2, 4).reshape(-1, ds * ds)
    m = torch.where(cells == 0.0, torch.full_like(cells, 1e5), cells).min(dim=-1).values.numpy()
    b0, st = bin0_of(case), np.float32(case['cfg'][2])
    with np.errstate(invalid='ignore'):
        div = (m - b0) / st
        mul = (m - b0) * (np.float32(1) / st)
        f64 = (m.astype(np.float64) - float(b0)) / float(st)
        pick = lambda b: np.where((b >= 0) & (b < D + 1), np.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)  # noqa: E731
    assert m.dtype == np.float32 and div.dtype == np.float32 and mul.dtype == np.float32
    assert np.array_equal(pick(div), pick(mul)) and np.array_equal(pick(div), pick(f64))
    assert len(set(pick(div).tolist())) > 4


_assert_step04_is_exact()


# ------------------------------------------------------------------------------------------------------------------ adapters
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class EmuApi:
    """the C entries of the CPU-emulated library, CPU tensors"""
    name = 'emu'

    def __init__(self):
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
        import emu_capi
        self.lib = emu_capi.lib()

    def dev(self, t):
        return t.clone()

    def cpu(self, t):
        return t

    def ws_bytes(self, BN, h, w, D):
        return self.lib.fbbev_depth_loss_ws_bytes(BN, h, w, D)

    def fwd(self, gt, probs, ds, D, lo, step, labels, out_f, out_i, ws):
        BN, H, W = gt.shape
        return self.lib.fbbev_depth_loss_fwd(_p(gt), BN, H, W, ds, _p(probs), D, float(lo) - float(step), float(step), _p(labels),
                                             _p(out_f), _p(out_i), _p(ws), ws.numel(), None)

    def grad(self, probs, labels, out_i, grad_loss, out):
        BN, D, h, w = probs.shape
        return self.lib.fbbev_depth_loss_grad(_p(probs), _p(labels), _p(out_i), _p(grad_loss), BN, D, h, w, _p(out), None)


class GpuApi:
    """fb_bev_amd._capi.depth_loss_fwd / depth_loss_grad on cuda:0"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi
        self.c = _capi
        self.device = torch.device('cuda:0')

    def dev(self, t):
        return t.to(self.device)

    def cpu(self, t):
        return t.cpu()

    def ws_bytes(self, BN, h, w, D):
        return self.c.lib().fbbev_depth_loss_ws_bytes(BN, h, w, D)

    def fwd(self, gt, probs, ds, D, lo, step, labels, out_f, out_i, ws):
        self.c.depth_loss_fwd(gt, probs, ds, D, lo, step, labels=labels, out_f=out_f, out_i=out_i, ws=ws)
        return 0

    def grad(self, probs, labels, out_i, grad_loss, out):
        assert self.c.depth_loss_grad(probs, labels, out_i, grad_loss, out=out) is out
        return 0


def _bits(t):
    return t.contiguous().view(torch.int32)


def run(api, case, gt, probs, grad_loss=GRAD_LOSSES[0]):
    """one forward and (with probs) one backward call -> (labels, out_f, out_i, grad or None) on the CPU.  Every output is a slice of a
    larger patterned buffer whose other words must come back intact; the inputs must come back unchanged."""
    BN, h, w, D = dims(case)
    ds, (lo, _, step), off = case['ds'], case['cfg'], case['offset']
    ncell, nel = BN * h * w, BN * D * h * w
    store = torch.cat([torch.full((off,), PATTERN), gt.reshape(-1), torch.full((GUARD,), PATTERN)])
    d_store = api.dev(store)
    d_gt = d_store[off:off + gt.numel()].view(gt.shape)
    assert d_gt.data_ptr() % 16 == (4 * off) % 16 and d_gt.is_contiguous()
    d_probs = None if probs is None else api.dev(probs)
    need = api.ws_bytes(BN, h, w, D)
    assert need == 2 * ((4 * BN * h + 15) // 16 * 16)
    bl = api.dev(torch.full((GUARD + ncell + GUARD,), IPATTERN, dtype=torch.int32))
    bf = api.dev(torch.full((GUARD + 2 + GUARD,), PATTERN))
    bi = api.dev(torch.full((GUARD + 1 + GUARD,), IPATTERN, dtype=torch.int32))
    bw = api.dev(torch.full((64 + need + 64,), 0xA5, dtype=torch.uint8))
    d_lab, d_f, d_i = bl[GUARD:GUARD + ncell].view(BN, h, w), bf[GUARD:GUARD + 2], bi[GUARD:GUARD + 1]
    assert api.fwd(d_gt, d_probs, ds, D, lo, step, d_lab, d_f, d_i, bw[64:64 + need]) == 0
    grad = None
    if probs is not None:
        bg = api.dev(torch.full((GUARD + nel + GUARD,), PATTERN))
        assert api.grad(d_probs, d_lab, d_i, api.dev(torch.tensor([grad_loss], dtype=torch.float32)),
                        bg[GUARD:GUARD + nel].view(BN, D, h, w)) == 0
        bg = api.cpu(bg)
        assert (bg[:GUARD] == PATTERN).all() and (bg[GUARD + nel:] == PATTERN).all(), 'guard words of grad_probs overwritten'
        grad = bg[GUARD:GUARD + nel].view(BN, D, h, w).clone()
        assert torch.equal(_bits(api.cpu(d_probs)), _bits(probs)), 'probs was written to'
    bl, bf, bi, bw = api.cpu(bl), api.cpu(bf), api.cpu(bi), api.cpu(bw)
    assert (bl[:GUARD] == IPATTERN).all() and (bl[GUARD + ncell:] == IPATTERN).all(), 'guard words of labels overwritten'
    assert (bf[:GUARD] == PATTERN).all() and (bf[GUARD + 2:] == PATTERN).all(), 'guard words of out_f overwritten'
    assert (bi[:GUARD] == IPATTERN).all() and (bi[GUARD + 1:] == IPATTERN).all(), 'guard words of out_i overwritten'
    assert (bw[:64] == 0xA5).all() and (bw[64 + need:] == 0xA5).all(), 'guard bytes of the workspace overwritten'
    assert torch.equal(_bits(api.cpu(d_store)), _bits(store)), 'gt was written to'
    return bl[GUARD:GUARD + ncell].view(BN, h, w).clone(), bf[GUARD:GUARD + 2].clone(), bi[GUARD:GUARD + 1].clone(), grad


# ------------------------------------------------------------------------------------------------------------------ checks
def check(api, case):
    """layers 1, 3, 4 and 5 on one case"""
    gt, lab, probs = reference(case)
    tag = f'{api.name} {case["name"]}'
    count = int((lab >= 0).sum())
    got_lab, got_f, got_i, got_g = run(api, case, gt, probs)
    # 1: labels and count, and the labels-only call
    assert torch.equal(got_lab, lab), f'{int((got_lab != lab).sum())} labels differ'
    assert int(got_i) == count
    only_lab, only_f, only_i, _ = run(api, case, gt, None)
    assert torch.equal(only_lab, lab) and int(only_i) == count and float(only_f[0]) == 0.0 and float(only_f[1]) == 0.0
    if case['name'] == 'allzero':
        assert count == 0
    else:
        assert count > 0 and count < lab.numel()
    # 3: floats
    want_sum, want_loss, _ = ref64(probs, lab)
    rel = lambda g, r: abs(g - r) / r if r > 0 else abs(g)  # noqa: E731
    observed(f'{tag}: count {count} of {lab.numel()} cells, loss {float(got_f[1])!r} against {want_loss!r}: relative error '
             f'{rel(float(got_f[1]), want_loss):.3e} (RHO_F = {RHO_F:.3e}), bce_sum {rel(float(got_f[0]), want_sum):.3e}')
    assert abs(float(got_f[1]) - want_loss) <= RHO_F * want_loss, (float(got_f[1]), want_loss)
    assert abs(float(got_f[0]) - want_sum) <= RHO_F * want_sum, (float(got_f[0]), want_sum)
    if count == 0:
        assert float(got_f[0]) == 0.0 and float(got_f[1]) == 0.0
    # 4: gradient
    for g in GRAD_LOSSES:
        if g != GRAD_LOSSES[0]:
            got_g = run(api, case, gt, probs, g)[3]
        want = grad_ref64(probs, lab, g)
        bg = (lab < 0)[:, None].expand_as(got_g)
        assert (_bits(got_g)[bg] == 0).all(), 'a background cell with a gradient that is not +0.0'
        err = (got_g.double() - want).abs()
        live = want != 0
        r = float((err[live] / want[live].abs()).max()) if live.any() else 0.0
        observed(f'{tag}: gradient for grad_loss {g}: worst relative error {r:.3e} (bound {RHO_G:.3e}), largest |grad| '
                 f'{float(want.abs().max()):.3e}')
        assert torch.isfinite(got_g).all()
        assert (err <= RHO_G * want.abs()).all(), r
        assert count == 0 or float(want.abs().max()) > 0
    return got_f, got_i


def check_exact(api, case):
    """layer 2: every term 0 or exactly 100"""
    gt, lab, probs = reference(case, exact=True)
    k, count = exact_k(probs, lab), int((lab >= 0).sum())
    got_lab, got_f, got_i, got_g = run(api, case, gt, probs)
    assert torch.equal(got_lab, lab) and int(got_i) == count
    want = torch.tensor([100.0 * k, 0.0], dtype=torch.float32)
    want[1] = want[0] / torch.tensor(float(max(count, 1)), dtype=torch.float32)
    observed(f'{api.name} {case["name"]} exact: {k} terms of 100 over {count} cells: bce_sum {float(got_f[0])!r}, loss {float(got_f[1])!r}')
    assert 100 * k < 2 ** 24 and (k > 0 or count == 0)
    assert torch.equal(_bits(got_f), _bits(want)), (got_f, want)
    assert torch.isfinite(got_g).all()


def check_repeat(api, case):
    """layer 6: two runs, identical bits"""
    gt, lab, probs = reference(case)
    a, b = (run(api, case, gt, probs) for _ in range(2))
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


def check_fixture(api):
    """tests/golden/depth_net_small.npz, recorded from the reference module: labels bit for bit, the loss at test_depth_net.py's bar"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'depth_net_small.npz'))
    gt, depth = torch.from_numpy(z['gt']), torch.from_numpy(z['depth'])
    B, N, D, h, w = depth.shape
    case = _case('fixture', B * N, gt.shape[-2], gt.shape[-1], 4, D, [1.0, 13.0, 1.0])
    assert (D, gt.shape[-2] // 4, gt.shape[-1] // 4) == (12, h, w)
    onehot = torch.from_numpy(z['labels'])
    lab = torch.where(onehot.sum(1) > 0, onehot.argmax(1), torch.full((), -1)).to(torch.int32).view(B * N, h, w)
    got_lab, got_f, got_i, _ = run(api, case, gt.reshape(B * N, *gt.shape[-2:]).contiguous(), depth.reshape(B * N, D, h, w).contiguous())
    assert torch.equal(got_lab, lab) and int(got_i) == int((lab >= 0).sum()) > 0
    loss = float(z['loss'])
    observed(f'{api.name} fixture: loss {float(got_f[1])!r} against the reference module\'s {loss!r}')
    assert abs(float(got_f[1]) - loss) < 1e-4 * max(1.0, abs(loss))


if __name__ == '__main__':                                           # the measurement behind RHO_F
    worst = 0.0
    for case in CASES:
        r = parent_error(case)
        worst = max(worst, r)
        observed(f'parent (fp32 torch get_depth_loss, CPU) {case["name"]}: relative error against float64 = {r:.3e}')
    observed(f'parent worst relative error: {worst:.3e}; 4 x worst = {4 * worst:.3e}; floor 2^-20 = {2.0 ** -20:.3e}; cap 1e-4')
