"""Case table, references and checks for fbbev_occ_lovasz_fwd / fbbev_occ_lovasz_grad (fb_bev_amd/csrc/occ_lovasz_kernels.h), shared by the
emulator test (tests/test_emu_occ_lovasz.py) and the GPU test (tests/test_gpu_occ_lovasz.py).  The shapes, layouts, logits and label sets
are those of tests/occ_loss_cases.py (imported, not edited), plus one planted voxel with a class 120 above the rest -- its softmax
underflows, so valid bg elements with e == 0 exist -- and the label set 'allvalid' (no 255 at all).

Layers of `check` (the numbering of the pull request that added the kernels):
  1. counts: fg_count equals a numpy bincount bit for bit.
  2. errors: errors_out against float64 |f - softmax|.  Asserted twice:
       (a) |e - e64| <= R_E (f + p64) with R_E = 4 x the worst ratio of the fp32 CPU torch restatement on this table, floor 2^-22.  Measured
           that way (`python tests/occ_lovasz_cases.py`) the worst ratio is 1.0 -- at the planted voxel p64 = e^-120 is 7.7e-53 and
           every fp32 softmax returns 0 -- so R_E = 4.0 and (a) alone would say little;
       (b) the same form with R_E_NORMAL over the elements with f + p64 >= 2^-100, where fp32 has its full relative precision, and
           |e - e64| <= 2^-99 below that (an underflowing value stays tiny).  R_E_NORMAL = 4 x the restatement's worst over those
           elements = 4 x 1.959e-06 = 7.836e-06 (b1_1x8243x16: x - max is rounded to fp32 before the exponential, so a small p carries
           the relative error 2^-24 |x - max|).
  3. sort, scan and closed form, bit for bit: from the device's own errors_out a numpy program forms the canonical order
     (np.lexsort((index, -e)) over the valid voxels), F, U and the two double expressions; coef must equal it in every bit, zeros
     included; loss_c must lie within n_valid 2^-52 (relative) of math.fsum of the exact products, rounded to fp32.
  4. backward: with the device's coef as the constant h and a seeded scale s, |grad - grad64| <= RHO_L A elementwise,
     A = |s| p[j] (|h[j]| + sum_c |h[c]| p[c]) in float64; exactly 0 where A == 0.  RHO_L = 4 x the worst err / A of fp32 torch autograd
     of s (h softmax(x)).sum() on the CPU over this table, floor 2^-20.  As in layer 2 the underflowing voxel makes that worst 1.0
     (RHO_L = 4.0, asserted), so the bound that says something is asserted as well: RHO_L_NORMAL = 4 x the parent's worst over the
     elements with A >= 2^-90 = 4 x 1.941e-06 = 7.762e-06 (b1_3x9x70, skewed labels), and |grad - grad64| <= 2^-89 below that.
  5. guard words around every output and the workspace intact, logits and labels unwritten (`run`); check_repeat: identical bytes.
  6. share of coef entries that differ from the coefficients of the float64 errors' canonical order: <= 1e-3 on SMALL_IDS.

Plain Python, numpy and CPU torch only; the adapters import their library on first use.
"""
import ctypes
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # `python tests/occ_lovasz_cases.py` finds the package
import occ_loss_cases as LC  # noqa: E402

GUARD, PATTERN, IPATTERN = LC.GUARD, LC.PATTERN, LC.IPATTERN
observed = LC.observed

R_E = 4 * 1.0                       # layer 2 (a): see the header
R_E_NORMAL = 4 * 1.959e-06          # layer 2 (b)
NORMAL = 2.0 ** -100
A_NORMAL = 2.0 ** -90
RHO_L = 4 * 1.0                     # layer 4, literal
RHO_L_NORMAL = 4 * 1.941e-06        # layer 4 over A >= A_NORMAL
assert R_E >= 2.0 ** -22 and R_E_NORMAL >= 2.0 ** -22 and RHO_L >= 2.0 ** -20 and RHO_L_NORMAL >= 2.0 ** -20

CHUNK = 4096                        # FBBEV_OCCLV_TILE: pairs per sort chunk
WALK_BLOCKS = 1024                  # FBBEV_OCCLV_MAX_BLOCKS: grid cap of the keys and gradient tile walks (the only capped grids)
_NAMES = ['b2_5x7x3', 'b1_17x33x16', 'b2_8x8x16_padded', 'b1_6x4x5_permuted', 'n2', 'n32', 'c18', 'b1_3x9x70', 'b1_1x8243x16']
CASES = [c for c in LC.CASES if c['name'].rsplit('_cl', 1)[0].rsplit('_planes', 1)[0] in _NAMES or c['name'] in _NAMES]
CASE_IDS = [c['name'] for c in CASES]
assert len(CASES) == 17, CASE_IDS
EXACT_CASES = [LC.by_name(n) for n in ('exact16_9x7x5_cl', 'exact16_9x7x5_planes', 'exact32_b2_5x6x3_cl', 'exact32_b2_5x6x3_planes')]
EXACT_IDS = [c['name'] for c in EXACT_CASES]
LABEL_KINDS = LC.LABEL_KINDS + ['allvalid']
SMALL_IDS = ['b2_5x7x3_cl', 'b1_17x33x16_cl', 'n2_cl', 'n32_cl', 'c18_cl']
REPEAT_IDS = ['b1_17x33x16_cl', 'b1_17x33x16_planes', 'b2_5x7x3_cl', 'b1_6x4x5_permuted', 'b1_1x8243x16_cl']
EMU_REPEAT_IDS = ['b2_5x7x3_cl', 'b1_6x4x5_permuted', 'b2_8x8x16_padded_planes']
BIG_IDS = ['b1_1x8243x16_cl', 'b1_1x8243x16_planes']


def voxels(case):
    return case['B'] * case['H'] * case['W'] * case['D']


def n_valid_of(case, kind):
    return int((labels(case, kind) != 255).sum())


def by_name(name):
    return LC.by_name(name)


# ------------------------------------------------------------------------------------------------------------------ inputs
def logical_logits(case, exact=False):
    """LC.logical_logits plus (real cases) one voxel with a class 120 above the rest: the first voxel whose row is finite, not
    constant and spread over less than 39 (none of LC's planted rows)"""
    L = LC.logical_logits(case, exact)
    if exact:
        return L
    B, C, H, W, D = L.shape
    V = L.permute(0, 2, 3, 4, 1).reshape(-1, C)
    spread = V.max(1)[0] - V.min(1)[0]
    ok = torch.isfinite(V).all(1) & (spread > 0) & (spread < 39)
    row = int(torch.nonzero(ok)[0])
    V = V.clone()
    V[row, row % C] = V[row].max() + 120.0
    return V.view(B, H, W, D, C).permute(0, 4, 1, 2, 3).contiguous()


def labels(case, kind):
    if kind != 'allvalid':
        return LC.labels(case, kind)
    t = LC.labels(case, 'uniform').clone().view(-1)
    idx = torch.nonzero(t == 255).view(-1)
    t[idx] = (idx % case['C']).to(torch.uint8)
    return t.view(case['B'], case['H'], case['W'], case['D'])


def scale_of(case):
    g = torch.Generator().manual_seed(LC._seed(case, 5))
    return (torch.rand(1, generator=g) * 0.5 + 0.05) * (-1.0 if case['C'] % 2 else 1.0)


# the table about itself (as occ_loss_cases.py asserts its tile counts)
assert sum(n_valid_of(c, 'uniform') > 2 * CHUNK and n_valid_of(c, 'uniform') % CHUNK != 0 for c in CASES) >= 2       # >= 3 sort chunks
assert sum(LC.tiles(c) > WALK_BLOCKS for c in CASES) >= 1       # more tiles than one pass of the capped grids (the sort's are not capped)


# ------------------------------------------------------------------------------------------------------------------ references
def softmax64(L):
    return F.softmax(torch.nan_to_num(L.double(), nan=0.0, posinf=0.0, neginf=0.0), dim=1)


def planes(t):
    """(B, C, H, W, D) -> (C, B*H*W*D): class planes in (b, h, w, d) order"""
    return t.permute(1, 0, 2, 3, 4).reshape(t.shape[1], -1)


def errors_ref(L, lab, dtype=torch.float64):
    """(e (C, N), f (C, N) bool, p (C, N)) at dtype; ignored voxels have e = 0"""
    C = L.shape[1]
    x = torch.nan_to_num(L.to(dtype), nan=0.0, posinf=0.0, neginf=0.0)
    p = planes(F.softmax(x, dim=1))
    t = lab.reshape(1, -1)
    f = t == torch.arange(C)[:, None]
    e = (f.to(dtype) - p).abs() * (t != 255).to(dtype)
    return e, f, p


def coef_from_errors(e, lab, C):
    """the canonical order and the closed form in numpy -> (coef (C, N) f32, loss (C,) float64 by math.fsum, G (C,), n_valid).
    e (C, N): float32 (the device's) or float64 (layer 6)"""
    t = lab.numpy().reshape(-1)
    idx = np.nonzero(t != 255)[0]
    n = idx.size
    coef = np.zeros((C, t.size), dtype=np.float32)
    loss = np.zeros(C)
    Gs = np.zeros(C, dtype=np.int64)
    for c in range(C):
        f = t[idx] == c
        G = int(f.sum())
        Gs[c] = G
        if G == 0:
            continue
        ev = e[c][idx]
        order = np.lexsort((idx, -ev))
        fs = f[order]
        Fk = np.cumsum(fs).astype(np.float64)
        k = np.arange(1, n + 1, dtype=np.float64)
        U = G + k - Fk
        with np.errstate(divide='ignore', invalid='ignore'):
            g = np.where(fs, 1.0 / U, (G - Fk) / (U * (U - 1.0))).astype(np.float32)
        coef[c, idx[order]] = np.where(fs, -g, g)
        loss[c] = math.fsum((ev[order].astype(np.float64) * g.astype(np.float64)).tolist())
    return coef, loss, Gs, n


def grad_ref64(L, coef_cn, s):
    """the backward formula in float64 -> (grad (B, C, H, W, D), A)"""
    B, C, H, W, D = L.shape
    p = softmax64(L)
    h = torch.from_numpy(coef_cn).double().view(C, B, H, W, D).permute(1, 0, 2, 3, 4)
    s = float(s)
    grad = s * p * (h - (h * p).sum(1, keepdim=True))
    A = abs(s) * p * (h.abs() + (h.abs() * p).sum(1, keepdim=True))
    fin = torch.isfinite(L)
    zero = torch.zeros_like(p)
    return torch.where(fin, grad, zero), torch.where(fin, A, zero)


def lovasz64(probas, labels, ignore=255):
    """occ_loss.lovasz_softmax's operations at the dtype of probas (the function itself casts with .float())"""
    B, C = probas.shape[:2]
    p = probas.reshape(B, C, -1).permute(1, 0, 2).reshape(C, -1)
    lab = labels.reshape(1, -1)
    valid = lab != ignore
    fg = ((lab == torch.arange(C)[:, None]) & valid).to(p.dtype)
    errors = (fg - p).abs() * valid.to(p.dtype)
    errors_sorted, perm = torch.sort(errors, dim=1, descending=True, stable=True)
    fg_sorted = torch.gather(fg, 1, perm)
    gts = fg_sorted.sum(1, keepdim=True)
    csum = fg_sorted.cumsum(1)
    intersection = gts - csum
    union = gts + (torch.arange(1, fg_sorted.shape[1] + 1, dtype=p.dtype)[None] - csum)
    jaccard = 1.0 - intersection / union
    grad = torch.cat([jaccard[:, :1], jaccard[:, 1:] - jaccard[:, :-1]], 1)
    losses = (errors_sorted * grad.detach()).sum(1)
    present = gts[:, 0] > 0
    return torch.where(present, losses, torch.zeros_like(losses)).sum() / present.to(p.dtype).sum().clamp(min=1)


_REF = {}


def inputs(case, kind, exact=False):
    key = (case['name'], kind, exact)
    if key not in _REF:
        L, lab = logical_logits(case, exact), labels(case, kind)
        e64, f, p64 = errors_ref(L, lab)
        _REF[key] = (L, lab, e64, f, p64)
    return _REF[key]


def parent_ratios(case, kind):
    """the fp32 CPU torch restatements against float64 -> (worst |e - e64| / (f + p64) over all valid elements, the same over the
    elements with f + p64 >= NORMAL, worst gradient err / A with the float64 order's coefficients as h, the same over the elements
    with A >= A_NORMAL)"""
    L, lab, e64, f, p64 = inputs(case, kind)
    e32, _, _ = errors_ref(L, lab, torch.float32)
    valid = (lab.reshape(1, -1) != 255).expand_as(e64)
    den = f.double() + p64
    ratio = (e32.double() - e64).abs() / den
    r_all = float(ratio[valid].max()) if valid.any() else 0.0
    normal = valid & (den >= NORMAL)
    r_normal = float(ratio[normal].max()) if normal.any() else 0.0
    coef, _, _, _ = coef_from_errors(e64.numpy(), lab, L.shape[1])
    s = scale_of(case)
    grad, A = grad_ref64(L, coef, s)
    x = L.clone().requires_grad_()
    B, C, H, W, D = L.shape
    h = torch.from_numpy(coef).view(C, B, H, W, D).permute(1, 0, 2, 3, 4)
    (s.float() * (h * F.softmax(torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0), dim=1)).sum()).backward()
    err = (x.grad.double() - grad).abs()
    ok = A > 0
    okn = A >= A_NORMAL
    return (r_all, r_normal, float((err[ok] / A[ok]).max()) if ok.any() else 0.0,
            float((err[okn] / A[okn]).max()) if okn.any() else 0.0)


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
        return self.lib.fbbev_occ_lovasz_ws_bytes(B, C, H, W, D)

    def fwd(self, view, lab, loss_c, fg_count, coef, errors, ws):
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        B, C, H, W, D = view.shape
        return self.lib.fbbev_occ_lovasz_fwd(p(view), *view.stride(), B, C, H, W, D, p(lab), p(loss_c), p(fg_count), p(coef), p(errors),
                                             p(ws), ws.numel(), None)

    def grad(self, view, lab, coef, scale, out):
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        B, C, H, W, D = view.shape
        return self.lib.fbbev_occ_lovasz_grad(p(view), *view.stride(), B, C, H, W, D, p(lab), p(coef), p(scale), p(out), None)


class GpuApi:
    """fb_bev_amd._capi.occ_lovasz_fwd / occ_lovasz_grad on cuda:0"""
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
        return self.c.lib().fbbev_occ_lovasz_ws_bytes(B, C, H, W, D)

    def fwd(self, view, lab, loss_c, fg_count, coef, errors, ws):
        B, C, H, W, D = view.shape
        shape = (C, B, H, W, D)
        self.c.occ_lovasz_fwd(view, lab, loss_c=loss_c, fg_count=fg_count, coef=coef.view(shape),
                              errors_out=None if errors is None else errors.view(shape), ws=ws)
        return 0

    def grad(self, view, lab, coef, scale, out):
        B, C, H, W, D = view.shape
        got = self.c.occ_lovasz_grad(view, lab, coef.view(C, B, H, W, D), scale, out=out)
        assert got is out
        return 0


def run(api, case, L, lab, scale, with_errors=True):
    """one forward and one backward call -> dict(loss_c, fg_count, coef (C, N), errors (C, N) or None, grad (B, C, H, W, D)) on the
    CPU.  Every output is a slice of a larger patterned buffer whose other words must come back intact; the inputs unchanged."""
    storage, size, stride, off = LC.lay_out(case, L)
    B, C, H, W, D = size
    nv = B * H * W * D
    d_storage = api.dev(storage)
    view = d_storage.as_strided(size, stride, off)
    d_lab, d_scale = api.dev(lab), api.dev(scale.float())
    need = api.ws_bytes(B, C, H, W, D)
    assert need > 0 and need % 16 == 0
    bl = api.dev(torch.full((GUARD + C + GUARD,), PATTERN))
    bi = api.dev(torch.full((GUARD + C + 1 + GUARD,), IPATTERN, dtype=torch.int32))
    bc = api.dev(torch.full((GUARD + C * nv + GUARD,), PATTERN))
    be = api.dev(torch.full((GUARD + C * nv + GUARD,), PATTERN)) if with_errors else None
    bw = api.dev(torch.full((64 + need + 64,), 0xA5, dtype=torch.uint8))
    coef = bc[GUARD:GUARD + C * nv]
    assert api.fwd(view, d_lab, bl[GUARD:GUARD + C], bi[GUARD:GUARD + C + 1], coef,
                   be[GUARD:GUARD + C * nv] if with_errors else None, bw[64:64 + need]) == 0
    g_storage = api.dev(torch.full_like(storage, PATTERN))
    g_view = g_storage.as_strided(size, stride, off)
    assert api.grad(view, d_lab, coef, d_scale, g_view) == 0
    bl, bi, bc, bw, g_back = api.cpu(bl), api.cpu(bi), api.cpu(bc), api.cpu(bw), api.cpu(g_storage)
    assert (bl[:GUARD] == PATTERN).all() and (bl[GUARD + C:] == PATTERN).all(), 'guard words of loss_c overwritten'
    assert (bi[:GUARD] == IPATTERN).all() and (bi[GUARD + C + 1:] == IPATTERN).all(), 'guard words of fg_count overwritten'
    assert (bc[:GUARD] == PATTERN).all() and (bc[GUARD + C * nv:] == PATTERN).all(), 'guard words of coef overwritten'
    assert (bw[:64] == 0xA5).all() and (bw[64 + need:] == 0xA5).all(), 'guard bytes of the workspace overwritten'
    errors = None
    if with_errors:
        be = api.cpu(be)
        assert (be[:GUARD] == PATTERN).all() and (be[GUARD + C * nv:] == PATTERN).all(), 'guard words of errors_out overwritten'
        errors = be[GUARD:GUARD + C * nv].view(C, nv).clone()
    inside = torch.zeros(storage.numel(), dtype=torch.bool)
    inside.as_strided(size, stride, off).fill_(True)
    assert int(inside.sum()) == L.numel()
    assert (g_back[~inside] == PATTERN).all(), 'grad_logits written outside the view'
    nn = lambda t: torch.nan_to_num(t, 1e9, 2e9, -2e9)  # noqa: E731
    assert torch.equal(nn(api.cpu(d_storage)), nn(storage)), 'the logits were written to'
    assert torch.equal(api.cpu(d_lab), lab), 'the labels were written to'
    return dict(loss_c=bl[GUARD:GUARD + C].clone(), fg_count=bi[GUARD:GUARD + C + 1].clone(), coef=bc[GUARD:GUARD + C * nv].view(C, nv).clone(),
                errors=errors, grad=g_back.as_strided(size, stride, off).contiguous())


# ------------------------------------------------------------------------------------------------------------------ checks
def _bits(t):
    return t.contiguous().view(torch.int32)


def check(api, case, kind, exact=False, order64=False):
    """layers 1 to 5 (and 6 with order64) on one case and label set"""
    L, lab, e64, f, p64 = inputs(case, kind, exact)
    C = case['C']
    tag = f'{api.name} {case["name"]} {kind}{" exact" if exact else ""}'
    s = scale_of(case)
    got = run(api, case, L, lab, s)
    # 1: counts
    t = lab.numpy().reshape(-1)
    want_i = np.append(np.bincount(t[t != 255], minlength=C)[:C], (t != 255).sum()).astype(np.int32)
    assert np.array_equal(got['fg_count'].numpy(), want_i), (got['fg_count'].numpy(), want_i)
    if kind == 'single':
        assert (want_i[:C] == 1).sum() >= 1
    if kind == 'absent':
        assert (want_i[:C] == 0).sum() >= C // 2 - 1
    if kind == 'allvalid':
        assert want_i[C] == t.size
    # 2: errors
    e = got['errors']
    valid = (lab.reshape(1, -1) != 255).expand_as(e)
    assert (e[~valid] == 0).all(), 'an error for a voxel labelled 255'
    assert ((e >= 0) & (e <= 1)).all()
    den = f.double() + p64
    err = (e.double() - e64).abs()
    normal = valid & (den >= NORMAL)
    r_all = float((err[valid] / den[valid]).max()) if valid.any() else 0.0
    r_normal = float((err[normal] / den[normal]).max()) if normal.any() else 0.0
    observed(f'{tag}: errors worst |e - e64| / (f + p64) = {r_all:.3e} (R_E = {R_E:.3e}), over f + p64 >= 2^-100: {r_normal:.3e} '
             f'(R_E_NORMAL = {R_E_NORMAL:.3e})')
    assert (err[valid] <= R_E * den[valid]).all(), r_all
    assert (err[normal] <= R_E_NORMAL * den[normal]).all(), r_normal
    assert (err[valid & ~normal] <= 2.0 ** -99).all()
    if exact:                                                            # p = 1 / C exactly
        want_e = (f.float() - 1.0 / C).abs() * valid.float()
        assert torch.equal(_bits(e), _bits(want_e))
    # 3: sort, scan and closed form from the device's own errors
    coef, loss, Gs, n = coef_from_errors(e.numpy(), lab, C)
    assert np.array_equal(Gs.astype(np.int32), want_i[:C]) and n == want_i[C]
    bad = int((_bits(got['coef']) != _bits(torch.from_numpy(coef))).sum())
    observed(f'{tag}: coef words that differ from the canonical order of the device errors = {bad} of {coef.size}')
    assert bad == 0
    assert (got['coef'][~valid] == 0).all() and (got['coef'][torch.from_numpy(Gs == 0)] == 0).all()
    rel = n * 2.0 ** -52
    lo, hi = np.float32(loss * (1 - rel)), np.float32(loss * (1 + rel))
    lc = got['loss_c'].numpy()
    worst = float(np.max(np.abs(lc.astype(np.float64) - loss) / np.maximum(loss, 1e-300))) if (loss > 0).any() else 0.0
    observed(f'{tag}: loss_c worst relative distance to fsum = {worst:.3e} (fp32 rounding included), sum = {float(loss.sum()):.6f}')
    assert ((lc >= lo) & (lc <= hi)).all(), (lc, loss)
    assert (lc[Gs == 0] == 0).all()
    if exact and C > 2:                                                  # fg errors 1 - 1/C above every bg error 1/C: by the counts alone
        G = torch.from_numpy(Gs).double()[:, None]                      # (float)(1.0 / (double)G), as the kernel rounds it
        want_c = torch.where(f & valid, (-(1.0 / G)).float().expand_as(e), torch.zeros_like(e))
        assert torch.equal(_bits(got['coef']), _bits(want_c))
    # 4: backward with the device's coef as the constant
    grad, A = grad_ref64(L, got['coef'].numpy(), s)
    gerr = (got['grad'].double() - grad).abs()
    live = A > 0
    assert (got['grad'][~live] == 0).all(), 'a gradient where nothing contributes (a voxel labelled 255 or a non-finite logit)'
    assert torch.isfinite(got['grad']).all()
    r = float((gerr[live] / A[live]).max()) if live.any() else 0.0
    big = A >= A_NORMAL
    rn = float((gerr[big] / A[big]).max()) if big.any() else 0.0
    observed(f'{tag}: gradient worst err / A = {r:.3e} (RHO_L = {RHO_L:.3e}), over A >= 2^-90: {rn:.3e} (RHO_L_NORMAL = '
             f'{RHO_L_NORMAL:.3e}), largest |grad| = {float(grad.abs().max()):.3e}')
    assert (gerr <= RHO_L * A).all(), r
    assert (gerr[big] <= RHO_L_NORMAL * A[big]).all(), rn
    assert (gerr[~big] <= 2.0 ** -89).all()
    if kind == 'all255':
        assert (got['loss_c'] == 0).all() and (got['coef'] == 0).all() and (got['grad'] == 0).all() and (got['fg_count'] == 0).all()
    else:
        assert live.any() and float(grad.abs().max()) > 0
    # 6: the order against float64
    if order64:
        coef64, _, _, _ = coef_from_errors(e64.numpy(), lab, C)
        share = float((got['coef'].numpy() != coef64).mean())
        observed(f'{tag}: share of coef entries that differ from the float64 order = {share:.3e}')
        assert share <= 1e-3, share
    return got


def check_repeat(api, case):
    """layer 5: two runs, identical bytes"""
    L, lab = inputs(case, 'uniform')[:2]
    a, b = (run(api, case, L, lab, scale_of(case), with_errors=i == 0) for i in range(2))      # (and a null errors_out changes nothing)
    for k in ('loss_c', 'fg_count', 'coef', 'grad'):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


if __name__ == '__main__':                                               # the measurements behind R_E, R_E_NORMAL and RHO_L
    worst = [0.0, 0.0, 0.0, 0.0]
    for case in CASES:
        for kind in LABEL_KINDS if case['name'] not in BIG_IDS else ['uniform']:
            if kind == 'all255':
                continue
            r = parent_ratios(case, kind)
            worst = [max(a, b) for a, b in zip(worst, r)]
            observed(f'parent (fp32 torch, CPU) {case["name"]} {kind}: errors worst ratio {r[0]:.3e}, over f + p64 >= 2^-100 {r[1]:.3e}; '
                     f'gradient worst err / A {r[2]:.3e}, over A >= 2^-90 {r[3]:.3e}')
    observed(f'parent worst: errors {worst[0]:.3e} (x 4 = {4 * worst[0]:.3e}), normal range {worst[1]:.3e} (x 4 = {4 * worst[1]:.3e}; '
             f'floor 2^-22 = {2.0 ** -22:.3e}), gradient {worst[2]:.3e} (x 4 = {4 * worst[2]:.3e}), normal range {worst[3]:.3e} '
             f'(x 4 = {4 * worst[3]:.3e}; floor 2^-20 = {2.0 ** -20:.3e})')
