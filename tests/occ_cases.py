"""Case table, input generators, references and checks for fbbev_occ_classes (fb_bev_amd/csrc/occ_kernels.h), shared by the emulator
test (tests/test_emu_occ_classes.py, through tests/emu/emu_capi.py's library) and the GPU test (tests/test_gpu_occ_classes.py, through
fb_bev_amd._capi.occ_classes).

Logits are multiples of 0.25 in [-10, 10] from a seeded generator, with planted voxels: exact ties of two, three and all scored classes
(the lowest index must win), NaN, +inf, -inf, all -inf, and a NaN in the void channel outside the scored slice (which must NOT force
class 0).  The reference for `classes` is the parent's chain of FBOCC.predict_occupancy evaluated by torch on the CPU: slice,
softmax(1), argmax, permute / flip / rot90 / permute, cast to uint8.  The parent decides after an fp32 softmax, where two different
logits could round to one probability; voxels where that happens (parent != the rule "lowest index among the maxima of the logits, 0
with a NaN or +inf") may be left out, and every check asserts that their share is 0 on these inputs.  The reference for `hist` is a
numpy bincount written here.  Everything is integers and bytes: no tolerance anywhere.

Plain Python, numpy and CPU torch only; the adapters import their library on first use.
"""
import ctypes
import os
import sys

import numpy as np
import torch

GUARD = 64                       # pattern bytes in front of and behind `classes`
PATTERN = 0xA5


def observed(text):
    print(f'[observed] {text}')


def _case(name, B, H, W, D, layout, C=19, c0=1, padded=False):
    return dict(name=name, B=B, H=H, W=W, D=D, C=C, c0=c0, layout=layout, padded=padded)


# tile of the kernel: 8 x 8 columns x the whole depth at D >= 16 (16 x 16 below), 256 voxels per step, four output bytes per lane
# where D % 4 == 0 and the pointers are aligned
CASES = [
    # 1: nothing is a multiple of a tile, a wave or 4 bytes: the byte stores of the transposed output hit every alignment
    _case('b2_5x7x3_cl', 2, 5, 7, 3, 'cl'), _case('b2_5x7x3_planes', 2, 5, 7, 3, 'planes'),
    # 2: the shipped depth with whole tiles, then one row and one column over
    _case('b1_16x16x16_cl', 1, 16, 16, 16, 'cl'), _case('b1_16x16x16_planes', 1, 16, 16, 16, 'planes'),
    _case('b1_17x33x16_cl', 1, 17, 33, 16, 'cl'), _case('b1_17x33x16_planes', 1, 17, 33, 16, 'planes'),
    # 3: the batch stride is larger than the tensor (a slice of a bigger buffer) and the storage offset is non-zero
    _case('b2_8x8x16_cl_padded', 2, 8, 8, 16, 'cl', padded=True), _case('b2_8x8x16_planes_padded', 2, 8, 8, 16, 'planes', padded=True),
    # 4, 5: n at its bounds
    _case('b1_6x6x4_n2_cl', 1, 6, 6, 4, 'cl', C=2, c0=0), _case('b1_6x6x4_n2_planes', 1, 6, 6, 4, 'planes', C=2, c0=0),
    _case('b1_6x6x4_n32_cl', 1, 6, 6, 4, 'cl', C=33, c0=1), _case('b1_6x6x4_n32_planes', 1, 6, 6, 4, 'planes', C=33, c0=1),
    # the kernel's other paths: a depth above 64 is walked in chunks (64 + 6, column runs instead of row runs); a channels-last row of
    # more than 40 floats is not staged through LDS but read in place
    _case('b1_3x9x70_cl', 1, 3, 9, 70, 'cl'), _case('b1_3x9x70_planes', 1, 3, 9, 70, 'planes'),
    _case('b1_9x3x20_c45_cl', 1, 9, 3, 20, 'cl', C=45, c0=20),
    # 6: the reference's hard-coded ring grid (the metric fixture's)
    _case('b1_200x200x2_cl', 1, 200, 200, 2, 'cl'),
]
CASE_IDS = [c['name'] for c in CASES]


def _seed(case, extra=0):
    return case['B'] * 7 + case['H'] * 131 + case['W'] * 17 + case['D'] * 3 + case['C'] * 1009 + extra


# ------------------------------------------------------------------------------------------------------------------ inputs
def logical_logits(case, skew=None):
    """(B, C, H, W, D) contiguous f32.  skew = (class, share): that share of the voxels gets `class` as its only maximum."""
    g = torch.Generator().manual_seed(_seed(case))
    B, C, H, W, D, c0 = (case[k] for k in ('B', 'C', 'H', 'W', 'D', 'c0'))
    n = C - c0
    nv = B * H * W * D
    V = torch.randint(-40, 41, (nv, C), generator=g).float() / 4    # one row per voxel
    done = lambda: V.view(B, H, W, D, C).permute(0, 4, 1, 2, 3).contiguous()  # noqa: E731
    order = torch.randperm(nv, generator=g)
    if skew is not None:
        cls, share = skew
        rows = order[:int(nv * share)]
        V[rows] = V[rows].clamp(max=9.75)
        V[rows, c0 + cls] = 10.0
        return done()
    k = max(nv // 40, 1)
    take = lambda i: order[i * k:(i + 1) * k]  # noqa: E731
    pick = lambda m: c0 + torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(k)])  # noqa: E731  (k, m) distinct scored channels
    rows = take(0)                                                  # two classes tie at the maximum
    V[rows[:, None], pick(min(2, n))] = 10.0
    rows = take(1)                                                  # three
    V[rows[:, None], pick(min(3, n))] = 10.0
    rows = take(2)                                                  # all scored classes equal
    V[rows, c0:] = torch.randint(-40, 41, (k, 1), generator=g).float() / 4
    V[take(3)[:, None], pick(1)] = float('nan')
    V[take(4)[:, None], pick(1)] = float('inf')
    V[take(5)[:, None], pick(1)] = float('-inf')
    V[take(6), c0:] = float('-inf')
    if c0 > 0:
        V[take(7), 0] = float('nan')                                # the void channel: outside the scored slice
    return done()


def lay_out(case, L):
    """-> (storage 1-D f32, size, stride, offset): L in the case's memory layout.  'cl': the NCDHW view of channels-last memory the MFMA
    head runner returns; 'planes': contiguous class planes; padded: a slice of a bigger buffer (batch stride + 37, offset 5)."""
    B, C, H, W, D = L.shape
    per = C * H * W * D
    sb, off = (per + 37, 5) if case['padded'] else (per, 0)
    storage = torch.full((off + B * sb,), 7.5)
    if case['layout'] == 'cl':
        stride = (sb, 1, W * D * C, D * C, C)
        src = L.permute(0, 2, 3, 4, 1)
    else:
        stride = (sb, H * W * D, W * D, D, 1)
        src = L
    for b in range(B):
        storage[off + b * sb: off + b * sb + per] = src[b].reshape(-1)
    view = storage.as_strided(tuple(L.shape), stride, off)
    assert torch.equal(torch.nan_to_num(view, 1e9, 2e9, -2e9), torch.nan_to_num(L, 1e9, 2e9, -2e9))
    return storage, tuple(L.shape), stride, off


def labels(case, kind, pred=None):
    """gt (B, W, H, D) uint8.  'uniform': every class, plus 255 and the value n itself; 'skewed': 95 % of the voxels are ONE
    (gt, prediction) pair (the inputs come from logical_logits(skew=...))."""
    g = torch.Generator().manual_seed(_seed(case, 1))
    B, H, W, D, n = case['B'], case['H'], case['W'], case['D'], case['C'] - case['c0']
    gt = torch.randint(0, n, (B, W, H, D), generator=g, dtype=torch.uint8)
    nv = gt.numel()
    order = torch.randperm(nv, generator=g)
    k = max(int(nv * (0.01 if kind == 'skewed' else 0.04)), 1)          # voxels labelled 255, and as many labelled n
    if kind == 'skewed':
        gt[pred == SKEW[1]] = SKEW[0]
    gt.view(-1)[order[:k]] = 255
    gt.view(-1)[order[k:2 * k]] = n
    return gt


SKEW = (1, 0)                    # (gt, prediction) of the skewed case, both < 2 so that n = 2 has it too


def masks(case):
    g = torch.Generator().manual_seed(_seed(case, 2))
    B, H, W, D = case['B'], case['H'], case['W'], case['D']
    return (torch.rand((B, W, H, D), generator=g) < 0.7).to(torch.uint8), (torch.rand((W, H), generator=g) < 0.6).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------ references
def parent_classes(L, c0):
    """FBOCC.predict_occupancy's chain on the CPU -> uint8 (B, X', Y', Z)"""
    occ = L[:, c0:].softmax(1)
    x = occ.argmax(1, keepdim=True)
    x = x.permute(0, 1, 4, 2, 3)
    x = torch.rot90(torch.flip(x, [3]), -1, [3, 4])
    x = x.permute(0, 3, 4, 2, 1)
    return x[..., 0].to(torch.uint8).contiguous()


def rule_classes(L, c0):
    """lowest index among the maxima of the scored logits, 0 with a NaN or +inf among them; H <-> W transposed"""
    S = L[:, c0:]
    bad = (torch.isnan(S) | (S == float('inf'))).any(1)
    idx = torch.nan_to_num(S, nan=0.0).argmax(1)       # torch's argmax returns the first maximal index
    first = (torch.nan_to_num(S, nan=0.0) == torch.nan_to_num(S, nan=0.0).max(1, keepdim=True).values).float().argmax(1)
    assert torch.equal(idx, first)
    return torch.where(bad, torch.zeros_like(first), first).permute(0, 2, 1, 3).to(torch.uint8).contiguous()


def hist_ref(n, pred, gt, mask, column_mask):
    keep = gt.numpy() < n
    if mask is not None:
        keep &= mask.numpy() != 0
    if column_mask is not None:
        keep &= (column_mask.numpy() != 0)[None, :, :, None]
    key = gt.numpy()[keep].astype(np.int64) * n + pred.numpy()[keep].astype(np.int64)
    return torch.from_numpy(np.bincount(key, minlength=n * n).reshape(n, n).astype(np.int32))


_REF = {}


def reference(case, skewed=False):
    """(L, parent classes), computed once per case and shared; callers leave them unchanged"""
    key = (case['name'], skewed)
    if key not in _REF:
        L = logical_logits(case, skew=(SKEW[1], 0.98) if skewed else None)
        S = L[:, case['c0']:]
        if not skewed:                                              # the planted voxels are there
            top = (S == S.max(1, keepdim=True).values).sum(1)
            assert (top == 2).any() and (top >= min(3, S.shape[1])).any() and (top == S.shape[1]).any()
            assert torch.isnan(S).any() and (S == float('inf')).any() and (S == float('-inf')).all(1).any()
            assert case['c0'] == 0 or (torch.isnan(L[:, 0]) & ~torch.isnan(S).any(1)).any()
        exp, rule = parent_classes(L, case['c0']), rule_classes(L, case['c0'])
        left_out = int((exp != rule).sum())
        observed(f'{case["name"]}{" skewed" if skewed else ""}: voxels where the fp32 softmax merges two logits = {left_out} of {exp.numel()}')
        assert left_out == 0
        _REF[key] = (L, exp)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------ adapters
class EmuApi:
    """the C entry of the CPU-emulated library, CPU tensors"""
    name = 'emu'

    def __init__(self):
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
        import emu_capi
        self.lib = emu_capi.lib()

    def dev(self, t):
        return None if t is None else t.clone()

    def cpu(self, t):
        return t

    def call(self, view, c0, out, gt, mask, cm, hist):
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        B, C, H, W, D = view.shape
        return self.lib.fbbev_occ_classes(p(view), *view.stride(), B, C, c0, H, W, D, p(out), p(gt), p(mask), p(cm), p(hist), None)


class GpuApi:
    """fb_bev_amd._capi.occ_classes on cuda:0"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi
        self.c = _capi
        self.device = torch.device('cuda:0')

    def dev(self, t):
        return None if t is None else t.to(self.device)

    def cpu(self, t):
        return t.cpu()

    def call(self, view, c0, out, gt, mask, cm, hist):
        got = self.c.occ_classes(view, c0=c0, gt=gt, mask=mask, column_mask=cm, hist=hist, out=out)
        assert got is out
        return 0


def run(api, case, L, gt=None, mask=None, cm=None, hist=None, misalign=0):
    """one call -> (classes (B, W, H, D) uint8, hist or None) on the CPU.  `classes` is a slice of a larger patterned buffer whose guard
    bytes must come back intact; gt / mask / column_mask must come back unchanged."""
    storage, size, stride, off = lay_out(case, L)
    B, C, H, W, D = size
    nvox = B * H * W * D
    view = api.dev(storage).as_strided(size, stride, off)
    buf = api.dev(torch.full((GUARD + misalign + nvox + GUARD,), PATTERN, dtype=torch.uint8))
    out = buf[GUARD + misalign: GUARD + misalign + nvox].view(B, W, H, D)
    d_gt, d_mask, d_cm, d_hist = api.dev(gt), api.dev(mask), api.dev(cm), api.dev(hist)
    code = api.call(view, case['c0'], out, d_gt, d_mask, d_cm, d_hist)
    assert code == 0, code
    back = api.cpu(buf)
    assert (back[:GUARD + misalign] == PATTERN).all() and (back[GUARD + misalign + nvox:] == PATTERN).all(), 'guard bytes overwritten'
    for was, now, what in ((gt, d_gt, 'gt'), (mask, d_mask, 'mask'), (cm, d_cm, 'column_mask')):
        assert was is None or torch.equal(was, api.cpu(now)), f'{what} was written to'
    nn = lambda t: torch.nan_to_num(t, 1e9, 2e9, -2e9)  # noqa: E731
    assert torch.equal(nn(api.cpu(view)), nn(L)), 'the logits were written to'
    return back[GUARD + misalign: GUARD + misalign + nvox].view(B, W, H, D).clone(), None if hist is None else api.cpu(d_hist)


# ------------------------------------------------------------------------------------------------------------------ checks
def check_classes(api, case):
    """classes alone (hist == NULL, gt == NULL), on an aligned and on an odd output address"""
    L, exp = reference(case)
    for misalign in (0, 3):
        got, _ = run(api, case, L, misalign=misalign)
        bad = int((got != exp).sum())
        observed(f'{api.name} {case["name"]} (+{misalign}): class bytes that differ from the parent chain = {bad} of {exp.numel()}')
        assert torch.equal(got, exp)


def check_hist(api, case, kind):
    """hist with and without mask / column_mask, added to a pre-filled table"""
    n = case['C'] - case['c0']
    L, exp = reference(case, skewed=(kind == 'skewed'))
    gt = labels(case, kind, exp)
    mask, cm = masks(case)
    assert (gt == 255).any() and (gt == n).any()
    if kind == 'skewed':
        share = ((gt == SKEW[0]) & (exp == SKEW[1])).float().mean().item()
        observed(f'{case["name"]} skewed: share of voxels in the one (gt, prediction) pair = {share:.3f}')
        assert share >= 0.95            # 98 % planted, 2 % labelled 255 or n
    pattern = (torch.arange(n * n, dtype=torch.int32) * 7 - 11).view(n, n)
    big = case['B'] * case['H'] * case['W'] * case['D'] > 20000
    for use_mask, use_cm in ((True, True),) if big else ((True, True), (True, False), (False, True), (False, False)):
        m, c = (mask if use_mask else None), (cm if use_cm else None)
        want = hist_ref(n, exp, gt, m, c)
        got, hist = run(api, case, L, gt=gt, mask=m, cm=c, hist=pattern.clone())
        assert torch.equal(got, exp)
        bad = int((hist - pattern != want).sum())
        observed(f'{api.name} {case["name"]} {kind} mask={use_mask} column_mask={use_cm}: bins that differ from bincount = {bad} of {n * n}; '
                 f'counted {int(want.sum())}, largest bin {int(want.max())}')
        assert torch.equal(hist - pattern, want)
        assert int(want.sum()) > 0
