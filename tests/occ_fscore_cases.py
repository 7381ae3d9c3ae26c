"""Case table, input generators, reference and checks for fbbev_occ_fscore_counts (fb_bev_amd/csrc/occ_fscore_kernels.h), shared by the
emulator test (tests/test_emu_occ_fscore.py, through tests/emu/emu_capi.py's library) and the GPU test (tests/test_gpu_occ_fscore.py,
through fb_bev_amd._capi.occ_fscore_counts).

The reference is the definition written out, independent of the product's tables and shifted arrays: the occupied voxels of both
maps as integer triples, their float64 coordinates `i * voxel_size + voxel_size / 2 + lower`, and for every point a look at all cells
within R + 1 of it: hit iff sqrt((dx*dx + dy*dy) + dz*dz) < threshold for some point of the other set.  The tables handed to the entry
are built here as well (coordinates cut from the 200-cell axis at an index offset, squared differences, the threshold constant by
math.nextafter, the offset list as the full cube or pruned).  Everything compared is an integer: no tolerance anywhere.

Plain Python, numpy and CPU torch only; the adapters import their library on first use.
"""
import ctypes
import math
import os
import sys

import numpy as np
import torch

GUARD = 16                       # int32 words in front of and behind `counts`
PATTERN = 0x5A5A5A5A
FREE = 17
E_BADARG, E_UNSUPPORTED = -1, -2
TILE = 16                        # columns per side of the kernel's tile


def observed(text):
    print(f'[observed] {text}')


def _case(name, B, X, Y, Z, i0=(0, 0, 0)):
    return dict(name=name, B=B, X=X, Y=Y, Z=Z, i0=i0)


CASES = [
    _case('b2_5x7x3', 2, 5, 7, 3, i0=(3, 120, 2)),               # 1: nothing is a multiple of a tile or a wave
    _case('b1_16x16x16', 1, 16, 16, 16, i0=(91, 40, 0)),         # 2: whole tiles
    _case('b1_17x33x16', 1, 17, 33, 16, i0=(150, 7, 0)),         # 3: one row and one column over
    _case('b1_9x6x1', 1, 9, 6, 1, i0=(60, 60, 7)),               # 4: Z at its bounds
    _case('b1_6x9x32', 1, 6, 9, 32, i0=(20, 180, 0)),
    _case('b1_200x200x16', 1, 200, 200, 16),                     # 6: the reference grid
]
CASE_IDS = [c['name'] for c in CASES]
BIG = 'b1_200x200x16'
REFUSED = _case('b1_4x4x33', 1, 4, 4, 33)                        # 5: FBBEV_E_UNSUPPORTED

VOXEL, LOWER = (0.4, 0.4, 0.4), (-40, -40, -1)                   # the reference's grid (range[:3])
# (threshold_acc, threshold_complete, voxel_size): a swapped pair of constants fails (0.4, 0.8) or (0.8, 0.4); (1.2, 1.2) gives R = 4
THRESHOLDS = [(0.4, 0.4, VOXEL), (0.6, 0.6, VOXEL), (0.4, 0.8, VOXEL), (0.8, 0.4, VOXEL), (1.2, 1.2, VOXEL), (0.6, 0.6, (0.5, 0.25, 0.4))]
VOIDS = [[17, 255], [0], []]                                     # [] : masked voxels (effective id 255) count as occupied
PATTERNS = ['sparse', 'dense', 'shift100', 'shift110', 'shift001', 'shift200', 'empty_pred', 'empty_gt', 'all_masked', 'planted']


# ------------------------------------------------------------------------------------------------------------------ tables
def coordinates(case, voxel):
    return [np.arange(i0, i0 + n) * vs + vs / 2 + r0 for i0, n, vs, r0 in zip(case['i0'], (case['X'], case['Y'], case['Z']), voxel, LOWER)]


def radius(thresholds, voxel):
    return max(int(math.floor(round(t / v, 9))) + 1 for t in thresholds for v in voxel)


def threshold_constant(thr):
    t = thr * thr
    while math.sqrt(t) >= thr:
        t = math.nextafter(t, -math.inf)
    while math.sqrt(math.nextafter(t, math.inf)) < thr:
        t = math.nextafter(t, math.inf)
    assert math.sqrt(t) < thr <= math.sqrt(math.nextafter(t, math.inf))
    return t


def tables(case, t_acc, t_cmpl, voxel, full_cube):
    R = radius((t_acc, t_cmpl), voxel)
    sq = []
    for c in coordinates(case, voxel):
        t = np.full((len(c), 2 * R + 1), np.inf)
        for i in range(len(c)):
            for o in range(-R, R + 1):
                if 0 <= i + o < len(c):
                    t[i, o + R] = (c[i] - c[i + o]) * (c[i] - c[i + o])
        sq.append(t)
    T_acc, T_cmpl = threshold_constant(t_acc), threshold_constant(t_cmpl)
    cube = [(ox, oy, oz) for ox in range(-R, R + 1) for oy in range(-R, R + 1) for oz in range(-R, R + 1)]
    if not full_cube:
        lo = [t.min(0) for t in sq]
        cube = [o for o in cube if (lo[0][o[0] + R] + lo[1][o[1] + R]) + lo[2][o[2] + R] <= max(T_acc, T_cmpl)]
    return dict(R=R, sq=sq, T_acc=T_acc, T_cmpl=T_cmpl, offsets=np.array(cube, dtype=np.int32).reshape(-1, 3))


def _adjacent_sides(case):
    """how many adjacent x pairs of the case's own coordinates are closer than 0.4, and how many are not"""
    c = coordinates(case, VOXEL)[0]
    d = np.sqrt(((c[1:] - c[:-1]) * (c[1:] - c[:-1]) + 0.0) + 0.0)
    return int((d < 0.4).sum()), int((d >= 0.4).sum())


for _c in CASES:                 # a case whose adjacent pairs all fall on one side of 0.4 would not test the rounding
    if _c['X'] >= 5:
        assert min(_adjacent_sides(_c)) > 0, (_c['name'], _adjacent_sides(_c))
assert _adjacent_sides(CASES[-1]) == (130, 69)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _seed(case, pattern):
    return case['X'] * 131 + case['Y'] * 17 + case['Z'] * 3 + PATTERNS.index(pattern) * 1009


def _ids(rng, occ):
    """class ids for an occupancy mask: free outside; inside mostly 0..16, some ids above 17, a few 255"""
    ids = rng.integers(0, 17, occ.shape)
    r = rng.random(occ.shape)
    ids = np.where(r < 0.1, rng.integers(18, 255, occ.shape), ids)
    ids = np.where(r > 0.97, 255, ids)
    return np.where(occ, ids, FREE).astype(np.uint8)


def _plant(case, P, G):
    """pairs straddling every tile edge in x and in y (straight and diagonal), and voxels at the faces and corners, where the halo
    lies outside the grid"""
    X, Y, Z = case['X'], case['Y'], case['Z']
    zs = sorted({0, Z // 2, Z - 1})
    for e in [t for t in range(TILE, X, TILE)] + [X - 1]:          # the last cell pair as well
        for y in sorted({0, Y // 2, Y - 1, min(TILE, Y - 1), min(TILE - 1, Y - 1)}):
            for z in zs:
                G[e - 1, y, z] = True
                P[e, y, z] = True
                if y + 1 < Y:
                    P[e, y + 1, z] = True
    for e in [t for t in range(TILE, Y, TILE)] + [Y - 1]:
        for x in sorted({0, X // 2, X - 1, min(TILE, X - 1), min(TILE - 1, X - 1)}):
            for z in zs:
                P[x, e - 1, z] = True
                G[x, e, z] = True
                if x + 1 < X and z + 1 < Z:
                    G[x + 1, e, z + 1] = True
    for x in (0, X - 1):
        for y in (0, Y - 1):
            for z in (0, Z - 1):
                G[x, y, z] = True
                P[min(x + 1, X - 1) if x == 0 else max(x - 1, 0), y, z] = True


def make_inputs(case, pattern):
    """-> pred, gt, mask: (B, X, Y, Z) uint8.  The patterns with a special frame have it in the middle of a batch of three."""
    rng = np.random.default_rng(_seed(case, pattern))
    X, Y, Z = case['X'], case['Y'], case['Z']
    special = pattern in ('empty_pred', 'empty_gt', 'all_masked')
    B = 3 if special else case['B']
    pred, gt, mask = [], [], []
    for b in range(B):
        density = {'sparse': 0.02, 'dense': 0.6, 'planted': 0.01}.get(pattern, 0.1)
        G = rng.random((X, Y, Z)) < density
        if pattern.startswith('shift'):
            d = [int(ch) for ch in pattern[5:]]
            P = np.zeros_like(G)
            P[d[0]:, d[1]:, d[2]:] = G[:X - d[0], :Y - d[1], :Z - d[2]]
        else:
            P = np.where(rng.random((X, Y, Z)) < 0.5, G, rng.random((X, Y, Z)) < density)
        if pattern == 'planted':
            _plant(case, P, G)
        m = (rng.random((X, Y, Z)) < 0.66).astype(np.uint8) * rng.integers(1, 256, (X, Y, Z)).astype(np.uint8)   # any non-zero byte
        if special and b == 1:
            if pattern == 'empty_pred':
                P[:] = False
            elif pattern == 'empty_gt':
                G[:] = False
            else:
                m[:] = 0
        pred.append(_ids(rng, P))
        gt.append(_ids(rng, G))
        mask.append(m)
    return np.stack(pred), np.stack(gt), np.stack(mask)


# ------------------------------------------------------------------------------------------------------------------ reference
def occupied(ids, mask, void):
    eff = ids.astype(np.int64) if mask is None else np.where(mask != 0, ids, 255).astype(np.int64)
    occ = np.ones(eff.shape, dtype=bool)
    for v in void:
        occ &= eff != v
    return occ


def _hits(Q, S, coords, thr, reach):
    """how many points of Q (bool volume) have a point of S closer than thr: every cell within `reach` of the point is looked at"""
    q = np.argwhere(Q)
    if len(q) == 0:
        return 0
    X, Y, Z = Q.shape
    cx, cy, cz = coords
    hit = np.zeros(len(q), dtype=bool)
    for ox in range(-reach, reach + 1):
        tx = q[:, 0] + ox
        okx = (tx >= 0) & (tx < X)
        dx = cx[q[:, 0]] - cx[np.clip(tx, 0, X - 1)]
        for oy in range(-reach, reach + 1):
            ty = q[:, 1] + oy
            oky = okx & (ty >= 0) & (ty < Y)
            dy = cy[q[:, 1]] - cy[np.clip(ty, 0, Y - 1)]
            dxy = dx * dx + dy * dy
            for oz in range(-reach, reach + 1):
                tz = q[:, 2] + oz
                ok = oky & (tz >= 0) & (tz < Z)
                dz = cz[q[:, 2]] - cz[np.clip(tz, 0, Z - 1)]
                there = S[np.clip(tx, 0, X - 1), np.clip(ty, 0, Y - 1), np.clip(tz, 0, Z - 1)]
                hit |= ok & there & (np.sqrt(dxy + dz * dz) < thr)
    return int(hit.sum())


def reference_counts(case, pred, gt, mask, void, t_acc, t_cmpl, voxel):
    """(B, 4) int64: n_gt, n_pred, n_cmpl, n_acc per frame"""
    coords = coordinates(case, voxel)
    reach = radius((t_acc, t_cmpl), voxel) + 1
    out = []
    for b in range(pred.shape[0]):
        m = None if mask is None else mask[b]
        P, G = occupied(pred[b], m, void), occupied(gt[b], m, void)
        out.append((int(G.sum()), int(P.sum()), _hits(G, P, coords, t_cmpl, reach), _hits(P, G, coords, t_acc, reach)))
    return np.array(out, dtype=np.int64)


_REF = {}


def reference(case, pattern, k, void, use_mask):
    """inputs and expected counts, computed once per combination and shared; callers leave them unchanged"""
    key = (case['name'], pattern, k, tuple(void), use_mask)
    if key not in _REF:
        t_acc, t_cmpl, voxel = THRESHOLDS[k]
        pred, gt, mask = make_inputs(case, pattern)
        want = reference_counts(case, pred, gt, mask if use_mask else None, void, t_acc, t_cmpl, voxel)
        _REF[key] = (pred, gt, mask if use_mask else None, want)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------ adapters
def void_words(void):
    bits = (ctypes.c_uint32 * 8)()
    for v in void:
        bits[v >> 5] |= 1 << (v & 31)
    return bits


class EmuApi:
    """the C entry of the CPU-emulated library, CPU tensors"""
    name = 'emu'

    def __init__(self):
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
        import emu_capi
        self.lib = emu_capi.lib()

    def dev(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).clone()

    def cpu(self, t):
        return t

    def call(self, pred, gt, mask, bits, sq, offsets, R, T_acc, T_cmpl, counts):
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        B, X, Y, Z = pred.shape
        return self.lib.fbbev_occ_fscore_counts(p(pred), p(gt), p(mask), ctypes.cast(bits, ctypes.c_void_p), p(sq[0]), p(sq[1]), p(sq[2]),
                                                p(offsets), offsets.shape[0], R, T_acc, T_cmpl, B, X, Y, Z, p(counts), None)


class GpuApi:
    """fb_bev_amd._capi.occ_fscore_counts on cuda:0"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi
        self.c = _capi
        self.device = torch.device('cuda:0')

    def dev(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def cpu(self, t):
        return t.cpu()

    def call(self, pred, gt, mask, bits, sq, offsets, R, T_acc, T_cmpl, counts):
        got = self.c.occ_fscore_counts(pred, gt, mask, bits, sq[0], sq[1], sq[2], offsets, R, T_acc, T_cmpl, counts=counts)
        assert got is counts
        return 0


def run(api, case, pred, gt, mask, void, k, full_cube, prefill=None):
    """one call -> (B, 4) int64 counts ADDED by the call.  `counts` is a slice of a larger patterned buffer, pre-filled with non-zero
    values; the guard words must come back intact and the three byte maps unwritten."""
    t_acc, t_cmpl, voxel = THRESHOLDS[k]
    tab = tables(case, t_acc, t_cmpl, voxel, full_cube)
    B = pred.shape[0]
    fill = (np.arange(4 * B, dtype=np.int32) * 7 + 3) if prefill is None else prefill
    host = np.full(GUARD + 4 * B + GUARD, PATTERN, dtype=np.int32)
    host[GUARD:GUARD + 4 * B] = fill
    buf = api.dev(host)
    counts = buf[GUARD:GUARD + 4 * B].view(B, 4)
    d_pred, d_gt, d_mask = api.dev(pred), api.dev(gt), api.dev(mask)
    code = api.call(d_pred, d_gt, d_mask, void_words(void), [api.dev(t) for t in tab['sq']], api.dev(tab['offsets']), tab['R'],
                    tab['T_acc'], tab['T_cmpl'], counts)
    assert code == 0, code
    back = api.cpu(buf).numpy()
    assert (back[:GUARD] == PATTERN).all() and (back[GUARD + 4 * B:] == PATTERN).all(), 'guard words overwritten'
    for was, now, what in ((pred, d_pred, 'classes'), (gt, d_gt, 'gt'), (mask, d_mask, 'mask')):
        assert was is None or np.array_equal(was, api.cpu(now).numpy()), f'{what} was written to'
    return (back[GUARD:GUARD + 4 * B].astype(np.int64) - fill.astype(np.int64)).reshape(B, 4)


# ------------------------------------------------------------------------------------------------------------------ checks
def thresholds_for(case, pattern):
    """the threshold rows a (case, pattern) runs: all of them, the reference grid one (the one `eval` uses)"""
    if case['name'] == BIG:
        return [0]
    return list(range(len(THRESHOLDS)))


def check_counts(api, case, pattern):
    """every threshold row; the void list, mask / no mask and full cube / pruned offsets rotate with the row, so that each shape meets
    each of them"""
    p = PATTERNS.index(pattern)
    for k in thresholds_for(case, pattern):
        big = case['name'] == BIG
        void = VOIDS[0] if big else VOIDS[(k + p) % 3]
        use_mask = big or (k + p) % 4 != 3
        full_cube = not big and (k + p) % 2 == 0
        pred, gt, mask, want = reference(case, pattern, k, void, use_mask)
        got = run(api, case, pred, gt, mask, void, k, full_cube)
        observed(f'{api.name} {case["name"]} {pattern} thresholds {THRESHOLDS[k][:2]} voxel {THRESHOLDS[k][2]} void {void} '
                 f'mask={use_mask} cube={full_cube}: counts {got.tolist()}, reference {want.tolist()}')
        assert np.array_equal(got, want)
        if pattern in ('dense', 'planted'):
            assert want[:, :2].min() > 0                            # both sets are there (2 % of 105 voxels may be none)
        if pattern == 'empty_pred' and 17 in void:
            assert want[1, 1] == 0 and want[1, 0] > 0 and want[0, 1] > 0 and want[2, 1] > 0
        if pattern == 'empty_gt' and 17 in void:
            assert want[1, 0] == 0 and want[1, 1] > 0 and want[0, 0] > 0 and want[2, 0] > 0
        if pattern == 'all_masked' and use_mask:
            nv = case['X'] * case['Y'] * case['Z']
            assert tuple(want[1]) == ((0, 0, 0, 0) if 255 in void else (nv, nv, nv, nv))


def check_voids_and_null_mask(api, case):
    """every void list, with and without a mask, at the thresholds of `eval`"""
    for void in VOIDS:
        for use_mask in (True, False):
            pred, gt, mask, want = reference(case, 'dense', 0, void, use_mask)
            got = run(api, case, pred, gt, mask, void, 0, full_cube=False)
            observed(f'{api.name} {case["name"]} void {void} mask={use_mask}: counts {got.tolist()}, reference {want.tolist()}')
            assert np.array_equal(got, want)
            assert (pred > 17).any() and (gt > 17).any()


def check_rounding_decides(api, case):
    """prediction = labels shifted one cell along x at threshold 0.4: the hits are neither none nor all, and a whole-cell rule
    ("threshold 0.4 -> the same cell only") would count none"""
    pred, gt, mask, want = reference(case, 'shift100', 0, VOIDS[0], True)
    got = run(api, case, pred, gt, mask, VOIDS[0], 0, full_cube=False)
    assert np.array_equal(got, want)
    P, G = occupied(pred[0], mask[0], VOIDS[0]), occupied(gt[0], mask[0], VOIDS[0])
    same_cell = int((P & G).sum())
    observed(f'{api.name} {case["name"]}: n_acc {int(want[0, 3])} of {int(want[0, 1])}, in the same cell {same_cell}')
    assert same_cell < want[0, 3] < want[0, 1]
