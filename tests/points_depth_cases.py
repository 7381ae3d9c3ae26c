"""Case table, input generators, references and checks for fbbev_points_to_depth (fb_bev_amd/csrc/points_depth_kernels.h), shared by the
emulator test (tests/test_emu_points_depth.py, through tests/emu/emu_capi.py's library) and the GPU test
(tests/test_gpu_points_depth.py, through fb_bev_amd._capi.points_to_depth).

EXACT LAYER.  Every camera's lidar2img is a signed permutation of the axes scaled by a power of two with a dyadic translation, post_rot
has a signed permutation of +-0.5 / +-1 entries in its upper 2 x 2 and (0, 0, 1) as its third row, post_tran is dyadic.  A point is
built backwards from a target (camera, q.x / ds, q.y / ds, depth) with few mantissa bits and rounded to fp32.  The chain is then
evaluated in float64 from the fp32 inputs for EVERY camera of the sample, and a point stays in the case only if every (point, camera)
pair is safe: either every product, sum and quotient of the pair is representable in fp32 (a dot product has one non-zero term, so
every association and contraction gives the same bits), or the pair's depth q.z is exact and outside [lo, hi) -- or NaN -- so that the
pair is dropped whatever its inexact pixel coordinates are.  Planted points (the edges of a case) are asserted to stay.  The float64
evaluation is then THE answer: a pixel with a kept point equals the minimum kept depth bit for bit, every other pixel is +0.0.

REAL LAYER (`shipped`, `stride5_batch`).  nuScenes-like calibration: focal 1266, principal point (816, 491), six cameras 60 degrees
apart with a sensor offset, post_rot = 0.44 x a rotation of a few degrees (one camera flipped), points in a 50 m disc.  The
reference is the float64 evaluation of the same formulas from the fp32 inputs.  Bounds, with u = 2^-24, gamma_k = k u / (1 - k u),
valid for any association and any contraction of the dot products (the kernel's fmaf chain or a BLAS's):
  c_i = sum_j M_ij p_j + t_i is three products and three sums in some order, no term passes more than 4 roundings:
      |c^_i - c_i| <= e_i = gamma_4 (sum_j |M_ij| |p_j| + |t_i|).
  U = c_0 / c_2 from the computed c^ (needs c_2 > 2 e_2), one correctly rounded division:
      |U^ - U| <= dU = (e_0 + |U| e_2) / (c_2 - e_2) + u (|U| + (e_0 + |U| e_2) / (c_2 - e_2));   V = c_1 / c_2 likewise.
  q_i = sum_j R_ij w_j + T_i on w = (U^, V^, c^_2) with input errors dw = (dU, dV, e_2):
      |q^_i - q_i| <= dq_i = sum_j |R_ij| dw_j + gamma_4 (sum_j |R_ij| (|w_j| + dw_j) + |T_i|).
  The pixel coordinate q_i / ds, one correctly rounded division: tau_i = dq_i / ds + u (|q_i| + dq_i) / ds   (i = 0, 1).
  The depth: dz = dq_2.
A point-camera pair with c_2 <= 2 e_2 has |q_2| <= 3 e_2 + ... far below lo (post_rot's third row is (0, 0, 1) here): it is decided
and dropped, as a NaN or an infinite coordinate is.  Every other pair is DECIDED when q_0 / ds and q_1 / ds are farther than tau
from every half-integer and q_2 is farther than dz from lo and hi; a pixel is CHECKED when every pair that can reach it (within
0.5 + tau of it in both coordinates) is decided.  On checked pixels emptiness must agree with the float64 map and
|got - min64| <= the largest dz of the pixel's kept pairs.  Unchecked pixels may be at most 2 % of the float64 map's non-empty
pixels (a condition on the seeds).  The fp32 torch restatement of the reference (fb_bev_amd.points_depth on CPU tensors) is held
to the same bounds on the same pixels first -- with the one allowance its own tie rule needs: where kept pairs of a pixel tie with
the nearest one in the fp32 key rank + depth / 100, it may give any of them.

REFERENCE FIXTURE (tests/golden/points_depth_ref.npz, written by tests/golden/make_golden_points_depth.py from the real class on the
exact-layer inputs of ds2_ties, edges, stride5_batch and keyties): same set of non-empty pixels; ours <= ref and
fl32(rank + ours / 100) == fl32(rank + ref / 100) everywhere; equal bits where the pixel's kept points do not tie in the key;
keyties holds at least one pixel where the fixture is strictly larger.

Memory: guard words around `out`, inputs unwritten, two runs identical, `points` at a 4-byte aligned address only (the case's `offset`).

Plain Python, numpy and CPU torch only; the adapters import their library on first use.
"""
import ctypes
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GUARD = 16
PATTERN = 7.5
CAP_POINTS = 64 * 256            # FBBEV_PD_MAX_CHUNKS * FBBEV_PD_THREADS of points_depth_kernels.h: one pass of the capped grid
U = 2.0 ** -24
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'points_depth_ref.npz')
FIXTURE_CASES = ('ds2_ties', 'edges', 'stride5_batch', 'keyties')
KEYTIES_ROWS = (187, 192)        # the rows of keyties that hold points; the fixture stores these rows only


def gamma(k):
    return k * U / (1 - k * U)


def observed(text):
    print(f'[observed] {text}')


def _case(name, B, N, H, W, ds, cfg, stride=3, offset=0, real=False):
    return dict(name=name, B=B, N=N, H=H, W=W, ds=ds, cfg=cfg, stride=stride, offset=offset, real=real)


CASES = [
    _case('px', 1, 1, 4, 4, 1, (1.0, 45.0)),
    _case('ds2_ties', 1, 1, 6, 10, 2, (1.0, 45.0)),
    _case('odd_dims', 1, 2, 7, 9, 2, (1.0, 45.0), offset=1),
    _case('stride5_batch', 3, 2, 32, 88, 1, (2.0, 42.0), stride=5, offset=1, real=True),
    _case('one_pixel', 1, 1, 4, 4, 1, (1.0, 45.0)),
    _case('edges', 1, 1, 4, 16, 1, (1.0, 45.0)),
    _case('blocks', 5, 1, 16, 16, 1, (1.0, 60.0), stride=4),
    _case('keyties', 1, 1, 192, 704, 1, (1.0, 45.0)),
    _case('shipped', 1, 6, 256, 704, 1, (2.0, 42.0), stride=5, real=True),
]
CASE_IDS = [c['name'] for c in CASES]
REAL_CASES = [c for c in CASES if c['real']]
REAL_IDS = [c['name'] for c in REAL_CASES]
BLOCK_COUNTS = (1, 255, 256, 257, CAP_POINTS + 1)


def by_name(name):
    return CASES[CASE_IDS.index(name)]


def dims(case):
    return case['B'], case['N'], case['H'] // case['ds'], case['W'] // case['ds']


# ------------------------------------------------------------------------------------------------------------------ exact cameras
_AXES = [(0, 1, 2, 1), (1, 2, 0, 1), (2, 0, 1, 1), (0, 2, 1, -1), (2, 1, 0, -1), (1, 0, 2, -1)]     # (image x, image y, depth, sign)


def exact_camera(k, H, W):
    """camera k of the exact layer -> M (4, 4), R (3, 3), T (3) float32"""
    ax, ay, az, sgn = _AXES[k % 6]
    s = 2.0 ** ((k % 3) - 1)
    M = np.zeros((4, 4), np.float32)
    M[0, ax], M[1, ay], M[2, az] = s, -s if k % 2 else s, sgn * s
    M[:3, 3] = (2.0 * (k % 2), -1.0 * (k % 3), 0.25 * (k % 2))
    M[3, 3] = 1.0
    R = np.zeros((3, 3), np.float32)
    R[2, 2] = 1.0
    T = np.zeros(3, np.float32)
    kind = k % 4
    if kind == 0:
        R[0, 0], R[1, 1] = 0.5, 0.5
    elif kind == 1:                                                  # flipped in x
        R[0, 0], R[1, 1] = -0.5, 0.5
        T[0] = float(W)
    elif kind == 2:                                                  # axes swapped
        R[0, 1], R[1, 0] = 1.0, 1.0
        T[:2] = (-1.5, 2.0)
    else:                                                            # flipped in y
        R[0, 0], R[1, 1] = 1.0, -1.0
        T[1] = float(H)
    return M, R, T


def back_project(M, R, T, ds, xt, yt, depth):
    """targets (q.x / ds, q.y / ds, depth) float64 arrays -> (P, 3) float32 points that camera (M, R, T) projects there"""
    M, R, T = M.astype(np.float64), R.astype(np.float64), T.astype(np.float64)
    q = np.stack([xt * ds - T[0], yt * ds - T[1]], 0)
    uv = np.linalg.inv(R[:2, :2]) @ q
    z = depth - T[2]
    c = np.stack([uv[0] * z, uv[1] * z, z], 0) - M[:3, 3:4]
    return (np.linalg.inv(M[:3, :3]) @ c).T.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ float64 chain
def _f32ok(a):
    """representable in fp32 (NaN and inf count: they propagate alike in every precision)"""
    with np.errstate(invalid='ignore', over='ignore'):
        return ~np.isfinite(a) | (a.astype(np.float32).astype(np.float64) == a)


def eval64(pts, M, R, T, ds, h, w, lo, hi):
    """one camera, float64 from the fp32 inputs.  pts (P, >= 3) float32.  -> dict of (P,) arrays: xs, ys (q / ds, unrounded), x, y
    (rounded half to even), z (q.z), kept, exact (every intermediate representable in fp32), zexact (the depth's chain alone)"""
    p = pts[:, :3].astype(np.float64)
    M, R, T = M.astype(np.float64), R.astype(np.float64), T.astype(np.float64)
    with np.errstate(all='ignore'):
        prod = M[None, :3, :3] * p[:, None, :]                                       # (P, 3, 3)
        dot = prod.sum(-1)
        c = dot + M[:3, 3]
        ok_c = _f32ok(prod).all(-1) & _f32ok(dot) & _f32ok(c)                        # (P, 3)
        one_term = ((prod != 0) & np.isfinite(prod)).sum(-1) <= 1
        ok_c &= one_term | ~np.isfinite(prod).all(-1)
        u, v = c[:, 0] / c[:, 2], c[:, 1] / c[:, 2]
        ok_div = _f32ok(u) & _f32ok(v) & (~np.isfinite(u) | (u * c[:, 2] == c[:, 0])) & (~np.isfinite(v) | (v * c[:, 2] == c[:, 1]))
        wv = np.stack([u, v, c[:, 2]], 1)
        prod2 = R[None] * wv[:, None, :]
        dot2 = prod2.sum(-1)
        q = dot2 + T
        ok_q = _f32ok(prod2).all(-1) & _f32ok(dot2) & _f32ok(q)
        ok_q &= (((prod2 != 0) & np.isfinite(prod2)).sum(-1) <= 1) | ~np.isfinite(prod2).all(-1)
        xs, ys = q[:, 0] / ds, q[:, 1] / ds
        ok_px = _f32ok(xs) & _f32ok(ys)
        x, y = np.rint(xs), np.rint(ys)
        kept = (x >= 0) & (x < w) & (y >= 0) & (y < h) & (q[:, 2] < hi) & (q[:, 2] >= lo)
    exact = ok_c.all(-1) & ok_div & ok_q.all(-1) & ok_px
    zexact = ok_c[:, 2] & ok_q[:, 2] & ((R[2, 0] == 0) & (R[2, 1] == 0))
    return dict(xs=xs, ys=ys, x=x, y=y, z=q[:, 2], kept=kept, exact=exact, zexact=zexact, c=c, u=u, v=v, q=q)


def map64(case, pts_list, M, R, T):
    """float64 min map (B, N, h, w) with +inf for empty pixels, from per-sample fp32 points"""
    B, N, h, w = dims(case)
    lo, hi = case['cfg']
    out = np.full((B, N, h, w), np.inf)
    for b in range(B):
        for n in range(N):
            e = eval64(pts_list[b], M[b, n], R[b, n], T[b, n], case['ds'], h, w, lo, hi)
            k = e['kept']
            np.minimum.at(out[b, n], (e['y'][k].astype(np.int64), e['x'][k].astype(np.int64)), e['z'][k])
    return out


def _safe(case, pts, Ms, Rs, Ts):
    """(P,) bool: every camera's pair of the point is exact, or dropped by an exact depth"""
    _, N, h, w = dims(case)
    lo, hi = case['cfg']
    ok = np.ones(pts.shape[0], bool)
    for n in range(N):
        e = eval64(pts, Ms[n], Rs[n], Ts[n], case['ds'], h, w, lo, hi)
        with np.errstate(invalid='ignore'):
            out_of_range = ~((e['z'] < hi) & (e['z'] >= lo))
        ok &= e['exact'] | (e['zexact'] & out_of_range)
    return ok


# ------------------------------------------------------------------------------------------------------------------ exact inputs
def _targets(case, b, rng):
    """-> list of (camera, xt, yt, depth, required) float64 arrays for sample b"""
    name = case['name']
    _, N, h, w = dims(case)
    lo, hi = case['cfg']
    A = lambda *v: np.array(v, np.float64)  # noqa: E731
    if name == 'px':
        return [(0, A(-1, 4, 1, 1, 2), A(1, 1, -1, 4, 2), A(5, 6, 7, 8, 9.5), True)]
    if name == 'ds2_ties':
        xs = A(-0.5, 0.5, 1.5, 2.5, w - 0.5, w + 0.5)
        ys = A(-0.5, 0.5, 1.5, 2.5, h + 0.5)
        return [(0, xs, np.full(6, 1.0), 3.0 + np.arange(6) * 0.25, True),
                (0, np.full(5, 3.0), ys, 6.0 + np.arange(5) * 0.25, True)]
    if name == 'odd_dims':
        n = 96
        return [(k, rng.integers(-4, 4 * w + 8, n) / 4.0, rng.integers(-4, 4 * h + 8, n) / 4.0,
                 rng.integers(4, 4 * 50, n) / 4.0, False) for k in range(N)]
    if name == 'stride5_batch':
        if b == 1:
            return []
        n = 160
        if b == 2:                                                   # entirely out of view: beyond the right and the lower edge
            return [(k, rng.integers(w + 1, w + 9, n) * 1.0, rng.integers(h + 1, h + 9, n) * 1.0, rng.integers(8, 160, n) / 4.0, False)
                    for k in range(N)]
        return [(k, rng.integers(-4, 4 * w + 4, n) / 4.0, rng.integers(-4, 4 * h + 4, n) / 4.0, rng.integers(4, 4 * 50, n) / 4.0, False)
                for k in range(N)]
    if name == 'one_pixel':
        d = np.concatenate([2.0 + np.arange(2048) / 64.0] * 2)      # every depth twice; the nearest is 2.0
        return [(0, np.full(4096, 2.0), np.full(4096, 1.0), rng.permutation(d), True)]
    if name == 'edges':
        f = lambda x: float(np.float32(x))  # noqa: E731
        below = lambda x: float(np.nextafter(np.float32(x), np.float32(-np.inf)))  # noqa: E731
        # u = 2 x is a power of two at these columns, so u z is exact for a 24-bit z
        return [(0, A(1, 2, 4, 8), np.zeros(4), A(f(lo), below(lo), below(hi), f(hi)), True),
                (0, A(3, 5, 6), A(1, 2, 3), A(7.5, 9.25, 11.0), True)]
    if name == 'blocks':
        n = BLOCK_COUNTS[b]
        return [(0, rng.integers(-2, 4 * w + 2, n) / 4.0, rng.integers(-2, 4 * h + 2, n) / 4.0, rng.integers(4, 4 * 64, n) / 4.0, False)]
    if name == 'keyties':
        r0, r1 = KEYTIES_ROWS
        yy, xx = np.meshgrid(np.arange(r0, r1), np.arange(0, w), indexing='ij')
        xx, yy = np.tile(xx.ravel(), 3) * 1.0, np.tile(yy.ravel(), 3) * 1.0
        base = rng.integers(8, 8 * 30, xx.size // 3) / 8.0
        near = np.tile(base, 3) + rng.integers(0, 12, xx.size) / 8.0                 # three per pixel, less than 1.5 m apart
        far = rng.random(xx.size) < 0.1
        near[far] += rng.integers(2, 6, int(far.sum())) * 2.0                        # some clearly apart: no tie with the nearest
        order = rng.permutation(xx.size)
        return [(0, xx[order], yy[order], near[order], False)]
    if name == 'shipped':
        n = 12000
        return [(k, rng.integers(0, 2 * w, n) / 2.0 - 0.25 * (k % 2), rng.integers(0, 2 * h, n) / 2.0, rng.integers(16, 8 * 40, n) / 8.0,
                 False) for k in range(N)]
    raise KeyError(name)


SHIPPED_POINTS = 34720
_EXACT = {}


def exact_inputs(case):
    """-> (pts_list: B float32 arrays (P_b, stride), M (B, N, 4, 4), R (B, N, 3, 3), T (B, N, 3)) float32; computed once"""
    name = case['name']
    if name in _EXACT:
        return _EXACT[name]
    B, N, h, w = dims(case)
    rng = np.random.default_rng(1000 + CASE_IDS.index(name))
    M = np.zeros((B, N, 4, 4), np.float32)
    R = np.zeros((B, N, 3, 3), np.float32)
    T = np.zeros((B, N, 3), np.float32)
    for b in range(B):
        for n in range(N):
            M[b, n], R[b, n], T[b, n] = exact_camera(n + (b if name == 'stride5_batch' else 0), case['H'], case['W'])
    pts_list = []
    for b in range(B):
        parts = []
        for cam, xt, yt, depth, required in _targets(case, b, rng):
            p = back_project(M[b, cam], R[b, cam], T[b, cam], case['ds'], xt, yt, depth)
            ok = _safe(case, p, M[b], R[b], T[b])
            if required or name == 'blocks':
                assert ok.all(), f'{name}: a planted point is not exact'
            parts.append(p[ok])
        p = np.concatenate(parts, 0) if parts else np.zeros((0, 3), np.float32)
        if name == 'edges':                                          # c.z = 0, behind the camera, NaN and inf coordinates
            extra = np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [2.0, 2.0, -8.0], [np.nan, 1.0, 4.0], [1.0, np.nan, 4.0],
                              [1.0, 1.0, np.nan], [np.inf, 1.0, 4.0], [1.0, -np.inf, 4.0], [1.0, 1.0, np.inf], [1.0, 1.0, -np.inf],
                              [np.inf, np.inf, np.inf]], np.float32)
            p = np.concatenate([p, extra], 0)
        if name == 'shipped':
            assert p.shape[0] >= SHIPPED_POINTS, p.shape
            p = p[rng.permutation(p.shape[0])[:SHIPPED_POINTS]]
        if name == 'blocks':
            assert p.shape[0] == BLOCK_COUNTS[b]
        rows = rng.standard_normal((p.shape[0], case['stride'])).astype(np.float32)   # the columns behind xyz are never read
        rows[:, :3] = p
        pts_list.append(rows)
    _EXACT[name] = (pts_list, M, R, T)
    return _EXACT[name]


# ------------------------------------------------------------------------------------------------------------------ real inputs
def _rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    m = np.eye(3)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


_REAL = {}


def real_inputs(case):
    """nuScenes-like calibration -> (pts_list, M, R, T) float32"""
    name = case['name']
    if name in _REAL:
        return _REAL[name]
    B, N, h, w = dims(case)
    H, W = case['H'], case['W']
    shipped = name == 'shipped'
    rng = np.random.default_rng(77 + CASE_IDS.index(name))
    M = np.zeros((B, N, 4, 4), np.float32)
    R = np.zeros((B, N, 3, 3), np.float32)
    T = np.zeros((B, N, 3), np.float32)
    scale = 0.44 if shipped else 0.44 * W / 704.0
    K = np.array([[1266.4, 0.0, 816.3], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]])
    cam_axes = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])     # lidar (x forward, y left, z up) -> camera
    for b in range(B):
        for n in range(N):
            yaw = 360.0 / N * n + rng.uniform(-3, 3)
            l2c = cam_axes @ _rot(1, rng.uniform(-1, 1)) @ _rot(2, -yaw)
            t = -l2c @ np.array([1.5 * math.cos(math.radians(yaw)), 1.5 * math.sin(math.radians(yaw)), 1.6]) + rng.uniform(-0.1, 0.1, 3)
            m = np.eye(4)
            m[:3, :3], m[:3, 3] = K @ l2c, K @ t
            M[b, n] = m
            r = np.eye(3)
            r[:2, :2] = scale * _rot(2, rng.uniform(-5.4, 5.4))[:2, :2]
            tr = np.array([-32.0 * scale / 0.44 + rng.uniform(-8, 8), -140.0 * scale / 0.44 + rng.uniform(-8, 8), 0.0])
            if n == 1:                                               # flipped: x -> W - x
                r = np.diag([-1.0, 1.0, 1.0]) @ r
                tr[0] = W - tr[0]
            R[b, n], T[b, n] = r, tr
    pts_list = []
    for b in range(B):
        P = SHIPPED_POINTS if shipped else (0 if b == 1 else 3000)
        rad = 50.0 * np.sqrt(rng.random(P))
        ang = rng.uniform(0, 2 * math.pi, P)
        xyz = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-2.0, 4.0, P)], 1)
        if not shipped and b == 2:                                   # entirely out of view: below every camera's lower edge
            xyz[:, 2] = rng.uniform(-60.0, -40.0, P)
            xyz[:, :2] *= 0.2
        rows = rng.standard_normal((P, case['stride'])).astype(np.float32)
        rows[:, :3] = xyz
        pts_list.append(rows)
    _REAL[name] = (pts_list, M, R, T)
    return _REAL[name]


def real_reference(case):
    """-> dict: min64 (B, N, h, w) with inf for empty, dz (B, N, h, w) the largest depth bound of a pixel's kept pairs, tie_hi the
    largest depth among the kept pairs that tie with the nearest in the reference's fp32 key, checked (B, N, h, w) bool"""
    key = case['name'] + '/ref'
    if key in _REAL:
        return _REAL[key]
    pts_list, M, R, T = real_inputs(case)
    B, N, h, w = dims(case)
    lo, hi = case['cfg']
    ds = case['ds']
    g4 = gamma(4)
    min64 = np.full((B, N, h, w), np.inf)
    dzmap = np.zeros((B, N, h, w))
    tie_hi = np.zeros((B, N, h, w))
    checked = np.ones((B, N, h, w), bool)
    worst_tau = 0.0
    for b in range(B):
        p = pts_list[b][:, :3].astype(np.float64)
        for n in range(N):
            Mm, Rr, Tt = M[b, n].astype(np.float64), R[b, n].astype(np.float64), T[b, n].astype(np.float64)
            assert Rr[2, 0] == 0 and Rr[2, 1] == 0 and Rr[2, 2] == 1 and Tt[2] == 0
            e = eval64(pts_list[b], M[b, n], R[b, n], T[b, n], ds, h, w, lo, hi)
            c = e['c']
            ec = g4 * (np.abs(Mm[None, :3, :3]) * np.abs(p[:, None, :])).sum(-1) + g4 * np.abs(Mm[:3, 3])      # (P, 3)
            front = c[:, 2] > 2 * ec[:, 2]
            assert 3 * ec[~front, 2].max(initial=0.0) < lo / 2       # the pairs near or behind the camera plane are far below lo
            cz = np.where(front, c[:, 2], 1.0)
            uu, vv = np.where(front, e['u'], 0.0), np.where(front, e['v'], 0.0)
            du = (ec[:, 0] + np.abs(uu) * ec[:, 2]) / (cz - ec[:, 2])
            du = du + U * (np.abs(uu) + du)
            dv = (ec[:, 1] + np.abs(vv) * ec[:, 2]) / (cz - ec[:, 2])
            dv = dv + U * (np.abs(vv) + dv)
            wabs = np.stack([np.abs(uu), np.abs(vv), np.abs(cz)], 1)
            dw = np.stack([du, dv, ec[:, 2]], 1)
            dq = (np.abs(Rr)[None] * dw[:, None, :]).sum(-1) + g4 * ((np.abs(Rr)[None] * (wabs + dw)[:, None, :]).sum(-1) + np.abs(Tt))
            q = np.where(front[:, None], e['q'], 0.0)
            tau = dq[:, :2] / ds + U * (np.abs(q[:, :2]) + dq[:, :2]) / ds
            dz = dq[:, 2]
            xs, ys, z = np.where(front, e['xs'], 0.0), np.where(front, e['ys'], 0.0), q[:, 2]
            half = lambda a: np.abs(a - (np.floor(a) + 0.5))  # noqa: E731  (distance to the nearest half-integer)
            in_range = (z < hi) & (z >= lo)
            near_range = (np.abs(z - lo) <= dz) | (np.abs(z - hi) <= dz)
            clearly_out = ~in_range & ~near_range
            decided = ~front | clearly_out | ((half(xs) > tau[:, 0]) & (half(ys) > tau[:, 1]) & ~near_range)
            worst_tau = max(worst_tau, float(tau[front & in_range].max(initial=0.0)))
            # an undecided pair unchecks every pixel it can reach
            und = np.nonzero(~decided)[0]
            for i in und:
                for X in {np.rint(xs[i] - tau[i, 0]), np.rint(xs[i] + tau[i, 0])}:
                    for Y in {np.rint(ys[i] - tau[i, 1]), np.rint(ys[i] + tau[i, 1])}:
                        if 0 <= X < w and 0 <= Y < h:
                            checked[b, n, int(Y), int(X)] = False
            k = e['kept'] & front
            yi, xi = e['y'][k].astype(np.int64), e['x'][k].astype(np.int64)
            np.minimum.at(min64[b, n], (yi, xi), z[k])
            np.maximum.at(dzmap[b, n], (yi, xi), dz[k])
            # the reference's tie rule on the fp32 depths a restatement would hold
            z32 = z[k].astype(np.float32)
            rank = (xi + yi * w).astype(np.float32)
            keyf = rank + z32 / np.float32(100.)
            assert keyf.dtype == np.float32
            minkey = np.full((h, w), np.inf, np.float32)
            np.minimum.at(minkey, (yi, xi), keyf)
            tied = keyf == minkey[yi, xi]
            np.maximum.at(tie_hi[b, n], (yi[tied], xi[tied]), z[k][tied])
    ref = dict(min64=min64, dz=dzmap, tie_hi=tie_hi, checked=checked, worst_tau=worst_tau)
    _REAL[key] = ref
    return ref


# ------------------------------------------------------------------------------------------------------------------ adapters
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class EmuApi:
    """the C entry of the CPU-emulated library, CPU tensors"""
    name = 'emu'

    def __init__(self):
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
        import emu_capi
        self.lib = emu_capi.lib()

    def dev(self, t):
        return t.clone()

    def cpu(self, t):
        return t

    def call(self, points, stride, offsets, max_points, M, R, T, H, W, ds, lo, hi, out):
        B, N = M.shape[:2]
        return self.lib.fbbev_points_to_depth(_p(points), stride, _p(offsets), max_points, B, N, _p(M), _p(R), _p(T), H, W, ds, lo, hi,
                                              _p(out), None)


class GpuApi:
    """fb_bev_amd._capi.points_to_depth on cuda:0"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi
        self.c = _capi
        self.device = torch.device('cuda:0')

    def dev(self, t):
        return t.to(self.device)

    def cpu(self, t):
        return t.cpu()

    def call(self, points, stride, offsets, max_points, M, R, T, H, W, ds, lo, hi, out):
        B, N = M.shape[:2]
        rows = points.as_strided((points.numel() // stride, 3), (stride, 1)) if points.numel() >= stride else points[:0].view(0, 3)
        h, w = H // ds, W // ds
        assert self.c.points_to_depth(rows, offsets, max_points, M, R, T, H, W, ds, lo, hi, out=out.view(B, N, h, w)) is not None
        return 0


def _bits(t):
    return t.contiguous().view(torch.int32)


def run(api, case, inputs):
    """one call -> (B, N, h, w) float32 on the CPU.  `out` is a slice of a patterned buffer whose other words must come back intact;
    points sit `offset` floats into their buffer (4-byte alignment only when offset is odd); every input must come back unchanged."""
    pts_list, M, R, T = inputs
    B, N, h, w = dims(case)
    lo, hi = case['cfg']
    stride, off = case['stride'], case['offset']
    counts = [p.shape[0] for p in pts_list]
    flat = np.concatenate([p.reshape(-1) for p in pts_list] + [np.zeros(0, np.float32)])
    store = torch.cat([torch.full((off,), PATTERN), torch.from_numpy(flat), torch.full((GUARD,), PATTERN)])
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    d_store, d_off = api.dev(store), api.dev(offsets)
    d_pts = d_store[off:off + flat.size]
    tM, tR, tT = (torch.from_numpy(a).contiguous() for a in (M, R, T))
    dM, dR, dT = api.dev(tM), api.dev(tR), api.dev(tT)
    n = B * N * h * w
    lead = GUARD + off                                               # an odd offset: `out` is 4-byte aligned only as well
    buf = api.dev(torch.full((lead + n + GUARD,), PATTERN))
    assert d_store.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    assert api.call(d_pts, stride, d_off, max(counts), dM, dR, dT, case['H'], case['W'], case['ds'], lo, hi, buf[lead:lead + n]) == 0
    buf = api.cpu(buf)
    assert (buf[:lead] == PATTERN).all() and (buf[lead + n:] == PATTERN).all(), 'guard words of out overwritten'
    assert torch.equal(_bits(api.cpu(d_store)), _bits(store)), 'points were written to'
    assert torch.equal(api.cpu(d_off), offsets), 'offsets were written to'
    for d, t in ((dM, tM), (dR, tR), (dT, tT)):
        assert torch.equal(_bits(api.cpu(d)), _bits(t)), 'a matrix was written to'
    return buf[lead:lead + n].view(B, N, h, w).clone()


# ------------------------------------------------------------------------------------------------------------------ checks
def expected_exact(case):
    key = case['name'] + '/want'
    if key not in _EXACT:
        m = map64(case, *exact_inputs(case))
        want = np.where(np.isfinite(m), m, 0.0)
        assert (want.astype(np.float32).astype(np.float64) == want).all()
        _EXACT[key] = (torch.from_numpy(want.astype(np.float32)), np.isfinite(m))
    return _EXACT[key]


def _case_asserts(case, want, filled):
    """the properties a case exists for, on the float64 answer"""
    name = case['name']
    lo, hi = case['cfg']
    pts_list = exact_inputs(case)[0]
    if name == 'px':
        assert filled.sum() == 1 and want[0, 0, 2, 2] == 9.5
    elif name == 'ds2_ties':
        row = want[0, 0, 1]
        # -0.5 -> -0.0 and 0.5 -> 0: pixel 0 holds the nearer (3.0); 1.5 and 2.5 -> 2 (3.5); w - 0.5 = 4.5 -> 4 (4.0); 5.5 -> 6: dropped
        assert row[0] == 3.0 and row[2] == 3.5 and row[4] == 4.0 and row[1] == 0 and row[3] == 0
        col = want[0, 0, :, 3]
        assert col[0] == 6.0 and col[2] == 6.5 and col[1] == 0                       # -0.5, 0.5 -> 0; 1.5, 2.5 -> 2; 3.5 -> 4: dropped
        assert filled.sum() == 5
    elif name == 'stride5_batch':
        assert pts_list[1].shape[0] == 0 and pts_list[2].shape[0] > 100
        assert filled[0].sum() > 20 and filled[1].sum() == 0 and filled[2].sum() == 0
    elif name == 'one_pixel':
        assert pts_list[0].shape[0] == 4096 and filled.sum() == 1 and want[0, 0, 1, 2] == 2.0
    elif name == 'edges':
        below = lambda x: float(np.nextafter(np.float32(x), np.float32(-np.inf)))  # noqa: E731
        assert float(want[0, 0, 0, 1]) == lo and want[0, 0, 0, 2] == 0 and float(want[0, 0, 0, 4]) == below(hi) and want[0, 0, 0, 8] == 0
        assert filled.sum() == 5 and not np.isfinite(pts_list[0]).all()
    elif name == 'blocks':
        assert tuple(p.shape[0] for p in pts_list) == BLOCK_COUNTS and all(filled[b].sum() > 0 for b in range(5))
    elif name == 'keyties':
        r0, r1 = KEYTIES_ROWS
        assert filled[0, 0, r0:r1].all() and not filled[0, 0, :r0].any()
    elif name == 'shipped':
        assert pts_list[0].shape == (SHIPPED_POINTS, 5) and all(filled[0, n].sum() > 1000 for n in range(6))
    elif name == 'odd_dims':
        assert all(filled[0, n].sum() >= 6 for n in range(2))


def check_exact(api, case):
    """layer 1 (and the memory checks of run)"""
    want, filled = expected_exact(case)
    _case_asserts(case, want.numpy(), filled)
    got = run(api, case, exact_inputs(case))
    bad = _bits(got) != _bits(want)
    observed(f'{api.name} {case["name"]} exact: {int(filled.sum())} non-empty pixels of {filled.size}, '
             f'{sum(p.shape[0] for p in exact_inputs(case)[0])} points, {int(bad.sum())} pixels differ')
    assert not bad.any(), f'{int(bad.sum())} pixels differ from the float64 minimum'
    assert (_bits(got)[torch.from_numpy(~filled)] == 0).all()       # +0.0, not -0.0
    return got


def check_repeat(api, case):
    a, b = (run(api, case, exact_inputs(case)) for _ in range(2))
    assert torch.equal(_bits(a), _bits(b))


def _keys(vals, h, w):
    """fl32(rank + v / 100) for a (..., h, w) float32 map"""
    rank = (np.arange(w, dtype=np.float32)[None, :] + np.arange(h, dtype=np.float32)[:, None] * np.float32(w))
    k = rank + vals.astype(np.float32) / np.float32(100.)
    assert k.dtype == np.float32
    return k


def tie_pixels(case):
    """(B, N, h, w) bool from the exact inputs: the pixel's kept points are not all separated in the reference's fp32 key"""
    key = case['name'] + '/ties'
    if key in _EXACT:
        return _EXACT[key]
    pts_list, M, R, T = exact_inputs(case)
    B, N, h, w = dims(case)
    lo, hi = case['cfg']
    ties = np.zeros((B, N, h, w), bool)
    for b in range(B):
        for n in range(N):
            e = eval64(pts_list[b], M[b, n], R[b, n], T[b, n], case['ds'], h, w, lo, hi)
            k = e['kept']
            yi, xi, z = e['y'][k].astype(np.int64), e['x'][k].astype(np.int64), e['z'][k].astype(np.float32)
            keyf = (xi + yi * w).astype(np.float32) + z / np.float32(100.)
            order = np.lexsort((z, keyf, xi + yi * w))
            pk, kk, zz = (xi + yi * w)[order], keyf[order], z[order]
            same = (pk[1:] == pk[:-1]) & (kk[1:] == kk[:-1]) & (zz[1:] != zz[:-1])
            flat = ties[b, n].reshape(-1)
            flat[pk[1:][same]] = True
    _EXACT[key] = ties
    return ties


def compare_with_reference_map(case, ours, ref):
    """the rule of check 2 on (B, N, h, w) float32 numpy maps -> number of pixels where ref is strictly larger"""
    B, N, h, w = dims(case)
    assert ours.shape == ref.shape == (B, N, h, w)
    assert np.array_equal(ours != 0, ref != 0), 'the sets of non-empty pixels differ'
    assert (ours <= ref).all()
    assert np.array_equal(_keys(ours, h, w), _keys(ref, h, w)), 'a pixel differs beyond a tie of the key'
    ties = tie_pixels(case)
    same = ours.view(np.int32) == ref.view(np.int32)
    assert same[~ties].all(), 'a pixel without a tie differs'
    return int((ref > ours).sum())


def fixture():
    return np.load(FIXTURE)


def fixture_map(case, z):
    """the fixture's map of a case as (B, N, h, w); keyties is stored as its rows KEYTIES_ROWS"""
    B, N, h, w = dims(case)
    m = z[f'{case["name"]}.map']
    if case['name'] == 'keyties':
        full = np.zeros((B, N, h, w), np.float32)
        full[:, :, KEYTIES_ROWS[0]:KEYTIES_ROWS[1]] = m
        return full
    return m.reshape(B, N, h, w)


def check_fixture(api):
    """layer 2: the kernel on the exact inputs against the map the reference class wrote"""
    z = fixture()
    larger = {}
    for name in FIXTURE_CASES:
        case = by_name(name)
        pts_list, M, R, T = exact_inputs(case)
        for b in range(case['B']):
            assert np.array_equal(z[f'{name}.points{b}'].view(np.int32), pts_list[b].view(np.int32)), 'the fixture is stale: regenerate it'
        assert np.array_equal(z[f'{name}.lidar2img'], M[:, :, :3]), 'the reference built other matrices from the info dicts'
        assert np.array_equal(z[f'{name}.post_rots'], R) and np.array_equal(z[f'{name}.post_trans'], T)
        got = run(api, case, (pts_list, M, R, T)).numpy()
        larger[name] = compare_with_reference_map(case, got, fixture_map(case, z))
        observed(f'{api.name} fixture {name}: {int((got != 0).sum())} non-empty pixels, {int(tie_pixels(case).sum())} with a key tie, '
                 f'the reference is strictly larger at {larger[name]}')
    assert larger['keyties'] >= 1, 'keyties has no pixel where the reference kept the farther of two tied points'
    assert tie_pixels(by_name('ds2_ties')).sum() == 0


def check_restatement_real(case):
    """the fp32 torch restatement (CPU route of points_to_depth) inside the real layer's bounds, ties allowed as the reference has them"""
    from fb_bev_amd.points_depth import points_to_depth
    ref = real_reference(case)
    pts_list, M, R, T = real_inputs(case)
    lo, hi = case['cfg']
    got = points_to_depth([torch.from_numpy(p) for p in pts_list], torch.from_numpy(M), torch.from_numpy(R), torch.from_numpy(T),
                          case['H'], case['W'], case['ds'], (lo, hi)).numpy().astype(np.float64)
    ck, filled = ref['checked'], np.isfinite(ref['min64'])
    assert np.array_equal((got != 0)[ck], filled[ck]), 'the restatement and float64 disagree on emptiness of a checked pixel'
    sel = ck & filled
    low, high = ref['min64'][sel] - ref['dz'][sel], ref['tie_hi'][sel] + ref['dz'][sel]
    assert ((got[sel] >= low) & (got[sel] <= high)).all()
    plain = sel & (ref['tie_hi'] == ref['min64'])
    ratio = float((np.abs(got[plain] - ref['min64'][plain]) / ref['dz'][plain]).max())
    observed(f'restatement {case["name"]}: worst |depth error| / bound {ratio:.3f} over {int(plain.sum())} checked pixels without a tie, '
             f'{int((sel & ~plain).sum())} with one')
    return ratio


def check_real(api, case):
    """layer 3"""
    ref = real_reference(case)
    check_restatement_real(case)
    got = run(api, case, real_inputs(case)).numpy().astype(np.float64)
    ck, filled = ref['checked'], np.isfinite(ref['min64'])
    unchecked = int((~ck & filled).sum())
    observed(f'{api.name} {case["name"]} real: {int(filled.sum())} non-empty pixels, {unchecked} unchecked '
             f'({100.0 * unchecked / max(int(filled.sum()), 1):.3f} %), worst tau {ref["worst_tau"]:.3e} px, '
             f'worst depth bound {float(ref["dz"].max()):.3e} m')
    assert filled.sum() > 0 and unchecked <= 0.02 * filled.sum()
    wrong = (got != 0)[ck] != filled[ck]
    assert not wrong.any(), f'{int(wrong.sum())} checked pixels disagree on emptiness'
    sel = ck & filled
    err = np.abs(got[sel] - ref['min64'][sel])
    ratio = float((err / ref['dz'][sel]).max())
    observed(f'{api.name} {case["name"]} real: worst |depth error| {float(err.max()):.3e} m, worst error / bound {ratio:.3f} over '
             f'{int(sel.sum())} checked pixels')
    assert (err <= ref['dz'][sel]).all()
    return ratio


# ------------------------------------------------------------------------------------------------------------------ host matrices
Q_CYCLE = (0.5, 0.5, 0.5, 0.5)           # 120 degrees about (1, 1, 1): x -> y -> z -> x
Q_FLIP_Y = (0.0, 0.0, 1.0, 0.0)          # 180 degrees about y
Q_BOTH = (-0.5, -0.5, 0.5, 0.5)          # Q_CYCLE * Q_FLIP_Y
CAM_NAMES = ['CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_FRONT_LEFT', 'CAM_BACK', 'CAM_BACK_LEFT', 'CAM_BACK_RIGHT']


def exact_info(case, b):
    """a sample info dict with dyadic unit quaternions whose matrix chain (loading.py:922-950) is exact in fp32 and gives the exact
    layer's lidar2img[b]: the camera's two rotations (120 degrees about the diagonal, 180 degrees about y) are undone by the lidar
    ego's (their product), the lidar ego's translation carries inverse(M3) t, and `intrins` is M3 itself.
    -> (curr, cam_names, intrins (N, 3, 3) float32 tensor)"""
    _, M, _, _ = exact_inputs(case)
    N = case['N']
    names = CAM_NAMES[:N]
    # every camera shares the lidar ego's pose, so the translation must be the same for all: it is put into the camera's own
    # ego2global translation instead (inverse(C S) G = identity rotation, translation = G.t - C.t with S.t = 0)
    curr = dict(ego2global_rotation=list(Q_BOTH), ego2global_translation=[0.0, 0.0, 0.0], cams={})
    Rb = _quat(Q_BOTH)
    for n, name in enumerate(names):
        m3, t = M[b, n, :3, :3].astype(np.float64), M[b, n, :3, 3].astype(np.float64)
        tl = np.linalg.inv(m3) @ t                                   # lidar2cam's translation (rotation: identity)
        # inverse(C S) G = (R_b, ct)^-1 (R_b, 0) = (I, -R_b^T ct)  =>  ct = -R_b tl
        ct = -(Rb @ tl)
        curr['cams'][name] = dict(sensor2ego_rotation=list(Q_FLIP_Y), sensor2ego_translation=[0.0, 0.0, 0.0],
                                  ego2global_rotation=list(Q_CYCLE), ego2global_translation=[float(v) for v in ct])
    return curr, names, torch.from_numpy(M[b, :, :3, :3].copy())


def _quat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


assert np.array_equal(_quat(Q_CYCLE) @ _quat(Q_FLIP_Y), _quat(Q_BOTH))


def real_info(seed, N=6):
    """random unit quaternions and nuScenes-sized translations -> (curr, cam_names, intrins)"""
    rng = np.random.default_rng(seed)

    def quat():
        q = rng.standard_normal(4)
        return [float(v) for v in q / np.linalg.norm(q)]
    pos = np.array([rng.uniform(300, 2000), rng.uniform(300, 2000), rng.uniform(-2, 2)])
    curr = dict(ego2global_rotation=quat(), ego2global_translation=[float(v) for v in pos], cams={})
    for name in CAM_NAMES[:N]:
        curr['cams'][name] = dict(sensor2ego_rotation=quat(), sensor2ego_translation=[float(v) for v in rng.uniform(-1.7, 1.7, 3)],
                                  ego2global_rotation=quat(), ego2global_translation=[float(v) for v in pos + rng.uniform(-1, 1, 3)])
    intr = np.tile(np.array([[1266.4, 0.0, 816.3], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]], np.float32), (N, 1, 1))
    intr[:, 0, 0] += rng.uniform(-10, 10, N).astype(np.float32)
    return curr, CAM_NAMES[:N], torch.from_numpy(intr)


def lidar2img_bound(curr, cam_names, intrins):
    """-> (float64 chain from the fp32 matrices (N, 4, 4), elementwise bound of an fp32 evaluation).  With A = C S, X = A^-1,
    L = X G, P = K L and g = gamma_4 (a 4-term dot product in any order):
      |A^ - A| <= g |C||S|;
      the inverse by LU with partial pivoting, n = 4, growth <= 2^(n-1) = 8: |X^ - A^^-1| <= 2 n 8 g |X||A||X| (Higham, Accuracy and
      Stability of Numerical Algorithms, 14.1 with 9.3's backward error), and |A^^-1 - X| <= |X| g |C||S| |X| to first order:
      E_X = 65 g |X| (|C||S|) |X|   (|A| <= |C||S|);
      E_L = E_X |G| + g (|X| + E_X) |G|;    E_P = |K| E_L + g |K| (|L| + E_L).
    The bound is componentwise in |A|, so it is 0 where the last row of the product is structurally 0 although the LU factors fill
    in there; callers hold the three rows that are read against it."""
    from fb_bev_amd.points_depth import quaternion_rotation_matrix

    def rigid(rot, tr):
        m = np.eye(4, dtype=np.float32)
        m[:3, :3] = quaternion_rotation_matrix(rot)
        m[:3, 3] = tr
        return m.astype(np.float64)
    g = gamma(4)
    G = rigid(curr['ego2global_rotation'], curr['ego2global_translation'])
    Ps, Es = [], []
    for n, name in enumerate(cam_names):
        cam = curr['cams'][name]
        S = rigid(cam['sensor2ego_rotation'], cam['sensor2ego_translation'])
        C = rigid(cam['ego2global_rotation'], cam['ego2global_translation'])
        K = np.eye(4)
        K[:3, :3] = intrins[n].numpy().astype(np.float64)
        X = np.linalg.inv(C @ S)
        EX = 65 * g * np.abs(X) @ (np.abs(C) @ np.abs(S)) @ np.abs(X)
        L = X @ G
        EL = EX @ np.abs(G) + g * (np.abs(X) + EX) @ np.abs(G)
        Ps.append(K @ L)
        Es.append(np.abs(K) @ EL + g * np.abs(K) @ (np.abs(L) + EL))
    return np.stack(Ps), np.stack(Es)
