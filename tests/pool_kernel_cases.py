"""The lift-splat pooling family -- fb_bev_amd/csrc/pool_kernels.h and pool_bwd_kernels.h behind fbbev_pool_tile_index,
fbbev_bev_pool_v2_dense_fwd[_add], fbbev_bev_pool_v2_dense_fwd_rows, fbbev_pool_zmean[_split|_rows] and fbbev_bev_pool_v2_dense_bwd[_z] --
at the smallest shapes at which each of its code paths exists: one case table, run on the MI355X by tests/test_gpu_pool_kernels.py and
on the CPU emulator by tests/test_emu_pool_kernels.py.  Plain Python and CPU torch; both adapters call the C ABI through ctypes, so an
output can be a strided, caller-owned, poisoned buffer.

GEOMETRY (`build`, asserted by `check` before anything is launched).  The main frustum is (B, N, D, H, W) = (2, 2, 40, 4, 6): 96 feature
pixels of 40 depth bins (two 32-lane trips of k_pool_bwd_pixel), 1 920 points per sample.  The grid is (B, Z, Y, X) = (2, 3, 11, 16):
YX = 176 is a multiple of 8 and of no tile size, so every plane ends in a partial tile (3 / 2 / 1 / 1 / 1 tiles per plane at 64 / 128 /
256 / 512 / 1024), 1 056 voxels are 16.5 flat 64-tiles and the samples' boundary at 528 lies inside a flat tile of every size from 64 up.
The occupied voxels and their interval lengths are written out by hand in `_MAIN` (plane -> voxel -> points): the hot voxels open plane
(b = 0, z = 1), whose first eight hold 556 points, so the tiles of every tiling share their first point or are shifted by the 15 points
of plane (0, 0); which point goes where is random, but frustum-consistent: point id = ((b*N+n)*D+d)*H*W+hw, feature row = its pixel, a
voxel of sample b holds points of sample b, every kept point appears once.  A second frustum (1, 1, 33, 3, 5) with a (1, 2, 3, 8) grid
has 15 pixels (the last half-wave of the backward is dead) and 33 bins (the second trip has one lane).  A third index set, `garbage`,
is the second with one more interval whose rank lies past the grid, in the partial last 32-voxel tile: k_tile_scatter must not let it
hide the tile's last valid interval (the property the mutation of its `rn >= n_voxels` term needed).

Two places where the geometry cannot be what its wish list says, both because two wishes exclude each other:
  * the plane without any interval is (b = 1, z = 1), not (b = 1, z = 2): the last voxel of the grid, which must be occupied, lies in
    plane (1, 2).  An empty plane in the MIDDLE of a sample is also the harder case for the two-stage plane walk of k_pool_zmean;
  * the tile sequences full / empty / full and (empty, empty, full) need more tiles than the coarse tilings have (flat 1024: 2 tiles,
    flat 512: 3, whose middle one holds the first voxel of sample 1).  `check` asserts each sequence for every tiling that has at
    least nine tiles, and full / empty / full down to five.

REFERENCES AND BOUNDS.  u = 2^-24.
Layer A (dyadic): depth in {k/16}, features, addend, row bias and gradients in {k/8, |k| <= 16}, zscale = 1/4.  A product d*f is a
multiple of 1/128 below 2, the longest interval has 361 points and a column three planes, so every partial sum of the forward is an
integer below 361 * 3 * 256 + 256 < 2^24 in units of 1/128: fp32 addition is exact in ANY order (`check` asserts the figure from the
shape).  Backward: og + zgrad / 4 is a multiple of 1/32 below 2.5; a row product with a feature is a multiple of 1/256, C = 160 of them
stay below 160 * 80 * 16 = 204 800; a chain over 40 bins below 40 * 80 * 16 = 51 200 in units of 1/512.  So every route equals the
float64 result word for word; the Z-mean equals the fp32 IEEE quotient of the exact sum by Z (+ one fp32 add of the bias); 16-bit
outputs equal float64 -> float32 -> .to(dtype).
Layer B (softmax depths, randn features):
  * serial-chain routes (dense2 but SPLIT_LONG, pipe, GATHER8, channels-last, small tiles, rows): the in-order fmaf chain of
    oracle.bev_pool_v2_fwd(use_fma=True), one fp32 add of the addend, one rounding to the output type: word for word.
  * Z-mean: word for word against the fp32 replay -- the chains of a column's planes added in ascending z inside a group, the groups in
    order, one division (+ one add of the bias).  Against float64: a chain of len points carries at most len * u * sum|d f| (gamma_len
    rounded up to first order is what the issue states, kept), the Z - 1 additions and the division at most Z * u * sum_z |plane sum|.
    The bias add of the rows form rounds once more: + u |mean + bias|, which a correct kernel reaches (half an ulp of the result is
    u |result| at a power of two), so ratios just below 1 are this term alone.
  * SPLIT_LONG: an interval of n > 32 points is summed in <= 25 chunks and the partial sums in order: any order of n additions is
    inside gamma_n * sum|d f|, gamma_n = n u / (1 - n u), against float64.  Intervals of <= 32 points: word for word.
  * backward: feat_grad is the in-order fmaf chain over the pixel's kept bins in ascending d -- oracle.bev_pool_v2_bwd on the index
    arrays sorted by (pixel, bin): word for word.  depth_grad = sum_c og f as CPL fmaf steps per lane and a 5-level half-wave tree: at
    most C + 5 roundings on any path, gamma_{C+5} * sum_c |og f| against float64.  The _z entry's gradient is og + zscale * zgrad with
    one multiply-add per element: a fused multiply-add where the compiler contracts (the GPU build), a rounded product and an add in
    the emulator build (-ffp-contract=off); each adapter states which (`fused_zgrad`), from its build flags.
Every call: `out` starts as NaN and comes back without one, the padding of a strided `out` keeps its sentinel, every input has the
same bits afterwards, the return code is the one the table computes from the launcher's own LDS rules.  depth holds NaN in every cell
of a dropped point and feat in every row of a pixel without a kept point.
"""
import ctypes
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from pool_rows_cases import words  # noqa: E402
from rows_train_cases import observed  # noqa: E402

U24 = 2.0 ** -24
NP_STAGE, ZC_CAP, SPLIT_LEN, SPLIT_GROUPS = 512, 1024, 32, 32
E_UNSUPPORTED = -2
SENTINEL = -1536.0          # exact in bf16 and f16
NAN = float('nan')

# include/fbbev.h
ST_SC1NT, ST_PLAIN, ST_NT = 1 << 17, 0, 1
CPL8, WG128, SWZ, CL = 0x4, 1 << 8, 0x400, 0x100000
BF16, F16, PIPE, GATHER8, SPLIT_LONG = 0x800000, 0x1000000, 0x4000000, 0x8000000, 0x2000000
CSPLIT = lambda n: n << 4          # noqa: E731  (0xF: 20 workgroups)
CHUNK = lambda k: k << 12          # noqa: E731
DTYPES = {0: torch.float32, BF16: torch.bfloat16, F16: torch.float16}

PLANAR_TILES, SMALL_TILES, PIPE_TILES, ZMEAN_TILES = (64, 128, 256, 512, 1024), (8, 16, 32), (64, 128, 256), (64, 128, 256)
CHANNELS = (16, 20, 80, 160)

# ------------------------------------------------------------------------------------------------------------------ geometry
# plane (b * Z + z) -> {voxel of the plane: points}.  Plane 1 = (b 0, z 1) opens with the hot voxels: relative to its first point the
# intervals are [0,13) [13,45) [45,78) [78,439) . [439,509) [509,549) [549,556): 13 >= 12 lies below 512, [509,549) crosses 512 three
# points into a batch, 7 points lie beyond.  Shifted by the 15 points of plane 0 (flat tiles of 256 and more) [454,524) crosses 58 in.
_MAIN = {
    0: {0: 1, 3: 2, 10: 3, 21: 4, 50: 5},
    1: {0: 13, 1: 32, 2: 33, 3: 361, 5: 70, 6: 40, 7: 7, 9: 9, 10: 8, 130: 1, 137: 2, 150: 3, 160: 4, 171: 4},
    2: {1: 100, 2: 301, 3: 50, 6: 31, 175: 3},
    3: {0: 2, 5: 7, 63: 8, 140: 9, 150: 1},
    4: {},
    5: {146: 2, 160: 5, 175: 4},
}
_ODD = {0: {0: 5, 1: 33, 5: 40, 9: 2, 23: 7}, 1: {2: 100, 3: 1, 10: 60, 20: 3, 23: 9}}
FRUSTA = {'main': dict(fr=(2, 2, 40, 4, 6), grid=(2, 3, 11, 16), layout=_MAIN),
          'odd': dict(fr=(1, 1, 33, 3, 5), grid=(1, 2, 3, 8), layout=_ODD),
          # the odd frustum with one more interval whose rank lies PAST the grid (what an overflowing fp32 rank leaves behind the valid
          # ones), in the partial last 32-voxel tile of the 48 voxels: nothing may pool it, and it must not hide the tile's last interval
          'garbage': dict(fr=(1, 1, 33, 3, 5), grid=(1, 2, 3, 8), layout=_ODD, garbage=(2, 3))}
_GEO = {}


def geometry(which='main', seed=0, zpad=0):
    """-> the frustum-consistent index set of frustum `which` (cached); zpad: the same voxels in a grid of Z + zpad planes"""
    key = (which, seed, zpad)
    if key in _GEO:
        return _GEO[key]
    spec = FRUSTA[which]
    B, N, D, H, W = spec['fr']
    _, Z0, Y, X = spec['grid']
    Z, YX, HW = Z0 + zpad, Y * X, H * W
    g = torch.Generator().manual_seed(1000 + seed)
    ranks, lengths, rd = [], [], []
    for b in range(B):
        mine = [(b * Z + p % Z0) * YX + v for p in sorted(spec['layout']) if p // Z0 == b for v in sorted(spec['layout'][p])]
        lens = [spec['layout'][p][v] for p in sorted(spec['layout']) if p // Z0 == b for v in sorted(spec['layout'][p])]
        if spec.get('garbage') and b == B - 1:
            mine, lens = mine + [B * Z * YX + spec['garbage'][0]], lens + [spec['garbage'][1]]
        K = sum(lens)
        # pixels of the sample: local pixel 0 keeps every bin, 1 none, 2 only bins >= 32; the other kept points are random
        pid = torch.arange(b * N * D * HW, (b + 1) * N * D * HW).view(N, D, HW)
        forced = [pid[0, :, 0].flatten(), pid[0, 32:, 2].flatten()[:1]] if b == 0 else [pid[N - 1, :3, HW - 1].flatten()]
        free = torch.ones(N, D, HW, dtype=torch.bool)
        free[0, :, 0] = free[0, :, 1] = False
        free[0, :, 2] = False
        if b == 0:
            free[0, 33:, 2] = True
        else:
            free[N - 1, :3, HW - 1] = False
        forced = torch.cat(forced)
        pool = pid[free]
        assert K >= forced.numel() and K - forced.numel() <= pool.numel(), (K, forced.numel(), pool.numel())
        kept = torch.cat([forced, pool[torch.randperm(pool.numel(), generator=g)[:K - forced.numel()]]])
        rd.append(kept[torch.randperm(K, generator=g)])
        ranks += mine
        lengths += lens
    ranks, lengths = torch.tensor(ranks, dtype=torch.int32), torch.tensor(lengths, dtype=torch.int32)
    rd = torch.cat(rd).to(torch.int32)
    starts = (torch.cumsum(lengths, 0) - lengths).to(torch.int32)
    P, n_int = int(lengths.sum()), ranks.numel()
    n_max = P + 37
    bn, hw = rd.long() // (D * HW), rd.long() % HW
    rf = (bn * HW + hw).to(torch.int32)
    rb = torch.repeat_interleave(ranks, lengths.long()).to(torch.int32)

    def pad(t):
        out = torch.full((n_max,), -7, dtype=torch.int32)
        out[:t.numel()] = t
        return out
    n_bad = 1 if spec.get('garbage') else 0
    geo = dict(which=which, Iv=n_int - n_bad, Pv=P - (spec['garbage'][1] if n_bad else 0), fr=(B, N, D, H, W), grid=(B, Z, Y, X), YX=YX, ZYX=Z * YX, NVOX=B * Z * YX, P=P, I=n_int, n_max=n_max,
               ranks_bev=pad(rb), ranks_depth=pad(rd), ranks_feat=pad(rf), interval_starts=pad(starts), interval_lengths=pad(lengths),
               interval_rank=pad(ranks), counts=torch.tensor([P, n_int], dtype=torch.int32), n_pix=B * N * HW, n_pts=B * N * D * HW)
    kept = torch.zeros(geo['n_pts'], dtype=torch.bool)
    kept[rd.long()] = True
    geo['kept'] = kept                                                   # per point id
    geo['kept_bins'] = kept.view(B * N, D, HW).permute(0, 2, 1).reshape(geo['n_pix'], D)       # (pixel, bin)
    geo['failed'] = dict(geo, P=0, I=0, Pv=0, Iv=0, counts=torch.tensor([-1, -1], dtype=torch.int32), failed_build=True,
                         **{k: torch.full((n_max,), -7, dtype=torch.int32) for k in
                            ('ranks_bev', 'ranks_depth', 'ranks_feat', 'interval_starts', 'interval_lengths', 'interval_rank')})
    if zpad == 0:
        check(geo)
    _GEO[key] = geo
    return geo


def build(C, seed=0, which='main', layer='A'):
    """-> geometry + values (`case`): the generator of the issue; check() has run on the geometry"""
    return dict(geometry(which, seed), **values(which, C, layer, seed))


def tilings(which='main'):
    """every (kind, tile size) the table uses with a frustum: planar per-plane tiles, flat tiles, flat small tiles, the backward's"""
    t = [('bwd', 128)]
    if which == 'main':
        t += [('planar', tv) for tv in PLANAR_TILES] + [('flat', tv) for tv in PLANAR_TILES] + [('small', tv) for tv in SMALL_TILES]
    return t


def tile_ids(geo, kind, tv):
    """-> (tile of every interval, number of tiles, voxels of every tile)"""
    r = geo['interval_rank'][:geo['I']].long()
    B, Z, Y, X = geo['grid']
    YX = geo['YX']
    if kind in ('planar', 'bwd'):
        tpp = (YX + tv - 1) // tv
        t = (r // YX) * tpp + (r % YX) // tv
        nv = torch.tensor([min(tv, YX - k * tv) for k in range(tpp)] * (B * Z))
        return t, B * Z * tpp, nv
    n = (geo['NVOX'] + tv - 1) // tv
    nv = torch.tensor([min(tv, geo['NVOX'] - k * tv) for k in range(n)])
    return r // tv, n, nv


def _has_seq(occ, pat, run=None, inside=True):
    """pattern of 1 (occupied) / 0 (empty) tiles somewhere in `occ`; with run: inside one run of `run` tiles / across a run boundary"""
    n = len(pat)
    for i in range(len(occ) - n + 1):
        if occ[i:i + n] == pat:
            if run is None or (i // run == (i + n - 1) // run) == inside:
                return True
    return False


def check(geo):
    """The properties the shapes were chosen for, for every tiling and tile size the table uses, on the host."""
    which = geo['which']
    B, N, D, H, W = geo['fr']
    Bg, Z, Y, X = geo['grid']
    P, n_int, YX, ZYX, NVOX = geo['P'], geo['I'], geo['YX'], geo['ZYX'], geo['NVOX']
    r = geo['interval_rank'][:n_int].long()
    if which == 'garbage':         # the last interval lies past the grid, in the tile of the last valid one, which is partial
        assert NVOX % 32 != 0 and r[-1] >= NVOX > r[-2] and r[-1] >> 5 == r[-2] >> 5 == (NVOX - 1) >> 5 and geo['Iv'] == n_int - 1
        return
    ln, st = geo['interval_lengths'][:n_int].long(), geo['interval_starts'][:n_int].long()
    rd, rf, rb = (geo[k][:P].long() for k in ('ranks_depth', 'ranks_feat', 'ranks_bev'))
    # the index set rules
    assert rd.unique().numel() == P and rd.min() >= 0 and rd.max() < geo['n_pts']
    assert torch.equal(rf, (rd // (D * H * W)) * (H * W) + rd % (H * W))
    assert torch.equal(rb // ZYX, rd // (N * D * H * W))                                   # a voxel of sample b holds points of sample b
    assert torch.equal(r, torch.unique(r)) and r.min() >= 0 and r.max() < NVOX
    assert torch.equal(st, torch.cumsum(ln, 0) - ln) and int(ln.sum()) == P and ln.min() >= 1
    for k in ('ranks_bev', 'ranks_depth', 'ranks_feat', 'interval_starts', 'interval_lengths', 'interval_rank'):
        assert geo[k].numel() == P + 37 and (geo[k][(P if k.startswith('ranks') else n_int):] == -7).all()
    assert geo['counts'].tolist() == [P, n_int]
    # layer A: every partial sum fits 24 bits (units: 1/128 forward, 1/256 and 1/512 backward)
    assert int(ln.max()) * Z * 16 * 16 + 16 * 16 < 2 ** 24 and 160 * 80 * 16 < 2 ** 24 and D * 80 * 16 < 2 ** 24
    # backward pixels
    kb = geo['kept_bins']
    cnt = kb.sum(1)
    assert (cnt == 0).any() and (cnt == D).any() and ((cnt > 0) & (kb[:, :32].sum(1) == 0)).any()
    trip0 = kb[:, :32].sum(1)
    pairs = trip0[:geo['n_pix'] // 2 * 2].view(-1, 2)
    assert (pairs[:, 0] != pairs[:, 1]).any() and ((pairs > 0).all(1) & (pairs[:, 0] != pairs[:, 1])).any()   # n0 != n1, both alive
    assert D > 32 and D % 32 != 0
    if which == 'odd':
        assert geo['n_pix'] % 2 == 1 and cnt[-1] > 0                                    # the last half-wave is dead, its partner not
        return
    # interval length classes; SPLIT_LEN on both sides; a chunk without points for the last lane groups of C = 80
    assert {1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33} <= set(ln.tolist()) and ln.max() >= 300
    for groups in (12, 25):                                                            # C = 80 at 4 / 8 channels per lane
        ngs = min(groups, SPLIT_GROUPS)
        chunk = ((ln + ngs - 1) // ngs + 3) // 4 * 4
        assert ((ln > SPLIT_LEN) & (chunk * (ngs - 1) >= ln)).any() and ((ln > SPLIT_LEN) & (chunk * (ngs - 1) < ln)).any()
    # grid corners and the samples' boundary
    assert r[0] == 0 and r[-1] == NVOX - 1 and (r == ZYX - 1).any() and (r == ZYX).any()
    per_plane = torch.bincount(r // YX, minlength=Bg * Z)
    assert per_plane[4] == 0 and (per_plane[[0, 1, 2, 3, 5]] > 0).all()                  # plane (b 1, z 1) has no interval at all
    for kind, tv in tilings(which):
        t, n_tiles, nv = tile_ids(geo, kind, tv)
        per_tile = torch.bincount(t, minlength=n_tiles)
        occ = (per_tile > 0).long().tolist()
        tag = (kind, tv)
        assert (per_tile[per_tile > 0] < nv[per_tile > 0]).all(), tag                   # every occupied tile also holds empty voxels
        # 1. the staging boundary, relative to the tile's first point
        first = torch.full((n_tiles,), P, dtype=torch.long).scatter_reduce(0, t, st, 'amin')
        pts = torch.zeros(n_tiles, dtype=torch.long).index_add_(0, t, ln)
        s = st - first[t]
        assert (pts > NP_STAGE).any(), tag
        cross = (s < NP_STAGE) & (s + ln > NP_STAGE)
        into = NP_STAGE - s
        assert (cross & (into % 4 != 0) & (into // 8 * 8 + 8 <= ln)).any(), tag         # inside a batch of 4 and a batch of 8
        assert ((s >= NP_STAGE) & (ln % 4 != 0)).any(), tag
        assert ((ln >= 12) & (s + ln <= NP_STAGE)).any(), tag
        # 4. tile occupancy
        if kind in ('planar', 'bwd'):
            tpp = (YX + tv - 1) // tv
            last = [occ[p * tpp + tpp - 1] for p in range(Bg * Z)]
            assert 1 in last and 0 in last, tag                                        # the partial last tile of a plane: occupied / empty
        else:
            strad = [k for k in range(n_tiles) if k * tv // ZYX != min(NVOX - 1, k * tv + tv - 1) // ZYX]
            assert tv < 64 or (strad and all(occ[k] for k in strad)), tag               # a flat tile straddles the samples, occupied
        if n_tiles >= 5:
            assert _has_seq(occ, [1, 0, 1]), tag
        if n_tiles >= 9:
            assert _has_seq(occ, [0, 0, 1]), tag
        if kind == 'planar' and tv in PIPE_TILES:
            # full / empty / full, empty / full, full / empty / empty / full; the six tiles of 256 hold fewer of them
            FEF, EF, FEEF = [1, 0, 1], [0, 1], [1, 0, 0, 1]
            inside, across = {64: ((FEF, EF, FEEF), (FEF, EF, FEEF)), 128: ((FEF, EF), (FEF, EF)), 256: ((EF,), (FEF,))}[tv]
            for pat in inside:
                assert _has_seq(occ, pat, 4, True), (tag, pat, 'inside a run of 4')
            for pat in across:
                assert _has_seq(occ, pat, 2, False), (tag, pat, 'across a run boundary of 2')
            assert any(occ[i] == 0 and occ[i + 1] == 1 for i in range(0, n_tiles - 1, 2)), tag     # an empty FIRST tile of a run
    # 2. the column capacity of k_pool_zmean_col: the hot pixel tile (b 0, k 0)
    for tv in ZMEAN_TILES:
        t, _, _ = tile_ids(geo, 'planar', tv)
        tpp = (YX + tv - 1) // tv
        pb = 0
        for z in range(Z):
            m = t == z * tpp
            npl = int(ln[m].sum())
            if z == Z - 1:
                nst = ZC_CAP - pb
                assert 0 < nst < npl, (tv, pb, npl)                                     # the count crosses the cap inside plane z = 2
                s = st[m] - int(st[m].min())
                into = nst - s
                assert ((s < nst) & (s + ln[m] > nst) & (into % 4 != 0) & (into // 4 * 4 + 4 <= ln[m])).any(), tv
                assert (s >= nst).any(), tv
            pb += npl


_VAL = {}


def values(which, C, layer, seed=0):
    key = (which, C, layer, seed)
    if key in _VAL:
        return _VAL[key]
    geo = geometry(which, seed)
    B, N, D, H, W = geo['fr']
    _, Z, Y, X = geo['grid']
    g = torch.Generator().manual_seed(77 + seed + 13 * C + (layer == 'B'))
    if layer == 'A':
        dy = lambda *s: torch.randint(-16, 17, s, generator=g).float() / 8                                     # noqa: E731
        depth = torch.randint(0, 17, (B, N, D, H, W), generator=g).float() / 16
        zscale = 0.25
    else:
        dy = lambda *s: torch.randn(*s, generator=g)                                                           # noqa: E731
        depth = torch.softmax(torch.randn(B, N, D, H, W, generator=g) * 2, dim=2)
        zscale = 1.0 / 3
    feat = dy(B, N, H, W, C)
    v = dict(C=C, layer=layer, depth_clean=depth, feat_clean=feat, addend=dy(B, C, Y, X), addend_rows=dy(B, Y * X, C), row_bias=dy(Y * X, C),
             og=dy(B, C, Z, Y, X), zgrad=dy(B, C, Y, X), zscale=zscale)
    # 6. stray-read poison
    v['depth'] = torch.where(geo['kept'].view(B, N, D, H, W), depth, torch.full_like(depth, NAN))
    v['feat'] = torch.where((geo['kept_bins'].sum(1) > 0).view(B, N, H, W, 1), feat, torch.full_like(feat, NAN))
    _VAL[key] = v
    return v


# ------------------------------------------------------------------------------------------------------------------ references
_REF = {}


def _points(case):
    P = case['Pv']
    return case['ranks_depth'][:P].long(), case['ranks_feat'][:P].long(), case['ranks_bev'][:P].long()


def ref_forward(case):
    """-> vol64 (NVOX, C) float64 sums, abs64 sums of |d f|, chain (NVOX, C) fp32 in-order fmaf chains (layer B only)"""
    key = ('fwd', case['which'], case['C'], case['layer'], case['grid'], bool(case.get('failed_build')))
    if key in _REF:
        return _REF[key]
    C, NVOX = case['C'], case['NVOX']
    rd, rf, rb = _points(case)
    prod = case['depth'].double().flatten()[rd][:, None] * case['feat'].double().view(-1, C)[rf]
    vol = torch.zeros(NVOX, C, dtype=torch.float64).index_add_(0, rb, prod)
    ab = torch.zeros(NVOX, C, dtype=torch.float64).index_add_(0, rb, prod.abs())
    assert not torch.isnan(vol).any()
    chain = None
    if case['layer'] == 'B':
        from oracle import oracle as O
        B, Z, Y, X = case['grid']
        P, n_int = case['Pv'], case['Iv']
        chain = O.bev_pool_v2_fwd(case['depth'], case['feat'], case['ranks_depth'][:P], case['ranks_feat'][:P], case['ranks_bev'][:P],
                                  (B, Z, Y, X, C), case['interval_starts'][:n_int], case['interval_lengths'][:n_int], use_fma=True)
        chain = chain.reshape(NVOX, C)
    _REF[key] = (vol, ab, chain)
    return _REF[key]


def _planes(case, rows):
    """(NVOX, C) -> (B, C, Z, YX)"""
    B, Z, Y, X = case['grid']
    return rows.view(B, Z, Y * X, -1).permute(0, 3, 1, 2)


def expected_volume(case, dtype, addend, layout):
    """-> the word-for-word expectation of a serial-chain route; layout 'planes' (B, C, Z, Y, X) | 'rows' (B, ZYX, C)"""
    vol, _, chain = ref_forward(case)
    B, Z, Y, X = case['grid']
    sums = vol.float() if case['layer'] == 'A' else chain
    if case['layer'] == 'A':
        assert torch.equal(sums.double(), vol)                                         # the exact sums ARE fp32 numbers
    if layout == 'planes':
        out = _planes(case, sums)
        if addend is not None:
            out = out + addend.view(B, -1, 1, Y * X)
        return out.reshape(B, -1, Z, Y, X).contiguous().to(dtype)
    out = sums.view(B, Z, Y * X, -1)
    if addend is not None:
        out = out + addend[:, None]
    return out.reshape(B, Z * Y * X, -1).contiguous().to(dtype)


def z_groups_of(Z, z_groups):
    zg = min(z_groups, Z)
    zper = (Z + zg - 1) // zg
    return [list(range(i * zper, min(Z, i * zper + zper))) for i in range(zg)]


def expected_zmean(case, z_groups=1, row_bias=None, rows=False):
    """-> (word-for-word fp32 expectation (B, C, YX), float64 mean, bound against float64)"""
    vol, ab, chain = ref_forward(case)
    B, Z, Y, X = case['grid']
    planes = _planes(case, vol.float() if case['layer'] == 'A' else chain)             # (B, C, Z, YX) fp32
    total = None
    for grp in z_groups_of(Z, z_groups):
        acc = torch.zeros_like(planes[:, :, 0])
        for z in grp:
            acc = acc + planes[:, :, z]
        total = acc if total is None else total + acc
    exp = total / torch.tensor(float(Z))
    mean64 = _planes(case, vol).sum(2) / Z
    if rows:
        exp, mean64 = exp.permute(0, 2, 1), mean64.permute(0, 2, 1)
    if row_bias is not None:
        exp, mean64 = exp + row_bias, mean64 + row_bias.double()
    lens = torch.zeros(case['NVOX'], dtype=torch.float64)
    lens[case['interval_rank'][:case['I']].long()] = case['interval_lengths'][:case['I']].double()
    chain_err = _planes(case, lens[:, None] * U24 * ab).sum(2)
    bound = (Z * U24 * _planes(case, vol).abs().sum(2) + chain_err) / Z
    if rows:
        bound = bound.permute(0, 2, 1)
    if row_bias is not None:
        bound = bound + U24 * mean64.abs()
    return exp.contiguous(), mean64, bound


def og_effective(case, api, z):
    og = case['og']
    if not z:
        return og
    zg, zs = case['zgrad'][:, :, None], torch.tensor(case['zscale'], dtype=torch.float32)      # (B, C, 1, Y, X); zscale as the C float
    if case['layer'] == 'A' or not api.fused_zgrad:
        return og + zg * zs
    return (zg.double() * float(zs) + og.double()).float()   # one rounding of the product-sum (the double's own lies 29 bits below)


def ref_backward(case, og_eff):
    """-> depth_grad64, its bound, feat_grad (float64 in layer A, the oracle's fmaf chains in layer B)"""
    B, N, D, H, W = case['fr']
    C = case['C']
    rd, rf, rb = _points(case)
    rows = og_eff.permute(0, 2, 3, 4, 1).reshape(case['NVOX'], C)
    prod = rows.double()[rb] * case['feat'].double().view(-1, C)[rf]
    dg = torch.zeros(case['n_pts'], dtype=torch.float64)
    dg[rd] = prod.sum(1)
    n = C + 5
    bound = torch.zeros(case['n_pts'], dtype=torch.float64)
    bound[rd] = prod.abs().sum(1) * (n * U24 / (1 - n * U24))
    if case['layer'] == 'A':
        fg = torch.zeros(case['n_pix'], C, dtype=torch.float64).index_add_(0, rf, rows.double()[rb] * case['depth'].double().flatten()[rd][:, None])
    else:
        from oracle import oracle as O
        order = torch.argsort(rf * case['n_pts'] + rd)                                  # pixel, then depth bin (rd grows with d inside a pixel)
        P = case['P']
        _, fg = O.bev_pool_v2_bwd(rows.view(*case['grid'], C), case['depth'], case['feat'], case['ranks_depth'][:P][order],
                                  case['ranks_feat'][:P][order], case['ranks_bev'][:P][order], use_fma=True)
        fg = fg.reshape(case['n_pix'], C)
    return dg.view(B, N, D, H, W), bound.view(B, N, D, H, W), fg.view(B, N, H, W, C)


# ------------------------------------------------------------------------------------------------------------------ the launcher's rules
def index_lds(tv):
    return (3 * tv + 2 * NP_STAGE) * 4


def planar_lds(CC, tv):
    return CC * (tv + 4) * 4 + index_lds(tv)


def csplit_of(flags, C):
    f = (flags >> 4) & 0xF
    n = 20 if f == 0xF else f
    return n if n >= 1 and C % (4 * n) == 0 else 1


def cpl_of(flags, CC):
    return 8 if flags & CPL8 and CC % 8 == 0 else 4


def store_of(flags):
    bits = (flags & 3) | ((flags >> 17) & 1) << 2
    return 0 if bits == 0 else 1 if bits == 1 else 4


def expect_dense(C, tv, flags, addend):
    """the return code of fbbev_bev_pool_v2_dense_fwd[_add] for the grids of this table (capi.hip: pool_dense_fwd)"""
    et = bool(flags & (BF16 | F16))
    if flags & CL:
        if et or addend:
            return E_UNSUPPORTED
        if tv in SMALL_TILES:
            return E_UNSUPPORTED if (C // 4) * tv > 1024 else 0
        return 0
    csplit = csplit_of(flags, C)
    CC = C // csplit
    nt = 128 if (flags >> 8) & 3 == 1 else 256
    if nt // (CC // cpl_of(flags, CC)) < 1 or planar_lds(CC, tv) > 160 * 1024:
        return E_UNSUPPORTED
    split = bool(flags & SPLIT_LONG)
    if flags & PIPE and not et and not split and nt == 256 and store_of(flags) == 4 and tv in PIPE_TILES:
        return E_UNSUPPORTED if planar_lds(CC, tv) + index_lds(tv) > 160 * 1024 else 0
    if split or flags & GATHER8:
        return 0 if tv in (64, 128) and store_of(flags) == 4 and not et and nt == 256 else E_UNSUPPORTED
    return 0


def expect_zmean(C, tv, flags):
    if tv > 256:
        return E_UNSUPPORTED
    CC = C // csplit_of(flags, C)
    if 256 // (CC // cpl_of(flags, CC)) < 1 or planar_lds(CC, tv) > 64 * 1024:
        return E_UNSUPPORTED
    return 0


# ------------------------------------------------------------------------------------------------------------------ adapters
class Out:
    """a caller-owned output: `shape` elements at `strides` inside a buffer whose other elements hold the sentinel; the view starts NaN"""

    def __init__(self, shape, strides=None, dtype=torch.float32, fill=NAN):
        t = torch.empty(shape, dtype=dtype)
        strides = tuple(t.stride()) if strides is None else tuple(strides)
        span = 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        self.base = torch.full((span + 8,), SENTINEL, dtype=dtype)
        self.shape, self.strides = tuple(shape), strides
        self.base.as_strided(self.shape, strides).fill_(fill)
        pad = torch.ones(span + 8, dtype=torch.bool)
        pad.as_strided(self.shape, strides).fill_(False)
        self.pad = pad

    def result(self, base, nan_free=True):
        assert (base[self.pad] == SENTINEL).all(), 'the padding of a strided output lost its sentinel'
        v = base.as_strided(self.shape, self.strides).contiguous()
        assert not nan_free or not torch.isnan(v.float()).any(), 'NaN in an output'
        return v


class _Abi:
    def _p(self, t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def _call(self, fn, ins, outs, build_args, nan_free=True):
        """ins / outs: dicts of CPU tensors / Out; build_args(dev) -> argument list.  -> (code, {name: result})"""
        dev = {k: (self.to(t) if t is not None else None) for k, t in ins.items()}
        dout = {k: self.to(o.base) for k, o in outs.items()}
        code = fn(*build_args({**dev, **dout}), self.stream())
        res = {k: outs[k].result(self.back(dout[k]), nan_free and code == 0) for k in outs}
        for k, t in ins.items():
            if t is not None and not k.startswith('ws'):
                assert torch.equal(words_any(self.back(dev[k])), words_any(t)), f'input {k} was written'
        res['_ws'] = {k: self.back(dev[k]) for k in ins if k.startswith('ws')}
        return code, res

    def gather_ins(self, case):
        return dict(depth=case['depth'], feat=case['feat'], rd=case['ranks_depth'], rf=case['ranks_feat'], ir=case['interval_rank'],
                    st=case['interval_starts'], ln=case['interval_lengths'])

    def tile_index(self, case, tv, flags, ws=None):
        """-> (code, workspace bytes as int32 words)"""
        B, Z, Y, X = case['grid']
        nb = self.lib().fbbev_pool_dense_workspace_bytes(B, Z, Y, X)
        ins = dict(ir=case['interval_rank'], st=case['interval_starts'], counts=case['counts'], ws=torch.full((nb // 4,), -99, dtype=torch.int32))
        code, res = self._call(self.lib().fbbev_pool_tile_index, ins, {},
                               lambda d: [self._p(d['ir']), self._p(d['st']), self._p(d['counts']), case['n_max'], B, Z, Y, X, tv, flags,
                                          self._p(d['ws']), nb])
        return code, res['_ws']['ws']

    def _fwd(self, entry, case, tv, flags, out, extra_ins, tail):
        """the tile index, then a forward entry on the same device workspace"""
        B, Z, Y, X = case['grid']
        nb = self.lib().fbbev_pool_dense_workspace_bytes(B, Z, Y, X)
        ins = dict(self.gather_ins(case), counts=case['counts'], ws=torch.full((nb // 4,), -99, dtype=torch.int32), **extra_ins)

        def args(d):
            code = self.lib().fbbev_pool_tile_index(self._p(d['ir']), self._p(d['st']), self._p(d['counts']), case['n_max'], B, Z, Y, X, tv,
                                                    flags, self._p(d['ws']), nb, self.stream())
            assert code == 0, code
            g = [self._p(d[k]) for k in ('depth', 'feat', 'rd', 'rf', 'ir', 'st', 'ln')] + [B, case['C'], Z, Y, X]
            return g + tail(d, nb)
        code, res = self._call(getattr(self.lib(), entry), ins, {'out': out}, args)
        return code, res['out']

    def dense_fwd(self, case, tv, flags, out, addend=None, contiguous=False):
        sb, sc = (0, 0) if contiguous else (out.strides[0], out.strides[1])
        if addend is None:
            return self._fwd('fbbev_bev_pool_v2_dense_fwd', case, tv, flags, out, {},
                             lambda d, nb: [self._p(d['out']), sb, sc, self._p(d['ws']), nb, tv, flags])
        return self._fwd('fbbev_bev_pool_v2_dense_fwd_add', case, tv, flags, out, {'addend': addend},
                         lambda d, nb: [self._p(d['out']), sb, sc, self._p(d['ws']), nb, tv, flags, self._p(d['addend'])])

    def rows(self, case, tv, flags, out, addend=None):
        """out (B, ZYX, C) with a batch stride; addend (B, YX, C) may be a view with a padded row stride"""
        ab = addend._base if addend is not None and addend._base is not None else addend
        return self._fwd('fbbev_bev_pool_v2_dense_fwd_rows', case, tv, flags | CL, out, {'addend': ab},
                         lambda d, nb: [self._p(d['out']), out.strides[0], self._p(d['addend']), addend.stride(1) if addend is not None else 0,
                                        self._p(d['ws']), nb, tv, flags | CL])

    def zmean(self, case, tv, flags, out, z_groups=None, rows=False, row_bias=None):
        if rows:
            return self._fwd('fbbev_pool_zmean_rows', case, tv, flags, out, {'bias': row_bias},
                             lambda d, nb: [self._p(d['bias']), self._p(d['out']), self._p(d['ws']), nb, tv, flags])
        if z_groups is None:
            return self._fwd('fbbev_pool_zmean', case, tv, flags, out, {}, lambda d, nb: [self._p(d['out']), self._p(d['ws']), nb, tv, flags])
        n = min(z_groups, case['grid'][1]) * out.base.numel()
        return self._fwd('fbbev_pool_zmean_split', case, tv, flags, out, {'ws_partial': torch.full((n,), NAN)},
                         lambda d, nb: [self._p(d['out']), self._p(d['ws']), nb, tv, flags, z_groups, self._p(d['ws_partial']), n * 4])

    def bwd(self, case, og_view, z, dg, fg):
        """og_view: a (B, C, Z, Y, X) view with (padded) batch / channel strides -> (code, depth_grad, feat_grad)"""
        B, N, D, H, W = case['fr']
        _, Z, Y, X = case['grid']
        C = case['C']
        nb = self.lib().fbbev_pool_dense_bwd_workspace_bytes(B, N, D, H, W, C, Z, Y, X)
        base = og_view._base if og_view._base is not None else og_view
        ins = dict(og=base, zgrad=case['zgrad'] if z else None, depth=case['depth'], feat=case['feat'], rd=case['ranks_depth'],
                   ir=case['interval_rank'], st=case['interval_starts'], counts=case['counts'], ws=torch.zeros(nb // 4, dtype=torch.int32))

        def args(d):
            head = [self._p(d['og']), og_view.stride(0), og_view.stride(1)] + ([self._p(d['zgrad']), case['zscale']] if z else [])
            return head + [self._p(d[k]) for k in ('depth', 'feat', 'rd', 'ir', 'st', 'counts')] + \
                [case['n_max'], B, N, D, H, W, C, Z, Y, X, self._p(d['dg']), self._p(d['fg']), self._p(d['ws']), nb]
        entry = 'fbbev_bev_pool_v2_dense_bwd_z' if z else 'fbbev_bev_pool_v2_dense_bwd'
        code, res = self._call(getattr(self.lib(), entry), ins, {'dg': dg, 'fg': fg}, args)
        return code, res['dg'], res['fg']


def words_any(t):
    return t.contiguous().view(torch.uint8)


class GpuApi(_Abi):
    """libfbbev_hip.so as fb_bev_amd._capi loads and declares it, on cuda:0 (device code: fused multiply-adds where the compiler contracts)"""
    name, fused_zgrad = 'gpu', True

    def __init__(self):
        from fb_bev_amd import _capi
        self.c = _capi
        self.device = torch.device('cuda:0')

    def lib(self):
        return self.c.lib()

    def stream(self):
        return self.c._stream()

    def to(self, t):
        return t.to(self.device)

    def back(self, t):
        torch.cuda.synchronize()
        return t.cpu()


class EmuApi(_Abi):
    """tests/emu/emu_capi.py: the same launchers and kernels compiled for the CPU with -ffp-contract=off"""
    name, fused_zgrad = 'emu', False

    def __init__(self):
        sys.path.insert(0, os.path.join(HERE, 'emu'))
        import emu_capi
        self.E = emu_capi

    def lib(self):
        return self.E.lib()

    def stream(self):
        return None

    def to(self, t):
        return t.clone()

    def back(self, t):
        return t


# ------------------------------------------------------------------------------------------------------------------ case table
def _name(route, C, tv, flags=0, **kw):
    parts = [route, f'c{C}', f'tv{tv}']
    st = store_of(flags)
    parts += [f'st{st}'] if st != 4 else []
    parts += ['cpl8'] if flags & CPL8 else []
    cs = (flags >> 4) & 0xF
    parts += [f'csplit{"20" if cs == 0xF else cs}'] if cs else []
    parts += ['wg128'] if flags & WG128 else []
    parts += [f'swz{(flags >> 12) & 0x1F}'] if flags & SWZ else []
    parts += [n for bit, n in ((BF16, 'bf16'), (F16, 'f16'), (PIPE, 'pipe'), (GATHER8, 'gather8'), (SPLIT_LONG, 'split')) if flags & bit]
    parts += [k if v is True else v if k == 'which' else f'{k}{v}' for k, v in kw.items() if v not in (False, None)]
    return '-'.join(parts)


def _table(route, rows):
    out = {}
    for r in rows:
        C, tv, flags = r[0], r[1], (r[2] if len(r) > 2 else 0) | ST_SC1NT
        kw = r[3] if len(r) > 3 else {}
        if kw.pop('plain_store', None) is not None:
            flags = (flags & ~ST_SC1NT)
        out[_name(route, C, tv, flags, **kw)] = dict(C=C, tv=tv, flags=flags, **kw)
    return out


TILE_INDEX_CASES = [('main', k, tv) for k, tv in tilings() if k != 'bwd'] + [('garbage', 'small', tv) for tv in SMALL_TILES] + \
    [('garbage', 'planar', 64), ('garbage', 'flat', 64)]
_V = [CPL8, CPL8 | CSPLIT(2), CSPLIT(0xF), WG128, WG128 | CPL8, SWZ, SWZ | CHUNK(2) | CPL8]
DENSE_CASES = _table('dense', (
    [(C, tv) for C in CHANNELS for tv in PLANAR_TILES] +                                                   # refusals by the LDS rule included
    [(80, tv, f) for tv in (64, 128) for f in _V] +
    [(80, tv, f, {'plain_store': True}) for tv in (64, 128) for f in (ST_PLAIN, ST_NT)] +
    [(80, tv, f, dict(add=a)) for tv in (64, 128) for f in (0, BF16, F16, BF16 | WG128, F16 | CPL8 | CSPLIT(2)) for a in (False, True)
     if f or a] +
    [(80, tv, f, dict(pad=True, add=a)) for tv in (64, 128) for f, a in ((0, False), (SWZ | CHUNK(2), True), (BF16, False), (F16, True))] +
    [(80, tv, f) for tv in (64, 128) for f in (GATHER8, GATHER8 | CPL8, SPLIT_LONG, SPLIT_LONG | CPL8)] +
    [(80, 128, GATHER8 | CSPLIT(2), dict(add=True, pad=True)), (80, 64, SPLIT_LONG | CSPLIT(2) | CPL8, dict(add=True, pad=True)),
     (80, 256, GATHER8), (80, 256, SPLIT_LONG), (80, 64, GATHER8 | WG128)] +                                # refused: tile / workgroup size
    [(20, 64, CPL8 | CSPLIT(2)), (20, 128, BF16), (20, 64, SPLIT_LONG), (20, 128, GATHER8 | CPL8, dict(add=True))] +   # CPL8 denied, CSPLIT -> 1
    [(16, 64, CPL8), (16, 128, CPL8 | CSPLIT(2), dict(add=True)), (16, 256, BF16), (16, 512, F16), (16, 1024, BF16, dict(add=True)),
     (16, 64, SPLIT_LONG | CPL8), (16, 128, GATHER8)] +
    [(160, 64, CPL8), (160, 128, CSPLIT(2) | CPL8), (160, 256, CSPLIT(2), dict(add=True)), (160, 64, F16), (160, 64, SPLIT_LONG | CPL8),
     (160, 128, GATHER8 | CPL8)] +
    [(16, 1024, WG128), (16, 1024, WG128 | CPL8), (20, 1024, WG128 | CPL8), (16, 512, WG128), (16, 64, 0, dict(which='garbage'))]))
PIPE_CASES = _table('dense', (
    [(C, tv, PIPE) for C in CHANNELS for tv in PIPE_TILES] +
    [(80, tv, PIPE | f, dict(add=a, pad=p)) for tv in PIPE_TILES
     for f, a, p in ((CPL8, False, False), (CPL8 | CSPLIT(2), True, False), (SWZ | CHUNK(2), False, True), (CSPLIT(0xF), True, True))]))
CL_CASES = _table('cl', (
    [(C, tv, CL) for C in CHANNELS for tv in PLANAR_TILES + SMALL_TILES] +
    [(80, tv, CL | f) for tv in (64, 128, 8, 16, 32) for f in (SWZ, SWZ | CHUNK(2))] +
    [(80, tv, CL | CPL8) for tv in (64, 256, 1024)] + [(16, 64, CL | CPL8), (160, 128, CL | CPL8)] +
    [(80, tv, CL | f, {'plain_store': True}) for tv in (64, 16) for f in (ST_PLAIN, ST_NT)] +
    [(16, tv, CL, dict(which='garbage')) for tv in (64, 8, 16, 32)] +
    [(80, 64, CL | BF16), (80, 64, CL, dict(add=True))]))                                                   # refused
ROWS_CASES = _table('rows', (
    [(80, tv, f, dict(add=a, pad=p)) for tv in (64, 128) for f, a, p in ((0, True, True), (BF16, True, True), (F16, False, True), (CPL8, False, False))] +
    [(16, 64, BF16, dict(add=True, pad=True)), (16, 1024, 0, dict(add=True))]))
ZMEAN_CASES = _table('zmean', (
    [(C, tv) for C in CHANNELS for tv in ZMEAN_TILES + (512,)] +
    [(80, tv, f) for tv in (64, 128) for f in (CPL8, CSPLIT(2), CPL8 | CSPLIT(2))] + [(160, 128, CSPLIT(2)), (160, 256, CSPLIT(0xF)), (16, 256, CPL8)] +
    [(80, tv, f, dict(zg=zg)) for tv in (64, 128) for f in (0, CPL8) for zg in (1, 2, 3, 64)] + [(16, 256, 0, dict(zg=2)), (160, 64, CPL8, dict(zg=3))] +
    [(80, tv, 0, dict(zg=3, zpad=1)) for tv in (64, 128)] + [(80, 64, CPL8, dict(zg=2, zpad=1)), (80, 64, 0, dict(zpad=1))] +
    [(C, tv, f, dict(rows=True, bias=b)) for C, tv, f in ((80, 64, 0), (80, 128, CPL8), (16, 256, 0), (160, 64, CSPLIT(2)), (20, 128, 0))
     for b in (False, True)]))
COL_CASES = {k: v for k, v in ZMEAN_CASES.items() if not v.get('rows') and v.get('zg') in (None, 1)}
BWD_CASES = {f'bwd-{w}-c{C}{"-z" if z else ""}{"-pad" if p else ""}': dict(which=w, C=C, z=z, pad=p)
             for w, C in (('main', 16), ('main', 80), ('main', 160), ('odd', 16), ('odd', 20), ('odd', 80), ('odd', 160), ('main', 132))
             for z in (False, True) for p in (False, True) if C != 132 or (not z and not p)}
FAILED_CASES = ['dense-c80-tv128', 'dense-c80-tv64-bf16-add', 'dense-c80-tv64-f16', 'dense-c80-tv128-gather8', 'dense-c80-tv64-split',
                'dense-c80-tv64-pipe', 'dense-c80-tv128-cpl8-csplit2-pipe-add', 'cl-c80-tv64', 'cl-c80-tv16', 'rows-c80-tv64-bf16-add-pad',
                'zmean-c80-tv64', 'zmean-c80-tv128-zg2', 'zmean-c80-tv64-rows-bias', 'bwd-main-c80', 'bwd-main-c160-z-pad']
KNOBS = {'FBBEV_POOL_PIPE_TPW': {'1': list(PIPE_CASES), '2': list(PIPE_CASES), '4': list(PIPE_CASES)},
         'FBBEV_ZMEAN_COL': {'1': list(COL_CASES)}}
ALL = dict(**DENSE_CASES, **PIPE_CASES, **CL_CASES, **ROWS_CASES, **ZMEAN_CASES)


# ------------------------------------------------------------------------------------------------------------------ checks
def _exact(tag, got, exp):
    bad = int((words(got) != words(exp)).sum())
    assert bad == 0, f'{tag}: {bad} of {exp.numel()} words differ from the reference'
    return bad


def _inside(tag, got, exp64, bound):
    err = (got.double() - exp64).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert (err <= bound).all(), f'{tag}: max err / bound = {ratio:.4f}'
    return float(err.max()) if err.numel() else 0.0, ratio


def check_tile_index(api, kind, tv, failed=False, which='main'):
    geo = geometry(which)
    case = geo['failed'] if failed else geo
    flags = 0 if kind == 'planar' else CL
    code, ws = api.tile_index(case, tv, flags)
    assert code == 0, code
    B, Z, Y, X = geo['grid']
    r, st = case['interval_rank'][:case['I']].long(), case['interval_starts'][:case['I']]
    if kind == 'small':
        nt = (geo['NVOX'] + tv - 1) // tv
        first, last = torch.full((nt,), -1, dtype=torch.int32), torch.full((nt,), -1, dtype=torch.int32)
        for i, rr in enumerate(r.tolist()):
            if rr >= geo['NVOX']:
                continue
            if first[rr // tv] < 0:
                first[rr // tv] = i
            last[rr // tv] = i
        exp = torch.cat([first, last])
    else:
        if kind == 'planar':
            tpp = (geo['YX'] + tv - 1) // tv
            target = torch.tensor([p * geo['YX'] + k * tv for p in range(B * Z) for k in range(tpp)] + [geo['NVOX']])
        else:
            nt = (geo['NVOX'] + tv - 1) // tv
            target = torch.arange(nt + 1) * tv                                         # the closing entry lies past every rank
        lo = torch.searchsorted(r, target)
        pt = torch.where(lo < case['I'], torch.cat([st, st.new_zeros(1)])[lo.clamp(max=case['I'])], torch.tensor(case['P'], dtype=torch.int32))
        exp = torch.stack([lo.to(torch.int32), pt.to(torch.int32)], 1).flatten()
    assert torch.equal(ws[:exp.numel()], exp), f'tile table {kind} {tv}: {int((ws[:exp.numel()] != exp).sum())} words differ'
    assert (ws[exp.numel():] == -99).all(), 'the tile index wrote past its table'
    observed(f'{api.name} tile_index {which} {kind} tv {tv}{" failed build" if failed else ""}: {exp.numel()} table words equal the host computation')


def _planes_out(case, p, dtype):
    B, Z, Y, X = case['grid']
    C, zyx = case['C'], Z * Y * X
    if p.get('pad'):
        sc = zyx + 8
        return Out((B, C, zyx), ((C + 1) * sc + 16, sc, 1), dtype)
    return Out((B, C, zyx), None, dtype)


def _case_of(p, layer, failed=False):
    geo = geometry(p.get('which', 'main'), 0, p.get('zpad', 0))
    v = values(p.get('which', 'main'), p['C'], layer)
    return dict(geo['failed'] if failed else geo, **v)


def check_forward(api, name, failed=False, layers=('A', 'B')):
    """one case of DENSE_CASES / PIPE_CASES / CL_CASES / ROWS_CASES / ZMEAN_CASES on both layers"""
    p = ALL[name]
    route = name.split('-')[0]
    C, tv, flags = p['C'], p['tv'], p['flags']
    dtype = DTYPES[flags & (BF16 | F16)]
    for layer in layers:
        case = _case_of(p, layer, failed)
        B, Z, Y, X = case['grid']
        tag = f'{api.name} {name}{" failed build" if failed else ""} layer {layer}'
        if route in ('dense', 'cl'):
            addend = case['addend'] if p.get('add') else None
            want = expect_dense(C, tv, flags, addend is not None)
            if route == 'cl':
                out = Out((B, Z * Y * X, C), None, dtype)
                code, got = api.dense_fwd(case, tv, flags, out, addend, contiguous=True)
            else:
                out = _planes_out(case, p, dtype)
                code, got = api.dense_fwd(case, tv, flags, out, addend)
            assert code == want, f'{tag}: code {code}, the launcher\'s rule says {want}'
            if want:
                observed(f'{tag}: refused ({code}) as the LDS / route rule of the table says')
                continue
            layout = 'rows' if route == 'cl' else 'planes'
            split = bool(flags & SPLIT_LONG) and layer == 'B' and not failed
            exp = expected_volume(case, dtype, addend, layout).view(got.shape)
            if not split:
                _exact(tag, got, exp)
                observed(f'{tag}: {exp.numel()} words equal the reference')
            else:
                vol, ab, _ = ref_forward(case)
                lens = torch.zeros(case['NVOX'], dtype=torch.long)
                lens[case['interval_rank'][:case['I']].long()] = case['interval_lengths'][:case['I']].long()
                long_ = (lens > SPLIT_LEN)[:, None].expand(-1, C)
                n = lens.double()[:, None]
                bound, ref64 = n * U24 / (1 - n * U24) * ab, vol
                if addend is not None:
                    a64 = case['addend'].double().view(B, C, 1, Y * X).expand(B, C, Z, Y * X).permute(0, 2, 3, 1).reshape(-1, C)
                    ref64 = vol + a64
                    bound = bound + U24 * (vol.abs() + bound + a64.abs())
                to_planes = lambda t: _planes(case, t).reshape(got.shape)             # noqa: E731
                m = to_planes(long_)
                assert m.any()
                _exact(tag + ' (intervals of <= 32 points)', torch.where(m, torch.zeros_like(got), got), torch.where(m, torch.zeros_like(exp), exp))
                err, ratio = _inside(tag, got[m], to_planes(ref64)[m], to_planes(bound)[m])
                observed(f'{tag}: intervals of <= 32 points word for word; {int(m.sum())} sums of longer ones max|err| = {err:.3e}, '
                         f'max err / bound = {ratio:.4f}')
        elif route == 'rows':
            zyx = Z * Y * X
            out = Out((B, zyx, C), ((zyx + 3) * C + 8, C, 1) if p.get('pad') else None, dtype)
            addend = None
            if p.get('add'):
                wide = torch.full((B, Y * X, C + (12 if p.get('pad') else 0)), NAN)
                addend = wide[:, :, :C]
                addend.copy_(case['addend_rows'])
            code, got = api.rows(case, tv, flags, out, addend)
            assert code == 0, code
            _exact(tag, got, expected_volume(case, dtype, case['addend_rows'] if addend is not None else None, 'rows'))
            observed(f'{tag}: {got.numel()} words equal the reference')
        else:
            want = expect_zmean(C, tv, flags)
            rows, bias = p.get('rows'), case['row_bias'] if p.get('bias') else None
            out = Out((B, Y * X, C) if rows else (B, C, Y * X))
            code, got = api.zmean(case, tv, flags, out, p.get('zg'), rows, bias)
            assert code == want, f'{tag}: code {code}, the launcher\'s rule says {want}'
            if want:
                observed(f'{tag}: refused ({code}) as the LDS rule of the table says')
                continue
            exp, mean64, bound = expected_zmean(case, p.get('zg') or 1, bias, bool(rows))
            _exact(tag, got, exp)
            err, ratio = _inside(tag, got, mean64, bound) if layer == 'B' else (float((got.double() - mean64).abs().max()), 0.0)
            observed(f'{tag}: {exp.numel()} words equal the fp32 replay; against float64 max|err| = {err:.3e}' +
                     (f', max err / bound = {ratio:.4f}' if layer == 'B' else ' (the quotient\'s own rounding)'))


def check_column_equals_plane_walk(api, name):
    """FBBEV_ZMEAN_COL=1 only: the column form of a case against the plane walk the rows entry still takes, word for word"""
    p = ALL[name]
    if expect_zmean(p['C'], p['tv'], p['flags']):
        return
    for layer in ('A', 'B'):
        case = _case_of(p, layer)
        B, Z, Y, X = case['grid']
        _, col = api.zmean(case, p['tv'], p['flags'], Out((B, p['C'], Y * X)), p.get('zg'))
        _, walk = api.zmean(case, p['tv'], p['flags'], Out((B, Y * X, p['C'])), None, True, None)
        _exact(f'{api.name} {name} column form against the plane walk, layer {layer}', col, walk.permute(0, 2, 1).contiguous())


def check_backward(api, name, failed=False):
    p = BWD_CASES[name]
    for layer in ('A', 'B'):
        case = _case_of(p, layer, failed)
        B, N, D, H, W = case['fr']
        _, Z, Y, X = case['grid']
        C, zyx = p['C'], Z * Y * X
        tag = f'{api.name} {name}{" failed build" if failed else ""} layer {layer}'
        if p['pad']:
            sc = zyx + 12
            base = torch.full((B * ((C + 2) * sc + 4),), NAN)
            og = base.as_strided((B, C, Z, Y, X), ((C + 2) * sc + 4, sc, Y * X, X, 1))
        else:
            og = torch.empty(B, C, Z, Y, X)
        og.copy_(case['og'])
        dg, fg = Out((B, N, D, H, W)), Out((B, N, H, W, C))
        code, gd, gf = api.bwd(case, og, p['z'], dg, fg)
        if C > 128 and C % 8:
            assert code == E_UNSUPPORTED, code
            observed(f'{tag}: refused ({code}): more than 128 channels that are no multiple of 8')
            return
        assert code == 0, code
        if failed:
            assert (words(gf) == 0).all() and (words(gd) == 0).all(), f'{tag}: a gradient of a failed build is not +0'
            observed(f'{tag}: both gradients are zero')
            continue
        dg64, bound, fgx = ref_backward(case, og_effective(case, api, p['z']))
        dead = ~case['kept_bins'].any(1).view(B, N, H, W)
        assert (words(gf[dead]) == 0).all(), f'{tag}: feat_grad of a pixel without a kept point is not +0'
        assert (words(gd.flatten()[~case['kept']]) == 0).all(), f'{tag}: depth_grad of a dropped point is not +0'
        if layer == 'A':
            _exact(tag + ' depth_grad', gd, dg64.float())
            _exact(tag + ' feat_grad', gf, fgx.float())
            observed(f'{tag}: depth_grad ({gd.numel()}) and feat_grad ({gf.numel()}) equal float64 word for word')
        else:
            _exact(tag + ' feat_grad', gf, fgx)
            err, ratio = _inside(tag + ' depth_grad', gd, dg64, bound)
            observed(f'{tag}: feat_grad equals the oracle word for word; depth_grad max|err| = {err:.3e}, max err / bound = {ratio:.4f}')


def check_failed_build(api, name):
    if name.startswith('bwd'):
        return check_backward(api, name, failed=True)
    check_forward(api, name, failed=True)


def run_knob(api, knob, value):
    """the cases of one knob setting (the caller has set the environment); -> how many ran"""
    n = 0
    for name in KNOBS[knob][value]:
        check_forward(api, name)
        if knob == 'FBBEV_ZMEAN_COL':
            check_column_equals_plane_walk(api, name)
        n += 1
    return n
