"""Hand-built index tensors for the channels-last ROWS pooling (fbbev_bev_pool_v2_dense_fwd_rows), shared by the emulator test and the
GPU test: the smallest shapes at which the kernel can still go wrong.

B = 3 samples of a (Z, Y, X) = (3, 5, 8) grid -- 120 voxels per sample, no multiple of a 64- or 128-voxel tile, so tiles of the flat
B*Z*Y*X rank space straddle samples.  The occupied voxels are sorted and unique, a random ~60 % of [0, 120) and [256, 360): sample 1
(voxels 120..239) has no point at all and the tile(s) covering 128..255 are empty at both tile sizes, while every occupied tile also
holds empty voxels.  Interval lengths are random in 1..9; the points gather from random depth cells and feature rows."""
import torch

B, Z, Y, X = 3, 3, 5, 8
YX, ZYX, NVOX = Y * X, Z * Y * X, B * Z * Y * X
N_CAM, D, H, W = 1, 4, 4, 8
T_RING = 2                  # frames of history: the ring is (B, T + 1, N, C), slot 0 has batch stride 3 * N * C
TILES = (64, 128)
CHANNELS = (16, 80)


def build(C, seed=0):
    """-> dict(depth, feat, ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths, interval_rank, counts, n_max,
    addend_rows (B, YX, C)); index arrays padded with -7 to n_max like the rank build's outputs."""
    g = torch.Generator().manual_seed(seed)
    cand = torch.cat([torch.arange(0, 120), torch.arange(256, NVOX)])
    keep = torch.rand(cand.numel(), generator=g) < 0.6
    keep[0] = keep[-1] = True                                       # first and last voxel of the grid
    keep[cand == 119] = True                                      # last voxel of sample 0 (shares tile 1 / tile 0 with sample 1)
    ranks = cand[keep].to(torch.int32)
    n_int = ranks.numel()
    lengths = torch.randint(1, 10, (n_int,), generator=g, dtype=torch.int32)
    starts = (torch.cumsum(lengths, 0) - lengths).to(torch.int32)
    P = int(lengths.sum())
    n_max = P + 37
    depth = torch.rand(B, N_CAM, D, H, W, generator=g)
    feat = torch.randn(B, N_CAM, H, W, C, generator=g)
    rd = torch.randint(0, depth.numel(), (P,), generator=g, dtype=torch.int32)
    rf = torch.randint(0, B * N_CAM * H * W, (P,), generator=g, dtype=torch.int32)
    rb = torch.repeat_interleave(ranks, lengths.long()).to(torch.int32)

    def pad(t):
        out = torch.full((n_max,), -7, dtype=torch.int32)
        out[:t.numel()] = t
        return out
    case = dict(depth=depth, feat=feat, ranks_bev=pad(rb), ranks_depth=pad(rd), ranks_feat=pad(rf), interval_starts=pad(starts),
                interval_lengths=pad(lengths), interval_rank=pad(ranks), counts=torch.tensor([P, n_int], dtype=torch.int32),
                n_max=n_max, P=P, I=n_int, addend_rows=torch.randn(B, YX, C, generator=g))
    check(case)
    return case


def check(case):
    """The properties the shapes were chosen for, asserted on the host before anything runs."""
    ranks = case['interval_rank'][:case['I']].long()
    assert torch.equal(ranks, torch.unique(ranks)) and ranks.min() >= 0 and ranks.max() < NVOX       # sorted, unique, in range
    ln = case['interval_lengths'][:case['I']]
    assert ln.min() >= 1 and ln.max() <= 9 and len(set(ln.tolist())) > 1
    per_sample = torch.bincount(ranks // ZYX, minlength=B)
    assert per_sample[1] == 0 and per_sample[0] > 0 and per_sample[2] > 0                            # one sample without any point
    for tv in TILES:
        per_tile = torch.bincount(ranks // tv, minlength=(NVOX + tv - 1) // tv)
        first, last = torch.arange(per_tile.numel()) * tv, (torch.arange(per_tile.numel()) * tv + tv - 1).clamp(max=NVOX - 1)
        straddles = first // ZYX != last // ZYX
        assert (per_tile == 0).any(), tv                                                              # a whole tile is empty
        assert ((per_tile == 0) & straddles).any(), tv                                                # ... one of them across two samples
        assert ((per_tile > 0) & straddles).any(), tv                                                 # an occupied tile straddles two samples
        assert (per_tile[per_tile > 0] < (last - first + 1)[per_tile > 0]).all(), tv                  # empty voxels inside every occupied tile


def expected_rows(case, C, dtype, with_addend):
    """CPU oracle: the loop-exact pooled volume (in-order fmaf chains) in the reference layout (B,Z,Y,X,C), + the addend row of
    (b, y, x) with one fp32 add, cast to the ring's type by torch (round to nearest even) -> (B, Z*Y*X, C)."""
    from oracle import oracle as O
    P, n_int = case['P'], case['I']
    vol = O.bev_pool_v2_fwd(case['depth'], case['feat'], case['ranks_depth'][:P], case['ranks_feat'][:P], case['ranks_bev'][:P],
                            (B, Z, Y, X, C), case['interval_starts'][:n_int], case['interval_lengths'][:n_int], use_fma=True)
    rows = vol.reshape(B, Z, YX, C)
    if with_addend:
        rows = rows + case['addend_rows'][:, None]
    return rows.reshape(B, ZYX, C).to(dtype)


def words(t):
    """raw storage words of an f32 / bf16 / f16 tensor (bit-for-bit comparisons; NaN-safe, -0.0 != +0.0)"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
