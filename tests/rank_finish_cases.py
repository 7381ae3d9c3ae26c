"""Inputs of the high-digit-first rank build (FBBEV_RANK_FINISH), shared by tests/test_emu_rank_finish.py (CPU emulator) and
tests/test_gpu_rank_finish.py (MI355X).  Not a test module.

Every case is a materialised `coor` (B, N, D, H, W, 3) on a grid with lower bound 0 and interval 1, built from a list of LOCAL
voxel ids per sample (a point sits in the centre of its voxel; the rest of the sample's points lie outside the grid), in a
seeded shuffled point order.  A sample's key has lbits = ceil(log2(voxels per sample)) bits; the route scatters by the high 10
and finishes the low lbits - 10 inside a bucket of 2^(lbits - 10) consecutive voxels, so the cases are stated in buckets:

  low1_B1       1 280 voxels (low digit of ONE bit, 640 buckets), B = 1
  low4_B3       41 x 39 x 10 = 15 990 voxels (16-voxel buckets, the last one partial), B = 3 with different point counts:
                sample 0: a bucket of exactly 64 points, one of 65, one of 3 000 (47 rounds: beyond the register staging),
                the last voxel of the grid, sparse others (most buckets empty); sample 1: all 9 000 kept points in ONE
                voxel (one interval, three 4 096-element tiles of the interval kernel, two of them without a head); sample 2: 300
                scattered points
  low10_B2      100 x 100 x 53 = 530 000 voxels (1 024-voxel buckets, 518 of them, the last one partial), B = 2: buckets of 64,
                65 and 4 000 points, the last voxel, a scattered second sample
  one_voxel_B1  B = 1, every kept point in one voxel
  empty_B2      P = 0
"""
import numpy as np
import torch

SHAPE = (2, 3, 1)          # N, D, H of every case: ranks_feat = (pid // DHW) * HW + pid % HW is not the identity


def grid_config(dims):
    X, Y, Z = dims
    return {'x': [0.0, float(X), 1.0], 'y': [0.0, float(Y), 1.0], 'z': [0.0, float(Z), 1.0], 'depth': [1.0, 2.0, 1.0]}


def _coor(dims, per_sample, npb, seed):
    X, Y, Z = dims
    N, D, H = SHAPE
    assert npb % (N * D * H) == 0
    g = np.random.default_rng(seed)
    out = np.full((len(per_sample), npb, 3), 1.0e6, dtype=np.float32)
    for b, vox in enumerate(per_sample):
        vox = np.asarray(vox, dtype=np.int64)
        assert vox.size <= npb and (vox.size == 0 or (vox.min() >= 0 and vox.max() < X * Y * Z))
        slot = g.permutation(npb)[:vox.size]
        out[b, slot, 0] = vox % X + 0.5
        out[b, slot, 1] = (vox // X) % Y + 0.5
        out[b, slot, 2] = vox // (X * Y) + 0.5
    return torch.from_numpy(out).view(len(per_sample), N, D, H, npb // (N * D * H), 3).contiguous()


def _bucket(g, bucket, low_bits, count, limit):
    """`count` points over the voxels of one bucket (with repeats), every voxel below `limit`"""
    lo = bucket << low_bits
    hi = min(lo + (1 << low_bits), limit)
    return g.integers(lo, hi, size=count)


def case(name, seed=0):
    """-> (dims, coor)"""
    g = np.random.default_rng(100 + seed)
    if name == 'low1_B1':
        dims = (16, 16, 5)
        return dims, _coor(dims, [g.integers(0, 1280, size=1500)], 2400, seed)
    if name == 'low4_B3':
        dims, V = (41, 39, 10), 15990
        s0 = np.concatenate([_bucket(g, 5, 4, 64, V), _bucket(g, 7, 4, 65, V), _bucket(g, 9, 4, 3000, V),
                             np.full(3, V - 1), _bucket(g, 999, 4, 20, V), g.integers(200 * 16, V, size=800)])
        s1 = np.full(9000, 7777 + seed)
        s2 = g.integers(0, V, size=300)
        return dims, _coor(dims, [s0, s1, s2], 12000, seed)
    if name == 'low10_B2':
        dims, V = (100, 100, 53), 530000
        s0 = np.concatenate([_bucket(g, 3, 10, 64, V), _bucket(g, 4, 10, 65, V), _bucket(g, 100, 10, 4000, V),
                             np.full(2, V - 1), _bucket(g, 517, 10, 50, V), g.integers(8 * 1024, V, size=1500)])
        s1 = g.integers(0, V, size=2000)
        return dims, _coor(dims, [s0, s1], 6000, seed)
    if name == 'one_voxel_B1':
        dims = (41, 39, 10)
        return dims, _coor(dims, [np.full(9000, 123)], 12000, seed)
    if name == 'empty_B2':
        dims = (16, 16, 5)
        return dims, _coor(dims, [[], []], 1200, seed)
    raise KeyError(name)


CASES = ['low1_B1', 'low4_B3', 'low10_B2', 'one_voxel_B1', 'empty_B2']


def depth_for(coor, seed=3):
    """a depth distribution for the depth-threshold entry: 40 % of the points under the threshold, one exactly on it"""
    g = torch.Generator().manual_seed(seed)
    d = torch.rand(coor.shape[:-1], generator=g) + 0.5
    d[torch.rand(d.shape, generator=g) < 0.4] = 0.005
    d.view(-1)[1] = 0.01
    return d.contiguous()


def oracle_index(dims, coor, depth=None, thr=0.01):
    """(ranks_bev, ranks_depth, ranks_feat, starts, lengths, interval_rank) of the oracle; empty tensors for P = 0"""
    from oracle import oracle as O
    ovt = O.ViewTransformerOracle(grid_config(dims), (8, 8), 8)
    if depth is not None:
        coor = coor.clone()
        coor.view(-1, 3)[~(depth.reshape(-1) > thr)] = 1.0e6
    rb, rd, rf, st, ln = ovt.voxel_pooling_prepare_v2(coor)
    if rb is None:
        e = torch.zeros(0, dtype=torch.int32)
        return e, e, e, e, e, e
    return rb, rd, rf, st, ln, rb[st.long()].contiguous()


def assert_index(got, exp, what=''):
    """got: (rb, rd, rf, st, ln, ir, counts) full-size CPU tensors; exp: exact-size tensors of oracle_index or another build"""
    P, I = (int(x) for x in got[6].tolist())
    assert (P, I) == (exp[0].numel(), exp[3].numel()), (what, P, I, exp[0].numel(), exp[3].numel())
    names = ('ranks_bev', 'ranks_depth', 'ranks_feat', 'interval_starts', 'interval_lengths', 'interval_rank')
    for k, (a, e) in enumerate(zip(got[:6], exp)):
        assert torch.equal(a[:P if k < 3 else I], e), (what, names[k])


def exact(got):
    P, I = (int(x) for x in got[6].tolist())
    return tuple(t[:P].clone() for t in got[:3]) + tuple(t[:I].clone() for t in got[3:6])


# ---------------------------------------------------------------- GPU side (run in a child process: the product reads the knobs once)
def gpu_build_all(out_path):
    """Every case + the depth entry + two builds on one workspace + capture-and-replay through fb_bev_amd on cuda:0, each
    checked against the oracle; the exact-size index tensors of every build are saved to out_path for the route-vs-route
    comparison of the parent process."""
    import os
    from fb_bev_amd import synthetic as S
    from fb_bev_amd.view_transformer import LSSViewTransformerFunction3D
    from oracle import oracle as O
    assert os.environ.get('FBBEV_RANK_SEG') == '2' and os.environ.get('FBBEV_RANK_FINISH') in ('0', '1')
    dev = torch.device('cuda:0')
    saved = {}

    def full(idx):
        torch.cuda.synchronize()
        return tuple(t.cpu() for t in (idx.ranks_bev, idx.ranks_depth, idx.ranks_feat, idx.interval_starts, idx.interval_lengths,
                                       idx.interval_rank, idx.counts))

    for name in CASES:
        dims, coor = case(name)
        vt = LSSViewTransformerFunction3D(grid_config(dims), (8, 8), 8).to(dev)
        n = coor.numel() // 3
        ws = vt._cache[('rank_ws', dev, n)] = torch.full((_ws_bytes(n),), 0xA5, dtype=torch.uint8, device=dev)   # garbage workspace
        got = full(vt.build_index(coor.to(dev)))
        assert_index(got, oracle_index(dims, coor), name)
        saved[name] = exact(got)
        if name == 'low4_B3':
            d = depth_for(coor)
            got = full(vt.build_index(coor.to(dev), depth=d.to(dev), depth_threshold=0.01))
            assert_index(got, oracle_index(dims, coor, d), name + ' depth')
            saved[name + '_depth'] = exact(got)
            _, coor2 = case(name, seed=1)                      # other inputs, the workspace as the build above left it
            got = full(vt.build_index(coor2.to(dev)))
            assert_index(got, oracle_index(dims, coor2), name + ' second build')
            saved[name + '_second'] = exact(got)
            assert vt._cache[('rank_ws', dev, n)] is ws

    # keys from the camera geometry: B = 2, two cameras, 8 x 22 feature pixels, 50 x 50 x 8 = 20 000 voxels (32-voxel buckets);
    # captured once, replayed with other camera tensors in the same buffers, against eager builds and the oracle
    cfg = S.PathConfig('RF', (64, 176), 8, S.CONFIGS['SMALL'].grid_config, 20, n_cams=2)
    ovt = O.ViewTransformerOracle(cfg.grid_config, cfg.input_size, cfg.downsample)
    vt = LSSViewTransformerFunction3D(cfg.grid_config, cfg.input_size, cfg.downsample).to(dev)
    cam0, cam1 = (S.camera_rig(cfg, 2, seed=s, bda_aug=True) for s in (0, 7))
    cam_s = [t.to(dev).clone() for t in cam0]
    eager0 = full(vt.build_index_from_cams(*cam_s))            # warm-up: allocates the cached workspace
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vt.build_index_from_cams(*cam_s)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        idx = vt.build_index_from_cams(*cam_s)
    g.replay()
    assert_index(full(idx), exact(eager0), 'replay 0')
    for dst, src in zip(cam_s, cam1):
        dst.copy_(src)
    g.replay()
    replay1 = full(idx)
    eager1 = full(vt.build_index_from_cams(*[t.to(dev) for t in cam1]))
    assert_index(replay1, exact(eager1), 'replay 1')
    coor1 = vt.get_lidar_coor(*[t.to(dev) for t in cam1]).cpu()           # the contract pins bit-exactness at coor
    erb, erd, erf, est, eln = ovt.voxel_pooling_prepare_v2(coor1)
    assert_index(replay1, (erb, erd, erf, est, eln, erb[est.long()].contiguous()), 'replay 1 vs oracle')
    assert exact(eager0)[0].numel() != exact(eager1)[0].numel() or not torch.equal(exact(eager0)[1], exact(eager1)[1])
    saved['geom_replay'] = exact(replay1)
    torch.save(saved, out_path)
    print('built', len(saved))


def _ws_bytes(n):
    from fb_bev_amd import _capi
    return _capi.rank_workspace_bytes(n)
