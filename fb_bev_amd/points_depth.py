"""LiDAR points -> multi-view depth maps: the producer of `gt_depth` for CM_DepthNet's depth supervision.

The reference makes this tensor in the data pipeline, on the CPU (PointToMultiViewDepth, mmdet3d/datasets/pipelines/loading.py:876-966):
per camera it projects the sweep, sorts the points by `pixel_rank + depth / 100`, keeps the first point of every pixel and ships the
(N, H, W) map through the loader.  Here:

  points_to_depth(...)         GPU tensors: fbbev_points_to_depth, a z-buffer (one projection and one integer atomic per point and
                               camera, no sort); CPU tensors: a torch restatement of the reference's argsort route.
  lidar2img_from_info(...)     the host matrix chain of loading.py:922-950 in fp32, with its own quaternion -> rotation matrix.
  PointToMultiViewDepth        the pipeline step under its reference name: same constructor, points2depthmap and __call__.

The two routes agree except where the reference itself is not determined: two kept points of one pixel whose fp32 sort keys
`rank + depth / 100` are equal tie in its unstable argsort, and it keeps either; the kernel always gives the smaller depth, which is
one of the answers the reference may give (see include/fbbev.h).
"""
import numpy as np
import torch

__all__ = ['points_to_depth', 'lidar2img_from_info', 'quaternion_rotation_matrix', 'PointToMultiViewDepth', 'PIPELINES']


# ---------------------------------------------------------------------------------------------------------------- host matrices
def quaternion_rotation_matrix(q):
    """(w, x, y, z) -> (3, 3) float64 rotation matrix of the normalised quaternion (what pyquaternion's
    Quaternion(q).rotation_matrix gives; a quaternion whose norm is 1 within 1e-14 is used as it is, as there)."""
    w, x, y, z = (float(v) for v in q)
    n = float(np.sqrt(w * w + x * x + y * y + z * z))
    if n == 0.0:
        raise ValueError('a zero quaternion has no rotation matrix')
    if abs(1.0 - n) >= 1e-14:
        w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], dtype=np.float64)


def _rigid(rotation, translation):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = quaternion_rotation_matrix(rotation)                  # float64 -> float32 at the assignment, as the reference
    m[:3, 3] = np.asarray(translation, dtype=np.float64)
    return torch.from_numpy(m)


def lidar2img_from_info(curr, cam_names, intrins):
    """(N, 4, 4) f32: cam2img . inverse(camego2global . cam2camego) . lidarego2global per camera (loading.py:922-950), every matrix
    and every product in fp32 as there.  curr: the sample's info dict (ego2global_rotation / _translation and, per camera under
    curr['cams'][name], sensor2ego_* and ego2global_*; quaternions as (w, x, y, z)); intrins (N, 3, 3)."""
    intrins = torch.as_tensor(intrins, dtype=torch.float32).cpu()
    lidarego2global = _rigid(curr['ego2global_rotation'], curr['ego2global_translation'])
    out = []
    for cid, name in enumerate(cam_names):
        cam = curr['cams'][name]
        cam2camego = _rigid(cam['sensor2ego_rotation'], cam['sensor2ego_translation'])
        camego2global = _rigid(cam['ego2global_rotation'], cam['ego2global_translation'])
        cam2img = torch.eye(4, dtype=torch.float32)
        cam2img[:3, :3] = intrins[cid]
        lidar2cam = torch.inverse(camego2global.matmul(cam2camego)).matmul(lidarego2global)
        out.append(cam2img.matmul(lidar2cam))
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------------------------- CPU route
def _depthmap_argsort(points_img, h, w, downsample, lo, hi):
    """points2depthmap in our words: (P, 3) projected points (x, y in pixels, depth) -> (h, w) f32, the first point of every pixel in
    the order of the fp32 key rank + depth / 100."""
    depth_map = torch.zeros((h, w), dtype=torch.float32)
    coor = torch.round(points_img[:, :2] / downsample)
    depth = points_img[:, 2]
    keep = (coor[:, 0] >= 0) & (coor[:, 0] < w) & (coor[:, 1] >= 0) & (coor[:, 1] < h) & (depth < hi) & (depth >= lo)
    coor, depth = coor[keep], depth[keep]
    ranks = coor[:, 0] + coor[:, 1] * w
    order = (ranks + depth / 100.).argsort()
    coor, depth, ranks = coor[order], depth[order], ranks[order]
    first = torch.ones(coor.shape[0], dtype=torch.bool)
    first[1:] = ranks[1:] != ranks[:-1]
    coor, depth = coor[first].to(torch.long), depth[first]
    depth_map[coor[:, 1], coor[:, 0]] = depth
    return depth_map


def _project(points, lidar2img, post_rot, post_tran):
    """loading.py:951-957 -> (P, 3): pixel x, pixel y, depth"""
    p = points[:, :3].matmul(lidar2img[:3, :3].T) + lidar2img[:3, 3].unsqueeze(0)
    p = torch.cat([p[:, :2] / p[:, 2:3], p[:, 2:3]], 1)
    return p.matmul(post_rot.T) + post_tran.unsqueeze(0)


def _split(points, offsets, B):
    """-> (one (sum P, C) tensor, offsets as a list of B + 1 ints or None when they are only known on the device, int32 offsets tensor
    or None, the largest per-sample count)"""
    if isinstance(points, (list, tuple)):
        if offsets is not None:
            raise ValueError('offsets go with one concatenated points tensor, not with a list')
        if len(points) != B:
            raise ValueError(f'{len(points)} point tensors for a batch of {B}')
        counts = [int(p.shape[0]) for p in points]
        C = min(int(p.shape[1]) for p in points) if points else 3
        flat = torch.cat([p[:, :C] for p in points], 0) if len(points) != 1 else points[0]
        offs = [0]
        for c in counts:
            offs.append(offs[-1] + c)
        return flat, offs, None, max(counts, default=0)
    if offsets is None:
        if B != 1:
            raise ValueError('one points tensor for a batch needs offsets (B + 1 row numbers)')
        return points, [0, int(points.shape[0])], None, int(points.shape[0])
    if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
        return points, None, offsets.to(torch.int32), int(points.shape[0])       # counts stay on the device: the bound is all rows
    offs = [int(v) for v in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
    if len(offs) != B + 1:
        raise ValueError(f'offsets must hold {B + 1} entries, got {len(offs)}')
    return points, offs, None, max((b - a for a, b in zip(offs[:-1], offs[1:])), default=0)


def points_to_depth(points, lidar2img, post_rots, post_trans, H, W, downsample, depth_cfg, offsets=None):
    """-> (B, N, H // downsample, W // downsample) f32 on the points' device: per pixel the depth of the nearest LiDAR point that
    projects into it and lies in [depth_cfg[0], depth_cfg[1]), 0 where there is none.
    points: a list of B tensors (P_i, >= 3), or one (sum P, C) tensor with `offsets` (B + 1 row numbers: a list, a CPU tensor, or
    an int32 tensor on the device, which is not read on the host); lidar2img (B, N, 4, 4), post_rots (B, N, 3, 3), post_trans
    (B, N, 3).  GPU tensors: the kernel (fbbev_points_to_depth).  CPU tensors: the reference's argsort route in torch."""
    lidar2img, post_rots, post_trans = (torch.as_tensor(t) for t in (lidar2img, post_rots, post_trans))
    B, N = int(lidar2img.shape[0]), int(lidar2img.shape[1])
    lo, hi = float(depth_cfg[0]), float(depth_cfg[1])
    flat, offs, d_offs, max_points = _split(points, offsets, B)
    if flat.is_cuda:
        from . import _capi
        dev = flat.device
        if d_offs is None:
            d_offs = torch.tensor(offs, dtype=torch.int32).to(dev, non_blocking=True)
        mats = [t.to(device=dev, dtype=torch.float32).contiguous() for t in (lidar2img, post_rots, post_trans)]
        if flat.dtype != torch.float32 or (flat.shape[1] > 1 and flat.stride(1) != 1):
            flat = flat.float().contiguous()
        return _capi.points_to_depth(flat, d_offs, max_points, *mats, H, W, downsample, lo, hi)
    if offs is None:
        offs = [int(v) for v in d_offs.tolist()]
    h, w = int(H) // int(downsample), int(W) // int(downsample)
    out = torch.zeros((B, N, h, w), dtype=torch.float32)
    flat = flat.float()
    for b in range(B):
        pts = flat[offs[b]:offs[b + 1]]
        for n in range(N):
            out[b, n] = _depthmap_argsort(_project(pts, lidar2img[b, n].float(), post_rots[b, n].float(), post_trans[b, n].float()),
                                          h, w, downsample, lo, hi)
    return out


# ---------------------------------------------------------------------------------------------------------------- pipeline step
class PointToMultiViewDepth(object):
    """The reference's pipeline step (loading.py:876-966): results['points'] (a tensor, or an object with `.tensor`),
    results['img_inputs'] = (imgs, rots, trans, intrins, post_rots, post_trans, bda), results['curr'], results['cam_names'] ->
    results['gt_depth'] (N, H // downsample, W // downsample).  Points on the GPU take the kernel."""

    def __init__(self, grid_config, downsample=1):
        self.downsample = downsample
        self.grid_config = grid_config

    def points2depthmap(self, points, height, width):
        lo, hi = self.grid_config['depth'][:2]
        return _depthmap_argsort(points.cpu().float(), height // self.downsample, width // self.downsample, self.downsample, lo, hi)

    def __call__(self, results):
        points = results['points']
        points = points.tensor if hasattr(points, 'tensor') else points
        imgs, _, _, intrins = results['img_inputs'][:4]
        post_rots, post_trans = results['img_inputs'][4:6]
        lidar2img = lidar2img_from_info(results['curr'], results['cam_names'], intrins)
        n = len(results['cam_names'])
        results['gt_depth'] = points_to_depth([points], lidar2img[None], post_rots[None, :n], post_trans[None, :n], imgs.shape[2],
                                              imgs.shape[3], self.downsample, self.grid_config['depth'])[0]
        return results

    def __repr__(self):
        return f'{self.__class__.__name__}(grid_config={self.grid_config}, downsample={self.downsample})'


PIPELINES = {'PointToMultiViewDepth': PointToMultiViewDepth}     # a config's pipeline entry of that type resolves here


def build_pipeline_step(cfg):
    """dict(type='PointToMultiViewDepth', ...) -> the step"""
    cfg = dict(cfg)
    typ = cfg.pop('type')
    if typ not in PIPELINES:
        raise KeyError(f'pipeline step {typ!r} is not part of this library')
    return PIPELINES[typ](**cfg)
