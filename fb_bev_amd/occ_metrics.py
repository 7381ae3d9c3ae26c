"""Occupancy mIoU (mmdet3d/datasets/occ_metrics.py:50-180 Metric_mIoU; used by nuscenes_dataset.py:683-752).

Two input paths that count the same integers:
  * device: CUDA tensors.  `add_logits` scores the head's logits with the ONE launch that also writes the class map
    (fbbev_occ_classes); `add_batch` takes class ids and goes through the same kernel on a one-hot view.  Every call hands the kernel a
    fresh zeroed int32 table and adds it into an int64 device tensor; nothing reaches the host before `hist` / `count_miou()` is read.
  * host: numpy arrays, including the 1-D `occ_pred[mask_camera]` form the reference's dataset passes (nuscenes_dataset.py:746) and the
    probability forms (:124-125): integer bincount arithmetic.  The path for scoring saved predictions.
Metric_FScore (KD-tree, off by default in the reference) is not part of this module.
"""
import numpy as np

# Occ3D-nuScenes label set
CLASS_NAMES = ['others', 'barrier', 'bicycle', 'bus', 'car', 'construction_vehicle', 'motorcycle', 'pedestrian', 'traffic_cone',
               'trailer', 'truck', 'driveable_surface', 'other_flat', 'sidewalk', 'terrain', 'manmade', 'vegetation', 'free']


def range_ring(grid_hw, voxel_size, min_d, max_d):
    """(X, Y) bool: columns whose centre distance lies in [min_d, max_d].  float64 numpy with the operations and their order of
    occ_metrics.py:133-136, so that boundary columns fall on the same side (at max_d = 30 the column 75 cells out is exactly 30.0)."""
    X, Y = grid_hw
    ii, jj = np.meshgrid(np.arange(X), np.arange(Y), indexing='ij')
    offs = np.stack([ii - X // 2, jj - Y // 2], -1) * voxel_size
    dist = np.linalg.norm(offs, 2, -1)
    return (dist <= max_d) & (dist >= min_d)


class Metric_mIoU:
    def __init__(self, save_dir='.', num_classes=18, use_lidar_mask=False, use_image_mask=False, min_d=-1, max_d=100,
                 grid_hw=(200, 200), voxel_size=0.4):
        self.class_names = list(CLASS_NAMES)
        self.save_dir = save_dir
        self.use_lidar_mask = use_lidar_mask
        self.use_image_mask = use_image_mask
        self.num_classes = num_classes
        self.voxel_size = voxel_size
        self.grid_hw = tuple(grid_hw)
        self.min_d, self.max_d = min_d, max_d
        self.cnt = 0
        self.column_mask = range_ring(self.grid_hw, voxel_size, min_d, max_d)     # (X, Y) bool, once per instance
        self._host = np.zeros((num_classes, num_classes), dtype=np.int64)
        self.device_hist = None                  # int64 (n, n) on the GPU, created by the first device call
        self._column_mask_dev = None

    # ------------------------------------------------------------------ results
    @property
    def hist(self):
        """the reference's float64 (n, n) array: row = label, column = prediction"""
        total = self._host.copy()
        if self.device_hist is not None:
            total += self.device_hist.cpu().numpy()
        return total.astype(np.float64)

    @staticmethod
    def per_class_iu(hist):
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))

    def count_miou(self):
        res = {}
        iou = self.per_class_iu(self.hist)
        print(f'===> per class IoU of {self.cnt} samples:')
        for i in range(self.num_classes - 1):
            print(f'===> {self.class_names[i]} - IoU = ' + str(round(iou[i] * 100, 4)))
            res[self.class_names[i]] = round(iou[i] * 100, 2)
        res['Overall'] = round(np.nanmean(iou[:self.num_classes - 1]) * 100, 2)
        print(f'===> mIoU of {self.cnt} samples: ' + str(res['Overall']))
        return res

    # ------------------------------------------------------------------ input
    def _scoring_mask(self, mask_lidar, mask_camera):
        assert self.use_image_mask                                  # occ_metrics.py:147
        return mask_camera

    def add_batch(self, semantics_pred, semantics_gt, mask_lidar, mask_camera):
        if _is_cuda(semantics_pred):
            return self._add_ids_device(semantics_pred, semantics_gt, self._scoring_mask(mask_lidar, mask_camera))
        self.cnt += 1
        n = self.num_classes
        pred, gt = np.asarray(semantics_pred), np.asarray(semantics_gt)
        cam = np.asarray(mask_camera).astype(bool)
        if pred.ndim in (4, 2):                                     # probabilities: (X, Y, Z, n) or (voxels, n)
            pred = pred.argmax(-1)
        if pred.ndim == 1:                                          # the masked form: one id per voxel of mask_camera
            full = gt.copy()
            full[cam] = pred
            pred = full
        if pred.shape[:2] != self.grid_hw:
            raise ValueError(f'grid {pred.shape[:2]} does not match grid_hw={self.grid_hw}')
        keep = self._scoring_mask(mask_lidar, cam).astype(bool) & self.column_mask[:, :, None]
        g, p = gt[keep].astype(np.int64), pred[keep].astype(np.int64)
        k = (g >= 0) & (g < n)
        self._host += np.bincount(n * g[k] + p[k], minlength=n * n).reshape(n, n)

    def add_logits(self, logits, semantics_gt, mask_camera, c0=1):
        """Score the head's logits (B, C, H, W, D) (any strides) against labels / mask (B, X, Y, Z) or (X, Y, Z) in the class map's
        axis order (X = W, Y = H), with one kernel launch; -> the class map uint8 (B, X, Y, Z)."""
        import torch
        from . import _capi
        B, C, H, W, D = logits.shape
        n = C - int(c0)
        if n != self.num_classes:
            raise ValueError(f'{n} scored classes, the metric has num_classes={self.num_classes}')
        if (W, H) != self.grid_hw:
            raise ValueError(f'grid {(W, H)} does not match grid_hw={self.grid_hw}')
        gt = _as_u8(semantics_gt, (B, W, H, D), 'semantics_gt')
        mask = None if mask_camera is None else _as_u8(mask_camera, (B, W, H, D), 'mask_camera')
        if self._column_mask_dev is None or self._column_mask_dev.device != logits.device:
            self._column_mask_dev = torch.from_numpy(self.column_mask.astype(np.uint8)).to(logits.device)
        table = torch.zeros((n, n), dtype=torch.int32, device=logits.device)
        classes = _capi.occ_classes(logits, c0=c0, gt=gt, mask=mask, column_mask=self._column_mask_dev, hist=table)
        if self.device_hist is None:
            self.device_hist = torch.zeros((n, n), dtype=torch.int64, device=logits.device)
        self.device_hist += table
        self.cnt += B
        return classes

    def _add_ids_device(self, ids, semantics_gt, mask):
        """class ids uint8 (X, Y, Z) or (B, X, Y, Z) on the GPU: the kernel on their one-hot logits, viewed as (B, n, Y, X, Z)"""
        import torch
        if ids.dtype != torch.uint8 or ids.dim() not in (3, 4):
            raise ValueError(f'class ids must be uint8 (X, Y, Z) or (B, X, Y, Z), got {ids.dtype} {tuple(ids.shape)}')
        ids = ids if ids.dim() == 4 else ids[None]
        classes = torch.arange(self.num_classes, device=ids.device, dtype=torch.uint8).view(1, -1, 1, 1, 1)
        onehot = (ids[:, None] == classes).float()                 # (B, n, X, Y, Z)
        self.add_logits(onehot.permute(0, 1, 3, 2, 4), semantics_gt, mask, c0=0)


def _is_cuda(t):
    return hasattr(t, 'is_cuda') and t.is_cuda


def _as_u8(t, shape, name):
    import torch
    if not _is_cuda(t):
        raise ValueError(f'{name} must be a GPU tensor on the device path')
    if t.dim() == 3:
        t = t[None]
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name} must be {tuple(shape)}, got {tuple(t.shape)}')
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else (t if t.dtype == torch.uint8 else t.to(torch.uint8))
