"""The two occupancy metrics of the reference (mmdet3d/datasets/occ_metrics.py): Metric_mIoU (:50-180; used by
nuscenes_dataset.py:683-752) and Metric_FScore (:182-282; `eval --eval_fscore`, :305-330).

Metric_mIoU: two input paths that count the same integers:
  * device: CUDA tensors.  `add_logits` scores the head's logits with the ONE launch that also writes the class map
    (fbbev_occ_classes); `add_batch` takes class ids and goes through the same kernel on a one-hot view.  Every call hands the kernel a
    fresh zeroed int32 table and adds it into an int64 device tensor; nothing reaches the host before `hist` / `count_miou()` is read.
  * host: numpy arrays, including the 1-D `occ_pred[mask_camera]` form the reference's dataset passes (nuscenes_dataset.py:746) and the
    probability forms (:124-125): integer bincount arithmetic.  The path for scoring saved predictions.

Metric_FScore: the reference turns the occupied voxels of prediction and labels into point clouds, builds two KD-trees per frame and
asks for each point whether its nearest neighbour in the other cloud is closer than a threshold.  The points are the centres of a
regular grid, so that question is a bounded stencil over two occupancy bitmaps, and a frame is four integers: n_gt, n_pred, n_cmpl
(labels with a prediction nearby) and n_acc (predictions with a label nearby).  The same two paths:
  * device: CUDA uint8 class maps (X, Y, Z) or (B, X, Y, Z): one call of fbbev_occ_fscore_counts; the counts are appended to an int64
    device tensor, one row of four per frame, and nothing reaches the host before tot_acc / tot_cmpl / tot_f1_mean / count_fscore()
    is read.
  * host: numpy arrays in the reference's call forms (probabilities and the 1-D `pred[mask_camera]` form included): shifted boolean
    arrays.  No scikit-learn, and the caller's arrays are left as they were (the reference writes 255 into them).
What rounds is decided once, on the host, in float64 (`fscore_tables`): the squared coordinate differences per axis, and per threshold
the largest float64 T with sqrt(T) < threshold, so that `sqrt(d2) < threshold` is `d2 <= T` and both paths only add and compare.  This
matters: at the threshold of `eval` (0.4 with 0.4 m voxels) two ADJACENT centres are closer than the threshold or not depending on the
last bits of `i * 0.4 + 0.2 - 40` (130 of the 199 adjacent pairs along x are, 69 are not), so reasoning in whole cells gives another
score than the reference's KD-tree.
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


# ---------------------------------------------------------------------------------------------------------------------- F-score
def fscore_threshold_constant(threshold):
    """T(threshold): the largest float64 d2 with sqrt(d2) < threshold.  sqrt is correctly rounded and monotone, so
    `sqrt(d2) < threshold` <=> `d2 <= T` for every float64 d2 >= 0."""
    thr = np.float64(threshold)
    if not thr > 0 or not np.isfinite(thr):
        raise ValueError(f'threshold must be positive and finite, got {threshold}')
    t = thr * thr
    while np.sqrt(t) >= thr:
        t = np.nextafter(t, -np.inf)
    while np.sqrt(np.nextafter(t, np.inf)) < thr:
        t = np.nextafter(t, np.inf)
    return float(t)


def fscore_radius(thresholds, voxel_size):
    """R: how many cells away along an axis a neighbour within a threshold can lie, plus one: max floor(thr / voxel_size[a]) + 1.  The
    quotient is rounded to nine decimals first: 1.2 / 0.4 is 2.9999999999999996 in float64, and three cells apart is then exactly the
    case that rounding decides, so it must be inside the stencil."""
    return max(int(np.floor(round(float(t) / float(v), 9))) + 1 for t in thresholds for v in voxel_size)


def fscore_axis_coordinates(n, voxel_size, lower):
    """the centre coordinates of n cells, with the expression and the order of voxel2points (occ_metrics.py:216-218), float64"""
    return np.arange(n) * voxel_size + voxel_size / 2 + lower


def fscore_tables(shape, voxel_size, pc_range, threshold_acc, threshold_complete):
    """Everything of the F-score that rounds, for a grid `shape` = (X, Y, Z):
      R       the stencil radius (fscore_radius)
      sq      three float64 arrays (n_a, 2R + 1): sq_a[i][o + R] = (c_a[i] - c_a[i + o]) ** 2, inf where i + o leaves the grid
      T_acc, T_cmpl   fscore_threshold_constant of the two thresholds
      offsets (n, 3) int32, sorted: the (ox, oy, oz) whose best case over the whole grid passes the larger T.  Rounding is monotone,
              so the sum of the per-axis minima bounds every sum from below and the test drops no offset that could hit."""
    R = fscore_radius((threshold_acc, threshold_complete), voxel_size)
    sq = []
    for a, n in enumerate(shape):
        c = fscore_axis_coordinates(int(n), voxel_size[a], pc_range[a])
        t = np.full((int(n), 2 * R + 1), np.inf, dtype=np.float64)
        for o in np.arange(-R, R + 1):
            i = np.arange(max(0, -o), n - max(0, o))
            if len(i):
                t[i, o + R] = (c[i] - c[i + o]) ** 2
        sq.append(t)
    T_acc, T_cmpl = fscore_threshold_constant(threshold_acc), fscore_threshold_constant(threshold_complete)
    best = [t.min(0) for t in sq]
    offsets = [(ox, oy, oz) for ox in np.arange(-R, R + 1) for oy in np.arange(-R, R + 1) for oz in np.arange(-R, R + 1)
               if (best[0][ox + R] + best[1][oy + R]) + best[2][oz + R] <= max(T_acc, T_cmpl)]
    return dict(R=R, sq=tuple(sq), T_acc=T_acc, T_cmpl=T_cmpl, offsets=np.array(offsets, dtype=np.int32).reshape(-1, 3))


def fscore_counts_host(P, G, tab):
    """(n_gt, n_pred, n_cmpl, n_acc) of one frame from the occupancy masks P, G (X, Y, Z) bool: for each listed offset o, the voxels q
    with q + o in the other set and (sq_x[qx][ox] + sq_y[qy][oy]) + sq_z[qz][oz] <= T -- the arithmetic of the kernel, on shifted views"""
    R, (sqx, sqy, sqz) = tab['R'], tab['sq']
    hit_p, hit_g = np.zeros_like(P), np.zeros_like(G)
    for ox, oy, oz in tab['offsets'].tolist():
        q = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip((ox, oy, oz), P.shape))      # q and q + o inside the grid
        t = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip((ox, oy, oz), P.shape))
        if any(s.stop <= s.start for s in q):
            continue
        d2 = (sqx[q[0], ox + R][:, None] + sqy[q[1], oy + R][None, :])[:, :, None] + sqz[q[2], oz + R][None, None, :]
        hit_p[q] |= P[q] & G[t] & (d2 <= tab['T_acc'])
        hit_g[q] |= G[q] & P[t] & (d2 <= tab['T_cmpl'])
    return int(G.sum()), int(P.sum()), int(hit_g.sum()), int(hit_p.sum())


class Metric_FScore:
    """The reference's class (occ_metrics.py:182-282) with its constructor, add_batch and count_fscore; `leaf_size` is kept and unused.
    tot_acc, tot_cmpl and tot_f1_mean are evaluated when read, from the frames' integer counts in arrival order, with the reference's
    float64 steps (:249-275)."""

    def __init__(self, leaf_size=10, threshold_acc=0.6, threshold_complete=0.6, voxel_size=[0.4, 0.4, 0.4],
                 range=[-40, -40, -1, 40, 40, 5.4], void=[17, 255], use_lidar_mask=False, use_image_mask=False):
        self.leaf_size = leaf_size
        self.threshold_acc = threshold_acc
        self.threshold_complete = threshold_complete
        self.voxel_size = voxel_size
        self.range = range
        self.void = void
        self.use_lidar_mask = use_lidar_mask
        self.use_image_mask = use_image_mask
        self.cnt = 0
        self.eps = 1e-8
        self._void_lut = np.zeros(256, dtype=bool)             # by effective id
        for v in void:
            if 0 <= int(v) <= 255:
                self._void_lut[int(v)] = True
        self._tables = {}                        # grid shape -> fscore_tables
        self._dev_tables = {}                    # (grid shape, device) -> the tables on that device
        self._host_counts = []                   # (n_gt, n_pred, n_cmpl, n_acc) per host-path frame
        self._order = []                         # arrival order: ('h', index) | ('d', first row, rows)
        self.device_counts = None                # int64 (capacity, 4) on the GPU; the first _dev_rows rows are frames
        self._dev_rows = 0
        self._totals_key, self._totals_val = None, None

    # ------------------------------------------------------------------ results
    def frame_counts(self):
        """int64 (frames, 4): n_gt, n_pred, n_cmpl, n_acc per frame in arrival order (reads the device tensor)"""
        dev = self.device_counts[:self._dev_rows].cpu().numpy() if self._dev_rows else np.zeros((0, 4), dtype=np.int64)
        rows = []
        for e in self._order:
            rows.extend([self._host_counts[e[1]]] if e[0] == 'h' else dev[e[1]:e[1] + e[2]].tolist())
        return np.array(rows, dtype=np.int64).reshape(-1, 4)

    def _totals(self):
        key = (len(self._order), self._dev_rows)
        if self._totals_key != key:
            tot_acc, tot_cmpl, tot_f1 = 0., 0., 0.
            for i, (n_gt, n_pred, n_cmpl, n_acc) in enumerate(self.frame_counts().tolist()):
                if n_pred == 0:                                                 # :249-252
                    accuracy, completeness, fmean = 0, 0, 0
                else:
                    if n_gt == 0:
                        raise ValueError(f'frame {i}: {n_pred} predicted voxels and no ground-truth voxel (the reference raises '
                                         f'inside KDTree on an empty point set)')
                    completeness = np.float64(n_cmpl) / np.float64(n_gt)        # complete_mask.mean()
                    accuracy = np.float64(n_acc) / np.float64(n_pred)
                    fmean = 2.0 / (1 / (accuracy + self.eps) + 1 / (completeness + self.eps))
                tot_acc += accuracy
                tot_cmpl += completeness
                tot_f1 += fmean
            self._totals_key, self._totals_val = key, (tot_acc, tot_cmpl, tot_f1)
        return self._totals_val

    @property
    def tot_acc(self):
        return self._totals()[0]

    @property
    def tot_cmpl(self):
        return self._totals()[1]

    @property
    def tot_f1_mean(self):
        return self._totals()[2]

    def count_fscore(self):
        res = {}
        print('\n######## F score: {} #######'.format(self.tot_f1_mean / self.cnt))
        res['f-score'] = round(self.tot_f1_mean / self.cnt, 4)
        return res

    # ------------------------------------------------------------------ tables
    def tables(self, shape):
        shape = tuple(int(n) for n in shape)
        if shape not in self._tables:
            self._tables[shape] = fscore_tables(shape, self.voxel_size, self.range, self.threshold_acc, self.threshold_complete)
        return self._tables[shape]

    def _device_tables(self, shape, device):
        import ctypes
        import torch
        key = (tuple(shape), str(device))
        if key not in self._dev_tables:
            tab = self.tables(shape)
            bits = (ctypes.c_uint32 * 8)()
            for v in np.nonzero(self._void_lut)[0].tolist():
                bits[v >> 5] |= 1 << (v & 31)
            self._dev_tables[key] = dict(void_bits=bits, sq=tuple(torch.from_numpy(t).to(device) for t in tab['sq']),
                                         offsets=torch.from_numpy(tab['offsets']).to(device))
        return self._dev_tables[key]

    # ------------------------------------------------------------------ input
    def _occupied(self, ids, cam):
        """(X, Y, Z) bool: the effective id (255 where cam is False) is none of `void` (voxel2points, :213)"""
        eff = np.where(cam, ids, 255).astype(np.int64)
        return ~((eff >= 0) & (eff <= 255) & self._void_lut[eff & 255])

    def add_batch(self, semantics_pred, semantics_gt, mask_lidar, mask_camera):
        assert self.use_image_mask                                  # occ_metrics.py:230
        if _is_cuda(semantics_pred):
            return self._add_device(semantics_pred, semantics_gt, mask_camera)
        pred, gt = np.asarray(semantics_pred), np.asarray(semantics_gt)
        cam = np.ones(gt.shape, dtype=bool) if mask_camera is None else np.asarray(mask_camera).astype(bool)
        if pred.ndim in (4, 2):                                     # probabilities: (X, Y, Z, n) or (voxels, n)
            pred = pred.argmax(-1)
        if pred.ndim == 1:                                          # the masked form: one id per voxel of mask_camera
            full = np.full(gt.shape, 255, dtype=np.int64)
            full[cam] = pred
            pred = full
        if pred.shape != gt.shape or gt.ndim != 3:
            raise ValueError(f'prediction {pred.shape} and labels {gt.shape} must be one (X, Y, Z) grid')
        # effective id: 255 where the camera mask hides the voxel (:234-240), without writing to the caller's arrays
        counts = fscore_counts_host(self._occupied(pred, cam), self._occupied(gt, cam), self.tables(gt.shape))
        if counts[0] == 0 and counts[1] > 0:
            raise ValueError(f'frame {self.cnt}: {counts[1]} predicted voxels and no ground-truth voxel (the reference raises inside '
                             f'KDTree on an empty point set)')
        self._order.append(('h', len(self._host_counts)))
        self._host_counts.append(counts)
        self.cnt += 1

    def _add_device(self, ids, semantics_gt, mask_camera):
        """class ids uint8 (X, Y, Z) or (B, X, Y, Z) on the GPU: one call of fbbev_occ_fscore_counts, one row of counts per frame"""
        import torch
        from . import _capi
        if ids.dtype != torch.uint8 or ids.dim() not in (3, 4):
            raise ValueError(f'class ids must be uint8 (X, Y, Z) or (B, X, Y, Z), got {ids.dtype} {tuple(ids.shape)}')
        ids = (ids if ids.dim() == 4 else ids[None]).contiguous()
        B, shape = ids.shape[0], tuple(ids.shape[1:])
        gt = _as_u8(semantics_gt, ids.shape, 'semantics_gt')
        mask = None if mask_camera is None else _as_u8(mask_camera, ids.shape, 'mask_camera')
        tab, dev = self.tables(shape), self._device_tables(shape, ids.device)
        counts = _capi.occ_fscore_counts(ids, gt, mask, dev['void_bits'], *dev['sq'], dev['offsets'], tab['R'], tab['T_acc'],
                                         tab['T_cmpl'])
        if self.device_counts is None or self._dev_rows + B > self.device_counts.shape[0]:
            grown = torch.zeros((max(64, 2 * (self._dev_rows + B)), 4), dtype=torch.int64, device=ids.device)
            if self._dev_rows:
                grown[:self._dev_rows] = self.device_counts[:self._dev_rows]
            self.device_counts = grown
        self.device_counts[self._dev_rows:self._dev_rows + B] = counts
        self._order.append(('d', self._dev_rows, B))
        self._dev_rows += B
        self.cnt += B


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
