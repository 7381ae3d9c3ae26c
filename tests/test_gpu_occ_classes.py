"""fbbev_occ_classes on the MI355X through fb_bev_amd._capi.occ_classes, at the shapes of tests/occ_cases.py (the emulator test runs the
same table): class bytes against the parent's softmax / argmax / shuffle chain, the confusion table against a numpy bincount, guard
bytes and read-only inputs, run-to-run identical bytes; the device path of occ_metrics.Metric_mIoU against the record of the
reference's class; FBOCC.predict_occupancy_classes against predict_occupancy on both head routes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_cases as OC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    return OC.GpuApi()


@pytest.mark.parametrize('case', OC.CASES, ids=OC.CASE_IDS)
def test_classes_equal_the_parent_chain(api, case):
    OC.check_classes(api, case)


@pytest.mark.parametrize('kind', ['uniform', 'skewed'])
@pytest.mark.parametrize('case', OC.CASES, ids=OC.CASE_IDS)
def test_hist_equals_bincount(api, case, kind):
    OC.check_hist(api, case, kind)


@pytest.mark.parametrize('name', ['b1_17x33x16_cl', 'b1_17x33x16_planes', 'b2_5x7x3_cl'])
def test_two_runs_give_identical_bytes(api, name):
    case = OC.CASES[OC.CASE_IDS.index(name)]
    n = case['C'] - case['c0']
    L, exp = OC.reference(case)
    gt = OC.labels(case, 'uniform')
    mask, cm = OC.masks(case)
    runs = [OC.run(api, case, L, gt=gt, mask=mask, cm=cm, hist=torch.zeros(n, n, dtype=torch.int32)) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0], exp)


# ------------------------------------------------------------------------------------------------------------------ metric, device path
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'occ_metric_miou.npz')


@pytest.fixture(scope='module')
def rec():
    return np.load(GOLDEN)


def _frames(rec, dev):
    return [tuple(torch.from_numpy(rec[f'{k}_{i}']).to(dev) for k in ('pred', 'gt', 'mask_camera')) for i in range(3)]


def _logits_with_classes(pred, seed):
    """channels-last logits (1, 19, H, W, D) whose scored argmax (c0 = 1) is pred (X = W, Y = H, Z): 5 on the class, noise below 1"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.eye(19)[pred.cpu().long() + 1] * 5 + torch.rand((*pred.shape, 19), generator=g)       # (X, Y, Z, C)
    return rows.permute(1, 0, 2, 3).contiguous().to(pred.device).permute(3, 0, 1, 2)[None]


def _check(metric, rec, r):
    assert np.array_equal(metric.hist, rec[f'hist_{r}'].astype(np.float64))
    res = metric.count_miou()
    assert list(res.keys()) == [str(k) for k in rec[f'miou_keys_{r}']]
    for k, v in zip(rec[f'miou_keys_{r}'], rec[f'miou_values_{r}']):
        assert res[str(k)] == v or (np.isnan(res[str(k)]) and np.isnan(v)), k


@pytest.mark.parametrize('r', [0, 1, 2])
@pytest.mark.parametrize('form', ['ids', 'logits'])
def test_metric_device_path_reproduces_the_reference(api, rec, r, form):
    from fb_bev_amd.occ_metrics import Metric_mIoU
    min_d, max_d = rec['rings'][r]
    m = Metric_mIoU(num_classes=18, use_image_mask=True, min_d=min_d, max_d=max_d)
    for i, (pred, gt, cam) in enumerate(_frames(rec, api.device)):
        if form == 'ids':
            m.add_batch(pred, gt, None, cam)
        else:
            logits = _logits_with_classes(pred, i)
            assert logits.stride(1) == 1 and logits.shape == (1, 19, 200, 200, 2)
            got = m.add_logits(logits, gt, cam, c0=1)
            assert got.dtype == torch.uint8 and torch.equal(got[0], pred)
    assert m.cnt == 3 and m.device_hist.dtype == torch.int64
    _check(m, rec, r)


def test_metric_accumulates_in_int64(api, rec):
    """one bin carried past 2^31: the per-call int32 table is added into an int64 tensor"""
    from fb_bev_amd.occ_metrics import Metric_mIoU
    m = Metric_mIoU(num_classes=18, use_image_mask=True)
    pred, gt, cam = _frames(rec, api.device)[0]
    m.add_batch(pred, gt, None, cam)
    per_call = m.hist.copy()
    free = int(per_call[17, 17])
    assert free > 10000
    m.device_hist[17, 17] = 2 ** 31 - free - 5
    for _ in range(3):
        m.add_batch(pred, gt, None, cam)
    want = per_call * 4
    want[17, 17] = 2 ** 31 - free - 5 + 3 * free
    assert want[17, 17] > 2 ** 31 + free
    assert np.array_equal(m.hist, want)


# ------------------------------------------------------------------------------------------------------------------ detector
@pytest.mark.parametrize('mfma', [True, False])
def test_predict_occupancy_classes_equals_predict_occupancy(api, mfma, monkeypatch):
    import test_gpu_full_model as FM
    from fb_bev_amd import _capi
    from fb_bev_amd.occ_metrics import Metric_mIoU
    dev = api.device
    m = FM._small_model(dev, execution=dict(mfma_conv3d=mfma), neck_channels=64).eval()    # 64 -> 32 -> 16 channels in the head: multiples of 16
    img_inputs, metas, gt_occ, _ = FM._inputs(dev, 2)
    seen = []
    real = _capi.occ_classes
    monkeypatch.setattr(_capi, 'occ_classes', lambda logits, **kw: (seen.append(logits.stride()), real(logits, **kw))[1])
    with torch.no_grad():
        want = m.predict_occupancy(img_inputs, metas(True)).to(torch.uint8)
        m.reset_history()
        got = m.predict_occupancy_classes(img_inputs, metas(True))
        assert got.dtype == torch.uint8 and got.shape == (2, 40, 40, 16)
        assert torch.equal(got, want)
        # the route really ran, and what it hands the kernel: the MFMA head runner returns a channels-last view; the vendor library
        # returns class planes or channels-last memory, as it chooses
        assert (m._runners is not None and m._runners[0] is not None) if mfma else m._runners is None
        OC.observed(f'mfma_conv3d={mfma}: logits strides {seen[-1]}')
        assert len(seen) == 1 and (seen[-1][1] == 1 or not mfma), seen
        # scoring in the same launch leaves what scoring the returned ids leaves
        gt = torch.where(gt_occ == 255, gt_occ, gt_occ - 1).to(torch.uint8)   # the sliced classes 0..17, 255 unlabelled
        cam = torch.rand(gt.shape, device=dev) < 0.7
        fused = Metric_mIoU(num_classes=18, use_image_mask=True, grid_hw=(40, 40), voxel_size=2.0, min_d=5, max_d=35)
        after = Metric_mIoU(num_classes=18, use_image_mask=True, grid_hw=(40, 40), voxel_size=2.0, min_d=5, max_d=35)
        m.reset_history()
        again = m.predict_occupancy_classes(img_inputs, metas(True), gt_occupancy=gt, mask_camera=cam, metric=fused)
        assert torch.equal(again, want)
        after.add_batch(again, gt, None, cam)
    assert fused.hist.sum() > 1000 and np.array_equal(fused.hist, after.hist)
    want_hist = OC.hist_ref(18, want.cpu(), gt.cpu(), cam.cpu().to(torch.uint8),
                            torch.from_numpy(fused.column_mask.astype(np.uint8)))
    assert np.array_equal(fused.hist, want_hist.numpy().astype(np.float64))
