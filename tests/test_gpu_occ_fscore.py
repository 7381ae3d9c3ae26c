"""fbbev_occ_fscore_counts on the MI355X through fb_bev_amd._capi.occ_fscore_counts, at the shapes of tests/occ_fscore_cases.py (the
emulator test runs the same table): the four counts per frame against the definition written out in numpy, guard words, read-only
maps, run-to-run identical counts; the device path of occ_metrics.Metric_FScore against the record of the reference's class;
FBOCC.predict_occupancy_classes(fscore=...) against the host path on the class map it returns.  Equalities only."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_fscore_cases as FC  # noqa: E402

pytestmark = pytest.mark.gpu

BIG_CASE = FC.CASES[FC.CASE_IDS.index(FC.BIG)]
SMALL = [c for c in FC.CASES if c['name'] != FC.BIG]
PAIRS = [(c, p) for c in SMALL for p in FC.PATTERNS] + [(BIG_CASE, 'planted')]


@pytest.fixture(scope='module')
def api():
    assert torch.cuda.is_available()
    return FC.GpuApi()


@pytest.mark.parametrize('case,pattern', PAIRS, ids=[f'{c["name"]}-{p}' for c, p in PAIRS])
def test_counts_equal_the_definition(api, case, pattern):
    FC.check_counts(api, case, pattern)


@pytest.mark.parametrize('case', [SMALL[0], SMALL[2]], ids=[SMALL[0]['name'], SMALL[2]['name']])
def test_void_lists_and_null_mask(api, case):
    FC.check_voids_and_null_mask(api, case)


def test_one_cell_apart_is_decided_by_rounding(api):
    FC.check_rounding_decides(api, SMALL[2])


def test_depth_33_is_refused(api):
    from fb_bev_amd import _capi
    c = FC.REFUSED
    ids = api.dev(np.full((c['B'], c['X'], c['Y'], c['Z']), FC.FREE, dtype=np.uint8))
    tab = FC.tables(c, 0.4, 0.4, FC.VOXEL, full_cube=False)
    counts = api.dev(np.full((c['B'], 4), 5, dtype=np.int32))
    with pytest.raises(_capi.FbbevError, match=f'invalid argument {FC.E_UNSUPPORTED}'):
        _capi.occ_fscore_counts(ids, ids, None, FC.void_words([17, 255]), *[api.dev(t) for t in tab['sq']], api.dev(tab['offsets']),
                                tab['R'], tab['T_acc'], tab['T_cmpl'], counts=counts)
    assert (counts.cpu() == 5).all()


def test_two_runs_give_identical_counts(api):
    case = SMALL[2]
    pred, gt, mask, want = FC.reference(case, 'dense', 1, FC.VOIDS[0], True)
    runs = [FC.run(api, case, pred, gt, mask, FC.VOIDS[0], 1, full_cube=False) for _ in range(2)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], want)


# ------------------------------------------------------------------------------------------------------------------ metric, device path
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'occ_fscore.npz')


@pytest.fixture(scope='module')
def rec():
    return np.load(GOLDEN)


def _frames(rec, dev=None):
    out = [tuple(rec[f'{k}_{i}'] for k in ('pred', 'gt', 'mask_camera')) for i in range(int(rec['cnt']))]
    return out if dev is None else [tuple(torch.from_numpy(a).to(dev) for a in f) for f in out]


def _metric(rec, r):
    from fb_bev_amd.occ_metrics import Metric_FScore
    t_acc, t_cmpl = rec['pairs'][r]
    return Metric_FScore(threshold_acc=float(t_acc), threshold_complete=float(t_cmpl), use_image_mask=True)


def _check_final(m, rec, r):
    assert (m.tot_acc, m.tot_cmpl, m.tot_f1_mean) == tuple(rec[f'totals_{r}'][-1])
    assert m.cnt == int(rec['cnt'])
    res = m.count_fscore()
    assert list(res.keys()) == ['f-score'] and res['f-score'] == rec[f'fscore_{r}']


@pytest.mark.parametrize('r', [0, 1, 2])
def test_metric_device_path_frame_by_frame(api, rec, r):
    m = _metric(rec, r)
    for i, (pred, gt, cam) in enumerate(_frames(rec, api.device)):
        m.add_batch(pred, gt, None, cam)
        assert (m.tot_acc, m.tot_cmpl, m.tot_f1_mean) == tuple(rec[f'totals_{r}'][i])
    assert m.device_counts.dtype == torch.int64
    assert np.array_equal(m.frame_counts()[:, :2], rec[f'sizes_{r}'])
    _check_final(m, rec, r)


@pytest.mark.parametrize('r', [0, 1, 2])
def test_metric_device_path_one_batch(api, rec, r):
    m = _metric(rec, r)
    pred, gt, cam = (torch.stack(t) for t in zip(*_frames(rec, api.device)))
    m.add_batch(pred, gt, None, cam)
    assert np.array_equal(m.frame_counts()[:, :2], rec[f'sizes_{r}'])
    _check_final(m, rec, r)


def test_metric_mixed_paths_keep_arrival_order(api, rec):
    """frames 0 and 2 on the device, 1 and 3 on the host: the float64 totals are order dependent and must be the record's"""
    m = _metric(rec, 2)
    host, dev = _frames(rec), _frames(rec, api.device)
    for i in range(int(rec['cnt'])):
        pred, gt, cam = dev[i] if i % 2 == 0 else host[i]
        m.add_batch(pred, gt, None, cam)
    h = _metric(rec, 2)
    for pred, gt, cam in host:
        h.add_batch(pred, gt, None, cam)
    assert np.array_equal(m.frame_counts(), h.frame_counts())
    _check_final(m, rec, 2)


def test_metric_device_path_empty_ground_truth_raises_when_read(api, rec):
    m = _metric(rec, 0)
    pred, gt, cam = _frames(rec, api.device)[0]
    m.add_batch(pred, gt, None, cam)
    m.add_batch(pred, torch.full_like(gt, 17), None, cam)             # accepted: nothing is read yet
    with pytest.raises(ValueError, match='frame 1'):
        m.tot_f1_mean


# ------------------------------------------------------------------------------------------------------------------ detector
def test_predict_occupancy_classes_scores_the_fscore(api):
    import test_gpu_full_model as FM
    from fb_bev_amd.occ_metrics import Metric_FScore, Metric_mIoU
    dev = api.device
    m = FM._small_model(dev, execution=dict(mfma_conv3d=True), neck_channels=64).eval()
    img_inputs, metas, gt_occ, _ = FM._inputs(dev, 2)
    new = lambda: Metric_FScore(threshold_acc=0.4, threshold_complete=0.6, use_image_mask=True)  # noqa: E731  (0.4 m cells)
    miou = lambda: Metric_mIoU(num_classes=18, use_image_mask=True, grid_hw=(40, 40), voxel_size=2.0, min_d=5, max_d=35)  # noqa: E731
    with torch.no_grad():
        plain = m.predict_occupancy_classes(img_inputs, metas(True))
        gt = torch.where(gt_occ == 255, gt_occ, gt_occ - 1).to(torch.uint8)
        cam = torch.rand(gt.shape, device=dev) < 0.7
        m.reset_history()
        alone = new()
        got = m.predict_occupancy_classes(img_inputs, metas(True), gt_occupancy=gt, mask_camera=cam, fscore=alone)
        assert got.dtype == torch.uint8 and torch.equal(got, plain)
        m.reset_history()
        both, with_f, without_f = new(), miou(), miou()
        again = m.predict_occupancy_classes(img_inputs, metas(True), gt_occupancy=gt, mask_camera=cam, metric=with_f, fscore=both)
        m.reset_history()
        m.predict_occupancy_classes(img_inputs, metas(True), gt_occupancy=gt, mask_camera=cam, metric=without_f)
    assert torch.equal(again, plain)
    assert with_f.hist.sum() > 1000 and np.array_equal(with_f.hist, without_f.hist)
    host = new()
    for b in range(got.shape[0]):
        host.add_batch(got[b].cpu().numpy(), gt[b].cpu().numpy(), None, cam[b].cpu().numpy())
    FC.observed(f'counts per frame {alone.frame_counts().tolist()}')
    assert alone.cnt == both.cnt == host.cnt == 2
    assert np.array_equal(alone.frame_counts(), host.frame_counts()) and np.array_equal(both.frame_counts(), host.frame_counts())
    assert alone.frame_counts()[:, :2].min() > 0
    assert (alone.tot_acc, alone.tot_cmpl, alone.tot_f1_mean) == (host.tot_acc, host.tot_cmpl, host.tot_f1_mean)
