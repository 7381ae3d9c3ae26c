"""CPU-side checks of the occupancy F-score: the error codes of fbbev_occ_fscore_counts (each returned before any launch, so the
product library answers without a GPU), and the host path of occ_metrics.Metric_FScore against the record that
tests/golden/make_golden_occ_fscore.py took from the reference's own class (scikit-learn KD-trees).  Equalities only."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from fb_bev_amd import _capi
from fb_bev_amd import occ_metrics as OM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'occ_fscore.npz')


@pytest.fixture(scope='module')
def rec():
    return np.load(GOLDEN)


def _frames(rec):
    return [tuple(rec[f'{k}_{i}'] for k in ('pred', 'gt', 'mask_camera')) for i in range(int(rec['cnt']))]


def _metric(rec, r):
    t_acc, t_cmpl = rec['pairs'][r]
    return OM.Metric_FScore(threshold_acc=float(t_acc), threshold_complete=float(t_cmpl), use_image_mask=True)


# ------------------------------------------------------------------------------------------------------------------ C entry
def test_error_codes_come_before_any_launch():
    """the order stated in include/fbbev.h: null pointers and sizes (-1), B == 0 (0), the documented limits (-2)"""
    lib = _capi.declare(ctypes.CDLL(_capi.LIB_PATH))
    NULL, P = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)          # non-null dummy; never dereferenced on these paths
    bits = (ctypes.c_uint32 * 8)()
    V = ctypes.cast(bits, ctypes.c_void_p)
    base = dict(classes=P, gt=P, mask=P, void_bits=V, sq_x=P, sq_y=P, sq_z=P, offsets=P, n_off=7, R=2, T_acc=0.16, T_cmpl=0.16,
                B=1, X=200, Y=200, Z=16, counts=P, stream=NULL)

    def call(**over):
        return lib.fbbev_occ_fscore_counts(*dict(base, **over).values())

    for name in ('classes', 'gt', 'void_bits', 'sq_x', 'sq_y', 'sq_z', 'offsets', 'counts'):
        assert call(**{name: NULL}) == -1, name
    for name in ('X', 'Y', 'Z', 'n_off'):
        assert call(**{name: 0}) == -1, name
        assert call(**{name: -3}) == -1, name
    assert call(B=-1) == -1 and call(R=-1) == -1
    assert call(B=0) == 0                                           # no launch
    assert call(B=0, Z=33) == 0 and call(B=0, R=9) == 0             # ... and it comes before the limits
    assert call(B=0, Z=0) == -1 and call(B=0, counts=NULL) == -1    # ... and after the argument checks
    assert call(Z=33) == -2 and call(Z=32, mask=NULL, classes=NULL) == -1
    assert call(R=5) == -2
    assert call(B=1 << 15, X=1 << 8, Y=1 << 8, Z=1) == -2           # 2^31 voxels
    assert call(B=1, X=(1 << 30) + 1, Y=1, Z=1) == -2
    assert call(Z=33, counts=NULL) == -1                            # a null pointer wins over a limit


# ------------------------------------------------------------------------------------------------------------------ the class
def test_constructor_is_the_references(rec):
    sig = inspect.signature(OM.Metric_FScore.__init__)
    params = [p for p in sig.parameters.values() if p.name != 'self']
    assert [p.name for p in params] == [str(n) for n in rec['ctor_names']]
    assert [repr(p.default) for p in params] == [str(d) for d in rec['ctor_defaults']]
    m = OM.Metric_FScore()
    assert m.leaf_size == 10 and (m.cnt, m.tot_acc, m.tot_cmpl, m.tot_f1_mean, m.eps) == (0, 0., 0., 0., 1e-8)
    with pytest.raises(AssertionError):                             # use_image_mask=False: the reference asserts as well
        m.add_batch(np.zeros((2, 2, 2), np.uint8), np.zeros((2, 2, 2), np.uint8), None, np.ones((2, 2, 2), bool))


@pytest.mark.parametrize('form', ['3d', '1d', 'probabilities'])
@pytest.mark.parametrize('r', [0, 1, 2])
def test_host_path_reproduces_the_reference(rec, r, form):
    m = _metric(rec, r)
    frames = _frames(rec)
    before = [tuple(a.copy() for a in f) for f in frames]
    for i, (pred, gt, cam) in enumerate(frames):
        if form == '3d':
            m.add_batch(pred, gt, None, cam)
        elif form == '1d':
            m.add_batch(pred[cam], gt, None, cam)
        elif i == 0:                                                # (voxels, n): one-hot rows of the visible voxels
            m.add_batch(np.eye(18, dtype=np.uint8)[pred[cam]], gt, None, cam)
        elif i == 2:                                                # (X, Y, Z, n)
            m.add_batch(np.eye(18, dtype=np.uint8)[pred], gt, None, cam)
        else:
            m.add_batch(pred, gt, None, cam)
        assert (m.tot_acc, m.tot_cmpl, m.tot_f1_mean) == tuple(rec[f'totals_{r}'][i]), i
        assert m.cnt == i + 1
    assert np.array_equal(m.frame_counts()[:, :2], rec[f'sizes_{r}'])
    res = m.count_fscore()
    assert list(res.keys()) == ['f-score'] and res['f-score'] == rec[f'fscore_{r}']
    for was, now in zip(before, frames):                            # the reference writes 255 into its arguments; this does not
        assert all(np.array_equal(a, b) for a, b in zip(was, now))


def test_the_record_has_the_case_rounding_decides(rec):
    """frame 2 is the labels shifted one cell along x: at 0.4 some of the pairs are closer than the threshold and some are not"""
    m = _metric(rec, 0)
    pred, gt, cam = _frames(rec)[2]
    m.add_batch(pred, gt, None, cam)
    n_gt, n_pred, n_cmpl, n_acc = m.frame_counts()[0]
    same_cell = int(((pred != 17) & (gt != 17) & (gt != 255) & cam).sum())
    assert same_cell < n_acc < n_pred and same_cell < n_cmpl < n_gt


def test_empty_ground_truth_raises_and_names_the_frame(rec):
    m = _metric(rec, 0)
    pred, gt, cam = _frames(rec)[0]
    m.add_batch(pred, gt, None, cam)
    with pytest.raises(ValueError, match='frame 1'):
        m.add_batch(pred, np.full_like(gt, 17), None, cam)
    assert m.cnt == 1
    m.add_batch(np.full_like(pred, 17), np.full_like(gt, 17), None, cam)      # both empty: the reference's n_pred == 0 branch
    assert m.cnt == 2 and m.tot_f1_mean == rec['totals_0'][0][2]


@pytest.mark.parametrize('thr', [0.4, 0.6, 0.8, 1.2])
def test_threshold_constant_brackets_the_threshold(thr):
    T = OM.fscore_threshold_constant(thr)
    assert math.sqrt(T) < thr <= math.sqrt(math.nextafter(T, math.inf))


def test_tables_of_the_reference_grid():
    """the numbers DESIGN quotes: adjacent centres on both sides of 0.4, 7 and 19 offsets, R = 4 at 1.2"""
    t = OM.fscore_tables((200, 200, 16), [0.4] * 3, [-40, -40, -1, 40, 40, 5.4], 0.4, 0.4)
    x, z = t['sq'][0], t['sq'][2]
    assert t['R'] == 2 and x.shape == (200, 5) and np.isinf(x[0, :2]).all() and np.isinf(x[199, 3:]).all()
    assert int((x[:199, 3] <= t['T_acc']).sum()) == 130 and int((z[:15, 3] <= t['T_acc']).sum()) == 8
    assert len(t['offsets']) == 7
    assert len(OM.fscore_tables((200, 200, 16), [0.4] * 3, [-40, -40, -1, 40, 40, 5.4], 0.6, 0.6)['offsets']) == 19
    assert OM.fscore_radius((1.2, 1.2), [0.4] * 3) == 4 and OM.fscore_radius((0.4, 0.8), [0.4] * 3) == 3
