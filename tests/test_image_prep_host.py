"""fb_bev_amd.image_prep on the host: the numpy restatement of PIL's resize / crop / transpose / rotate against the fixture the
reference class wrote (tests/golden/image_prep_ref.npz) and, where PIL is installed, against PIL itself; sample_augmentation,
post_transform and PrepareImageInputs.get_inputs against the fixture; build_plan's validator."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_prep_cases as C  # noqa: E402
from fb_bev_amd import image_prep as IP  # noqa: E402


def test_fixture_is_current():
    z = C.fixture()
    C.check_fixture_inputs(z)
    assert str(z['pil_version'])


@pytest.mark.parametrize('case', C.FIXTURE_CASES, ids=[c['name'] for c in C.FIXTURE_CASES])
def test_restatement_equals_the_fixture(case):
    C.case_asserts(case)
    assert np.array_equal(C.expected(case)[0], C.fixture()[f'{case["name"]}.canvas'])


@pytest.mark.parametrize('case', C.CASES, ids=C.CASE_IDS)
def test_restatement_equals_live_pil(case):
    Image = pytest.importorskip('PIL.Image')
    fr = C.frames_of(case)
    want = C.expected(case)[0]
    for i, (resize, dims, crop, flip, rotate) in enumerate(case['augs']):
        img = Image.fromarray(fr[i]).resize(dims).crop(crop)
        if flip:
            img = img.transpose(method=Image.FLIP_LEFT_RIGHT)
        assert np.array_equal(np.array(img.rotate(rotate)), want[i]), (case['name'], i)


def test_module_does_not_import_pil():
    import subprocess
    code = 'import sys; import fb_bev_amd.image_prep; assert not any(m == "PIL" or m.startswith("PIL.") for m in sys.modules)'
    subprocess.check_call([sys.executable, '-c', code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.mark.parametrize('is_train', [True, False])
def test_sample_augmentation_draws_as_the_reference(is_train):
    want = C.fixture()['aug.train' if is_train else 'aug.test']
    for row, seed in zip(want, C.AUG_SEEDS):
        np.random.seed(seed)
        got = IP.sample_augmentation(C.DATA_CONFIG, 90, 160, is_train)
        assert np.array_equal(C.augs_array([got])[0], row), seed
    if not is_train:
        assert IP.sample_augmentation(C.DATA_CONFIG, 90, 160, False, flip=True, scale=0.5) == (0.5, (80, 45), (5, 20, 75, 45), True, 0)


def _exact_chains(names):
    """rots, trans, sensor2sensors of info_dict() in float64 (its quaternions and translations are dyadic: exact)"""
    info = C.info_dict()['cams']

    def rigid(q, t):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = IP.quaternion_rotation_matrix(q), t
        return m
    s2k = []
    for n in names:
        cam, ego = info[n], info['CAM_FRONT']
        s2k.append(np.linalg.inv(rigid(ego['ego2global_rotation'], ego['ego2global_translation'])) @
                   rigid(cam['ego2global_rotation'], cam['ego2global_translation']) @
                   rigid(cam['sensor2ego_rotation'], cam['sensor2ego_translation']))
    s2k = np.stack(s2k)
    assert (s2k == np.round(s2k * 8) / 8).all()                                   # multiples of 1 / 8: nothing was rounded
    return dict(rots=s2k[:, :3, :3], trans=s2k[:, :3, 3], sensor2sensors=np.tile(np.eye(4), (len(names), 1, 1)))


def check_get_inputs(place):
    """PrepareImageInputs.get_inputs on info_dict() against what the reference class returned; place: array -> the frame handed over"""
    z = C.fixture()
    step = IP.build_pipeline_step(dict(type='PrepareImageInputs', data_config=C.DATA_CONFIG, is_train=True))
    assert isinstance(step, IP.PrepareImageInputs)
    np.random.seed(C.GET_INPUTS_SEED)
    results = dict(curr=C.info_dict(), frames={k: place(v) for k, v in C.pipeline_frames().items()})
    (imgs, rots, trans, intrins, post_rots, post_trans), (sensor2egos, ego2globals) = step.get_inputs(results)
    names = [str(n) for n in results['cam_names']]
    exact = _exact_chains(names)
    assert names == [str(n) for n in z['get_inputs.cam_names']]
    assert np.array_equal(C.augs_array([results['img_augs'][n] for n in names]), z['get_inputs.augs'])
    assert np.array_equal(np.stack(results['canvas']), z['get_inputs.canvas'])
    for key, t in (('imgs', imgs), ('rots', rots), ('trans', trans), ('intrins', intrins), ('post_rots', post_rots),
                   ('post_trans', post_trans), ('sensor2egos', sensor2egos), ('ego2globals', ego2globals),
                   ('sensor2sensors', results['sensor2sensors'])):
        want = z[f'get_inputs.{key}']
        assert t.dtype == torch.float32 and tuple(t.shape) == want.shape, key
        got = t.cpu().numpy()
        if key == 'imgs':
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), key                     # the images bit for bit
        elif key in exact:
            # through torch's .inverse(): an LU whose last bit belongs to the host's LAPACK build (the fixture itself is 2^-23 off the
            # exact identity in sensor2sensors).  The info dict is dyadic, so float64 gives THE answer; the fixture and ours are both
            # held to it within 4 roundings of fp32 at the matrix's largest entry (a 4 x 4 LU: no entry passes more)
            bound = 4 * 2.0 ** -24 * np.abs(exact[key]).max()
            assert np.abs(want - exact[key]).max() <= bound and np.abs(got - exact[key]).max() <= bound, key
        else:
            assert np.array_equal(got, want), key                                                   # no inverse: value for value
    again = step(dict(curr=C.info_dict(), frames={k: place(v) for k, v in C.pipeline_frames().items()}))
    assert len(again['img_inputs']) == 6 and len(again['aux_cam_params']) == 2


def test_get_inputs_on_host_frames_equals_the_fixture():
    check_get_inputs(lambda a: a)
    check_get_inputs(lambda a: torch.from_numpy(np.ascontiguousarray(a)))


def test_sequential_is_not_implemented():
    with pytest.raises(NotImplementedError):
        IP.PrepareImageInputs(C.DATA_CONFIG, sequential=True)
    with pytest.raises(KeyError):
        IP.build_pipeline_step(dict(type='LoadOccupancy'))


def test_post_transform_matches_the_fixture_rows():
    z = C.fixture()
    for a, rot, tran in zip(z['get_inputs.augs'], z['get_inputs.post_rots'], z['get_inputs.post_trans']):
        r, t = IP.post_transform(float(a[0]), tuple(int(v) for v in a[3:7]), bool(a[7]), float(a[8]))
        assert np.array_equal(r.numpy().view(np.int32), rot.view(np.int32)) and np.array_equal(t.numpy().view(np.int32), tran.view(np.int32))


def test_tables():
    xmin, n, taps = IP.resample_table(160, 160, 0, 160)                     # resize 1.0: the identity
    assert (n > 0).all() and all(taps[i, i - xmin[i]] == 1 << 22 and np.count_nonzero(taps[i]) == 1 for i in range(160))
    xmin, n, taps = IP.resample_table(160, 60, -3, 70)                      # three outputs in front of, seven behind the resized image
    assert not n[:3].any() and not n[63:].any() and (n[3:63] > 0).all() and not taps[:3].any() and not taps[63:].any()
    assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all() and xmin[0] == xmin[3] and xmin[-1] == 160
    assert (taps.sum(1)[3:63] - (1 << 22)).__abs__().max() <= 16             # normalised coefficients, each rounded to 2^-22
    assert IP.resample_table(160, 60, -3, 70)[2] is taps                     # cached
    with pytest.raises(ValueError):
        taps[0, 0] = 1                                                       # and read-only
    assert IP.rotate_fixed(70, 25, 0) == IP.rotate_fixed(70, 25, 360.0) == IP.rotate_fixed(70, 25, -720) == (65536, 0, 32768, 0, 65536, 32768)
    a = IP.rotate_fixed(70, 25, 180)
    assert [(a[2] + x * a[0]) >> 16 for x in (0, 69)] == [69, 0] and [(a[5] + y * a[4]) >> 16 for y in (0, 24)] == [24, 0]
    with pytest.raises(ValueError):
        IP.rotate_fixed(25, 25, 90)


def test_build_plan_validates():
    ok = C._aug(90, 160, 25, 70, 0.47, 2, 10, True, 5.4)
    plan, need = IP.build_plan([ok, ok, C._aug(90, 160, 25, 70, 0.47, 2, 10, False, 0)], 90, 160, 25, 70)
    assert plan.dtype == torch.int32 and plan.dim() == 1 and not plan.is_cuda and len(need) == 5
    rec = plan[:3 * IP.PLAN_REC].view(3, IP.PLAN_REC)
    assert rec[0, 10] == rec[1, 10] == rec[2, 10] and rec[0, 11] == rec[2, 11]          # one table for all three
    assert rec[0, 2] == 1 and rec[2, 2] == 0 and tuple(rec[2, 4:10].tolist()) == (65536, 0, 32768, 0, 65536, 32768)
    L = IP.limits()
    assert need[0] <= L['max_taps'] and need[1] <= L['max_box_w'] and need[2] <= L['max_box_h']
    for Hs, Ws, fH, fW, bad in ((900, 1600, 256, 704, C._aug(900, 1600, 256, 704, 0.47, 2, 10, False, 45.0)),   # a tile's box at 45 degrees
                                (900, 1600, 25, 70, C._aug(900, 1600, 25, 70, 0.1, 0, 0, False, 0)),            # 21 taps and more
                                (90, 160, 25, 70, (0.47, (75, 42), (2, 10, 71, 35), False, 0)),                 # a crop that is not fW x fH
                                (90, 160, 25, 70, (0.0, (0, 0), (0, 0, 70, 25), False, 0))):                    # an empty resized image
        with pytest.raises(ValueError):
            IP.build_plan([bad], Hs, Ws, fH, fW)
    for resize in (0.25, 0.38, 0.55, 1.0, 2.0):                                # the route the header promises
        for rot in (-10.0, 0.0, 10.0):
            IP.build_plan([C._aug(900, 1600, 256, 704, resize, 0, 0, rot < 0, rot)], 900, 1600, 256, 704)
