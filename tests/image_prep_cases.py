"""Case table, sources, references and checks for fbbev_image_prep (fb_bev_amd/csrc/image_prep_kernels.h), shared by the host test
(tests/test_image_prep_host.py: the numpy restatement against the fixture and against live PIL), the emulator test
(tests/test_emu_image_prep.py, through tests/emu/emu_capi.py's library) and the GPU test (tests/test_gpu_image_prep.py).

Every comparison is equality of bits; there is no tolerance anywhere.
  expected canvas (n, fH, fW, 3) uint8   fb_bev_amd.image_prep.transform_reference, the numpy restatement of PIL's resize / crop /
                                         transpose / rotate (pinned to PIL by the fixture and, where PIL is installed, live)
  expected floats                        (float32(v) - mean) * inv_std of that canvas in numpy float32, after the channel swap
Memory: `out` and `canvas` sit between guard bands of a pattern that must survive; frames and plan must come back unchanged; two
runs give the same bits.

A case is one launch: a source kind, (Hs, Ws), (fH, fW) and per image (resize, crop_x0, crop_y0, flip, rotate).  T = the kernel's
tile (fb_bev_amd.image_prep.limits(), the numbers fbbev_image_prep_limits exports).  Plain Python, numpy and CPU torch only; the
adapters import their library on first use.
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fb_bev_amd import image_prep as IP  # noqa: E402

GUARD = 64                        # floats in front of and behind `out`; bytes around `canvas`
PATTERN = 7.5
PATTERN_U8 = 0xA5
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'image_prep_ref.npz')
TW, TH = IP.LIMITS['tile_w'], IP.LIMITS['tile_h']


def observed(text):
    print(f'[observed] {text}')


# ------------------------------------------------------------------------------------------------------------------ sources
_SRC = {}


def source(kind, Hs, Ws):
    """(Hs, Ws, 3) uint8.  noise: random bytes; edges: 0 / 255 step edges over a checkerboard at periods 1, 2 and 3 (bicubic
    overshoot leaves [0, 255] in both passes)"""
    key = (kind, Hs, Ws)
    if key not in _SRC:
        if kind == 'noise':
            a = np.random.default_rng(Hs * 10007 + Ws).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
        elif kind == 'edges':
            y, x = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing='ij')
            a = np.zeros((Hs, Ws, 3), np.uint8)
            for c, period in enumerate((1, 2, 3)):
                a[..., c] = np.where(((x // period) + (y // period)) % 2 == 0, 255, 0)
            a[:, Ws // 2:Ws // 2 + Ws // 8] = 255                    # a white bar and a black bar: step edges
            a[:, Ws // 4:Ws // 4 + Ws // 8] = 0
            a[Hs // 2:Hs // 2 + Hs // 6] = 255 - a[Hs // 2:Hs // 2 + Hs // 6]
        else:
            raise KeyError(kind)
        a.setflags(write=False)
        _SRC[key] = a
    return _SRC[key]


# ------------------------------------------------------------------------------------------------------------------ cases
def _aug(Hs, Ws, fH, fW, resize, cx, cy, flip, rot):
    return (resize, (int(Ws * resize), int(Hs * resize)), (cx, cy, cx + fW, cy + fH), flip, rot)


def _case(name, Hs, Ws, fH, fW, images, kind='noise', pad=0, big=False, fixture=False):
    return dict(name=name, Hs=Hs, Ws=Ws, fH=fH, fW=fW, augs=[_aug(Hs, Ws, fH, fW, *im) for im in images], kind=kind, pad=pad, big=big,
                fixture=fixture)


_SEVEN = [(0.44, 0, 14, False, 0), (0.53, 9, 17, True, 5.4), (0.38, 0, 6, True, -5.4), (0.4175, 3, -2, False, 1.234567),
          (1.3, 40, 60, False, 360.0), (1.0, 50, 30, True, 10.0), (0.47, 2, 10, True, -10.0)]
_TRAIN6 = [(0.53, 100, 200, True, 5.4), (0.38, 0, 60, True, -5.4), (0.4175, 3, 100, False, 1.234567), (0.55, 170, 230, False, -3.3),
           (0.49, 40, 170, True, 0.05), (0.44, 0, 140, False, 4.0)]

CASES = [_case(f'size_{fW}x{fH}', 90, 160, fH, fW, [(0.85, 5, 7, (fW + fH) % 2 == 1, 2.0)])
         for fW, fH in ((1, 1), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH), (TW, TH + 1), (TW + 1, TH + 1), (2 * TW + 3, 2 * TH + 3),
                        (1, 2 * TH + 3), (2 * TW + 3, 1))]
CASES += [
    _case('mini_test_pipeline', 90, 160, 25, 70, [(0.44, 0, 14, False, 0)], fixture=True),
    _case('full_test_pipeline', 900, 1600, 256, 704, [(0.44, 0, 140, False, 0)], big=True),
    _case('crop_past_right_bottom', 90, 160, 25, 70, [(0.38, 0, 14, False, 0)], fixture=True),      # resized 60 x 34: 10 columns, 5 rows of padding
    _case('crop_negative_y0', 90, 160, 25, 70, [(0.47, 2, -6, False, 0)], fixture=True),
    _case('flip', 90, 160, 25, 70, [(0.47, 2, 10, True, 0)], fixture=True),
    _case('rot_plus', 90, 160, 25, 70, [(0.47, 2, 10, False, 5.4)], fixture=True),
    _case('rot_minus', 90, 160, 25, 70, [(0.47, 2, 10, False, -5.4)], fixture=True),
    _case('flip_rot_plus10', 90, 160, 25, 70, [(0.47, 2, 10, True, 10.0)], fixture=True),
    _case('flip_rot_minus10', 90, 160, 25, 70, [(0.47, 2, 10, True, -10.0)], fixture=True),
    _case('rot_360', 90, 160, 25, 70, [(0.47, 2, 10, False, 360.0)], fixture=True),
    _case('upscale', 90, 160, 40, 100, [(1.3, 20, 30, False, 3.0)], fixture=True),
    _case('resize_one', 90, 160, 40, 100, [(1.0, 20, 30, False, 0)], fixture=True),
    _case('saturation_down', 90, 160, 30, 80, [(0.6, 4, 6, False, 0)], kind='edges', fixture=True),
    _case('saturation_up', 90, 160, 40, 100, [(1.3, 20, 30, True, -4.0)], kind='edges', fixture=True),
    _case('narrow_source', 7, 5, 3, 2, [(0.5, 0, 0, False, 0)], fixture=True),
    _case('quarter_rot10', 90, 160, 20, 40, [(0.25, 0, 0, False, -10.0)]),
    _case('double_rot10', 90, 160, 100, 130, [(2.0, 100, 50, True, 10.0)]),
    _case('batch7_strided', 90, 160, 25, 70, _SEVEN, pad=52, fixture=True),
    _case('full_train6', 900, 1600, 256, 704, _TRAIN6, big=True),
]
CASE_IDS = [c['name'] for c in CASES]
SMALL = [c for c in CASES if not c['big']]
SMALL_IDS = [c['name'] for c in SMALL]
BIG = [c for c in CASES if c['big']]
BIG_IDS = [c['name'] for c in BIG]
FIXTURE_CASES = [c for c in CASES if c['fixture']]
SATURATION = ('saturation_down', 'saturation_up')
# (channels_last, swap, canvas): every case runs the first; the others on VARIANT_CASES
VARIANTS = [(False, True, True), (True, True, True), (False, False, False), (True, False, False), (True, True, False)]
VARIANT_CASES = ('size_%dx%d' % (TW + 1, TH + 1), 'batch7_strided', 'flip_rot_plus10')


def by_name(name):
    return CASES[CASE_IDS.index(name)]


def frames_of(case):
    """(n, Hs, Ws, 3) uint8: image i is the case's source rolled by 3 i rows and 5 i columns"""
    src = source(case['kind'], case['Hs'], case['Ws'])
    return np.stack([np.roll(src, (3 * i, 5 * i), (0, 1)) for i in range(len(case['augs']))])


_WANT = {}


def expected(case):
    """-> (canvas (n, fH, fW, 3) uint8, stats of the unclamped sums); computed once"""
    if case['name'] not in _WANT:
        stats = {}
        fr = frames_of(case)
        cv = np.stack([IP.transform_reference(fr[i], a, stats=stats) for i, a in enumerate(case['augs'])])
        assert cv.shape == (len(case['augs']), case['fH'], case['fW'], 3)
        cv.setflags(write=False)
        _WANT[case['name']] = (cv, stats)
    return _WANT[case['name']]


def expected_floats(canvas, swap, channels_last):
    """(n, 3, fH, fW) float32 in numpy float32 arithmetic; channels-last: the (n, fH, fW, 3) memory image"""
    mean, inv = IP.norm_constants()
    v = canvas[..., ::-1] if swap else canvas
    hwc = (v.astype(np.float32) - mean) * inv
    assert hwc.dtype == np.float32
    return np.ascontiguousarray(hwc if channels_last else np.moveaxis(hwc, -1, 1))


def case_asserts(case):
    """the property a case exists for, on the restatement's answer"""
    cv, stats = expected(case)
    name = case['name']
    if name in SATURATION:
        assert stats['lo'] < 0 and stats['hi'] > 255, f'{name}: the unclamped sums stay in [0, 255] ({stats}): the case proves nothing'
        assert (cv == 0).any() and (cv == 255).any()
    if name == 'crop_past_right_bottom':
        assert not cv[0, :, 60:].any() and not cv[0, 20:].any() and cv[0, :20, :60].any()
    if name == 'crop_negative_y0':
        assert not cv[0, :6].any() and cv[0, 6:].any()
    if name == 'resize_one':
        assert np.array_equal(cv[0], frames_of(case)[0, 30:70, 20:120])
    if name == 'rot_360':
        assert np.array_equal(cv[0], IP.transform_reference(frames_of(case)[0], _aug(90, 160, 25, 70, 0.47, 2, 10, False, 0)))
    if name == 'narrow_source':
        hx, hn, _ = IP.resample_table(5, 2, 0, 2)
        assert hx[0] == 0 and hx[1] + hn[1] == 5 and hn.max() < 2 * 4 + 1        # the windows clip at both ends of the source


# ------------------------------------------------------------------------------------------------------------------ adapters
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class EmuApi:
    """the C entry of the CPU-emulated library, CPU tensors"""
    name = 'emu'

    def __init__(self):
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
        import emu_capi
        self.lib = emu_capi.lib()

    def dev(self, t):
        return t.clone()

    def cpu(self, t):
        return t

    def stream(self):
        return None


class GpuApi:
    """the C entry of the product library on cuda:0, device tensors"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi
        self.lib = _capi.lib()
        self.device = torch.device('cuda:0')

    def dev(self, t):
        return t.to(self.device)

    def cpu(self, t):
        return t.cpu()

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def limits_of(api):
    vals = [ctypes.c_int(0) for _ in range(7)]
    assert api.lib.fbbev_image_prep_limits(*[ctypes.cast(ctypes.pointer(v), ctypes.c_void_p) for v in vals]) == 0
    return dict(zip(('tile_w', 'tile_h', 'max_taps', 'max_box_w', 'max_box_h', 'max_src_rows', 'max_src_cols'), (v.value for v in vals)))


def run(api, case, channels_last=False, swap=True, canvas=True):
    """one launch -> (out as its memory image: (n, 3, fH, fW) or (n, fH, fW, 3) float32 numpy, canvas (n, fH, fW, 3) uint8 or None)"""
    fr = frames_of(case)
    n, Hs, Ws, fH, fW = fr.shape[0], case['Hs'], case['Ws'], case['fH'], case['fW']
    stride = Hs * Ws * 3 + case['pad']
    store = torch.full((n * stride + 4,), PATTERN_U8, dtype=torch.uint8)
    for i in range(n):
        store[i * stride:i * stride + Hs * Ws * 3] = torch.from_numpy(fr[i].reshape(-1).copy())
    plan, need = IP.build_plan(case['augs'], Hs, Ws, fH, fW)
    plan = plan.clone()
    d_store, d_plan = api.dev(store), api.dev(plan)
    assert d_store.data_ptr() % 16 == 0
    count = n * 3 * fH * fW
    buf = api.dev(torch.full((GUARD + count + GUARD,), PATTERN))
    assert buf.data_ptr() % 16 == 0
    cbuf = api.dev(torch.full((GUARD + count + GUARD,), PATTERN_U8, dtype=torch.uint8)) if canvas else None
    mean, inv = IP.norm_constants()
    m3, s3 = (ctypes.c_float * 3)(*mean.tolist()), (ctypes.c_float * 3)(*inv.tolist())
    hn = (ctypes.c_int * 5)(*need)
    flags = (1 if swap else 0) | (2 if channels_last else 0)
    code = api.lib.fbbev_image_prep(_p(d_store), stride, n, Hs, Ws, fH, fW, _p(d_plan), ctypes.cast(hn, ctypes.c_void_p),
                                    ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), flags,
                                    ctypes.c_void_p(buf.data_ptr() + 4 * GUARD),
                                    None if cbuf is None else ctypes.c_void_p(cbuf.data_ptr() + GUARD), api.stream())
    assert code == 0, f'fbbev_image_prep returned {code}'
    buf = api.cpu(buf)
    assert (buf[:GUARD] == PATTERN).all() and (buf[GUARD + count:] == PATTERN).all(), 'guard words of out overwritten'
    assert torch.equal(api.cpu(d_store), store), 'frames were written to'
    assert torch.equal(api.cpu(d_plan), plan), 'the plan was written to'
    out = buf[GUARD:GUARD + count].numpy().reshape((n, fH, fW, 3) if channels_last else (n, 3, fH, fW)).copy()
    cv = None
    if canvas:
        cbuf = api.cpu(cbuf)
        assert (cbuf[:GUARD] == PATTERN_U8).all() and (cbuf[GUARD + count:] == PATTERN_U8).all(), 'guard bytes of canvas overwritten'
        cv = cbuf[GUARD:GUARD + count].numpy().reshape(n, fH, fW, 3).copy()
    return out, cv


# ------------------------------------------------------------------------------------------------------------------ checks
def check(api, case, channels_last=False, swap=True, canvas=True):
    case_asserts(case)
    want, _ = expected(case)
    out, cv = run(api, case, channels_last, swap, canvas)
    if canvas:
        bad = int((cv != want).sum())
        observed(f'{api.name} {case["name"]}: {want.size} canvas bytes, {bad} differ')
        assert np.array_equal(cv, want)
    wf = expected_floats(want, swap, channels_last)
    bad = int((out.view(np.int32) != wf.view(np.int32)).sum())
    observed(f'{api.name} {case["name"]} cl={channels_last} swap={swap}: {wf.size} floats, {bad} differ')
    assert np.array_equal(out.view(np.int32), wf.view(np.int32))
    return out, cv


def check_repeat(api, case):
    a, b = (run(api, case) for _ in range(2))
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


def fixture():
    return np.load(FIXTURE)


def check_fixture_inputs(z):
    """the fixture was made from today's sources and parameters"""
    for case in FIXTURE_CASES:
        name = case['name']
        src = z[f'source.{case["kind"]}.{case["Hs"]}x{case["Ws"]}']
        assert np.array_equal(src, source(case['kind'], case['Hs'], case['Ws'])), f'{name}: the fixture is stale: regenerate it'
        assert np.array_equal(z[f'{name}.augs'], augs_array(case['augs'])), f'{name}: the fixture is stale: regenerate it'


def augs_array(augs):
    """(n, 9) float64: resize, newW, newH, crop x0 y0 x1 y1, flip, rotate"""
    return np.array([[a[0], *a[1], *a[2], float(a[3]), float(a[4])] for a in augs], np.float64)


def check_fixture(api):
    """the kernel's canvas against the bytes the reference class made with PIL"""
    z = fixture()
    check_fixture_inputs(z)
    for case in FIXTURE_CASES:
        _, cv = run(api, case)
        assert np.array_equal(cv, z[f'{case["name"]}.canvas']), case['name']


# ------------------------------------------------------------------------------------------------------------------ the pipeline step
CAM_NAMES = ['CAM_FRONT_LEFT', 'CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_LEFT', 'CAM_BACK', 'CAM_BACK_RIGHT']
# occupancy_configs/fb_occ's data_config in miniature: 90 x 160 frames, a 25 x 70 input
DATA_CONFIG = dict(cams=CAM_NAMES, Ncams=5, input_size=(25, 70), src_size=(90, 160), resize=(-0.06, 0.11), rot=(-5.4, 5.4), flip=True,
                   crop_h=(0.0, 0.0), resize_test=0.00)
AUG_SEEDS = (0, 1, 2, 3)
GET_INPUTS_SEED = 11
Q_CYCLE = (0.5, 0.5, 0.5, 0.5)           # 120 degrees about (1, 1, 1)
Q_FLIP_Y = (0.0, 0.0, 1.0, 0.0)          # 180 degrees about y
Q_BOTH = (-0.5, -0.5, 0.5, 0.5)          # their product: every rotation matrix below has entries 0 and +-1


def info_dict():
    """a sample info dict whose quaternions are dyadic units and whose translations are small dyadic numbers: every matrix of the
    sensor chains, every product and every inverse is exact in fp32, whatever formula makes the rotation matrix"""
    cams = {}
    for k, name in enumerate(CAM_NAMES):
        cams[name] = dict(data_path=name, cam_intrinsic=[[1266.5 + k, 0.0, 816.25], [0.0, 1266.5 + k, 491.5], [0.0, 0.0, 1.0]],
                          sensor2ego_rotation=list((Q_CYCLE, Q_FLIP_Y, Q_BOTH)[k % 3]), sensor2ego_translation=[1.5 - 0.25 * k, 0.5 * k, 1.25],
                          ego2global_rotation=list((Q_BOTH, Q_CYCLE, Q_FLIP_Y)[k % 3]), ego2global_translation=[8.0 + k, -4.0, 0.5 * k])
    return dict(cams=cams)


def pipeline_frames():
    """{camera: (90, 160, 3) uint8}"""
    src = source('noise', 90, 160)
    return {name: np.roll(src, (7 * k, 11 * k), (0, 1)) for k, name in enumerate(CAM_NAMES)}
