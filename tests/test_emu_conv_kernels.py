"""The case tables of tests/conv_cases.py on the CPU emulator build of the kernels: proves without a GPU that the float64 references
and the derived bounds hold for a correct implementation (and are not vacuous: the observed err / bound figures are printed).
tests/test_gpu_conv_kernels.py runs the same tables on the MI355X.  Also here, because it needs no GPU: the table's exactness premise
and the bias-length guard of the four forward wrappers of fb_bev_amd._capi.

Two cases are shrunk here and only here, because the emulator runs every lane as a fiber (the weight gradient took 29 s per call at
full size, six calls; the tiled case 55 s in its two tests):
  * tiled (3, (5, 9, 9), 32, 128): two samples instead of three -- 16 tiles of 1-thick partial edges in two groups of 8, gy = 2;
  * wgrad (2, (12, 10, 6), 20, 80, k 3): the same Cin tail (20 of 64), second cout block with 16 live couts and 27 taps on
    (2, (13, 4, 4)) -- 416 voxels, a full chunk of 256 that crosses the sample boundary at 208 and a short last chunk of 160.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as T  # noqa: E402

# the emulator-only shapes (see the docstring)
WGRAD = dict(T.WGRAD_CASES)
WGRAD['b2_12x10x6_i20_o80_k3'] = T._wg(2, (13, 4, 4), 20, 80, 3, 1, 1, 256, 2)
TILED = dict(T.TILED_CASES)
TILED['b3_5x9x9_i32_o128_res'] = T._cv(2, (5, 9, 9), 32, 128, relu=False, res=True)
F32_KINDS = [('f32', n, c) for n, c in T.FORWARD_CASES.items()] + [('2d', n, c) for n, c in T.FORWARD_2D_CASES.items()] + \
    [('transposed', n, c) for n, c in T.TRANSPOSED_CASES.items()]
BF16_KINDS = [('bf16', n, c) for n, c in T.BF16_CASES.items()] + [('tiled', n, c) for n, c in TILED.items()] + \
    [('transposed_bf16', n, c) for n, c in T.TRANSPOSED_CASES.items()]
_ids = lambda rows: [f'{k}-{n}' for k, n, _ in rows]  # noqa: E731


@pytest.fixture(scope='module')
def api():
    return T.EmuApi()


@pytest.mark.parametrize('kind,name,case', F32_KINDS + BF16_KINDS, ids=_ids(F32_KINDS + BF16_KINDS))
def test_conv_integer_operands_equal_float64_emulated(api, kind, name, case):
    T.check_conv_exact(api, kind, name, case)


@pytest.mark.parametrize('kind,name,case', F32_KINDS, ids=_ids(F32_KINDS))
def test_conv_f32_real_operands_inside_the_derived_bound_emulated(api, kind, name, case):
    T.check_conv_real_f32(api, kind, name, case)


@pytest.mark.parametrize('kind,name,case', BF16_KINDS, ids=_ids(BF16_KINDS))
def test_conv_bf16_real_operands_inside_the_derived_bound_emulated(api, kind, name, case):
    T.check_conv_real_bf16(api, kind, name, case)


@pytest.mark.parametrize('name', list(T.DGRAD_CASES))
def test_dgrad_integer_operands_equal_float64_emulated(api, name):
    T.check_dgrad_exact(api, name, T.DGRAD_CASES[name])


@pytest.mark.parametrize('name', list(T.DGRAD_CASES))
def test_dgrad_real_operands_inside_the_derived_bound_emulated(api, name):
    T.check_dgrad_real(api, name, T.DGRAD_CASES[name])


@pytest.mark.parametrize('name', list(WGRAD))
def test_wgrad_integer_operands_equal_float64_on_both_routes_emulated(api, name):
    T.check_wgrad_plan(api, WGRAD[name])
    T.check_wgrad_exact(api, name, WGRAD[name])


@pytest.mark.parametrize('name', list(WGRAD))
def test_wgrad_real_operands_inside_the_derived_bound_and_bit_stable_emulated(api, name):
    T.check_wgrad_plan(api, WGRAD[name])
    T.check_wgrad_real(api, name, WGRAD[name])


@pytest.mark.parametrize('name', list(T.BLEND_EXACT_CASES))
def test_blend_dyadic_ratios_equal_float64_emulated(api, name):
    T.check_blend_exact(api, name, T.BLEND_EXACT_CASES[name])


@pytest.mark.parametrize('name', list(T.BLEND_REAL_CASES))
def test_blend_real_ratios_inside_the_derived_bound_emulated(api, name):
    T.check_blend_real(api, name, T.BLEND_REAL_CASES[name])


def test_case_tables_keep_every_integer_sum_below_2_to_24():
    T.check_tables_stay_exact()
    for c in WGRAD.values():
        assert c['n_chunks'] * c['chunk'] >= c['B'] * T._prod(T.out_dims(c['dims'], c['k'], c['s'], c['p'])) > (c['n_chunks'] - 1) * c['chunk']


def test_forward_wrappers_refuse_a_bias_shorter_than_the_padded_cout():
    T.check_bias_guard()


def test_folded_convolutions_hand_the_wrappers_a_padded_bias():
    """what fb_bev_amd.mfma_conv3d builds for a 19-channel layer passes the guard: 32 floats, zero beyond Cout"""
    import torch
    import torch.nn as nn
    from fb_bev_amd import mfma_conv3d as M
    for folded in (M.FoldedConv3d(nn.Conv3d(16, 19, 1)), M.FoldedConv3d(nn.Conv3d(32, 19, 3, padding=1), nn.BatchNorm3d(19).eval(), precision='bf16'),
                   M.FoldedConv3d(nn.ConvTranspose3d(16, 19, 2, stride=2)), M.FoldedConv2d(nn.Conv2d(16, 19, 3, padding=1))):
        assert folded.cout == 19 and folded.bias.numel() == 32 and torch.equal(folded.bias[19:], torch.zeros(13))
