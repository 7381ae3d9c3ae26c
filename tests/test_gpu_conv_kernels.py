"""The convolution kernels of fb_bev_amd/csrc/conv3d_kernels.h called directly on the MI355X at tile-edge shapes: fbbev_conv3d_ndhwc
(plain and transposed), fbbev_conv2d_nhwc, fbbev_conv3d_ndhwc_bf16, fbbev_conv3d_k3s1_tiled_bf16, fbbev_conv3d_dgrad_ndhwc, both routes
of fbbev_conv3d_wgrad_ndhwc_ex and fbbev_blend_levels_ndhwc, every case of tests/conv_cases.py through fb_bev_amd._capi.  The case
tables, the float64 references and the derived bounds are described there; tests/test_emu_conv_kernels.py proves on the CPU emulator
build that a correct implementation meets them.  The table runs as written.  The figures the tests print are kept in
profiles/r11_conv_kernels_observed.txt."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as T  # noqa: E402

F32_KINDS = [('f32', n, c) for n, c in T.FORWARD_CASES.items()] + [('2d', n, c) for n, c in T.FORWARD_2D_CASES.items()] + \
    [('transposed', n, c) for n, c in T.TRANSPOSED_CASES.items()]
BF16_KINDS = [('bf16', n, c) for n, c in T.BF16_CASES.items()] + [('tiled', n, c) for n, c in T.TILED_CASES.items()] + \
    [('transposed_bf16', n, c) for n, c in T.TRANSPOSED_CASES.items()]
_ids = lambda rows: [f'{k}-{n}' for k, n, _ in rows]  # noqa: E731


@pytest.fixture(scope='module')
def api():
    import torch
    assert torch.cuda.is_available()
    return T.GpuApi()


@pytest.mark.parametrize('kind,name,case', F32_KINDS + BF16_KINDS, ids=_ids(F32_KINDS + BF16_KINDS))
def test_conv_integer_operands_equal_float64(api, kind, name, case):
    T.check_conv_exact(api, kind, name, case)


@pytest.mark.parametrize('kind,name,case', F32_KINDS, ids=_ids(F32_KINDS))
def test_conv_f32_real_operands_inside_the_derived_bound(api, kind, name, case):
    T.check_conv_real_f32(api, kind, name, case)


@pytest.mark.parametrize('kind,name,case', BF16_KINDS, ids=_ids(BF16_KINDS))
def test_conv_bf16_real_operands_inside_the_derived_bound(api, kind, name, case):
    T.check_conv_real_bf16(api, kind, name, case)


@pytest.mark.parametrize('name', list(T.DGRAD_CASES))
def test_dgrad_integer_operands_equal_float64(api, name):
    T.check_dgrad_exact(api, name, T.DGRAD_CASES[name])


@pytest.mark.parametrize('name', list(T.DGRAD_CASES))
def test_dgrad_real_operands_inside_the_derived_bound(api, name):
    T.check_dgrad_real(api, name, T.DGRAD_CASES[name])


@pytest.mark.parametrize('name', list(T.WGRAD_CASES))
def test_wgrad_integer_operands_equal_float64_on_both_routes(api, name):
    T.check_wgrad_plan(api, T.WGRAD_CASES[name])
    T.check_wgrad_exact(api, name, T.WGRAD_CASES[name])


@pytest.mark.parametrize('name', list(T.WGRAD_CASES))
def test_wgrad_real_operands_inside_the_derived_bound_and_bit_stable(api, name):
    T.check_wgrad_plan(api, T.WGRAD_CASES[name])
    T.check_wgrad_real(api, name, T.WGRAD_CASES[name])


@pytest.mark.parametrize('name', list(T.BLEND_EXACT_CASES))
def test_blend_dyadic_ratios_equal_float64(api, name):
    T.check_blend_exact(api, name, T.BLEND_EXACT_CASES[name])


@pytest.mark.parametrize('name', list(T.BLEND_REAL_CASES))
def test_blend_real_ratios_inside_the_derived_bound(api, name):
    T.check_blend_real(api, name, T.BLEND_REAL_CASES[name])
