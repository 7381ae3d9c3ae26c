"""The training-side row kernels called directly on the MI355X at tile-edge shapes: fbbev_rows_wgrad_x3, fbbev_rows_linear_x3 / _add /
_train, fbbev_softmax_groups / _bwd, fbbev_sum_leading, fbbev_sum_partials and fbbev_layernorm_bwd, every case of
tests/rows_train_cases.py through fb_bev_amd._capi.  The case table, the int64 / float64 references and the derived bounds are
described there; tests/test_emu_rows_train_kernels.py proves on the CPU emulator build that a correct implementation meets them.
Every shape runs under the default plan: no test here sets a knob.  The figures the tests print are kept in
profiles/r10_rows_train_kernels_observed.txt."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_train_cases as T  # noqa: E402

# fbbev_softmax_groups forward against float64: the project's bar (test_softmax_groups_forward_and_backward_emulated).  The largest
# value observed on the MI355X with its fast exponential is in profiles/r10_rows_train_kernels_observed.txt.
SOFTMAX_FWD_BAR = 3e-7


@pytest.fixture(scope='module')
def api():
    import torch
    assert torch.cuda.is_available()
    return T.GpuApi()


@pytest.mark.parametrize('name', list(T.WGRAD_CASES))
def test_rows_wgrad_integer_operands_equal_int64(api, name):
    case = T.WGRAD_CASES[name]
    T.check_wgrad_plan(api, case)
    T.check_wgrad_exact(api, name, case)


@pytest.mark.parametrize('name', [k for k, c in T.WGRAD_CASES.items() if c['real']])
def test_rows_wgrad_real_operands_inside_the_derived_bound(api, name):
    case = T.WGRAD_CASES[name]
    T.check_wgrad_plan(api, case)
    T.check_wgrad_real(api, name, case)


@pytest.mark.parametrize('name', list(T.WGRAD_ADDEND_CASES))
def test_rows_wgrad_periodic_addend(api, name):
    case = T.WGRAD_ADDEND_CASES[name]
    T.check_wgrad_plan(api, case)
    T.check_wgrad_exact(api, name, case)
    if case['real']:
        T.check_wgrad_real(api, name, case)


@pytest.mark.parametrize('name', list(T.LINEAR_CASES))
def test_rows_linear_integer_operands_equal_int64(api, name):
    T.check_linear_exact(api, name, T.LINEAR_CASES[name])


@pytest.mark.parametrize('name', [k for k, c in T.LINEAR_CASES.items() if c['real']])
def test_rows_linear_real_operands_inside_the_derived_bound(api, name):
    T.check_linear_real(api, name, T.LINEAR_CASES[name])


@pytest.mark.parametrize('n_groups', T.SOFTMAX_COUNTS)
@pytest.mark.parametrize('group', T.SOFTMAX_GROUPS)
def test_softmax_groups(api, group, n_groups):
    T.check_softmax(api, group, n_groups, fwd_bar=SOFTMAX_FWD_BAR)


def test_softmax_groups_rejects_group_12(api):
    T.check_softmax_rejects_group_12(api)


@pytest.mark.parametrize('N', T.SUM_LEADING_N)
@pytest.mark.parametrize('B', T.SUM_LEADING_B)
def test_sum_leading(api, B, N):
    T.check_sum_leading(api, B, N)


@pytest.mark.parametrize('ln', T.SUM_PARTIALS_LEN)
@pytest.mark.parametrize('n', T.SUM_PARTIALS_N)
def test_sum_partials(api, n, ln):
    T.check_sum_partials(api, n, ln)


@pytest.mark.parametrize('rows,C', T.LAYERNORM_BWD_CASES)
def test_layernorm_bwd(api, rows, C):
    T.check_layernorm_bwd(api, rows, C)
