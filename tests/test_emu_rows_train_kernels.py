"""The case table of tests/rows_train_cases.py on the CPU emulator build of the kernels: proves without a GPU that the int64 / float64
references and the derived bounds hold for a correct implementation (and are not vacuous: the observed err / bound figures are
printed).  tests/test_gpu_rows_train_kernels.py runs the same table on the MI355X.

Three cases are shrunk here and only here, because the emulator runs every lane as a fiber (the two wgrad cases took 28 s and 22 s
at full size, the linear case has 513 row tiles):
  * wgrad (80, 512, 4165): four output chunks at 453 rows under FBBEV_WGRAD_SPLITS = 8 (the emulator build reads the knob on every
    call; 8 is the fewest splits the plan accepts) -- 15 steps in seven splits of 2 steps and a last split of one step with 5 rows;
  * wgrad (512, 80, 2079): the same four input chunks at 527 rows (17 splits of one step, 15 rows in the last);
  * the 65 573-row linear case (three row tiles per persistent workgroup, partial last tile): 603 rows under
    FBBEV_ROWS_LINEAR_SLOTS = 2 -- slot 0 walks tiles 0, 2 and 4, and tile 4 has 91 rows.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_train_cases as T  # noqa: E402


@pytest.fixture(scope='module')
def api():
    return T.EmuApi()


KNOBS = ('FBBEV_WGRAD_SPLITS', 'FBBEV_ROWS_LINEAR_SLOTS', 'FBBEV_ROWS_LINEAR_RT', 'FBBEV_ROWS_LINEAR_P', 'FBBEV_ROWS_LINEAR_NT')


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _env(monkeypatch, case):
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)


WGRAD = dict(T.WGRAD_CASES)
WGRAD['i80_o512_r4165'] = T._wg(80, 512, 453, True, ks=15, kps=2, n_split=8, nti=5, n_oc=4, n_ic=1, amt=8, env={'FBBEV_WGRAD_SPLITS': '8'})
WGRAD['i512_o80_r2079'] = T._wg(512, 80, 527, True, ks=17, kps=1, n_split=17, nti=8, n_oc=1, n_ic=4, amt=5)
LINEAR = dict(T.LINEAR_CASES)
LINEAR['r65573_i80_o160_three_tiles_per_workgroup'] = T._lin(603, 80, 160, False, 201, env={'FBBEV_ROWS_LINEAR_SLOTS': '2'})


@pytest.mark.parametrize('name', list(WGRAD))
def test_rows_wgrad_integer_operands_equal_int64_emulated(api, name, monkeypatch):
    case = WGRAD[name]
    _env(monkeypatch, case)
    T.check_wgrad_plan(api, case)
    T.check_wgrad_exact(api, name, case)


@pytest.mark.parametrize('name', [k for k, c in WGRAD.items() if c['real']])
def test_rows_wgrad_real_operands_inside_the_derived_bound_emulated(api, name, monkeypatch):
    case = WGRAD[name]
    _env(monkeypatch, case)
    T.check_wgrad_plan(api, case)
    T.check_wgrad_real(api, name, case)


@pytest.mark.parametrize('name', list(T.WGRAD_ADDEND_CASES))
def test_rows_wgrad_periodic_addend_emulated(api, name):
    case = T.WGRAD_ADDEND_CASES[name]
    T.check_wgrad_plan(api, case)
    T.check_wgrad_exact(api, name, case)
    if case['real']:
        T.check_wgrad_real(api, name, case)


@pytest.mark.parametrize('name', list(LINEAR))
def test_rows_linear_integer_operands_equal_int64_emulated(api, name, monkeypatch):
    _env(monkeypatch, LINEAR[name])
    T.check_linear_exact(api, name, LINEAR[name])


@pytest.mark.parametrize('name', [k for k, c in LINEAR.items() if c['real']])
def test_rows_linear_real_operands_inside_the_derived_bound_emulated(api, name):
    T.check_linear_real(api, name, LINEAR[name])


@pytest.mark.parametrize('n_groups', T.SOFTMAX_COUNTS)
@pytest.mark.parametrize('group', T.SOFTMAX_GROUPS)
def test_softmax_groups_emulated(api, group, n_groups):
    T.check_softmax(api, group, n_groups, fwd_bar=3e-7)


def test_softmax_groups_rejects_group_12_emulated(api):
    T.check_softmax_rejects_group_12(api)


@pytest.mark.parametrize('N', T.SUM_LEADING_N)
@pytest.mark.parametrize('B', T.SUM_LEADING_B)
def test_sum_leading_emulated(api, B, N):
    T.check_sum_leading(api, B, N)


@pytest.mark.parametrize('ln', T.SUM_PARTIALS_LEN)
@pytest.mark.parametrize('n', T.SUM_PARTIALS_N)
def test_sum_partials_emulated(api, n, ln):
    T.check_sum_partials(api, n, ln)


@pytest.mark.parametrize('rows,C', T.LAYERNORM_BWD_CASES)
def test_layernorm_bwd_emulated(api, rows, C):
    T.check_layernorm_bwd(api, rows, C)
