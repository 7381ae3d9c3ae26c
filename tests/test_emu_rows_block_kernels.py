"""The case tables of tests/rows_block_cases.py on the CPU emulator build of the kernels: proves without a GPU that the exact
references and the derived bounds hold for a correct implementation (and are not vacuous: the observed err / bound figures are
printed).  tests/test_gpu_rows_block_kernels.py runs the same tables on the MI355X.

Emulator-only knobs: FBBEV_FFN_HC (the emulator build reads it on every call: both hidden-chunk instantiations in one process) and
FBBEV_ROWS_LINEAR_RT = 2 for the two-row-tiles-per-workgroup walk of the LayerNorm route, which the device reaches from 262 017
rows on (300 rows here: three tiles, the last workgroup's second tile does not exist).
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_block_cases as B  # noqa: E402

KNOBS = ('FBBEV_FFN_HC', 'FBBEV_ROWS_LINEAR_RT', 'FBBEV_ROWS_LINEAR_SLOTS', 'FBBEV_ROWS_LINEAR_P', 'FBBEV_ROWS_LINEAR_NT')
LAYERS = (False, True)
LAYER_IDS = ('integers', 'real')


@pytest.fixture(scope='module')
def api():
    return B.EmuApi()


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _layers(cases):
    """(name, real) for every case and layer; a statistics case has real operands only"""
    return [pytest.param(name, real, id=f'{name}-{LAYER_IDS[real]}') for name, c in cases.items() for real in LAYERS
            if real or c['stats'] is None]


@pytest.mark.parametrize('name,real', _layers(B.LINEAR_LN_CASES))
def test_rows_linear_ln_emulated(api, name, real):
    B.check_linear_ln(api, name, B.LINEAR_LN_CASES[name], real)


def test_rows_linear_ln_two_row_tiles_per_workgroup_emulated(api, monkeypatch):
    case = B.LINEAR_LN_RT2_EMU
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)
    B.check_linear_ln(api, 'r300_i80_o80_rt2', case, False)


def test_rows_linear_ln_refusals_emulated(api):
    B.check_linear_ln_refusals(api)


@pytest.mark.parametrize('hc', ('32', '64'))
@pytest.mark.parametrize('name,real', _layers(B.FFN_CASES))
def test_rows_ffn_emulated(api, name, real, hc, monkeypatch):
    monkeypatch.setenv('FBBEV_FFN_HC', hc)
    B.check_ffn(api, name, B.FFN_CASES[name], real, tag=f', HC={hc}')


def test_rows_ffn_refusals_emulated(api):
    B.check_ffn_refusals(api)


@pytest.mark.parametrize('name,real', _layers(B.TAIL_CASES))
def test_rows_tail_ffn_rows_and_planes_emulated(api, name, real):
    B.check_tail(api, name, B.TAIL_CASES[name], real)


def test_rows_tail_ffn_refusals_emulated(api):
    B.check_tail_refusals(api)


@pytest.mark.parametrize('real', LAYERS, ids=LAYER_IDS)
@pytest.mark.parametrize('name', list(B.PLANES_CASES))
def test_rows_linear_planes_emulated(api, name, real):
    B.check_planes(api, name, B.PLANES_CASES[name], real)


def test_rows_linear_planes_refusals_emulated(api):
    B.check_planes_refusals(api)


@pytest.mark.parametrize('with_res', (False, True), ids=('plain', 'residual'))
@pytest.mark.parametrize('C', B.LAYERNORM_C)
@pytest.mark.parametrize('rows', B.LAYERNORM_ROWS)
def test_layernorm_forward_emulated(api, rows, C, with_res):
    B.check_layernorm(api, rows, C, with_res, B.EPS)
    B.check_layernorm(api, rows, C, with_res, 0.0)


@pytest.mark.parametrize('with_res', (False, True), ids=('plain', 'residual'))
@pytest.mark.parametrize('stats', B.LAYERNORM_STATS)
def test_layernorm_forward_statistics_emulated(api, stats, with_res):
    B.check_layernorm(api, 9, 80, with_res, B.EPS, stats)
    B.check_layernorm(api, 37, 124, with_res, B.EPS, stats)


def test_layernorm_forward_refusals_emulated(api):
    B.check_layernorm_refusals(api)
