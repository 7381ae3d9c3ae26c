"""The fused row kernels of the encoder block called directly on the MI355X at tile-edge shapes: fbbev_rows_linear_x3_ln,
fbbev_rows_ffn_x3, fbbev_rows_tail_ffn_x3 / _planes, fbbev_rows_linear_x3_planes / _planes_e and fbbev_layernorm (forward), every
case of tests/rows_block_cases.py through fb_bev_amd._capi's library.  The case tables, the exact / float64 references and the
derived bounds are described there; tests/test_emu_rows_block_kernels.py proves on the CPU emulator build that a correct
implementation meets them.  Every shape runs under the default plan: no test here sets a knob, except the one child process that
runs the FFN table with 64 hidden units per chunk (FBBEV_FFN_HC is read once per process).  The figures the tests print are kept in
profiles/r25_rows_block_kernels_observed.txt."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import rows_block_cases as B  # noqa: E402

LAYERS = (False, True)
LAYER_IDS = ('integers', 'real')


@pytest.fixture(scope='module')
def api():
    import torch
    assert torch.cuda.is_available()
    return B.GpuApi()


def _layers(cases):
    """(name, real) for every case and layer; a statistics case has real operands only"""
    return [pytest.param(name, real, id=f'{name}-{LAYER_IDS[real]}') for name, c in cases.items() for real in LAYERS
            if real or c['stats'] is None]


@pytest.mark.parametrize('name,real', _layers(B.LINEAR_LN_CASES))
def test_rows_linear_ln(api, name, real):
    B.check_linear_ln(api, name, B.LINEAR_LN_CASES[name], real)


def test_rows_linear_ln_two_row_tiles_per_workgroup(api):
    """262 145 rows = 2 049 row tiles: the launcher's RT = 2, and the last workgroup's second tile does not exist"""
    B.check_linear_ln(api, 'r262145_i80_o80_rt2', B.LINEAR_LN_RT2_GPU, False)


def test_rows_linear_ln_refusals(api):
    B.check_linear_ln_refusals(api)


@pytest.mark.parametrize('name,real', _layers(B.FFN_CASES))
def test_rows_ffn(api, name, real):
    B.check_ffn(api, name, B.FFN_CASES[name], real, tag=', HC=32')


def test_rows_ffn_64_unit_chunks():
    """The HC = 64 instantiation (FBBEV_FFN_HC=64; the knob is read once per process, hence a child process): every case, both layers."""
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import rows_block_cases as B\n'
            'print("checks:", B.run_all_ffn(B.GpuApi(), tag=", HC=64"))\n') % (ROOT, HERE)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, FBBEV_FFN_HC='64'), capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    n = sum(1 if c['stats'] else 2 for c in B.FFN_CASES.values())
    assert r.stdout.count('[observed]') == n and f'checks: {n}' in r.stdout


def test_rows_ffn_refusals(api):
    B.check_ffn_refusals(api)


@pytest.mark.parametrize('name,real', _layers(B.TAIL_CASES))
def test_rows_tail_ffn_rows_and_planes(api, name, real):
    B.check_tail(api, name, B.TAIL_CASES[name], real)


def test_rows_tail_ffn_refusals(api):
    B.check_tail_refusals(api)


@pytest.mark.parametrize('real', LAYERS, ids=LAYER_IDS)
@pytest.mark.parametrize('name', list(B.PLANES_CASES))
def test_rows_linear_planes(api, name, real):
    B.check_planes(api, name, B.PLANES_CASES[name], real)


def test_rows_linear_planes_refusals(api):
    B.check_planes_refusals(api)


@pytest.mark.parametrize('with_res', (False, True), ids=('plain', 'residual'))
@pytest.mark.parametrize('C', B.LAYERNORM_C)
@pytest.mark.parametrize('rows', B.LAYERNORM_ROWS)
def test_layernorm_forward(api, rows, C, with_res):
    B.check_layernorm(api, rows, C, with_res, B.EPS)
    B.check_layernorm(api, rows, C, with_res, 0.0)


@pytest.mark.parametrize('with_res', (False, True), ids=('plain', 'residual'))
@pytest.mark.parametrize('stats', B.LAYERNORM_STATS)
def test_layernorm_forward_statistics(api, stats, with_res):
    B.check_layernorm(api, 9, 80, with_res, B.EPS, stats)
    B.check_layernorm(api, 37, 124, with_res, B.EPS, stats)


def test_layernorm_forward_refusals(api):
    B.check_layernorm_refusals(api)
