"""The case table of tests/pool_kernel_cases.py on the MI355X through fb_bev_amd._capi: every entry of the lift-splat pooling family --
fbbev_pool_tile_index, fbbev_bev_pool_v2_dense_fwd[_add], fbbev_bev_pool_v2_dense_fwd_rows, fbbev_pool_zmean[_split|_rows],
fbbev_bev_pool_v2_dense_bwd[_z] -- route by route and tile size by tile size, on a hand-built geometry whose properties (a tile beyond
the 512 staged points, an interval across that boundary inside a gather batch, empty tiles inside a pipelined run, a column beyond the
1 024 staged pairs, ...) are asserted on the host before anything is launched.  Layer A: dyadic inputs, every route equals float64
word for word.  Layer B: real values, word for word against the in-order fmaf chains of the oracle or inside the bounds derived in
the table.  tests/test_emu_pool_kernels.py runs the same table on the CPU emulator.  The observed figures are kept in
profiles/r26_pool_kernels_observed.txt.

FBBEV_POOL_PIPE_TPW and FBBEV_ZMEAN_COL are read once per process by the product build; each setting runs its cases in a fresh child
process, one after the other.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_kernel_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    return T.GpuApi()


@pytest.mark.parametrize('failed', [False, True], ids=['built', 'failed_build'])
@pytest.mark.parametrize('which,kind,tv', T.TILE_INDEX_CASES, ids=lambda v: str(v))
def test_tile_index(api, which, kind, tv, failed):
    T.check_tile_index(api, kind, tv, failed, which)


@pytest.mark.parametrize('name', list(T.DENSE_CASES))
def test_dense_fwd(api, name):
    T.check_forward(api, name)


@pytest.mark.parametrize('name', list(T.PIPE_CASES))
def test_dense_fwd_pipelined_default_run_length(api, name):
    T.check_forward(api, name)


@pytest.mark.parametrize('name', list(T.CL_CASES))
def test_dense_fwd_channels_last(api, name):
    T.check_forward(api, name)


@pytest.mark.parametrize('name', list(T.ROWS_CASES))
def test_dense_fwd_rows(api, name):
    T.check_forward(api, name)


@pytest.mark.parametrize('name', list(T.ZMEAN_CASES))
def test_zmean(api, name):
    T.check_forward(api, name)


@pytest.mark.parametrize('name', list(T.BWD_CASES))
def test_dense_bwd(api, name):
    T.check_backward(api, name)


@pytest.mark.parametrize('name', T.FAILED_CASES)
def test_failed_build_writes_zeros(api, name):
    T.check_failed_build(api, name)


@pytest.mark.parametrize('knob,value', [(k, v) for k in T.KNOBS for v in T.KNOBS[k]])
def test_knob_cases_in_a_child_process(knob, value):
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import pool_kernel_cases as T\n'
            'print("ran", T.run_knob(T.GpuApi(), %r, %r))\n') % (ROOT, os.path.join(ROOT, 'tests'), knob, value)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **{knob: value}), capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    n = len(T.KNOBS[knob][value])
    assert f'ran {n}' in r.stdout and r.stdout.count('[observed]') >= 2 * n
