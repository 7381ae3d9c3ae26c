"""The case table of tests/pool_kernel_cases.py on the CPU emulator build of the launchers and kernels: proves without a GPU that the
geometry holds every property it was built for, and that the references, the exact layer and the derived bounds hold for a correct
implementation of every route (the observed figures are printed).  tests/test_gpu_pool_kernels.py runs the same table on the MI355X,
where the barriers, the LDS reuse and the wave shuffles are real.

The emulator re-reads FBBEV_POOL_PIPE_TPW and FBBEV_ZMEAN_COL on every call, so the knob tests switch them in process.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_kernel_cases as T  # noqa: E402


@pytest.fixture(scope='module')
def api():
    return T.EmuApi()


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for knob in T.KNOBS:
        monkeypatch.delenv(knob, raising=False)


@pytest.mark.parametrize('which', list(T.FRUSTA))
def test_the_geometry_holds_every_property_it_was_built_for(which):
    T.check(T.geometry(which))
    for C in T.CHANNELS:
        assert T.build(C, which=which)['feat'].shape[-1] == C


@pytest.mark.parametrize('failed', [False, True], ids=['built', 'failed_build'])
@pytest.mark.parametrize('which,kind,tv', T.TILE_INDEX_CASES, ids=lambda v: str(v))
def test_tile_index_emulated(api, which, kind, tv, failed):
    T.check_tile_index(api, kind, tv, failed, which)


@pytest.mark.parametrize('name', list(T.DENSE_CASES))
def test_dense_fwd_emulated(api, name):
    T.check_forward(api, name)


@pytest.mark.parametrize('tpw', ['default', '1', '2', '4'])
@pytest.mark.parametrize('name', list(T.PIPE_CASES))
def test_dense_fwd_pipelined_emulated(api, name, tpw, monkeypatch):
    if tpw != 'default':
        monkeypatch.setenv('FBBEV_POOL_PIPE_TPW', tpw)
    T.check_forward(api, name)


@pytest.mark.parametrize('name', list(T.CL_CASES))
def test_dense_fwd_channels_last_emulated(api, name):
    T.check_forward(api, name)


@pytest.mark.parametrize('name', list(T.ROWS_CASES))
def test_dense_fwd_rows_emulated(api, name):
    T.check_forward(api, name)


@pytest.mark.parametrize('name', list(T.ZMEAN_CASES))
def test_zmean_emulated(api, name):
    T.check_forward(api, name)


@pytest.mark.parametrize('name', list(T.COL_CASES))
def test_zmean_column_form_emulated(api, name, monkeypatch):
    monkeypatch.setenv('FBBEV_ZMEAN_COL', '1')
    T.check_forward(api, name)
    T.check_column_equals_plane_walk(api, name)


@pytest.mark.parametrize('name', list(T.BWD_CASES))
def test_dense_bwd_emulated(api, name):
    T.check_backward(api, name)


@pytest.mark.parametrize('name', T.FAILED_CASES)
def test_failed_build_writes_zeros_emulated(api, name):
    T.check_failed_build(api, name)
