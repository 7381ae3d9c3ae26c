"""The case table of tests/history_kernel_cases.py on the MI355X through fb_bev_amd._capi: every exported entry of the temporal history
fusion -- fbbev_history_flow, _stream_prologue, _warp[_e], _warp_vm, _warp_vm_src, _frame_vm, _conv[_e], _conv_vm, _conv_bf16,
_conv_bf16x3, _fused_vm, _fused_x3_vm, _step_x3_vm -- at the smallest shapes at which each of its code paths exists.  Layer A: inputs
without a rounding to make, the rings and volumes equal the float64 reference bit for bit on every route.  Layer B: real values on
grids that are no 2^k + 1 inside the bounds derived in the table.  tests/test_emu_history_kernels.py runs the same table on the CPU
emulator.  The observed figures are kept in profiles/r20_history_kernels_observed.txt.

FBBEV_HISTORY_VM_TU, FBBEV_HX3_WAVES and FBBEV_HISTORY_STEP_WAVES are read once per process; each setting runs its cases in a fresh
child process, one after another.
"""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import history_kernel_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    return T.GpuApi()


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in (T.KNOB_YB, T.KNOB_WARP) + T.KNOBS_ONCE:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize('name', list(T.FLOW_CASES))
def test_flow(api, name):
    T.check_flow(api, name)


@pytest.mark.parametrize('name', list(T.PROLOGUE_CASES))
def test_stream_prologue(api, name):
    T.check_prologue(api, name)


@pytest.mark.parametrize('name', list(T.WARP_CASES))
def test_warp_exact(api, name):
    T.check_warp(api, name)


@pytest.mark.parametrize('name', list(T.WARP_REAL))
def test_warp_real_inside_the_derived_bound(api, name):
    T.check_warp(api, name, real=True)


@pytest.mark.parametrize('name', list(T.WARP_VM_CASES))
def test_warp_vm_exact(api, name):
    T.check_warp_vm(api, name)


@pytest.mark.parametrize('name', list(T.WARP_VM_REAL))
def test_warp_vm_real_inside_the_derived_bound(api, name):
    T.check_warp_vm(api, name, real=True)


@pytest.mark.parametrize('name', list(T.WARP_SRC_CASES))
def test_warp_vm_src_exact(api, name):
    T.check_warp_vm(api, name, table=T.WARP_SRC_CASES)


@pytest.mark.parametrize('name', list(T.FRAME_CASES))
def test_frame_vm_exact(api, name):
    T.check_frame_vm(api, name)


@pytest.mark.parametrize('name', list(T.CONV_CASES))
def test_conv_exact(api, name):
    T.check_conv(api, name)


@pytest.mark.parametrize('name', T.CONV_REAL)
def test_conv_real_inside_the_derived_bound(api, name):
    T.check_conv(api, name, real=True)


@pytest.mark.parametrize('name', list(T.STEP_CASES))
def test_fused_and_step_exact(api, name):
    T.check_step(api, name)


@pytest.mark.parametrize('name', list(T.STEP_REAL))
def test_fused_and_step_real_inside_the_derived_bounds(api, name):
    T.check_step(api, name, real=True)


def test_shorthand_entries(api):
    T.check_shorthands(api)


def test_return_codes(api):
    T.check_codes(api)


@pytest.mark.parametrize('name,value', list(T.KNOB_RUNS))
def test_once_per_process_knob_exact_in_a_child_process(name, value):
    r = subprocess.run([sys.executable, '-c', T.knob_child_code('GpuApi', name, value)], env=dict(os.environ, **{name: value}),
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    n = len(T.KNOB_RUNS[(name, value)])
    assert f'ran {n}' in r.stdout and r.stdout.count('[observed]') >= n
