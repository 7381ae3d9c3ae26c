"""The case table of tests/history_kernel_cases.py on the CPU emulator build of the launchers and kernels: proves without a GPU that the
float64 reference, the exact layer, the derived bounds and the stated launch geometry hold for a correct implementation (the observed
figures are printed).  tests/test_gpu_history_kernels.py runs the same table on the MI355X.

No case is left to the GPU (T.STEP_GPU_ONLY is empty): the slowest here are the two fbbev_history_fused_vm cases on the 9 x 17 x 65 grid
at 80 channels -- the smallest grid on which that kernel has a partial x tile AND a band that overhangs Y while every axis is 2^k + 1
long -- at about 20 s (T = 1) and about a minute (T = 3).

FBBEV_HISTORY_VM_YB and FBBEV_HISTORY_WARP are read on every call and are switched in process by the checks.  FBBEV_HISTORY_VM_TU,
FBBEV_HX3_WAVES and FBBEV_HISTORY_STEP_WAVES are function-local `static const` in capi.hip: read once per process in the emulator build
too, so their cases run in fresh child processes here as on the GPU.
"""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import history_kernel_cases as T  # noqa: E402


@pytest.fixture(scope='module')
def api():
    return T.EmuApi()


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in (T.KNOB_YB, T.KNOB_WARP) + T.KNOBS_ONCE:
        monkeypatch.delenv(k, raising=False)


def test_warp_reference_equals_the_oracle_grid_sample_in_double():
    """on the flows and the shape of test_gpu_history.py::test_warp_kernel_vs_reference_grid_sample_and_oracle the two differ only by
    what the fp32 coordinate chain contributes"""
    diff, allow = T.anchor_difference()
    print(f'table reference vs oracle.history_oracle.grid_sample_3d in double: max|diff| = {diff:.3e}, fp32 coordinate allowance {allow:.3e}')
    assert diff <= allow


def test_the_table_proves_its_own_claims():
    inst = T.table_claims()
    for name, kern in sorted(inst.items()):
        print(f'{name}: {kern}')


@pytest.mark.parametrize('name', list(T.FLOW_CASES))
def test_flow_emulated(api, name):
    T.check_flow(api, name)


@pytest.mark.parametrize('name', list(T.PROLOGUE_CASES))
def test_stream_prologue_emulated(api, name):
    T.check_prologue(api, name)


@pytest.mark.parametrize('name', list(T.WARP_CASES))
def test_warp_exact_emulated(api, name):
    T.check_warp(api, name)


@pytest.mark.parametrize('name', list(T.WARP_REAL))
def test_warp_real_inside_the_derived_bound_emulated(api, name):
    T.check_warp(api, name, real=True)


@pytest.mark.parametrize('name', list(T.WARP_VM_CASES))
def test_warp_vm_exact_emulated(api, name):
    T.check_warp_vm(api, name)


@pytest.mark.parametrize('name', list(T.WARP_VM_REAL))
def test_warp_vm_real_inside_the_derived_bound_emulated(api, name):
    T.check_warp_vm(api, name, real=True)


@pytest.mark.parametrize('name', list(T.WARP_SRC_CASES))
def test_warp_vm_src_exact_emulated(api, name):
    T.check_warp_vm(api, name, table=T.WARP_SRC_CASES)


@pytest.mark.parametrize('name', list(T.FRAME_CASES))
def test_frame_vm_exact_emulated(api, name):
    T.check_frame_vm(api, name)


@pytest.mark.parametrize('name', list(T.CONV_CASES))
def test_conv_exact_emulated(api, name):
    T.check_conv(api, name)


@pytest.mark.parametrize('name', T.CONV_REAL)
def test_conv_real_inside_the_derived_bound_emulated(api, name):
    T.check_conv(api, name, real=True)


@pytest.mark.parametrize('name', [n for n in T.STEP_CASES if n not in T.STEP_GPU_ONLY])
def test_fused_and_step_exact_emulated(api, name):
    T.check_step(api, name)


@pytest.mark.parametrize('name', list(T.STEP_REAL))
def test_fused_and_step_real_inside_the_derived_bounds_emulated(api, name):
    T.check_step(api, name, real=True)


def test_shorthand_entries_emulated(api):
    T.check_shorthands(api)


def test_return_codes_emulated(api):
    T.check_codes(api)


@pytest.mark.parametrize('name,value', list(T.KNOB_RUNS))
def test_once_per_process_knob_exact_in_a_child_process_emulated(name, value):
    r = subprocess.run([sys.executable, '-c', T.knob_child_code('EmuApi', name, value)], env=dict(os.environ, **{name: value}),
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    n = len(T.KNOB_RUNS[(name, value)])
    assert f'ran {n}' in r.stdout and r.stdout.count('[observed]') >= n
