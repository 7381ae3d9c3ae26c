"""The case table of tests/msda_kernel_cases.py on the MI355X through fb_bev_amd._capi: every entry of the plain multi-scale deformable
attention family -- fbbev_msda_fwd, fbbev_msda_fwd_fused, fbbev_msda_bwd, fbbev_msda_bwd_ws, fbbev_msda_bwd_ex -- at the smallest shapes
at which each of its code paths exists.  Layer A: dyadic inputs, the output and the three gradients equal the float64 reference bit for
bit on the atomic, band-binned and deterministic routes.  Layer B: real values at sizes that are no powers of two inside the bounds
derived in the table.  tests/test_emu_msda_kernels.py runs the same table on the CPU emulator.  The observed figures are kept in
profiles/r17_msda_kernels_observed.txt.

FBBEV_MSDA_BWD_LDS_KB is read once per process by the product build; each setting runs its cases in a fresh child process.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msda_kernel_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    return T.GpuApi()


@pytest.mark.parametrize('name', list(T.FWD_CASES))
def test_fwd_exact(api, name):
    T.check_fwd(api, name)


@pytest.mark.parametrize('name', list(T.FWD_CASES))
def test_fwd_real_inside_the_derived_bound(api, name):
    T.check_fwd(api, name, real=True)


def test_fwd_grid_stride_second_trip_exact(api):
    T.check_fwd_grid_stride(api)


@pytest.mark.parametrize('name', list(T.FUSED_CASES))
def test_fwd_fused_exact_and_bit_equal_to_the_composed_path(api, name):
    T.check_fused(api, name)


@pytest.mark.parametrize('name', T.FUSED_REAL)
def test_fwd_fused_real_inside_the_derived_bound(api, name):
    T.check_fused(api, name, real=True)


def test_fwd_fused_codes(api):
    T.check_fused_codes(api)


@pytest.mark.parametrize('name', list(T.ATOMIC_CASES))
def test_bwd_atomic_exact(api, name):
    T.check_atomic(api, name)


@pytest.mark.parametrize('name', list(T.ATOMIC_CASES))
def test_bwd_atomic_real_inside_the_derived_bounds(api, name):
    T.check_atomic(api, name, real=True)


@pytest.mark.parametrize('name', list(T.DET_CASES))
def test_bwd_ex_deterministic_exact(api, name):
    T.check_det(api, name)


@pytest.mark.parametrize('name', list(T.WS_CASES))
def test_bwd_ws_exact(api, name):
    T.check_ws(api, name)


@pytest.mark.parametrize('name', [k for k, p in T.WS_CASES.items() if p['real']])
def test_bwd_ws_real_inside_the_derived_bounds(api, name):
    T.check_ws(api, name, real=True)


def test_bwd_ws_inf_poisons_exactly_the_planes_of_its_spans(api):
    seen = set()
    for name in T.WS_POISON:
        seen |= set(T.check_ws_poison(api, name))
    assert seen == set(T.POISON_VARIANTS), set(T.POISON_VARIANTS) - seen


@pytest.mark.parametrize('name', list(T.NO_PLAN_CASES))
def test_bwd_ws_without_a_plan_accumulates_through_the_atomic_kernel(api, name):
    T.check_no_plan(api, name)
    T.check_capi_no_plan(api, name)


def test_deterministic_mode_wrapper_contracts(api):
    T.check_deterministic_wrapper(api)


def test_autograd_function_routes_exact(api):
    T.check_autograd_function(api)


@pytest.mark.parametrize('kb', list(T.KNOB_RUNS))
def test_bwd_ws_lds_knob_exact_in_a_child_process(kb):
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import msda_kernel_cases as T\n'
            'print("ran", T.run_knob(T.GpuApi(), %r))\n') % (ROOT, os.path.join(ROOT, 'tests'), kb)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **{T.KNOB: kb}), capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    assert f'ran {len(T.KNOB_RUNS[kb])}' in r.stdout and r.stdout.count('[observed]') >= len(T.KNOB_RUNS[kb])
