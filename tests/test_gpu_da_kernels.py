"""The case table of tests/da_kernel_cases.py on the MI355X through fb_bev_amd._capi: every forward and backward entry of the
depth-aware cross-attention family at the smallest shapes at which each of its code paths exists.  Layer A: dyadic inputs, the result
equals the float64 reference bit for bit (slots, and the four gradients against float64 autograd).  Layer B: real values at
the shipped level sizes inside the bounds derived in the table -- the forward entries, the entries that project in the kernel (also 30
times closer than plain bf16 operands) and the four gradients of the LDS-plane backward routes.  tests/test_emu_da_kernels.py runs the same table
on the CPU emulator.  The observed figures are kept in profiles/r14_da_kernels_observed.txt.

Four knobs are read once per process by the product build; each setting runs its cases in a fresh child process.
"""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import da_kernel_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    return T.GpuApi()


@pytest.mark.parametrize('name', list(T.FWD_CASES))
def test_fwd_exact(api, name):
    T.check_fwd(api, name)


@pytest.mark.parametrize('name', [k for k, c in T.FWD_CASES.items() if c['real']])
def test_fwd_real_inside_the_derived_bound(api, name):
    T.check_fwd(api, name, real=True)


@pytest.mark.parametrize('name', list(T.ZT_CASES))
def test_fwd_zt_exact(api, name):
    T.check_zt(api, name)


@pytest.mark.parametrize('name', [k for k, c in T.ZT_CASES.items() if c['real']])
def test_fwd_zt_real_inside_the_derived_bound(api, name):
    T.check_zt(api, name, real=True)


@pytest.mark.parametrize('name', list(T.PLANES_CASES))
def test_fwd_planes_exact(api, name):
    T.check_fwd_planes(api, name)


@pytest.mark.parametrize('name', [k for k, c in T.PLANES_CASES.items() if c['real']])
def test_fwd_planes_real_inside_the_derived_bound(api, name):
    T.check_fwd_planes(api, name, real=True)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['f32', 'bf16', 'fp16'])
@pytest.mark.parametrize('name', list(T.FUSED_CASES))
def test_fused_exact(api, name, dtype):
    T.check_fused(api, name, dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', T.FUSED_REAL)
def test_fused_real_inside_the_derived_bound_and_30x_better_than_bf16_operands(api, name, dtype):
    T.check_fused_real(api, name, dtype)


@pytest.mark.parametrize('name', list(T.BWD_CASES))
def test_bwd_exact(api, name):
    T.check_bwd(api, name)


@pytest.mark.parametrize('name', T.BWD_REAL)
def test_bwd_real_inside_the_derived_bounds(api, name):
    T.check_bwd_real(api, name)


@pytest.mark.parametrize('key', list(T.KNOB_RUNS))
def test_knob_settings_exact_in_a_child_process(key):
    env, runs = T.KNOB_RUNS[key]
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import da_kernel_cases as T\n'
            'print("ran", T.run_knob(T.GpuApi(), %r))\n') % (ROOT, os.path.join(ROOT, 'tests'), key)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    assert f'ran {len(runs)}' in r.stdout and r.stdout.count('[observed]') >= len(runs)
