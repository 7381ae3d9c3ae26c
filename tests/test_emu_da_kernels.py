"""The case table of tests/da_kernel_cases.py on the CPU emulator build of the launchers and kernels: proves without a GPU that the
float64 reference, the exact layer and the derived bounds hold for a correct implementation (the observed figures are printed).
tests/test_gpu_da_kernels.py runs the same table on the MI355X.  No case is shrunk here: the table's shapes are small enough for the
emulator (the whole file takes about two minutes).

The emulator re-reads the plan knobs on every call, so the knob tests switch them in process.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import da_kernel_cases as T  # noqa: E402

KNOBS = ('FBBEV_DA_FUSED_HW', 'FBBEV_DA_PIPE_WPS', 'FBBEV_DA_BWD_OWNED', 'FBBEV_DA_BWD_TOKENS', 'FBBEV_DA_BWD_CHUNKS', 'FBBEV_DA_BWD_THREADS',
         'FBBEV_DA_BWD_COPIES', 'FBBEV_DA_BWD_LDS_KB', 'FBBEV_DA_BWD_PREPASS', 'FBBEV_DA_BWD_UNIT_PLANES')


@pytest.fixture(scope='module')
def api():
    return T.EmuApi()


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_reference_equals_the_oracle_composite(seed):
    """the float64 reference of the table == oracle.backward_projection_oracle.da_spatial_cross_attention on the da_cases.da_case seeds"""
    from da_cases import da_case
    args, exp, _ = da_case(seed, grad=True)
    value, ss, ls, pred, ref_cam, mask, qdepth, offsets, attn, d0, dstep = args
    with torch.no_grad():
        got, S = T.reference(value, ss, ls, pred, ref_cam, mask, qdepth, offsets, attn, d0, dstep)
    err = (got - exp.detach()).abs().max().item()
    print(f'reference vs oracle, seed {seed}: max|diff| = {err:.3e} on a scale of {exp.abs().max().item():.3f}')
    assert err <= 1e-13 * max(1.0, S.max().item())


@pytest.mark.parametrize('name', list(T.FWD_CASES))
def test_fwd_exact_emulated(api, name):
    T.check_fwd(api, name)


@pytest.mark.parametrize('name', [k for k, c in T.FWD_CASES.items() if c['real']])
def test_fwd_real_inside_the_derived_bound_emulated(api, name):
    T.check_fwd(api, name, real=True)


@pytest.mark.parametrize('name', list(T.ZT_CASES))
def test_fwd_zt_exact_emulated(api, name):
    T.check_zt(api, name)


@pytest.mark.parametrize('name', [k for k, c in T.ZT_CASES.items() if c['real']])
def test_fwd_zt_real_inside_the_derived_bound_emulated(api, name):
    T.check_zt(api, name, real=True)


@pytest.mark.parametrize('name', list(T.PLANES_CASES))
def test_fwd_planes_exact_emulated(api, name):
    T.check_fwd_planes(api, name)


@pytest.mark.parametrize('name', [k for k, c in T.PLANES_CASES.items() if c['real']])
def test_fwd_planes_real_inside_the_derived_bound_emulated(api, name):
    T.check_fwd_planes(api, name, real=True)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['f32', 'bf16', 'fp16'])
@pytest.mark.parametrize('name', list(T.FUSED_CASES))
def test_fused_exact_emulated(api, name, dtype):
    T.check_fused(api, name, dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', T.FUSED_REAL)
def test_fused_real_inside_the_derived_bound_and_30x_better_than_bf16_operands_emulated(api, name, dtype):
    T.check_fused_real(api, name, dtype)


@pytest.mark.parametrize('name', list(T.BWD_CASES))
def test_bwd_exact_emulated(api, name):
    T.check_bwd(api, name)


@pytest.mark.parametrize('name', T.BWD_REAL)
def test_bwd_real_inside_the_derived_bounds_emulated(api, name):
    T.check_bwd_real(api, name)


@pytest.mark.parametrize('name', ['det_atomic_dh20', 'det_ws_grid_chunked', 'det_ws_grid_owned', 'det_planes'])
def test_bwd_ex_entries_without_the_flag_exact_emulated(api, name):
    """the flags-word entries with flags = 0 forward to the plain routes (fb_bev_amd._capi never calls them so: emulator only)"""
    T.check_bwd(api, name, det='flag_off')


@pytest.mark.parametrize('key', list(T.KNOB_RUNS))
def test_knob_settings_exact_emulated(api, key, monkeypatch):
    for k, v in T.KNOB_RUNS[key][0].items():
        monkeypatch.setenv(k, v)
    assert T.run_knob(api, key) == len(T.KNOB_RUNS[key][1])
