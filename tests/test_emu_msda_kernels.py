"""The case table of tests/msda_kernel_cases.py on the CPU emulator build of the launchers and kernels: proves without a GPU that the
float64 reference, the exact layer, the derived bounds and the stated band plans hold for a correct implementation (the observed
figures are printed).  tests/test_gpu_msda_kernels.py runs the same table on the MI355X.  One case is left to the GPU:
FWD_GRID_STRIDE, whose 65 536 workgroups of 256 fibers would take the emulator minutes.

The emulator re-reads FBBEV_MSDA_BWD_LDS_KB on every call, so the knob test switches it in process.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msda_kernel_cases as T  # noqa: E402


@pytest.fixture(scope='module')
def api():
    return T.EmuApi()


@pytest.fixture(autouse=True)
def default_knob(monkeypatch):
    monkeypatch.delenv(T.KNOB, raising=False)


def test_reference_equals_the_oracle_grid_sample_in_double():
    """the float64 reference of the table == oracle.msda_grid_sample in double on test_oracle_msda.CASES"""
    from oracle import oracle as O
    from test_oracle_msda import CASES, make_case
    for case in CASES:
        value, ss, ls, loc, w = make_case(**case)
        exp = O.msda_grid_sample(value.double(), ss, loc.double(), w.double())
        with torch.no_grad():
            got, S = T.reference(value, [tuple(s) for s in case['shapes']], loc, w)
        err = (got - exp).abs().max().item()
        print(f'reference vs oracle {case["shapes"]}: max|diff| = {err:.3e} on a scale of {exp.abs().max().item():.3f}')
        assert err <= 1e-13 * max(1.0, S.max().item())


def test_the_table_proves_its_own_claims():
    T.table_claims()


@pytest.mark.parametrize('name', list(T.FWD_CASES))
def test_fwd_exact_emulated(api, name):
    T.check_fwd(api, name)


@pytest.mark.parametrize('name', list(T.FWD_CASES))
def test_fwd_real_inside_the_derived_bound_emulated(api, name):
    T.check_fwd(api, name, real=True)


@pytest.mark.parametrize('name', list(T.FUSED_CASES))
def test_fwd_fused_exact_and_bit_equal_to_the_composed_path_emulated(api, name):
    T.check_fused(api, name)


@pytest.mark.parametrize('name', T.FUSED_REAL)
def test_fwd_fused_real_inside_the_derived_bound_emulated(api, name):
    T.check_fused(api, name, real=True)


def test_fwd_fused_codes_emulated(api):
    T.check_fused_codes(api)


@pytest.mark.parametrize('name', list(T.ATOMIC_CASES))
def test_bwd_atomic_exact_emulated(api, name):
    T.check_atomic(api, name)


@pytest.mark.parametrize('name', list(T.ATOMIC_CASES))
def test_bwd_atomic_real_inside_the_derived_bounds_emulated(api, name):
    T.check_atomic(api, name, real=True)


@pytest.mark.parametrize('name', list(T.DET_CASES))
def test_bwd_ex_deterministic_exact_emulated(api, name):
    T.check_det(api, name)


@pytest.mark.parametrize('name', list(T.WS_CASES))
def test_bwd_ws_exact_emulated(api, name):
    T.check_ws(api, name)


@pytest.mark.parametrize('name', [k for k, p in T.WS_CASES.items() if p['real']])
def test_bwd_ws_real_inside_the_derived_bounds_emulated(api, name):
    T.check_ws(api, name, real=True)


def test_bwd_ws_inf_poisons_exactly_the_planes_of_its_spans_emulated(api):
    seen = set()
    for name in T.WS_POISON:
        seen |= set(T.check_ws_poison(api, name))
    assert seen == set(T.POISON_VARIANTS), set(T.POISON_VARIANTS) - seen


@pytest.mark.parametrize('name', list(T.NO_PLAN_CASES))
def test_bwd_ws_without_a_plan_accumulates_through_the_atomic_kernel_emulated(api, name):
    T.check_no_plan(api, name)


@pytest.mark.parametrize('kb', list(T.KNOB_RUNS))
def test_bwd_ws_lds_knob_exact_emulated(api, kb, monkeypatch):
    monkeypatch.setenv(T.KNOB, kb)
    assert T.run_knob(api, kb) == len(T.KNOB_RUNS[kb])
