"""fbbev_occ_loss_stats / fbbev_occ_loss_grad on the CPU emulator: the kernel source of fb_bev_amd/csrc/occ_loss_kernels.h and its
launchers, unedited, at the shapes of tests/occ_loss_cases.py.  Counts against a numpy bincount, exact sums where p = 1/C, every
statistic and the gradient against their float64 restatements; guard words and read-only inputs are checked by occ_loss_cases.run.
test_reference_backward_is_the_float64_autograd runs no kernel: it validates the reference the others are held against."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_loss_cases as LC  # noqa: E402


@pytest.fixture(scope='module')
def api():
    return LC.EmuApi()


@pytest.mark.parametrize('focal', [False, True], ids=['ce', 'focal'])
@pytest.mark.parametrize('case', LC.CASES, ids=LC.CASE_IDS)
def test_stats_and_gradient(api, case, focal):
    # the grid-stride cases start 1 000 - 2 000 workgroups of 256 fibers per launch, seconds each here: two label sets on the
    # emulator, all five on the GPU (tests/test_gpu_occ_loss.py)
    for kind in ['uniform', 'skewed'] if LC.tiles(case) > LC.STATS_BLOCKS else LC.LABEL_KINDS:
        LC.check(api, case, kind, focal)


@pytest.mark.parametrize('case', LC.EXACT_CASES, ids=LC.EXACT_IDS)
def test_sums_are_exact_where_p_is(api, case):
    LC.check_exact(api, case)


@pytest.mark.parametrize('name', LC.REPEAT_IDS)
def test_two_runs_give_identical_bytes(api, name):
    LC.check_repeat(api, LC.by_name(name))


@pytest.mark.parametrize('focal', [False, True], ids=['ce', 'focal'])
def test_reference_backward_is_the_float64_autograd(focal):
    """the float64 backward FORMULA the gradient is held against equals float64 autograd of the float64 statistics"""
    case = LC.by_name('b2_5x7x3_cl')
    L, lab, cw, plane, gS, sf, _, grad, A = LC.reference(case, 'uniform', focal)
    x = L.double().requires_grad_()                                  # a float64 leaf: the gradient is not rounded to fp32
    got, _ = LC.stats_torch(x, lab, cw, plane, case['e'], focal, torch.float64)
    assert torch.equal(got, sf)
    (got * gS.double()).sum().backward()
    err = (x.grad.double() - grad).abs()
    LC.observed(f'float64 formula against float64 autograd ({"focal" if focal else "ce"}): worst err / A = '
                f'{float((err[A > 0] / A[A > 0]).max()):.3e}')
    assert (err <= 1e-12 * A).all()
    assert (A >= grad.abs() * (1 - 1e-12)).all()


def test_empty_batch_zeroes_the_statistics(api):
    """B == 0: 0, no launch, stats_f and stats_i zeroed (real buffers: the entry clears them through the runtime)"""
    import ctypes
    C = 19
    sf, si = torch.full((3 * C + 4,), 7.5), torch.full((C + 1,), 9, dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dummy = torch.zeros(4)
    code = api.lib.fbbev_occ_loss_stats(p(dummy), 0, 0, 0, 0, 0, 0, C, 4, 4, 2, p(dummy), None, None, 18, 0, 2.0, 0.25, p(sf), p(si),
                                        None, 0, None)
    assert code == 0 and (sf == 0).all() and (si == 0).all()
    assert api.lib.fbbev_occ_loss_grad(p(dummy), 0, 0, 0, 0, 0, 0, C, 4, 4, 2, p(dummy), None, None, 18, 0, 2.0, 0.25, p(dummy), p(dummy),
                                       None) == 0
