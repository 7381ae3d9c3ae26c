"""fbbev_occ_lovasz_fwd / fbbev_occ_lovasz_grad on the CPU emulator: the kernel source of fb_bev_amd/csrc/occ_lovasz_kernels.h and its
launchers, unedited, at the shapes of tests/occ_lovasz_cases.py.  Counts against a numpy bincount, the errors against float64, the
coefficients bit for bit against the canonical order of the device's own errors, the gradient against its float64 restatement; guard
words and read-only inputs are checked by occ_lovasz_cases.run.  The two reference tests run no kernel: they validate what the others
are held against."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_lovasz_cases as VC  # noqa: E402


@pytest.fixture(scope='module')
def api():
    return VC.EmuApi()


# a scatter workgroup is 256 fibers meeting at ~350 wave rendezvous: ~50 ms per full chunk here.  Cases above 400 voxels take two label
# sets on the emulator, the three-chunk case one (its other layout runs in test_four_passes_over_three_chunks), and the 33-chunk case
# (1 900 scatter workgroups, minutes) is left to the GPU, which runs all six label sets on every case (tests/test_gpu_occ_lovasz.py)
EMU_CASES = [c for c in VC.CASES if c['name'] not in VC.BIG_IDS + ['b1_17x33x16_planes']]


@pytest.mark.parametrize('case', EMU_CASES, ids=[c['name'] for c in EMU_CASES])
def test_counts_errors_coefficients_and_gradient(api, case):
    kinds = ['uniform'] if VC.voxels(case) > VC.CHUNK else (['uniform', 'absent'] if VC.voxels(case) > 400 else VC.LABEL_KINDS)
    for kind in kinds:
        VC.check(api, case, kind, order64=case['name'] in VC.SMALL_IDS)


@pytest.mark.parametrize('case', VC.EXACT_CASES, ids=VC.EXACT_IDS)
def test_ties_are_broken_by_voxel_index_alone(api, case):
    """p = 1 / C for every voxel: every bg error ties, every fg error ties; the order is stability's"""
    for kind in ('uniform', 'skewed', 'allvalid'):
        VC.check(api, case, kind, exact=True)


def test_two_classes_all_errors_equal(api):
    """C = 2 and p = 1/2: fg and bg errors tie as well, the order is the voxel order"""
    VC.check(api, VC.by_name('n2_cl'), 'uniform', exact=True)


@pytest.mark.parametrize('name', VC.EMU_REPEAT_IDS)
def test_two_runs_give_identical_bytes(api, name):
    VC.check_repeat(api, VC.by_name(name))


@pytest.mark.parametrize('env', [{'FBBEV_OCC_LOVASZ_GROUP_PAIRS': 'x3'}, {'FBBEV_OCC_LOVASZ_GROUP_PAIRS': 'x1'},
                                 {'FBBEV_OCC_LOVASZ_DIGIT_BITS': '8'}, {'FBBEV_OCC_LOVASZ_DIGIT_BITS': '8', 'FBBEV_OCC_LOVASZ_GROUP_PAIRS': 'x5'}],
                         ids=['groups_of_3', 'groups_of_1', 'four_passes', 'four_passes_groups_of_5'])
def test_class_groups_and_digit_width_change_no_bit(api, env, monkeypatch):
    """the classes sorted in groups (the emulator's knob shrinks the group to what the shipped shape meets at B = 4) and four 8-bit
    passes instead of three 10-bit ones: same loss_c, fg_count, coef and gradient, every layer of the check included"""
    case = VC.by_name('b2_8x8x16_padded_cl')
    L, lab = VC.inputs(case, 'uniform')[:2]
    base = VC.run(api, case, L, lab, VC.scale_of(case))
    for k, v in env.items():
        monkeypatch.setenv(k, str(int(v[1:]) * VC.voxels(case)) if v.startswith('x') else v)
    got = VC.check(api, case, 'uniform')
    for k in ('loss_c', 'fg_count', 'coef', 'errors', 'grad'):
        assert torch.equal(got[k].view(torch.int32), base[k].view(torch.int32)), k


def test_reference_closed_form_is_the_projects_formula():
    """the closed form the kernels are held against equals occ_loss.lovasz_softmax in float64 (restated without its .float() cast), and
    its gradient formula equals float64 autograd of it"""
    from fb_bev_amd import occ_loss
    case = VC.by_name('b2_5x7x3_cl')
    for kind in ('uniform', 'single', 'skewed'):
        L, lab, e64, f, p64 = VC.inputs(case, kind)
        C = case['C']
        coef, loss, Gs, n = VC.coef_from_errors(e64.numpy(), lab, C)
        want = float(loss[Gs > 0].sum() / max(int((Gs > 0).sum()), 1))
        x = L.double().requires_grad_()
        got = VC.lovasz64(torch.softmax(torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0), 1), lab)
        # the closed form rounds every coefficient to fp32 once (as the kernels do): relative 2^-24 per non-negative term
        assert abs(float(got.detach()) - want) <= 1.001 * 2.0 ** -24 * abs(want), (float(got.detach()), want)
        mine = float(occ_loss.lovasz_softmax(torch.softmax(torch.nan_to_num(L, nan=0.0, posinf=0.0, neginf=0.0), 1), lab, ignore=255))
        assert abs(mine - want) <= 2e-5 * abs(want) + 1e-6, (mine, want)       # VC.lovasz64 restates the function that ships
        got.backward()
        s = 1.0 / max(int((Gs > 0).sum()), 1)
        grad, A = VC.grad_ref64(L, coef, s)
        err = (x.grad - grad).abs()
        VC.observed(f'closed form against the float64 formula ({kind}): loss {abs(float(got.detach()) - want):.3e}, gradient worst err / A = '
                    f'{float((err[A > 0] / A[A > 0]).max()):.3e}')
        assert (err <= 1.001 * 2.0 ** -24 * A + 1e-300).all()


def test_empty_batch_zeroes_the_outputs(api):
    """B == 0: 0, no launch, loss_c and fg_count zeroed"""
    C = 19
    lc, fc = torch.full((C,), 7.5), torch.full((C + 1,), 9, dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dummy = torch.zeros(4)
    code = api.lib.fbbev_occ_lovasz_fwd(p(dummy), 0, 0, 0, 0, 0, 0, C, 4, 4, 2, p(dummy), p(lc), p(fc), None, None, None, 0, None)
    assert code == 0 and (lc == 0).all() and (fc == 0).all()
    assert api.lib.fbbev_occ_lovasz_grad(p(dummy), 0, 0, 0, 0, 0, 0, C, 4, 4, 2, p(dummy), None, p(dummy), p(dummy), None) == 0


def test_four_passes_over_three_chunks(api, monkeypatch):
    """8-bit digits where a class has three chunks: one colscan workgroup per class, a prefix over earlier chunks in every pass"""
    monkeypatch.setenv('FBBEV_OCC_LOVASZ_DIGIT_BITS', '8')
    VC.check(api, VC.by_name('b1_17x33x16_planes'), 'skewed')
