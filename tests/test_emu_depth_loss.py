"""fbbev_depth_loss_fwd / fbbev_depth_loss_grad on the CPU emulator: the kernel source of fb_bev_amd/csrc/depth_loss_kernels.h and its
launchers, unedited, at the shapes of tests/depth_loss_cases.py, through tests/emu/emu_capi.lib().  Labels and count against the CPU
CM_DepthNet bit for bit, exact sums where every probability is 0 or 1, the loss and the gradient against their float64 restatements;
guard words and read-only inputs are checked by depth_loss_cases.run.  The module-level CPU behaviour is checked here as well: a
flagged CM_DepthNet on CPU tensors runs today's code."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_loss_cases as DC  # noqa: E402


@pytest.fixture(scope='module')
def api():
    return DC.EmuApi()


@pytest.mark.parametrize('case', DC.CASES, ids=DC.CASE_IDS)
def test_labels_loss_and_gradient(api, case):
    DC.check(api, case)


@pytest.mark.parametrize('case', DC.CASES, ids=DC.CASE_IDS)
def test_sums_are_exact_where_p_is_0_or_1(api, case):
    DC.check_exact(api, case)


@pytest.mark.parametrize('case', DC.CASES, ids=DC.CASE_IDS)
def test_two_runs_give_identical_bits(api, case):
    DC.check_repeat(api, case)


def test_reference_fixture(api):
    DC.check_fixture(api)


def test_reference_gradient_is_the_float64_autograd_of_torch_bce():
    """the float64 FORMULA the gradient is held against equals float64 autograd of binary_cross_entropy's mean over the foreground
    cells, away from p = 0 and p = 1 (where torch's backward is its epsilon formula, not a derivative)"""
    case = DC.by_name('odd3')
    gt, lab, probs = DC.reference(case)
    BN, D, h, w = probs.shape
    p = probs.double().clamp(1e-6, 1 - 1e-6).requires_grad_()
    fg = (lab >= 0)[:, None].expand_as(p)
    tgt = (torch.arange(D).view(1, D, 1, 1) == lab.long()[:, None]).double()
    bce = torch.nn.functional.binary_cross_entropy(p, tgt, reduction='none')
    ((bce * fg).sum() / int((lab >= 0).sum()) * float(np.float32(0.37))).backward()
    want = DC.grad_ref64(p.detach(), lab, 0.37)
    assert float(want.abs().max()) > 0
    assert ((p.grad - want).abs() <= 1e-12 * want.abs()).all()


def test_empty_batch_zeroes_the_outputs(api):
    """BN == 0: 0, no launch, out_f and out_i zeroed (real buffers: the entry clears them through the runtime)"""
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    out_f, out_i, dummy = torch.full((2,), 7.5), torch.full((1,), 9, dtype=torch.int32), torch.zeros(4)
    assert api.lib.fbbev_depth_loss_fwd(p(dummy), 0, 8, 8, 4, p(dummy), 12, 0.0, 1.0, p(dummy), p(out_f), p(out_i), None, 0, None) == 0
    assert (out_f == 0).all() and (out_i == 0).all()


def test_a_flagged_depth_net_on_cpu_tensors_runs_the_default_route():
    case = DC.by_name('odd3')
    gt, lab, probs = DC.reference(case)
    plain, flagged = DC._net(case), DC._net(case)
    flagged.fused_depth_loss = True
    from fb_bev_amd.depth_net import CM_DepthNet
    assert CM_DepthNet(use_dcn=False, in_channels=8, mid_channels=8, fused_depth_loss=True).fused_depth_loss is True
    assert plain.fused_depth_loss is False
    a = plain.get_depth_loss(gt[None], probs[None])['loss_depth']
    b = flagged.get_depth_loss(gt[None], probs[None])['loss_depth']
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and float(a) > 0
