"""fbbev_image_prep on the CPU emulator: the kernel source of fb_bev_amd/csrc/image_prep_kernels.h and its launcher, unedited, at
the cases of tests/image_prep_cases.py, through tests/emu/emu_capi.lib().  Bit equality with the numpy restatement (which
tests/test_image_prep_host.py holds to PIL) and with the fixture the reference class wrote."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_prep_cases as C  # noqa: E402


@pytest.fixture(scope='module')
def api():
    return C.EmuApi()


def test_limits_are_the_planner_s(api):
    from fb_bev_amd import image_prep as IP
    assert C.limits_of(api) == IP.limits()


@pytest.mark.parametrize('case', C.SMALL, ids=C.SMALL_IDS)
def test_cases(api, case):
    C.check(api, case)


@pytest.mark.parametrize('variant', C.VARIANTS[1:], ids=lambda v: 'cl%d_swap%d_canvas%d' % tuple(int(x) for x in v))
@pytest.mark.parametrize('name', C.VARIANT_CASES)
def test_layouts_swap_and_canvas(api, name, variant):
    C.check(api, C.by_name(name), *variant)


@pytest.mark.parametrize('name', ('batch7_strided', 'size_%dx%d' % (2 * C.TW + 3, 2 * C.TH + 3)))
def test_two_runs_give_identical_bits(api, name):
    C.check_repeat(api, C.by_name(name))


def test_reference_fixture(api):
    C.check_fixture(api)
