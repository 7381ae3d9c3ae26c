"""fbbev_occ_classes on the CPU emulator: the kernel source of fb_bev_amd/csrc/occ_kernels.h and its launcher, unedited, at the
shapes of tests/occ_cases.py.  Class bytes against the parent's softmax / argmax / shuffle chain, the confusion table against a numpy
bincount; guard bytes, read-only inputs and the added-to table are checked by occ_cases.run / check_hist."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_cases as OC  # noqa: E402


@pytest.fixture(scope='module')
def api():
    return OC.EmuApi()


@pytest.mark.parametrize('case', OC.CASES, ids=OC.CASE_IDS)
def test_classes_equal_the_parent_chain(api, case):
    OC.check_classes(api, case)


@pytest.mark.parametrize('kind', ['uniform', 'skewed'])
@pytest.mark.parametrize('case', OC.CASES, ids=OC.CASE_IDS)
def test_hist_equals_bincount(api, case, kind):
    OC.check_hist(api, case, kind)
