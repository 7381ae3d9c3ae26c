"""fbbev_occ_fscore_counts on the CPU emulator: the kernel source of fb_bev_amd/csrc/occ_fscore_kernels.h and its launcher, unedited,
at the shapes of tests/occ_fscore_cases.py.  The four counts per frame against the definition written out in numpy (float64 coordinates,
square root, `<`); guard words, read-only maps and the added-to counts are checked by occ_fscore_cases.run.  The reference grid runs
once, with the planted pattern."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_fscore_cases as FC  # noqa: E402

SMALL = [c for c in FC.CASES if c['name'] != FC.BIG]
PAIRS = [(c, p) for c in SMALL for p in FC.PATTERNS] + [(FC.CASES[FC.CASE_IDS.index(FC.BIG)], 'planted')]


@pytest.fixture(scope='module')
def api():
    return FC.EmuApi()


@pytest.mark.parametrize('case,pattern', PAIRS, ids=[f'{c["name"]}-{p}' for c, p in PAIRS])
def test_counts_equal_the_definition(api, case, pattern):
    FC.check_counts(api, case, pattern)


@pytest.mark.parametrize('case', [SMALL[0], SMALL[2]], ids=[SMALL[0]['name'], SMALL[2]['name']])
def test_void_lists_and_null_mask(api, case):
    FC.check_voids_and_null_mask(api, case)


def test_one_cell_apart_is_decided_by_rounding(api):
    FC.check_rounding_decides(api, SMALL[2])


def test_depth_33_is_refused(api):
    import numpy as np
    c = FC.REFUSED
    ids = np.full((c['B'], c['X'], c['Y'], c['Z']), FC.FREE, dtype=np.uint8)
    tab = FC.tables(c, 0.4, 0.4, FC.VOXEL, full_cube=False)
    counts = api.dev(np.full((c['B'], 4), 5, dtype=np.int32))
    code = api.call(api.dev(ids), api.dev(ids), None, FC.void_words([17, 255]), [api.dev(t) for t in tab['sq']], api.dev(tab['offsets']),
                    tab['R'], tab['T_acc'], tab['T_cmpl'], counts)
    assert code == FC.E_UNSUPPORTED
    assert (counts == 5).all()
