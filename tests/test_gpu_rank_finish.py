"""The high-digit-first rank build (FBBEV_RANK_FINISH=1) on the MI355X against the two-pass segmented route (=0) and the oracle: the
cases of tests/rank_finish_cases.py (small two-digit grids forced onto the segmented plan with FBBEV_RANK_SEG=2, buckets of 64, 65
and several thousand points, one-voxel samples, P = 0, the depth-threshold entry, garbage workspaces, two builds on one workspace)
and one capture-and-replay of the build from camera tensors.  tests/test_emu_rank_finish.py runs the same cases on the CPU emulator.

The product reads both knobs once per process, so each route builds everything in a fresh child process, checks it against the
oracle there and hands its index tensors back; the routes are then compared here, bit for bit."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def builds(tmp_path_factory):
    out = {}
    for route in ('0', '1'):
        path = str(tmp_path_factory.mktemp('rank_finish') / f'route{route}.pt')
        code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import rank_finish_cases as T\n'
                'T.gpu_build_all(%r)\n') % (ROOT, os.path.join(ROOT, 'tests'), path)
        env = dict(os.environ, FBBEV_RANK_SEG='2', FBBEV_RANK_FINISH=route)
        r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (route, r.stdout[-1000:], r.stderr[-3000:])
        assert 'built 8' in r.stdout
        out[route] = torch.load(path)
    return out


def test_each_route_equals_the_oracle_in_its_child_process(builds):
    assert set(builds['0']) == set(builds['1']) and len(builds['1']) == 8


def test_finish_route_equals_two_pass_route_bit_for_bit(builds):
    names = ('ranks_bev', 'ranks_depth', 'ranks_feat', 'interval_starts', 'interval_lengths', 'interval_rank')
    for case, new in builds['1'].items():
        old = builds['0'][case]
        for k, (a, b) in enumerate(zip(new, old)):
            assert a.dtype == torch.int32 and torch.equal(a, b), (case, names[k])
    assert builds['1']['empty_B2'][0].numel() == 0
    assert builds['1']['one_voxel_B1'][4].tolist() == [9000]
    assert builds['1']['geom_replay'][0].numel() > 1000
