"""GPU: the device-resident sequence state of the history fusion (TemporalHistoryFusion(stream_state=True)) and its hipGraph replay
(graphed.GraphedStream) against the default eager route.  Every comparison is bit equality: the routes run the same tap function,
the same fmaf chains, the same convolution kernels and single-rounded bias arithmetic."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'history_fusion_seq4.npz')

STARTS = [[True, False], [False, False], [False, True], [False, False], [False, False], [True, True]]
# ring type, T, C, (Z, Y, X): an odd frame tail | ten 16-byte groups per voxel, a ragged last x chunk, the four-frame unroll | bf16 storage
CASES = [(torch.float32, 3, 16, (4, 10, 12)), (torch.float16, 16, 80, (2, 6, 30)), (torch.bfloat16, 3, 80, (4, 10, 12))]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _modules(dev, dt, T, C, grid, n, seed=3):
    """n modules on the same random weights (non-trivial running statistics), all on the default route."""
    from fb_bev_amd.history_fusion import TemporalHistoryFusion
    Z, Y, X = grid
    dx = [0.8, 0.8, 0.8]
    bx = [-X * 0.4 + 0.4, -Y * 0.4 + 0.4, -Z * 0.4 + 0.4]              # the ego sits at the grid's centre: bx - dx/2 = -size/2
    torch.manual_seed(seed)
    mods = [TemporalHistoryFusion(dx, bx, single_bev_num_channels=C, history_cat_num=T, history_dtype=dt).to(dev).eval()
            for _ in range(n)]
    _randomise(mods[0], seed)
    for m in mods[1:]:
        m.load_state_dict(mods[0].state_dict())
    assert all(m._voxel_major() for m in mods)
    return mods


def _randomise(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for seq in (m.history_keyframe_time_conv, m.history_keyframe_cat_conv):
            seq[0].weight.copy_(torch.randn(seq[0].weight.shape, generator=g) * 0.2)
            seq[0].bias.copy_(torch.randn(seq[0].bias.shape, generator=g) * 0.1)
            seq[1].weight.copy_(torch.rand(seq[1].weight.shape, generator=g) + 0.5)
            seq[1].bias.copy_(torch.randn(seq[1].bias.shape, generator=g) * 0.1)
            seq[1].running_mean.copy_(torch.randn(seq[1].running_mean.shape, generator=g) * 0.1)
            seq[1].running_var.copy_(torch.rand(seq[1].running_var.shape, generator=g) + 0.5)


class _Frames:
    """Frame i of a two-sample stream: a random current volume, ego / bda of the recorded sequence (cycled), STARTS (cycled); a sample
    that starts a sequence gets a new sequence id."""

    def __init__(self, dev, C, grid, seed=5):
        self.z, self.dev, self.C, self.grid = np.load(G), dev, C, grid
        self.g = torch.Generator().manual_seed(seed)
        self.sid = [0, 1]

    def __call__(self, i, starts=None):
        Z, Y, X = self.grid
        k = i % 4
        curr = torch.randn(2, self.C, Y, X, Z, generator=self.g).to(self.dev)
        bda = torch.from_numpy(self.z[f'f{k}.bda']).to(self.dev)
        st = STARTS[i % 6] if starts is None else starts
        self.sid = [s + 10 if st[b] else s for b, s in enumerate(self.sid)]
        metas = [dict(sequence_group_idx=self.sid[b], start_of_sequence=st[b], curr_to_prev_ego_rt=self.z[f'f{k}.ego'][b])
                 for b in range(2)]
        return curr, metas, bda


def _vt(cam_params, context, depth, img_metas=None, mlvl_feats=None):
    """Stand-in view transformation: the volume is handed over as `context`."""
    return context


def _same(a, b, what):
    assert torch.equal(a.history_sweep_time, b.history_sweep_time), what
    assert torch.equal(a.history_forward_augs, b.history_forward_augs), what
    assert torch.equal(a.history_seq_ids, b.history_seq_ids), what
    assert torch.equal(a.history_as_reference(), b.history_as_reference()), what


@pytest.mark.parametrize('dt,T,C,grid', CASES)
def test_stream_state_and_replay_equal_the_eager_route(dev, dt, T, C, grid):
    """Six frames -- frames 2..5 are captured / replayed, a restart of one sample and of both happens under replay -- on three
    modules: default eager, stream_state eager, GraphedStream.  Output, ring, sweep times and forward augmentations after every
    frame."""
    from fb_bev_amd.graphed import GraphedStream
    eager, stream, graphed = _modules(dev, dt, T, C, grid, 3)
    stream.stream_state = True
    g = GraphedStream(_vt, graphed)
    assert graphed.stream_state
    frames = _Frames(dev, C, grid)
    dummy = torch.zeros(1, device=dev)
    with torch.no_grad():
        for i in range(6):
            curr, metas, bda = frames(i)
            o0 = eager.fuse_history(curr, metas, bda)
            o1 = stream.fuse_history(curr, metas, bda)
            o2 = g([], curr, dummy, metas, bda)
            assert o0.shape == o1.shape == o2.shape
            assert torch.equal(o1, o0) and torch.equal(o2, o0), i
            _same(stream, eager, i)
            _same(graphed, eager, i)
    assert stream._st_ok and eager._st is None                          # the device-state route ran / the default route never touched it
    assert all(gr is not None for gr in g._graphs)                      # both parities were captured


def test_replayed_frame_does_not_synchronise(dev):
    from fb_bev_amd.graphed import GraphedStream
    dt, T, C, grid = CASES[2]
    eager, graphed = _modules(dev, dt, T, C, grid, 2)
    g = GraphedStream(_vt, graphed)
    frames = _Frames(dev, C, grid)
    dummy = torch.zeros(1, device=dev)
    with torch.no_grad():
        for i in range(5):
            curr, metas, bda = frames(i)
            exp = eager.fuse_history(curr, metas, bda)
            if i == 4:                                                  # frames 2 and 3 captured: this one only replays
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode('error')
            try:
                out = g([], curr, dummy, metas, bda)
            finally:
                torch.cuda.set_sync_debug_mode('default')
            assert torch.equal(out, exp), i


def test_new_weights_and_reset_capture_again(dev):
    """load_state_dict of other weights after frame 3 (both graphs exist): the next frames run eagerly on the new folded weights and
    are captured again; likewise after reset().  Equal to the eager module given the same weights at the same points."""
    from fb_bev_amd.graphed import GraphedStream
    dt, T, C, grid = CASES[0]
    eager, graphed, other = _modules(dev, dt, T, C, grid, 3)
    _randomise(other, 11)
    g = GraphedStream(_vt, graphed)
    frames = _Frames(dev, C, grid)
    dummy = torch.zeros(1, device=dev)
    with torch.no_grad():
        for i in range(15):
            if i == 4:
                assert all(gr is not None for gr in g._graphs)
                eager.load_state_dict(other.state_dict())
                graphed.load_state_dict(other.state_dict())
            if i == 10:
                assert all(gr is not None for gr in g._graphs)          # frames 4-5 eager, 6-7 captured, 8-9 replayed
                eager.reset()
                graphed.reset()
            curr, metas, bda = frames(i, starts=[False, False] if i == 10 else None)   # a first frame without a start: sweep 1
            exp = eager.fuse_history(curr, metas, bda)
            out = g([], curr, dummy, metas, bda)
            assert torch.equal(out, exp), i
            _same(graphed, eager, i)
            if i in (4, 5, 10, 11):
                assert g._graphs == [None, None], i
        assert all(gr is not None for gr in g._graphs)


def test_switching_the_mode_between_frames(dev):
    """Two device-state frames, two default-route frames (the mirrors carry the state over), two device-state frames again (the state
    is refreshed from the mirrors): equal to an all-eager run throughout."""
    dt, T, C, grid = CASES[2]
    eager, stream = _modules(dev, dt, T, C, grid, 2)
    frames = _Frames(dev, C, grid)
    with torch.no_grad():
        for i in range(6):
            stream.stream_state = i not in (2, 3)
            curr, metas, bda = frames(i)
            exp = eager.fuse_history(curr, metas, bda)
            out = stream.fuse_history(curr, metas, bda)
            assert torch.equal(out, exp), i
            _same(stream, eager, i)
            assert stream._st_ok == stream.stream_state, i
    assert stream.begin_frame(2, grid, dev) is None                     # the direct slot is not part of the device-state route
    stream.fused_x3 = True
    with pytest.raises(ValueError, match='stream_state'):
        stream.fuse_history(*frames(6))


def test_detector_stream_graph_equals_the_default_detector(dev):
    """FBOCC(execution=dict(stream_graph=True)): five frames of predict_occupancy -- two eager, two captured, one replayed, with the
    real FBViewTransform inside the graphs -- equal the same model without the knob: class ids, then (after a reset) raw
    probabilities."""
    from test_gpu_full_model import _inputs, _small_model
    base = _small_model(dev).eval()
    m = _small_model(dev, dict(stream_graph=True)).eval()
    m.load_state_dict(base.state_dict())
    img_inputs, metas, _, _ = _inputs(dev, 2)
    ego = torch.eye(4); ego[0, 3] = 1.5; ego[1, 3] = -0.7
    with torch.no_grad():
        for raw in (False, True):
            for i in range(5):
                mt = [dict(d, curr_to_prev_ego_rt=ego) for d in metas(i == 0)]
                frame = [img_inputs[0] + 0.1 * i] + img_inputs[1:]
                exp = base.predict_occupancy(frame, mt, return_raw_occ=raw)
                got = m.predict_occupancy(frame, mt, return_raw_occ=raw)
                assert torch.equal(got, exp), (raw, i)
            assert all(gr is not None for gr in m._stream._graphs)
            assert torch.equal(m.history.history_as_reference(), base.history.history_as_reference())
            base.reset_history()
            m.reset_history()
        m.history.fused_x3 = True
        with pytest.raises(ValueError, match='stream_state'):
            m.predict_occupancy(img_inputs, metas(True))
