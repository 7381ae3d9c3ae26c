"""hipGraph replay of an inference call with fixed shapes.

The fused view-transformation path has no host synchronisation and no shape-dependent control flow (the point / interval
counts stay on the device, the index cache is keyed on the device), so a whole forward can be captured ONCE into a hipGraph
and replayed: at small batches the eager path is bound by the ~40 kernel launches of a forward, not by the GPU
(FB-OCC shapes, B=1: 0.98 ms eager, 0.45 ms replayed -- tools/scope_table.py).  The reference has no counterpart (its
voxel-ranking step synchronises with the host four times, view_transformer.py:547-605).

    g = Graphed(model, cam_params, context, depth)        # warm-up + capture with these example inputs
    out = g(cam_params2, context2, depth2)                # copies the inputs into the captured buffers, replays

Inputs are arbitrarily nested lists / tuples / dicts of tensors (non-tensor leaves must stay equal to the captured ones);
tensor shapes, dtypes and devices are fixed by the example.  The returned tensors are the graph's own output buffers,
overwritten by the next call (`clone=True` returns copies).

A camera stream (B = 1 inference, the deployment case) is the view transformation FOLLOWED by the history step of every frame, and
that step carries state from frame to frame.  `GraphedStream` replays the pair:

    g = GraphedStream(view_transform, history)            # TemporalHistoryFusion; its stream_state is switched on
    out = g(cam_params, context, depth, img_metas, bda)   # fused (B, Cout, Y, X, Z) volume, valid until the next call

The sequence state lives on the device (TemporalHistoryFusion(stream_state=True)), so a frame is the host bookkeeping, one small
pinned upload, the copies of the tensor inputs and one replay.  The history ring alternates between two buffers: two graphs, one
per parity.  Nothing is warmed up on fake data and no state is rolled back: the first two frames of a stream run eagerly on the
device-state route (allocator, folded weights, index workspaces), the next two are each captured and then replayed, and from then
on frames only replay.  The graphs are dropped and built again the same way when the input shapes / dtypes / devices, the number of
samples, the folded weights, the module's mode, the ring's type change or the history is reset.
"""
import torch


def _flatten(x, out):
    if isinstance(x, torch.Tensor):
        out.append(x)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _flatten(v, out)
    elif isinstance(x, dict):
        for k in sorted(x):
            _flatten(x[k], out)
    else:
        out.append(('const', x))
    return out


def _rebuild(x, it):
    if isinstance(x, torch.Tensor):
        return next(it)
    if isinstance(x, (list, tuple)):
        return type(x)(_rebuild(v, it) for v in x)
    if isinstance(x, dict):
        return {k: _rebuild(x[k], it) for k in sorted(x)}
    next(it)
    return x


class Graphed:
    def __init__(self, fn, *args, warmup=3, clone=False, **kwargs):
        leaves = _flatten((args, kwargs), [])
        tensors = [t for t in leaves if isinstance(t, torch.Tensor)]
        if not tensors or not all(t.is_cuda for t in tensors):
            raise ValueError('Graphed needs GPU tensors (hipGraph capture)')
        self._fn, self._clone = fn, clone
        self._spec = leaves
        self._static = [t.clone() if isinstance(t, torch.Tensor) else t for t in leaves]
        it = iter(self._static)
        self._args, self._kwargs = _rebuild((args, kwargs), it)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(max(1, warmup)):              # allocator warm-up and lazily built caches, outside the capture
                fn(*self._args, **self._kwargs)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self._out = fn(*self._args, **self._kwargs)

    def __call__(self, *args, **kwargs):
        leaves = _flatten((args, kwargs), [])
        if len(leaves) != len(self._spec):
            raise ValueError('Graphed: the call does not have the structure of the captured example')
        for new, ref, dst in zip(leaves, self._spec, self._static):
            if isinstance(ref, torch.Tensor):
                if not isinstance(new, torch.Tensor) or new.shape != ref.shape or new.dtype != ref.dtype or new.device != ref.device:
                    raise ValueError('Graphed: tensor shapes / dtypes / devices are fixed by the captured example')
                if new.data_ptr() != dst.data_ptr():
                    dst.copy_(new)
            elif new != ref:
                raise ValueError('Graphed: non-tensor arguments must equal the captured ones')
        self.graph.replay()
        if not self._clone:
            return self._out
        return _rebuild(self._out, iter([t.clone() if isinstance(t, torch.Tensor) else t for t in _flatten(self._out, [])]))


class GraphedStream:
    def __init__(self, view_transform, history, clone=False):
        """view_transform(cam_params, context, depth, img_metas=..., mlvl_feats=...) -> (B, C, Y, X, Z) volume (FBViewTransform in eval
        mode); history: the TemporalHistoryFusion that fuses it.  clone=True returns copies instead of the graphs' own buffers."""
        history._stream_check()
        history.stream_state = True
        self._vt, self._h, self._clone = view_transform, history, clone
        self._key = None
        self._drop()

    def _drop(self):
        self._graphs, self._outs, self._nxt = [None, None], [None, None], [None, None]
        self._pool = self._static = self._spec = self._args = self._bufs_id = self._grid = self._fold = None
        self._warm = 0                     # consecutive frames on the device-state route since the graphs were dropped

    def _config_key(self, leaves, n_samples):
        h = self._h
        sig = tuple((tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else None for t in leaves)
        return (sig, n_samples, h._fold_key(), h._epoch, h.training, h.stream_state, h.history_dtype, h.history_compute,
                h.ring_layout, h.use_mfma_convs, h.do_history)

    def _buffers(self):
        h = self._h
        return None if h._bufs is None or h._st is None else (id(h._st), h._bufs[0].data_ptr(), h._bufs[1].data_ptr())

    def __call__(self, cam_params, context, depth, img_metas, bda, mlvl_feats=None):
        h = self._h
        h._stream_check()
        leaves = _flatten((cam_params, context, depth, bda, mlvl_feats), [])
        key = self._config_key(leaves, len(img_metas))
        if key != self._key:
            self._drop()
            self._key = key
        graphs = h.stream_state and not h.training and not torch.is_grad_enabled() and context.is_cuda
        if self._bufs_id is not None and self._bufs_id != self._buffers():       # the ring or the state was re-allocated behind the graphs
            self._drop()
        if not graphs or self._warm < 2 or h.history_bev is None or not h._st_ok:
            # eager: the warm-up frames of a stream, and every frame the device-state route does not take
            if self._bufs_id is not None:
                self._drop()
            out = h.fuse_history(self._vt(cam_params, context, depth, img_metas=img_metas, mlvl_feats=mlvl_feats), img_metas, bda)
            self._warm = self._warm + 1 if h._st_ok else 0
            return out
        if self._static is None:
            self._spec = leaves
            self._static = [t.clone() if isinstance(t, torch.Tensor) else t for t in leaves]
            self._args = _rebuild((cam_params, context, depth, bda, mlvl_feats), iter(self._static))
            self._pool = torch.cuda.graph_pool_handle()            # the two graphs never run at the same time: one pool
        else:
            for new, ref, dst in zip(leaves, self._spec, self._static):
                if isinstance(ref, torch.Tensor):
                    if new.data_ptr() != dst.data_ptr():
                        dst.copy_(new)
                elif new != ref:
                    raise ValueError('GraphedStream: non-tensor arguments must equal the captured ones')
        p = 0 if h.history_bev.data_ptr() != h._bufs[0].data_ptr() else 1        # the ring buffer this frame writes
        h._stream_host(img_metas, context.device)                  # assertion, mirrors, the one upload: before capture / replay
        if self._graphs[p] is None:
            cam_s, ctx_s, depth_s, bda_s, mlvl_s = self._args
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._pool), torch.no_grad():        # one stream: a linear graph
                vol = self._vt(cam_s, ctx_s, depth_s, img_metas=img_metas, mlvl_feats=mlvl_s)
                out, nxt = h._stream_device(vol, bda_s)
                out = out.permute(0, 1, 3, 4, 2)                   # (B,Cout,Y,X,Z) view, as fuse_history returns it
            _, _, Y, X, Z = vol.shape
            self._graphs[p], self._outs[p], self._nxt[p], self._grid = g, out, nxt, (Z, Y, X)
            self._bufs_id, self._fold = self._buffers(), h._folded_pair()       # (the folded weights the graphs read stay alive)
        self._graphs[p].replay()
        h._stream_commit(self._nxt[p], self._grid)
        return self._outs[p].clone() if self._clone else self._outs[p]
