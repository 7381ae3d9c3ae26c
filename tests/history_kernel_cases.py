"""Case table, float64 reference, input builders, bounds and adapters for the temporal history fusion kernels, shared by the GPU test
(tests/test_gpu_history_kernels.py, through fb_bev_amd._capi) and the emulator test (tests/test_emu_history_kernels.py, through
tests/emu/emu_capi.py): every exported fbbev_history_* entry at the smallest shapes at which each of its code paths exists.  It is laid
out like tests/msda_kernel_cases.py.

The reference is written from fbocc.py's arithmetic, not from the kernels.
  warp (`taps`, `blend`)   fbocc.py:205 rt_flow @ (x, y, z, 1); :208-209 normalise; grid_sample's un-normalise (align_corners=True).  The
      reference itself evaluates that chain in fp32, so it is restated in numpy.float32, one operation per step, left to right: numpy's
      float32 operations are single correctly rounded operations like fbbev_mul / fbbev_add (rt.h), hence floors, tap indices and the
      three-factor tap weights (wx * wy) * wz are reproducible bit for bit.  The 8 taps are then blended in float64 with zero padding: a
      tap outside the grid, or a coordinate that is NaN or beyond 1e9, contributes 0.
  convolutions (`conv_ref`)  out = relu(b2 + sum_t W2_t . relu(W1 . x_t + b1_t)) in float64.  compute 'bf16' restates the route's operand
      roundings (weights, frames and the ReLU'd intermediate to bf16); fp32 and the split-operand route (x3) round no operand.
  flow: the five-matrix product in float64 (oracle.history_oracle.rt_flow).  prologue: the host recurrence of fbocc.py:220-261, 279-281,
  313-314 in fp32 (sweep values are small integers: exact).  frame_vm: a transpose and one nearest-even rounding.

Layer A, exact.  Inputs for which a correct kernel has no rounding to make, so the output equals float64 bit for bit (integer view for
16-bit rings).  Warps: every grid axis 2^k + 1 long and a dyadic flow (axis permutation / flip, translations in quarters): `taps`
asserts that the fp32 chain then equals the float64 chain.  Tap weights are multiples of 1/64; with small-integer data the fmaf chain
is exact in fp32.  A 16-bit ring takes integers up to 100 (bf16) / 2000 (fp16) so that blends need up to 13 / 17 bits: the ONE
nearest-even rounding of the store is exercised (`warp_data` plants half subnormals and +-65504 for fp16; `table_claims` asserts that
inexact blends and exact ties occur).  Convolutions: integer frames in [-2, 2], W1 in {-1, 0, 1}, small integer biases and W2:
|intermediate| <= 2 C + 8: 8 significant bits at C <= 80 (the bf16 route's operand type; `conv_ref` asserts it on the actual
intermediates), so all routes equal float64.  The fused / step entries take even-integer history with flows of half and whole voxels: ring and intermediate stay integers.

Layer B, real values (grids that are no 2^k + 1, a real rotation, sub-voxel translations, partial exit from the grid, randn data),
componentwise against float64 inside bounds derived here, u = 2^-24, gamma_n = n u / (1 - n u):
  warp       the taps and weights are reproduced, the kernel's only error is its 8-step fmaf chain: gamma_8 S, S = sum_k |a_k w_k|.  A
             16-bit ring adds the store's rounding of a value that may sit e = gamma_8 S off the reference: half an ulp of the ring
             type at |ref| + e (bf16: 2^(floor(log2 v) - 8); fp16: 2^(max(floor(log2 v), -14) - 11)) -- `ring_half_ulp`.
  conv fp32  GEMM 1 is a k-ordered chain of C fused multiply-adds started from the bias (or the bias added last): e1 = gamma_(C+1) S1,
             S1 = |b1| + sum |W1| |x|.  ReLU is 1-Lipschitz: |dy| <= e1.  GEMM 2: sum |W2| dy + gamma_(T1 C + 1) (|b2| + sum |W2| (|y| + dy)).
  conv bf16  the same with the operands the route defines and u' = 2^-23 per accumulation step (the 16-bit MFMA's block accumulate is not
             documented to round to nearest at every step; one ulp per step covers truncation), plus, for every intermediate whose
             float64 value lies within e1 of a bf16 rounding boundary (or of 0), the other neighbour: dy = e1 + 2 ulp_bf16(y); all other
             intermediates are the same bf16 number on both sides: dy = 0.
  conv x3    v = hi + lo + r with hi = bf16(v), lo = bf16(v - hi): |r| <= 2^-16 |v| whatever the rounding direction (fp16 parts: less).
             GEMM 1 splits W1 only: e1 = (2^-16 + gamma'_(C+1)) S1.  GEMM 2 computes a_hi b_hi + a_lo b_hi + a_hi b_lo = a b - a_lo b_lo -
             (remainders): |a_lo b_lo| <= 2^-16 |a b|, so 3 * 2^-16 (1 + 2^-8) S2 + gamma'_(T1 C + 1) S2 + sum |W2| e1.
Every layer-B check prints `[observed] <case>: max err / bound`; no constant is taken from the code under test.

`table_claims` restates the launch geometry (chunks, bands, bricks, channels per workgroup, frames per batch, the LDS box) and asserts
that every case reaches the path its name claims, and lists the template instantiation each case launches.

Plain Python, numpy and CPU torch only; the adapters import their library on first use.
"""
import ctypes
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from da_kernel_cases import observed  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3          # include/fbbev.h
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ET = {F32: 0, BF16: 1, F16: 2}
TYPES = {'f32': F32, 'bf16': BF16, 'f16': F16}
U = 2.0 ** -24
f32 = np.float32
KNOB_YB, KNOB_WARP = 'FBBEV_HISTORY_VM_YB', 'FBBEV_HISTORY_WARP'           # read on every call
KNOBS_ONCE = ('FBBEV_HISTORY_VM_TU', 'FBBEV_HX3_WAVES', 'FBBEV_HISTORY_STEP_WAVES')   # read once per process in every build


def gamma(n, u=U):
    return n * u / (1 - n * u)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


# ------------------------------------------------------------------------------------------------------------------ reference: warp
def _chain(m, fx, fy, fz, dims, dt):
    """the sampling coordinate of fbocc.py in precision dt, one operation per step, left to right -> [ix, iy, iz]"""
    out = []
    one, two = dt(1), dt(2)
    with np.errstate(all='ignore'):
        for r, size in enumerate(dims):
            g = ((m[4 * r] * fx + m[4 * r + 1] * fy) + m[4 * r + 2] * fz) + m[4 * r + 3]
            g = g / dt(size - 1) * two - one
            out.append((g + one) / two * dt(size - 1))
    return out


def taps(flow, Z, Y, X, dyadic=False):
    """flow (4, 4) fp32 -> idx (8, N) int64 (0 where the tap is outside), w (8, N) float64 (the fp32 weight; 0 outside), ok (8, N); voxel
    n = (z Y + y) X + x; tap order x fastest, then y, then z.  dyadic: asserts that the fp32 chain equals the float64 chain."""
    m = np.asarray(flow, dtype=f32).reshape(16)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    fx, fy, fz = (a.reshape(-1).astype(f32) for a in (x, y, z))
    c = _chain(m, fx, fy, fz, (X, Y, Z), f32)
    assert all(a.dtype == f32 for a in c)
    if dyadic:
        c64 = _chain(m.astype(np.float64), fx.astype(np.float64), fy.astype(np.float64), fz.astype(np.float64), (X, Y, Z), np.float64)
        with np.errstate(all='ignore'):                             # (a coordinate that is NaN or beyond 1e9 contributes 0 on both sides)
            f32ok = np.all([np.abs(a) < 1.0e9 for a in c], axis=0)
            f64ok = np.all([np.abs(b) < 1.0e9 for b in c64], axis=0)
        assert np.array_equal(f32ok, f64ok) and all(np.array_equal(a.astype(np.float64)[f32ok], b[f32ok]) for a, b in zip(c, c64)), \
            'the fp32 chain is not exact'
    with np.errstate(all='ignore'):
        fin = np.ones(fx.shape, bool)
        for a in c:
            fin &= np.abs(a) < f32(1.0e9)                       # NaN fails
        fl = [np.floor(a) for a in c]
        w1 = [a - b for a, b in zip(c, fl)]
        w0 = [(b + f32(1)) - a for a, b in zip(c, fl)]
        i0 = [np.where(fin, b, f32(-2)).astype(np.int64) for b in fl]
    idx, w, ok = [], [], []
    for k in range(8):
        sx, sy, sz = k & 1, (k >> 1) & 1, k >> 2
        cx, cy, cz = i0[0] + sx, i0[1] + sy, i0[2] + sz
        good = (cx >= 0) & (cx < X) & (cy >= 0) & (cy < Y) & (cz >= 0) & (cz < Z)
        with np.errstate(all='ignore'):
            wk = ((w1[0] if sx else w0[0]) * (w1[1] if sy else w0[1])) * (w1[2] if sz else w0[2])
        assert wk.dtype == f32
        idx.append(np.where(good, (cz * Y + cy) * X + cx, 0))
        w.append(np.where(good, wk, f32(0)).astype(np.float64))
        ok.append(good)
    return np.stack(idx), np.stack(w), np.stack(ok)


def blend(a, tp):
    """a (..., N) float64, tp = taps(...) -> (out (..., N), S (..., N)): the 8 taps blended in float64 with zero padding, and the same sum
    on absolute values"""
    idx, w, ok = tp
    out = np.zeros(a.shape[:-1] + (idx.shape[1],))
    S = np.zeros_like(out)
    for k in range(8):
        v = np.where(ok[k], a[..., idx[k]], 0.0) * w[k]
        out += v
        S += np.abs(v)
    return out, S


def warp_planes_ref(hist, flows, grid, dyadic=False):
    """hist (B, CH, N) tensor, flows (B, 4, 4) -> (ref, S) float64 arrays (B, CH, N)"""
    Z, Y, X = grid
    h = hist.double().numpy()
    res = [blend(h[b], taps(flows[b].numpy(), Z, Y, X, dyadic)) for b in range(h.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def warp_rows_ref(hist, flows, grid, dyadic=False):
    """voxel-major: hist (B, T, N, C) -> (ref, S) float64 (B, T, N, C)"""
    Z, Y, X = grid
    h = hist.double().numpy().transpose(0, 1, 3, 2)
    res = [blend(h[b], taps(flows[b].numpy(), Z, Y, X, dyadic)) for b in range(h.shape[0])]
    return (np.stack([r[0] for r in res]).transpose(0, 1, 3, 2).copy(), np.stack([r[1] for r in res]).transpose(0, 1, 3, 2).copy())


def to_type(a64, dt):
    """float64 array -> tensor of the ring type: ONE nearest-even rounding.  The value must be an fp32 number (layer A; layer B goes
    through bounds), so that the two steps double -> float -> dt round once."""
    t = torch.from_numpy(np.ascontiguousarray(a64))
    f = t.float()
    assert torch.equal(f.double(), t), 'not an fp32 number'
    return f.to(dt)


def ring_half_ulp(v, dt):
    """half an ulp of the ring type at magnitude v (float64 array); 0 for fp32 (stored as is)"""
    if dt == F32:
        return np.zeros_like(v)
    e = np.floor(np.log2(np.maximum(v, 1e-300)))
    return 2.0 ** (e - 8) if dt == BF16 else 2.0 ** (np.maximum(e, -14) - 11)


def warp_bound(ref, S, dt):
    e = gamma(8) * S
    return e + ring_half_ulp(np.abs(ref) + e, dt)


# ------------------------------------------------------------------------------------------------------------------ reference: convolutions
def _bf16(a64):
    return torch.from_numpy(np.ascontiguousarray(a64)).float().to(BF16).double().numpy()


def conv_ref(x, w1, bias1, w2, bias2, compute='f32', want_bound=False, exact_bits=None):
    """x (B, T1, C, N) tensor of the ring type (channel-major), w1 (C, C), bias1 (B, T1, C), w2 (Cout, T1 C), bias2 (Cout) -> out (B, Cout, N)
    float64 [, bound].  compute 'f32' | 'bf16' | 'x3'.  exact_bits: asserts that every intermediate has at most that many significant
    bits (layer A: the route's operand type holds it)."""
    B, T1, C, N = x.shape
    Cout = w2.shape[0]
    X = x.double().numpy()
    W1, W2 = w1.double().numpy(), w2.double().numpy().reshape(Cout, T1, C)
    b1, b2 = bias1.double().numpy(), bias2.double().numpy()
    if compute == 'bf16':
        X, W1, W2 = _bf16(X), _bf16(W1), _bf16(W2)
    pre = np.einsum('oc,btcn->bton', W1, X) + b1[..., None]
    y = np.maximum(pre, 0.0)
    if compute == 'bf16':
        yq = _bf16(y)
    else:
        yq = y
    if exact_bits is not None:
        m, _ = np.frexp(y)
        assert np.array_equal(m * 2.0 ** exact_bits, np.round(m * 2.0 ** exact_bits)), f'an intermediate needs more than {exact_bits} bits'
    out = np.maximum(np.einsum('otc,btcn->bon', W2, yq) + b2[None, :, None], 0.0)
    if not want_bound:
        return out
    u = U if compute == 'f32' else 2.0 ** -23
    S1 = np.einsum('oc,btcn->bton', np.abs(W1), np.abs(X)) + np.abs(b1)[..., None]
    if compute == 'x3':
        e1 = (2.0 ** -16 + gamma(C + 1, u)) * S1
    else:
        e1 = gamma(C + 1, u) * S1
    if compute == 'bf16':
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(pre), 1e-300))) - 7)
        frac = np.abs(y - yq) / ulp
        near = (0.5 - frac) * ulp <= e1
        dy = np.where(pre > e1, np.where(near, e1 + 2 * ulp, 0.0), np.where(pre > -e1, 3 * e1, 0.0))
    else:
        dy = e1
    S2 = np.einsum('otc,btcn->bon', np.abs(W2), np.abs(yq) + dy) + np.abs(b2)[None, :, None]
    bound = np.einsum('otc,btcn->bon', np.abs(W2), dy) + gamma(T1 * C + 1, u) * S2
    if compute == 'x3':
        bound = bound + 3 * 2.0 ** -16 * (1 + 2.0 ** -8) * S2
    return out, bound


# ------------------------------------------------------------------------------------------------------------------ flows
def _flow(rot, t):
    m = torch.eye(4)
    m[:3, :3] = torch.tensor(rot, dtype=F32)
    m[:3, 3] = torch.tensor(t, dtype=F32)
    return m


I3 = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
QT = [[0.0, -1.0, 0], [1.0, 0, 0], [0, 0, 1.0]]                  # a quarter turn about z: x' = -y + tx, y' = x + ty


def flow_named(name, grid):
    Z, Y, X = grid
    c, s = math.cos(0.2), math.sin(0.2)
    if name == 'shift':            # quarters of a voxel on every axis: every tap weight a multiple of 1/64, none 0 or 1
        return _flow(I3, [1.25, -0.5, 0.25])
    if name == 'quarter':          # the grid's rows become columns; part of a non-square grid leaves
        return _flow(QT, [Y - 1 + 0.25, -0.75, -0.5])
    if name == 'flipz':
        return _flow([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]], [0.5, Y - 1 - 0.25, Z - 1 - 0.25])
    if name == 'outside':          # the whole sample lands outside the grid
        return _flow(I3, [1024.0, 0.0, 0.0])
    if name == 'nan':              # NaN and 1e12 coordinates: zeros
        m = _flow(I3, [float('nan'), 0.0, 0.0])
        m[1, 3] = 1.0e12
        return m
    if name == 'half':             # half a voxel in x, whole voxels else: even integers blend to integers
        return _flow(I3, [0.5, 1.0, 0.0])
    if name == 'quarter_int':
        return _flow(QT, [Y - 1.0, 0.0, 0.0])
    if name == 'real_shift':
        return _flow(I3, [3.25, -1.5, 0.3])
    if name == 'real_rot':         # a real rotation, sub-voxel translation, partial exit
        return _flow([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], [4.0, -6.0, -0.2])
    if name == 'real_rot_small':
        return _flow([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], [1.3, -0.7, 0.15])
    raise KeyError(name)


def flows_for(names, grid):
    return torch.stack([flow_named(n, grid) for n in names])


# ------------------------------------------------------------------------------------------------------------------ data
def warp_data(shape, dt, seed, real=False, even=False, ch_axis=-1):
    """Layer A: integers (bf16: to 100, fp16: to 2000, fp32: to 4).  fp16: channels c % 4 == 1 hold half subnormals (multiples of 2^-24
    up to 1000 of them) and channels c % 4 == 2 carry +-65504 among the integers -- taps never mix channels, so every blend stays a
    multiple of one quantum within 24 bits.  even: even integers in [-2, 2] (the fused entries).  real: randn in the type."""
    g = torch.Generator().manual_seed(seed)
    if real:
        return torch.randn(shape, generator=g).to(dt)
    if even:
        return (torch.randint(-1, 2, shape, generator=g) * 2).float().to(dt)
    hi = {F32: 4, BF16: 100, F16: 2000}[dt]
    t = torch.randint(-hi, hi + 1, shape, generator=g).float()
    if dt == F16:
        tc = t.movedim(ch_axis, 0)                                      # a view: channel first
        sub = torch.randint(-1000, 1001, tc.shape, generator=g).float() * 2.0 ** -24
        big = torch.where(torch.rand(tc.shape, generator=g) < 0.1, torch.where(torch.rand(tc.shape, generator=g) < 0.5, 65504.0, -65504.0), tc)
        tc[1::4] = sub[1::4]
        tc[2::4] = big[2::4]
    return t.to(dt)


def padded(shape, dt, pad, fill=float('nan'), tail=8):
    """a (B, ...) view with a batch stride `pad` elements longer than dense, inside a 64-byte aligned buffer filled with `fill`, `tail`
    more elements behind the last sample (long enough where a check wants an overshoot of a row reported, not a fault)"""
    B, inner = shape[0], int(np.prod(shape[1:]))
    base = torch.full((B * (inner + pad) + tail,), fill, dtype=dt)
    strides = [1] * len(shape)
    for i in range(len(shape) - 2, 0, -1):
        strides[i] = strides[i + 1] * shape[i + 1]
    strides[0] = inner + pad
    return base.as_strided(tuple(shape), tuple(strides))


def put(view, t):
    view.copy_(t)
    return view


# ------------------------------------------------------------------------------------------------------------------ adapters
class _Abi:
    """the C ABI of the history family on one library; tensors go through `to` (CPU views keep their strides and offset on the device)"""

    def call(self, entry, *args):
        conv = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        code = getattr(self.lib(), entry)(*conv, self.stream())
        self.sync()
        return code

    def whole(self, d):
        """the CPU copy of the whole buffer behind a device view"""
        return self.back(d._base if d._base is not None else d)

    @staticmethod
    def f3(v):
        return ctypes.cast((ctypes.c_float * 3)(*[float(x) for x in v]), ctypes.c_void_p)


class GpuApi(_Abi):
    """libfbbev_hip.so as fb_bev_amd._capi loads and declares it, on cuda:0"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi
        self.c = _capi
        self.device = torch.device('cuda:0')

    def lib(self):
        return self.c.lib()

    def stream(self):
        return self.c._stream()

    def sync(self):
        torch.cuda.synchronize()

    def to(self, t):
        base = t._base if t._base is not None else t
        d = base.to(self.device)
        return d if t._base is None else d.as_strided(t.shape, t.stride(), t.storage_offset())

    def back(self, t):
        torch.cuda.synchronize()
        return t.cpu()


class EmuApi(_Abi):
    """tests/emu/emu_capi.py: the same launchers and kernels compiled for the CPU"""
    name = 'emu'

    def __init__(self):
        sys.path.insert(0, os.path.join(HERE, 'emu'))
        import emu_capi
        self.E = emu_capi

    def lib(self):
        return self.E.lib()

    def stream(self):
        return None

    def sync(self):
        pass

    def to(self, t):
        base = t._base if t._base is not None else t
        d = base.clone()
        return d if t._base is None else d.as_strided(t.shape, t.stride(), t.storage_offset())

    def back(self, t):
        return t.clone()


class knob:
    """a knob that the library reads on every call, set for the duration of a check"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------------------------ comparisons
def _exact(tag, what, got, exp):
    """got, exp tensors of one type: equal bit for bit"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (tag, what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = (bits(got) != bits(exp)).sum().item()
    if bad:
        d = (got.double() - exp.double()).abs()
        where = np.unravel_index(int(torch.nan_to_num(d, nan=float('inf')).argmax()), tuple(got.shape))
        raise AssertionError(f'{tag}: {bad} of {exp.numel()} elements of {what} differ from float64, max|diff| = {d.max().item():.3e} at {where}')


def _inside(tag, what, got, ref, bound):
    g = got.double().numpy()
    assert not np.isnan(g).any(), f'{tag}: NaN left in {what}'
    assert g.shape == ref.shape == bound.shape, (tag, what, g.shape, ref.shape, bound.shape)
    err = np.abs(g - ref)
    ratio = (err / np.maximum(bound, 1e-300)).max()
    observed(f'{tag} {what}: max err {err.max():.3e} / bound -> ratio {ratio:.3f}')
    assert ratio <= 1.0, f'{tag}: {what} leaves the derived bound: ratio {ratio:.3f}, max err {err.max():.3e}'


def _nan_guard(tag, whole, touched):
    """whole: flat CPU copy of a buffer, touched: boolean mask of the elements the entry may write: all others are still NaN"""
    rest = whole.view(-1)[~touched.view(-1)]
    assert torch.isnan(rest.float()).all(), f'{tag}: wrote outside its output'


def _mask_of(view):
    """boolean mask over the flat base of a CPU view: the elements the view covers"""
    base = view._base
    m = torch.zeros(base.numel(), dtype=torch.bool)
    m.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
    return m


# ------------------------------------------------------------------------------------------------------------------ planar warp
G_A, G_B, G_LDS = (2, 9, 17), (4, 7, 11), (9, 33, 33)              # 306, 308 and 9801 voxels


def _pw(CH, dt, flows, grid=G_A, lds=False, seed=0):
    return dict(CH=CH, dt=dt, flows=tuple(flows), grid=grid, lds=lds, seed=seed)


WARP_CASES = {}
for _n, _dt in TYPES.items():
    for _ch in (1, 3, 4, 9, 37):
        WARP_CASES[f'warp_{_n}_ch{_ch}'] = _pw(_ch, _n, ('shift', 'quarter', 'flipz'), seed=_ch)
    WARP_CASES[f'warp_{_n}_ch4_outside_and_nan'] = _pw(4, _n, ('outside', 'nan'), seed=50)
    WARP_CASES[f'warp_{_n}_ch9_lds_staged_fallback_empty'] = _pw(9, _n, ('shift', 'quarter', 'outside'), grid=G_LDS, lds=True, seed=60)
WARP_REAL = {f'warp_{_n}_ch{_ch}_real': _pw(_ch, _n, ('real_shift', 'real_rot_small'), grid=G_B, seed=70 + _ch)
             for _n in TYPES for _ch in (9, 37)}
WARP_REAL.update({f'warp_{_n}_ch9_lds_real': _pw(9, _n, ('real_shift', 'real_rot'), grid=(8, 20, 30), lds=True, seed=80) for _n in ('f32', 'f16')})


def planar_geometry(B, CH, grid):
    """the gather kernel's launch restated: (n_chunks, cpb, n_groups)"""
    zyx = grid[0] * grid[1] * grid[2]
    n_chunks = -(-zyx // 256)
    cpb = 64
    while cpb > 8 and B * n_chunks * -(-CH // cpb) < 4096:
        cpb >>= 1
    return n_chunks, cpb, -(-CH // cpb)


def lds_geometry(B, CH, grid, flows):
    """the brick kernel's launch restated -> None (the gather kernel runs) or per sample the set of brick kinds {'staged', 'fallback', 'empty'}"""
    Z, Y, X = grid
    if Z * Y * X < 4096 or X < 16:
        return None
    TX = 64
    while TX // 2 >= X:
        TX //= 2
    BZ = min(Z, 8)
    TY = max(1, min(Y, 4096 // (BZ * TX)))
    kinds = []
    for fl in flows:
        m = np.asarray(fl, dtype=f32).reshape(16)
        seen = set()
        for z0 in range(0, Z, BZ):
            for y0 in range(0, Y, TY):
                for x0 in range(0, X, TX):
                    x1, y1, z1 = min(x0 + TX, X) - 1, min(y0 + TY, Y) - 1, min(z0 + BZ, Z) - 1
                    cs = [(f32(a), f32(b), f32(c)) for c in (z0, z1) for b in (y0, y1) for a in (x0, x1)]
                    co = [_chain(m, np.array([a]), np.array([b]), np.array([c]), (X, Y, Z), f32) for a, b, c in cs]
                    co = np.array(co)[:, :, 0]                       # (8 corners, 3 axes)
                    if not (np.abs(co) < 1.0e9).all():
                        seen.add('fallback')
                        continue
                    bs = []
                    for a, size in enumerate((X, Y, Z)):
                        lo = max(int(np.floor(co[:, a].min())) - 1, 0)
                        hi = min(int(np.floor(co[:, a].max())) + 2, size - 1)
                        bs.append(hi - lo + 1 if hi >= lo else 0)
                    if bs[0] <= 80 and 80 * bs[1] * bs[2] <= 12288:
                        seen.add('empty' if 0 in bs else 'staged')
                    else:
                        seen.add('fallback')
        kinds.append(seen)
    return kinds


def check_warp(api, name, real=False):
    p = (WARP_REAL if real else WARP_CASES)[name]
    dt, grid, CH = TYPES[p['dt']], p['grid'], p['CH']
    Z, Y, X = grid
    N, B = Z * Y * X, len(p['flows'])
    flows = flows_for(p['flows'], grid)
    data = warp_data((B, CH, N), dt, p['seed'], real=real, ch_axis=1)
    hist = put(padded((B, CH, N), dt, 24), data)                       # a padded input batch stride, NaN in the padding
    big = torch.full((B, CH + 5, N), float('nan'), dtype=dt)           # the output is channels 3 .. 3 + CH of a larger buffer
    out = big[:, 3:3 + CH]
    d_hist, d_flow, d_out = api.to(hist), api.to(flows), api.to(out)
    with knob(**{KNOB_WARP: 'lds' if p['lds'] else None}):
        code = api.call('fbbev_history_warp_e', d_hist, hist.stride(0), d_flow, B, CH, Z, Y, X, d_out, out.stride(0), ET[dt])
    assert code == 0, (name, code)
    got = api.back(d_out)
    ref, S = warp_planes_ref(data, flows, grid, dyadic=not real)
    if real:
        _inside(name, 'out', got, ref, warp_bound(ref, S, dt))
    else:
        _exact(name, 'out', got, to_type(ref, dt))
    _nan_guard(name, api.whole(d_out), _mask_of(out))
    for b, f in enumerate(p['flows']):
        if f in ('outside', 'nan'):
            assert (got[b].float() == 0).all(), f'{name}: sample {b} ({f}) is not all zeros'


# ------------------------------------------------------------------------------------------------------------------ voxel-major warps
G_VM80, G_VM16, G_VMB = (2, 5, 33), (2, 5, 65), (3, 7, 11)


def _vm(dt, C, T, grid, flows=('shift', 'quarter'), yb=2, seed=0, src=None):
    return dict(dt=dt, C=C, T=T, grid=grid, flows=tuple(flows), yb=yb, seed=seed, src=src)


WARP_VM_CASES = {}
for _n in TYPES:
    for _c in ((16,) if _n == 'f32' else (16, 80)):
        for _t in (1, 2, 3, 5) + ((4,) if _n == 'f16' and _c == 80 else ()):        # fp16: four frames per batch
            WARP_VM_CASES[f'warp_vm_{_n}_c{_c}_t{_t}'] = _vm(_n, _c, _t, G_VM80 if _c == 80 else G_VM16, seed=_c + _t)
WARP_VM_CASES['warp_vm_f16_c16_t3_outside_and_nan'] = _vm('f16', 16, 3, G_VM16, flows=('outside', 'nan'), seed=7)
WARP_VM_CASES['warp_vm_bf16_c80_t2_default_bands'] = _vm('bf16', 80, 2, G_VM80, yb=None, seed=8)
WARP_VM_REAL = {f'warp_vm_{_n}_c{_c}_t3_real': _vm(_n, _c, 3, G_VMB, flows=('real_shift', 'real_rot_small'), seed=90)
                for _n, _c in (('f32', 16), ('bf16', 80), ('f16', 80))}
WARP_SRC_CASES = {f'warp_vm_src_{_n}_t{_t}': _vm(_n, 16, _t, G_VM16, flows=('shift', 'quarter', 'flipz', 'shift'), seed=20 + _t, src=(0, 1, 2, 3))
                  for _n in TYPES for _t in (1, 2, 3, 5)}
WARP_SRC_CASES['warp_vm_src_bf16_c80_t3'] = _vm('bf16', 80, 3, G_VM80, flows=('quarter', 'shift'), seed=30, src=(1, 0))


def vm_geometry(dt, C, T, grid, yb=None, tu=None):
    """the voxel-major warp's launch restated -> dict(groups, items, n_xc, last_chunk, YB, nyb, last_band, TU, batches, tail_twice)"""
    Z, Y, X = grid
    VE = 4 if dt == 'f32' else 8
    groups = C // VE
    items = X * groups
    n_xc = -(-items // 256)
    YB = max(1, min(Y, 128 // Z if yb is None else yb))
    nyb = -(-Y // YB)
    TU = tu or (4 if dt == 'f16' else 2)
    return dict(groups=groups, items=items, n_xc=n_xc, last_chunk=items - 256 * (n_xc - 1), YB=YB, nyb=nyb, last_band=Y - YB * (nyb - 1),
                TU=TU, batches=-(-T // TU), tail_twice=T % TU != 0 and T > 0, instantiation=f'k_history_warp_vm<{ET[TYPES[dt]]}, {TU}, 1>')


def _sentinel(shape, dt, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(-3, 4, shape, generator=g).float().to(dt)


def check_warp_vm(api, name, real=False, table=None):
    p = (table or (WARP_VM_REAL if real else WARP_VM_CASES))[name]
    dt, grid, C, T = TYPES[p['dt']], p['grid'], p['C'], p['T']
    Z, Y, X = grid
    N, B = Z * Y * X, len(p['flows'])
    flows = flows_for(p['flows'], grid)
    data = warp_data((B, T, N, C), dt, p['seed'], real=real)
    src, ring_in = data, data
    nxt = padded((B, T + 1, N, C), dt, 64)                             # the next ring: slot 0 holds the current frame and is left alone
    slot0 = _sentinel((B, N, C), dt, p['seed']) if p['src'] is None else warp_data((B, N, C), dt, p['seed'] + 1)
    nxt[:, 0] = slot0
    out = nxt[:, 1:]
    if p['src'] is not None:                                           # a started sample samples the current frame; its old ring is not read
        src, ring_in = data.clone(), data.clone()
        for b, f in enumerate(p['src']):
            if f:
                ring_in[b] = float('nan')
                src[b] = slot0[b][None]
    hist = put(padded((B, T, N, C), dt, 32), ring_in)
    d_hist, d_flow, d_nxt = api.to(hist), api.to(flows), api.to(nxt)
    d_out = d_nxt[:, 1:]
    with knob(**{KNOB_YB: p['yb']}):
        if p['src'] is None:
            code = api.call('fbbev_history_warp_vm', d_hist, hist.stride(0), d_flow, B, T, C, Z, Y, X, d_out, out.stride(0), ET[dt])
        else:
            flags = torch.tensor(p['src'], dtype=torch.int32)
            code = api.call('fbbev_history_warp_vm_src', d_hist, hist.stride(0), d_nxt, nxt.stride(0), api.to(flags), d_flow, B, T, C,
                            Z, Y, X, d_out, out.stride(0), ET[dt])
    assert code == 0, (name, code)
    got = api.back(d_nxt)
    ref, S = warp_rows_ref(src, flows, grid, dyadic=not real)
    if real:
        _inside(name, 'ring', got[:, 1:], ref, warp_bound(ref, S, dt))
    else:
        _exact(name, 'ring', got[:, 1:].contiguous(), to_type(ref, dt))
    _exact(name, 'slot 0 (must be left alone)', got[:, 0].contiguous(), slot0)
    _nan_guard(name, api.whole(d_nxt), _mask_of(nxt))
    for b, f in enumerate(p['flows']):
        if f in ('outside', 'nan'):
            assert (got[b, 1:].float() == 0).all(), f'{name}: sample {b} ({f}) is not all zeros'


# ------------------------------------------------------------------------------------------------------------------ frame_vm
FRAME_CASES = {}
for _i, (_N, _inner) in enumerate(((1, 1), (63, 1), (63, 3), (64, 4), (65, 5), (65, 1), (200, 8), (200, 1))):
    for _j, _c in enumerate((8, 40, 48, 80, 512)):
        if _N in (65, 200) or (_i + _j) % 2 == 0:
            _n = ('f32', 'bf16', 'f16')[(_i + _j) % 3]
            FRAME_CASES[f'frame_vm_{_n}_n{_N}_c{_c}_inner{_inner}'] = dict(dt=_n, N=_N, C=_c, inner=_inner, seed=_i * 5 + _j)
for _n in TYPES:
    FRAME_CASES.setdefault(f'frame_vm_{_n}_n65_c80_inner5', dict(dt=_n, N=65, C=80, inner=5, seed=99))
    FRAME_CASES.setdefault(f'frame_vm_{_n}_n200_c48_inner1', dict(dt=_n, N=200, C=48, inner=1, seed=98))


def check_frame_vm(api, name):
    p = FRAME_CASES[name]
    dt, N, C, inner, B = TYPES[p['dt']], p['N'], p['C'], p['inner'], 2
    g = torch.Generator().manual_seed(p['seed'])
    curr = torch.randn(B, C, N, generator=g)
    if dt == F16:
        curr[:, :, ::3] *= 2.0 ** -16                                  # half subnormals after the rounding
    # a padded slot stride; inner > 1: seven slots of NaN behind each sample's, so that a row index with its two factors mixed up (at most
    # (N / inner) ^ 2 < 8 N here) lands in the guard and is reported
    slot = padded((B, N, C), dt, 40 + (7 * N * C if inner > 1 else 0))
    d_slot = api.to(slot)
    code = api.call('fbbev_history_frame_vm', api.to(curr), B, C, N, inner, d_slot, slot.stride(0), ET[dt])
    assert code == 0, (name, code)
    got = api.back(d_slot)
    rows = curr.transpose(1, 2)                                        # (B, N, C): row i of the planes
    if inner > 1:                                                      # plane position i = p * inner + z lands in row z * (N / inner) + p
        rows = rows.reshape(B, N // inner, inner, C).transpose(1, 2).reshape(B, N, C)
    _exact(name, 'slot', got.contiguous(), rows.to(dt).contiguous())   # one nearest-even rounding
    _nan_guard(name, api.whole(d_slot), _mask_of(slot))


# ------------------------------------------------------------------------------------------------------------------ flow and prologue
DX_A, LOWER_A = (0.5, 0.5, 0.25), (-40.0, -40.0, -1.0)              # dyadic: inv(feat2bev) . feat2bev = I exactly
DX_B, LOWER_B = (0.4, 0.4, 0.4), (-40.0, -40.0, -1.0)


def _rigid(g, B):
    a = (torch.rand(B, generator=g) - 0.5) * 0.6
    m = torch.eye(4).repeat(B, 1, 1)
    m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1] = torch.cos(a), -torch.sin(a), torch.sin(a), torch.cos(a)
    m[:, :3, 3] = torch.randn(B, 3, generator=g)
    return m


def _bda(g, B, flip=True):
    m = _rigid(g, B)[:, :3, :3].clone()
    if flip:
        m[1::2] = m[1::2] * torch.tensor([1.0, -1.0, 1.0])
    return m.contiguous()


def _fwd(bda):
    m = torch.zeros(bda.shape[0], 4, 4)
    m[:, :3, :3] = bda
    m[:, 3, 3] = 1.0
    return m


def flow_bound(hist_augs, ego, bda, dx, lower):
    """Componentwise: rt_flow = A1 A2 A3 A4 A5 with A1 = inv(feat2bev) (entries 1/dx, -t/dx: one rounding each), A4 = inv(bda) by
    cofactors (a 2x2 minor: 3 roundings on |ab| + |cd|; the determinant: 3 minors, 3 products, 2 sums; one division: at most 12 u of
    the ABSOLUTE cofactor form adj|bda| / |det|, and the same again through the determinant's own absolute form <= that of the entry's
    row) and four products of 4-term dot products (gamma_4 each, nested: gamma_16): 16 + 1 + 24 = 41 u, stated as gamma_48 of the product
    of the absolute matrices."""
    d = torch.tensor(dx, dtype=torch.float64)
    lo = torch.tensor(lower, dtype=torch.float64)
    B = bda.shape[0]
    inv = torch.zeros(4, 4, dtype=torch.float64)
    f2b = torch.zeros(4, 4, dtype=torch.float64)
    for k in range(3):
        inv[k, k], inv[k, 3] = 1 / d[k], (lo[k] / d[k]).abs()
        f2b[k, k], f2b[k, 3] = d[k], lo[k].abs()
    inv[3, 3] = f2b[3, 3] = 1
    m = bda.double()
    ab = m.abs()
    adj = torch.zeros(B, 3, 3, dtype=torch.float64)
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (c + 1) % 3, (c + 2) % 3, (r + 1) % 3, (r + 2) % 3
            adj[:, r, c] = ab[:, r1, c1] * ab[:, r2, c2] + ab[:, r1, c2] * ab[:, r2, c1]
    det = torch.linalg.det(m).abs()
    absdet = (ab[:, 0, :] * adj[:, :, 0]).sum(-1)
    fi = torch.zeros(B, 4, 4, dtype=torch.float64)
    fi[:, :3, :3] = adj / det[:, None, None] * (absdet / det)[:, None, None]
    fi[:, 3, 3] = 1
    prod = inv @ hist_augs.double().abs() @ ego.double().abs() @ fi @ f2b
    # + the reference's own error: its float64 inverses go through an LU factorisation, whose error is normwise, not componentwise
    return gamma(48) * prod + 2.0 ** -40 * prod.amax((1, 2), keepdim=True)


def _call_flow(api, hist_augs, ego, bda, dx, lower):
    B = bda.shape[0]
    d_flow = api.to(torch.full((B, 4, 4), float('nan')))
    code = api.call('fbbev_history_flow', api.to(hist_augs), api.to(ego), api.to(bda), api.f3(dx), api.f3(lower), B, d_flow)
    assert code == 0, code
    return api.back(d_flow)


FLOW_CASES = {'flow_b1': 1, 'flow_b65_second_workgroup': 65}


def check_flow(api, name):
    from oracle import history_oracle as H
    B = FLOW_CASES[name]
    g = torch.Generator().manual_seed(B)
    # identity ego motion, the history's augmentation = the frame's (a flip for every other sample), dyadic voxels: flow = I exactly
    bda = torch.eye(3).repeat(B, 1, 1)
    bda[1::2, 1, 1] = -1.0
    bda[2::3, 0, 0] = -1.0
    flow = _call_flow(api, _fwd(bda), torch.eye(4).repeat(B, 1, 1), bda, DX_A, LOWER_A)
    assert torch.equal(flow, torch.eye(4).repeat(B, 1, 1)), f'{name}: identity ego motion does not give flow = I'      # (values: -0 == 0)
    # real motion, flipped bda
    hist_augs, ego, bda = _fwd(_bda(g, B)), _rigid(g, B), _bda(g, B)
    flow = _call_flow(api, hist_augs, ego, bda, DX_B, LOWER_B)
    # the kernel takes dx and the lower bound as fp32 numbers: the reference takes the same numbers
    dx32 = torch.tensor(DX_B, dtype=F32).double()
    exp = H.rt_flow(hist_augs.double(), H.forward_aug_matrix(bda.double()), ego.double(), dx32, torch.tensor(LOWER_B, dtype=F32).double() + dx32 / 2)
    _inside(name, 'flow', flow, exp.numpy(), flow_bound(hist_augs, ego, bda, DX_B, LOWER_B).numpy())


PROLOGUE_CASES = {'prologue_t0': 0, 'prologue_t1': 1, 'prologue_t16': 16}
FREQ = 0.5


def check_prologue(api, name):
    """two consecutive calls on one state; B = 4 holds every flag value"""
    T, C, B = PROLOGUE_CASES[name], 80, 4
    g = torch.Generator().manual_seed(40 + T)
    b1, wt = torch.randn(C, generator=g), torch.randn(C, generator=g)
    augs_h = _fwd(_bda(g, B))
    sweep_h = torch.randint(0, 6, (B, T), generator=g).float()
    d_augs, d_sweep = api.to(augs_h.clone()), api.to(sweep_h.clone() if T else torch.zeros(1))
    for i, fl in enumerate(([0, 1, 2, 3], [3, 0, 0, 1])):
        flags = torch.tensor(fl, dtype=torch.int32)
        ego, bda = _rigid(g, B), _bda(g, B)
        fwd = _fwd(bda)
        start, empty = (flags & 1).bool(), (flags & 2).bool()
        augs_h[empty], sweep_h[empty] = fwd[empty], 0.0                 # :227-238
        sweep_h = sweep_h + 1                                           # :252
        sweep_h[start], augs_h[start] = 0.0, fwd[start]                 # :253-261
        used_exp = augs_h.clone()
        sw = torch.cat([torch.zeros(B, 1), sweep_h], dim=1)             # :279-281
        bias_exp = b1[None, :] + (sw * FREQ).reshape(B * (T + 1), 1) * wt[None, :]      # three single-rounded fp32 operations
        sweep_h, augs_h = sw[:, :-1].contiguous(), fwd.clone()          # :313-314
        d_used, d_flow, d_bias = (api.to(torch.full(s, float('nan'))) for s in ((B, 4, 4), (B, 4, 4), (B * (T + 1), C)))
        code = api.call('fbbev_history_stream_prologue', api.to(flags), api.to(ego), api.to(bda), api.to(b1), api.to(wt), api.f3(DX_B),
                        api.f3(LOWER_B), FREQ, B, T, C, d_augs, d_sweep, d_used, d_flow, d_bias)
        assert code == 0, (name, code)
        _exact(name, f'call {i}: augmentations used', api.back(d_used), used_exp)
        _exact(name, f'call {i}: bias rows', api.back(d_bias), bias_exp)
        _exact(name, f'call {i}: augmentation state', api.back(d_augs), augs_h)
        if T:
            _exact(name, f'call {i}: sweep state', api.back(d_sweep), sweep_h)
        # rt_flow: the bits of fbbev_history_flow on the augmentations used (pinned against float64 by check_flow)
        _exact(name, f'call {i}: rt_flow', api.back(d_flow), _call_flow(api, used_exp, ego, bda, DX_B, LOWER_B))


# ------------------------------------------------------------------------------------------------------------------ convolutions
def conv_data(B, T1, C, Cout, N, dt, seed, real=False):
    """-> x (B, T1, C, N) in the ring type, w1 (C, C), bias1 (B, T1, C), w2 (Cout, T1 C), bias2 (Cout); layer A: module docstring"""
    g = torch.Generator().manual_seed(seed)
    if real:
        return (torch.randn(B, T1, C, N, generator=g).to(dt), torch.randn(C, C, generator=g) / math.sqrt(C),
                torch.randn(B, T1, C, generator=g) * 0.5, torch.randn(Cout, T1 * C, generator=g) / math.sqrt(T1 * C),
                torch.randn(Cout, generator=g) * 0.5)
    w1 = torch.randint(-1, 2, (C, C), generator=g).float()
    w1[:, 0] = 1.0                                                      # no all-zero row (the fp16 x3 route scales rows by their largest entry)
    w2 = torch.randint(-3, 4, (Cout, T1 * C), generator=g).float()
    return (torch.randint(-2, 3, (B, T1, C, N), generator=g).float().to(dt), w1, torch.randint(-8, 9, (B, T1, C), generator=g).float(),
            w2, torch.randint(-8, 9, (Cout,), generator=g).float())


def _cv(route, dt, C, Cout, T1, N, seed=0):
    return dict(route=route, dt=dt, C=C, Cout=Cout, T1=T1, N=N, seed=seed)


# route: 'gen' k_history_conv (planes, no workspace) | 'reg' k_history_conv_t planes | 'vm' k_history_conv_t voxel-major |
#        'bf16' / 'bf16_vm' k_history_conv_bf16 | 'x3' k_history_conv_bf16x3
CONV_CASES = {}
for _n in TYPES:
    for _i, (_r, _c, _co, _t1, _N) in enumerate((('gen', 32, 16, 2, 65), ('gen', 128, 128, 1, 63), ('gen', 16, 48, 17, 130), ('gen', 32, 16, 1, 1),
                                                 ('reg', 16, 16, 17, 130), ('reg', 80, 80, 2, 65), ('reg', 80, 80, 1, 1), ('reg', 16, 16, 2, 63))):
        CONV_CASES[f'conv_{_r}_{_n}_c{_c}_o{_co}_t{_t1}_n{_N}'] = _cv(_r, _n, _c, _co, _t1, _N, seed=_i)
    for _c in (16, 80):
        for _t1, _N in ((1, 65), (3, 63), (3, 1), (1, 64)):
            for _r in ('vm', 'bf16', 'bf16_vm'):
                CONV_CASES[f'conv_{_r}_{_n}_c{_c}_t{_t1}_n{_N}'] = _cv(_r, _n, _c, _c, _t1, _N, seed=_c + _t1 + _N)
        if _n != 'f32':
            for _t1, _N in ((1, 257), (3, 255), (3, 1), (1, 256)):       # 16 * 8 waves * FBBEV_HX3_NV = 256 voxels per workgroup
                CONV_CASES[f'conv_x3_{_n}_c{_c}_t{_t1}_n{_N}'] = _cv('x3', _n, _c, _c, _t1, _N, seed=_c + _t1 + _N)
CONV_REAL = [k for k, p in CONV_CASES.items() if (p['T1'], p['N']) in ((2, 65), (17, 130), (3, 63), (3, 255), (1, 63))]
ROUTE_COMPUTE = {'gen': 'f32', 'reg': 'f32', 'vm': 'f32', 'bf16': 'bf16', 'bf16_vm': 'bf16', 'x3': 'x3'}


def conv_instantiation(p, nw=8):
    et, mt = ET[TYPES[p['dt']]], p['C'] // 16
    return {'gen': f'k_history_conv<{et}>', 'reg': f'k_history_conv_t<{mt}, {mt}, {et}, false>', 'vm': f'k_history_conv_t<{mt}, {mt}, {et}, true>',
            'bf16': f'k_history_conv_bf16<{mt}, {mt}, {et}, false>', 'bf16_vm': f'k_history_conv_bf16<{mt}, {mt}, {et}, true>',
            'x3': f'k_history_conv_bf16x3<{mt}, {mt}, {et}, 2, {nw}, 1>'}[p['route']]


def _ws(T1, C, Cout, B):
    return torch.zeros((2 + T1) * C * max(C, Cout, 96) + B * T1 * C + 16)


def call_conv(api, route, x, w1, bias1, w2, bias2):
    """x (B, T1, C, N) channel-major CPU tensor: laid out as the route's ring (padded batch stride) -> (code, out (B, Cout, N))"""
    B, T1, C, N = x.shape
    Cout, dt = w2.shape[0], x.dtype
    vm = route in ('vm', 'bf16_vm', 'x3')
    ring = put(padded((B, T1, N, C), dt, 48), x.transpose(2, 3)) if vm else put(padded((B, T1 * C, N), dt, 48), x.reshape(B, T1 * C, N))
    vol = padded((B, Cout, N), F32, 0)                                 # (8 NaN floats behind the last plane)
    d_out = api.to(vol)
    ws = api.to(_ws(T1, C, Cout, B))
    head = (api.to(ring), ring.stride(0), api.to(w1), api.to(bias1.reshape(B * T1, C)), api.to(w2), api.to(bias2), B, T1, C, Cout, N, d_out)
    if route == 'gen':
        code = api.call('fbbev_history_conv_e', *head, None, 0, ET[dt])
    elif route == 'reg':
        code = api.call('fbbev_history_conv_e', *head, ws, ws.numel() * 4, ET[dt])
    elif route == 'vm':
        code = api.call('fbbev_history_conv_vm', *head, ws, ws.numel() * 4, ET[dt])
    elif route in ('bf16', 'bf16_vm'):
        code = api.call('fbbev_history_conv_bf16', *head, ws, ws.numel() * 4, 1 if vm else 0, ET[dt])
    else:
        code = api.call('fbbev_history_conv_bf16x3', *head, ws, ws.numel() * 4, ET[dt])
    _nan_guard(route, api.whole(d_out), _mask_of(vol))
    return code, api.back(d_out)


def check_conv(api, name, real=False):
    p = CONV_CASES[name]
    dt, B = TYPES[p['dt']], 2
    x, w1, bias1, w2, bias2 = conv_data(B, p['T1'], p['C'], p['Cout'], p['N'], dt, p['seed'] + (500 if real else 0), real)
    code, got = call_conv(api, p['route'], x, w1, bias1, w2, bias2)
    assert code == 0, (name, code)
    compute = ROUTE_COMPUTE[p['route']]
    if real:
        ref, bound = conv_ref(x, w1, bias1, w2, bias2, compute, want_bound=True)
        _inside(name + '_real', 'out', got, ref, bound)
    else:
        ref = conv_ref(x, w1, bias1, w2, bias2, 'f32', exact_bits=8)
        assert np.array_equal(ref, conv_ref(x, w1, bias1, w2, bias2, 'bf16'))        # the restated roundings change nothing here
        _exact(name, 'out', got, to_type(ref, F32))


# ------------------------------------------------------------------------------------------------------------------ fused and step entries
def _st(entry, dt, T, grid, flows, chunks=None, yb=None, C=80, seed=0):
    return dict(entry=entry, dt=dt, T=T, grid=grid, flows=tuple(flows), chunks=chunks, yb=yb, C=C, seed=seed)


G_FUSED = (9, 17, 65)          # 128 / 9 = 14 rows per band: two bands, the second three rows; X = 65: a full 64-voxel tile and a 1-voxel tile
STEP_CASES = {
    'fused_vm_bf16_t3': _st('fused', 'bf16', 3, G_FUSED, ('half', 'quarter_int'), seed=1),
    'fused_vm_f16_t1': _st('fused', 'f16', 1, G_FUSED, ('quarter_int', 'half'), seed=2),
    'fused_x3_bf16_z2_t1': _st('fused_x3', 'bf16', 1, (2, 9, 17), ('half', 'quarter_int'), seed=3),
    'fused_x3_f16_z3_t3': _st('fused_x3', 'f16', 3, (3, 9, 17), ('quarter_int', 'half'), seed=4),
    'fused_x3_bf16_z3_t3': _st('fused_x3', 'bf16', 3, (3, 9, 17), ('half', 'outside'), seed=5),
    'fused_x3_f16_z2_t1': _st('fused_x3', 'f16', 1, (2, 9, 17), ('half', 'quarter_int'), seed=6),
    'step_x3_bf16_t3_chunks1': _st('step', 'bf16', 3, G_VM80, ('half', 'quarter_int'), chunks=1, yb=2, seed=7),
    'step_x3_bf16_t3_chunks3': _st('step', 'bf16', 3, G_VM80, ('half', 'quarter_int'), chunks=3, yb=2, seed=8),
    'step_x3_f16_t5_chunks64_clamped': _st('step', 'f16', 5, G_VM80, ('quarter_int', 'half'), chunks=64, yb=2, seed=9),
    'step_x3_f16_t1_c16_chunks3': _st('step', 'f16', 1, G_VM16, ('half', 'quarter_int'), chunks=3, yb=2, C=16, seed=10),
    'step_x3_bf16_t2_chunks0_default': _st('step', 'bf16', 2, G_VM80, ('half', 'quarter_int'), chunks=0, yb=1, seed=11),
}
STEP_REAL = {
    'fused_vm_bf16_t1_real': _st('fused', 'bf16', 1, (2, 7, 11), ('real_shift', 'real_rot_small'), seed=12),
    'fused_x3_f16_t3_real': _st('fused_x3', 'f16', 3, (3, 9, 17), ('real_shift', 'real_rot_small'), seed=13),
    'step_x3_bf16_t3_chunks3_real': _st('step', 'bf16', 3, G_VM80, ('real_shift', 'real_rot_small'), chunks=3, yb=2, seed=14),
}
STEP_GPU_ONLY = ()             # (the two fbbev_history_fused_vm cases at 9 x 17 x 65 take the emulator about 20 s and about a minute: they run there too)
STEP_ENTRY = {'fused': 'fbbev_history_fused_vm', 'fused_x3': 'fbbev_history_fused_x3_vm', 'step': 'fbbev_history_step_x3_vm'}
STEP_COMPUTE = {'fused': 'bf16', 'fused_x3': 'x3', 'step': 'x3'}


def step_geometry(p, step_waves=None):
    """the step entries' launch geometry restated"""
    Z, Y, X = p['grid']
    if p['entry'] == 'fused':
        YB = max(1, min(Y, 128 // Z))
        return dict(n_xc=-(-X // 64), last_tile=X - 64 * ((X - 1) // 64), YB=YB, nyb=-(-Y // YB), last_band=Y - YB * ((Y - 1) // YB),
                    instantiation=f'k_history_fused_bf16<{ET[TYPES[p["dt"]]]}>')
    if p['entry'] == 'fused_x3':
        return dict(n_xt=-(-X // 16), n_yt=-(-Y // 8), over_x=X % 16, over_y=Y % 8, instantiation=f'k_history_fused_x3<{ET[TYPES[p["dt"]]]}>')
    v = vm_geometry(p['dt'], p['C'], p['T'], p['grid'], p['yb'])
    chunks = min(p['chunks'] or 10, v['nyb'])
    nw = 8 if chunks <= 1 else (step_waves or 4)
    segs = []
    for i in range(chunks):
        yb0, yb1 = v['nyb'] * i // chunks, v['nyb'] * (i + 1) // chunks
        segs.append((yb0 * v['YB'], min(yb1 * v['YB'], Y)))
    mt = p['C'] // 16
    return dict(v, chunks=chunks, segments=segs, nw=nw, conv=f'k_history_conv_bf16x3<{mt}, {mt}, {ET[TYPES[p["dt"]]]}, 2, {nw}, 1>')


def check_step(api, name, real=False):
    p = (STEP_REAL if real else STEP_CASES)[name]
    dt, grid, C, T = TYPES[p['dt']], p['grid'], p['C'], p['T']
    Z, Y, X = grid
    N, B = Z * Y * X, len(p['flows'])
    flows = flows_for(p['flows'], grid)
    data = warp_data((B, T, N, C), dt, p['seed'], real=real, even=not real)
    x0, w1, bias1, w2, bias2 = conv_data(B, T + 1, C, C, N, dt, p['seed'] + 100, real)
    curr = x0[:, 0].transpose(1, 2).contiguous()                       # (B, N, C): the current frame, in slot 0 of the next ring
    hist = put(padded((B, T, N, C), dt, 32), data)
    nxt = padded((B, T + 1, N, C), dt, 64, tail=8 * X * C)             # (a band that overshoots Y by up to eight rows reads NaN)
    nxt[:, 0] = curr
    d_nxt = api.to(nxt)
    vol = padded((B, C, N), F32, 0, tail=8 * X)                        # (eight grid rows of NaN behind the last plane)
    d_out = api.to(vol)
    ws = api.to(_ws(T + 1, C, C, B))
    args = [api.to(hist), hist.stride(0), d_nxt, nxt.stride(0), api.to(flows), api.to(w1), api.to(bias1.reshape(B * (T + 1), C)), api.to(w2),
            api.to(bias2), B, T, C, C, Z, Y, X, d_out, ws, ws.numel() * 4, ET[dt]]
    if p['entry'] == 'step':
        args.append(p['chunks'])
    with knob(**{KNOB_YB: p['yb']}):
        code = api.call(STEP_ENTRY[p['entry']], *args)
    assert code == 0, (name, code)
    ring, out = api.back(d_nxt), api.back(d_out)
    # half 1: the ring slots written == the warp reference; slot 0 and the padding untouched
    ref, S = warp_rows_ref(data, flows, grid, dyadic=not real)
    if real:
        _inside(name, 'ring', ring[:, 1:], ref, warp_bound(ref, S, dt))
    else:
        _exact(name, 'ring', ring[:, 1:].contiguous(), to_type(ref, dt))
    _exact(name, 'slot 0 (must be left alone)', ring[:, 0].contiguous(), curr)
    _nan_guard(name, api.whole(d_nxt), _mask_of(nxt))
    _nan_guard(name, api.whole(d_out), _mask_of(vol))
    # half 2: the volume == the convolution reference applied to THAT ring (as the entry wrote it)
    xr = ring.transpose(2, 3).contiguous()                             # (B, T + 1, C, N)
    compute = STEP_COMPUTE[p['entry']]
    if real:
        cref, bound = conv_ref(xr, w1, bias1, w2, bias2, compute, want_bound=True)
        _inside(name, 'volume', out, cref, bound)
    else:
        _exact(name, 'volume', out, to_type(conv_ref(xr, w1, bias1, w2, bias2, 'f32', exact_bits=8), F32))


# ------------------------------------------------------------------------------------------------------------------ knobs read once per process
KNOB_RUNS = {
    # two frames per batch for an fp16 ring: k_history_warp_vm<2, 2, 1>; T = 5 leaves a clamped tail that T = 5 at four per batch does too,
    # T = 2 is an exact batch only here
    ('FBBEV_HISTORY_VM_TU', '2'): [('vm', 'warp_vm_f16_c80_t2'), ('vm', 'warp_vm_f16_c80_t3'), ('vm', 'warp_vm_f16_c16_t5'),
                                    ('step', 'step_x3_f16_t5_chunks64_clamped')],
    # 256-thread workgroups in fbbev_history_conv_bf16x3: k_history_conv_bf16x3<.., NW = 4, ..>, 128 voxels per workgroup
    ('FBBEV_HX3_WAVES', '4'): [('conv', 'conv_x3_bf16_c80_t3_n255'), ('conv', 'conv_x3_f16_c16_t1_n257'), ('conv', 'conv_x3_f16_c80_t3_n1'),
                                ('conv129', 'conv_x3_bf16_c16_t1_n257')],
    # 512-thread convolution workgroups in the pipelined step: NW = 8 on the band segments
    ('FBBEV_HISTORY_STEP_WAVES', '8'): [('step', 'step_x3_bf16_t3_chunks3'), ('step', 'step_x3_f16_t1_c16_chunks3'),
                                         ('step', 'step_x3_f16_t5_chunks64_clamped')],
}


def run_knob(api, name, value):
    """the layer-A cases of one once-per-process knob setting; the caller has set the environment before the library was loaded"""
    assert os.environ.get(name) == value, os.environ.get(name)
    for kind, case in KNOB_RUNS[(name, value)]:
        if kind == 'vm':
            check_warp_vm(api, case)
        elif kind == 'step':
            check_step(api, case)
        elif kind == 'conv':
            check_conv(api, case)
        else:                                                          # N = 129: one voxel past the 128-voxel workgroup of four waves
            p = dict(CONV_CASES[case], N=129)
            x, w1, bias1, w2, bias2 = conv_data(2, p['T1'], p['C'], p['Cout'], 129, TYPES[p['dt']], 77)
            code, got = call_conv(api, 'x3', x, w1, bias1, w2, bias2)
            assert code == 0, code
            _exact(case + '_n129', 'out', got, to_type(conv_ref(x, w1, bias1, w2, bias2, 'f32', exact_bits=8), F32))
        observed(f'{name}={value} {case}: exact')
    return len(KNOB_RUNS[(name, value)])


def knob_child_code(api_class, name, value):
    return ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import history_kernel_cases as T\n'
            'print("ran", T.run_knob(T.%s(), %r, %r))\n') % (ROOT, HERE, api_class, name, value)


# ------------------------------------------------------------------------------------------------------------------ return codes
def check_codes(api):
    """a few codes of the shared operand rule per entry (history_ring_operand in capi.hip: stride below frames x frame: BADARG; a stride
    that is no multiple of VE or a pointer off 16 bytes: UNSUPPORTED; either ring's BADARG comes first), the empty call, and the order
    where two defects coincide.  Everything is rejected before a launch, so dummy pointers do -- except the empty calls, which get real
    NaN-filled outputs that must stay NaN."""
    lib = api.lib()
    P, P8, NULL = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10008), None
    s = api.stream()
    Z, Y, X, T, C = 2, 3, 5, 2, 16
    N = Z * Y * X
    dense = T * N * C
    wv = lambda h, hs, o, os_, c=C, et=1: lib.fbbev_history_warp_vm(h, hs, P, 1, T, c, Z, Y, X, o, os_, et, s)  # noqa: E731
    assert wv(P, 8, P, 0) == E_BADARG
    assert wv(P, 0, P, 8) == E_BADARG
    assert wv(P, dense + 4, P, 0) == E_UNSUPPORTED                     # a stride that is no multiple of 8
    assert wv(P8, 0, P, 0) == E_UNSUPPORTED and wv(P, 0, P8, 0) == E_UNSUPPORTED
    assert wv(P8, 0, P, 8) == E_BADARG                         # misaligned source AND short destination: BADARG first
    assert wv(P, 8, P, 0, c=12) == E_BADARG                    # the rings are checked before C % VE
    assert wv(P, 0, P, 0, c=12) == E_UNSUPPORTED
    assert wv(P, 0, P, 0, et=3) == E_BADARG and wv(NULL, 0, P, 0) == E_BADARG
    src = lambda h, hs, cu, cs, o, os_: lib.fbbev_history_warp_vm_src(h, hs, cu, cs, P, P, 1, T, C, Z, Y, X, o, os_, 1, s)  # noqa: E731
    assert src(P, 8, P, 0, P, 0) == E_BADARG and src(P, 0, P, 8, P, 0) == E_BADARG
    assert src(P, 0, P8, 0, P, 0) == E_UNSUPPORTED and src(P, 0, NULL, 0, P, 0) == E_BADARG
    assert src(P, 8, P8, 0, P, 0) == E_BADARG
    we = lambda hs, os_, et=0: lib.fbbev_history_warp_e(P, hs, P, 1, 3, Z, Y, X, P, os_, et, s)  # noqa: E731
    assert we(3 * N - 1, 0) == E_BADARG and we(0, 3 * N - 1) == E_BADARG and we(0, 0, et=-1) == E_BADARG
    assert lib.fbbev_history_warp_e(P, 0, P, 1, 3, 1, Y, X, P, 0, 0, s) == E_BADARG                 # a size-1 axis
    fr = lambda o, os_, c=C, n=N, inner=1: lib.fbbev_history_frame_vm(P, 1, c, n, inner, o, os_, 1, s)  # noqa: E731
    assert fr(P, N * C - 8) == E_BADARG and fr(P8, 0) == E_UNSUPPORTED and fr(P, N * C + 4) == E_UNSUPPORTED
    assert fr(P, 0, c=520) == E_UNSUPPORTED and fr(P, 0, c=12) == E_UNSUPPORTED and fr(P, 0, inner=4) == E_BADARG
    assert fr(P8, N * C - 8) == E_BADARG
    T1 = 3
    cargs = lambda f, fs, b1=P, c=C, co=C: (f, fs, P, b1, P, P, 1, T1, c, co, N, P)  # noqa: E731
    assert lib.fbbev_history_conv_e(*cargs(P, T1 * C * N - 1), None, 0, 0, s) == E_BADARG
    assert lib.fbbev_history_conv_e(*cargs(P, 0, c=24), None, 0, 0, s) == E_UNSUPPORTED
    assert lib.fbbev_history_conv_e(*cargs(P, 0, b1=P8), None, 0, 0, s) == E_UNSUPPORTED
    assert lib.fbbev_history_conv_e(*cargs(P, T1 * C * N - 1, b1=P8), None, 0, 0, s) == E_BADARG
    for fn, tail in ((lib.fbbev_history_conv_vm, (1,)), (lib.fbbev_history_conv_bf16, (1, 1)), (lib.fbbev_history_conv_bf16x3, (1,))):
        assert fn(*cargs(P, T1 * C * N - 8), P, 1 << 20, *tail, s) == E_BADARG, fn
        assert fn(*cargs(P8, 0), P, 1 << 20, *tail, s) == E_UNSUPPORTED, fn
        assert fn(*cargs(P, T1 * C * N + 4), P, 1 << 20, *tail, s) == E_UNSUPPORTED, fn
        assert fn(*cargs(P, 0, c=32, co=32), P, 1 << 20, *tail, s) == E_UNSUPPORTED, fn          # not 16 or 80: before the ring
        assert fn(*cargs(P, T1 * C * N - 8, c=32, co=32), P, 1 << 20, *tail, s) == E_UNSUPPORTED, fn
        assert fn(*cargs(P, 0, b1=P8), P, 1 << 20, *tail, s) == E_UNSUPPORTED, fn
    assert lib.fbbev_history_conv_vm(*cargs(P, 0), None, 0, 1, s) == E_WORKSPACE
    assert lib.fbbev_history_conv_bf16(*cargs(P, 0), P, 16, 1, 1, s) == E_WORKSPACE
    assert lib.fbbev_history_conv_bf16x3(*cargs(P, 0), P, 1 << 20, 0, s) == E_UNSUPPORTED            # an fp32 ring
    C8 = 80
    d8, n8 = T * N * C8, (T + 1) * N * C8
    stp = lambda fn, hs, ns, *tail, h=P, c=C8, et=1, ws=1 << 22: fn(h, hs, P, ns, P, P, P, P, P, 1, T, c, c, Z, Y, X, P, P, ws, et, *tail, s)  # noqa: E731
    for fn, tail in ((lib.fbbev_history_fused_vm, ()), (lib.fbbev_history_fused_x3_vm, ()), (lib.fbbev_history_step_x3_vm, (3,))):
        assert stp(fn, d8 - 8, 0, *tail) == E_BADARG, fn
        assert stp(fn, 0, n8 - 8, *tail) == E_BADARG, fn
        assert stp(fn, 0, 0, *tail, h=P8) == E_UNSUPPORTED, fn
        assert stp(fn, d8 + 4, 0, *tail) == E_UNSUPPORTED, fn
        assert stp(fn, 0, 0, *tail, et=0) == E_UNSUPPORTED, fn
        assert stp(fn, 0, n8 - 8, *tail, h=P8) == E_BADARG, fn         # misaligned history AND short next ring: BADARG first
        assert stp(fn, 0, 0, *tail, ws=32) == E_WORKSPACE, fn
    assert stp(lib.fbbev_history_fused_vm, 0, 0, c=16) == E_UNSUPPORTED and stp(lib.fbbev_history_fused_x3_vm, 0, 0, c=16) == E_UNSUPPORTED
    assert stp(lib.fbbev_history_step_x3_vm, 0, 0, 65) == E_BADARG and stp(lib.fbbev_history_step_x3_vm, 0, 0, -1) == E_BADARG
    # empty calls: 0, nothing written
    out = api.to(torch.full((64,), float('nan')))
    po = ctypes.c_void_p(out.data_ptr())
    assert lib.fbbev_history_warp_vm(P, 0, P, 0, T, C, Z, Y, X, po, 0, 1, s) == 0
    assert lib.fbbev_history_warp_vm(P, 0, P, 1, 0, C, Z, Y, X, po, 0, 1, s) == 0
    assert lib.fbbev_history_warp_vm_src(P, 0, P, 0, P, P, 1, 0, C, Z, Y, X, po, 0, 1, s) == 0
    assert lib.fbbev_history_warp_e(P, 0, P, 1, 0, Z, Y, X, po, 0, 0, s) == 0 and lib.fbbev_history_warp_e(P, 0, P, 0, 3, Z, Y, X, po, 0, 0, s) == 0
    assert lib.fbbev_history_frame_vm(P, 0, C, N, 1, po, 0, 1, s) == 0 and lib.fbbev_history_frame_vm(P, 1, C, 0, 1, po, 0, 1, s) == 0
    assert lib.fbbev_history_conv_e(P, 0, P, P, P, P, 0, T1, C, C, N, po, None, 0, 0, s) == 0
    assert lib.fbbev_history_conv_e(P, 0, P, P, P, P, 1, T1, C, C, 0, po, None, 0, 0, s) == 0
    assert lib.fbbev_history_conv_vm(P, 0, P, P, P, P, 0, T1, C, C, N, po, None, 0, 1, s) == 0
    assert lib.fbbev_history_conv_bf16(P, 0, P, P, P, P, 1, T1, C, C, 0, po, None, 0, 1, 1, s) == 0
    assert lib.fbbev_history_conv_bf16x3(P, 0, P, P, P, P, 0, T1, C, C, N, po, None, 0, 1, s) == 0
    for fn, tail in ((lib.fbbev_history_fused_vm, ()), (lib.fbbev_history_fused_x3_vm, ()), (lib.fbbev_history_step_x3_vm, (3,))):
        assert fn(P, 0, po, 0, P, P, P, P, P, 0, T, C8, C8, Z, Y, X, po, P, 1 << 22, 1, *tail, s) == 0, fn
    assert lib.fbbev_history_flow(P, P, P, api.f3(DX_A), api.f3(LOWER_A), 0, po, s) == 0
    assert lib.fbbev_history_flow(P, P, P, api.f3((0.5, 0.0, 0.5)), api.f3(LOWER_A), 1, po, s) == E_BADARG
    assert lib.fbbev_history_stream_prologue(P, P, P, P, P, api.f3(DX_A), api.f3(LOWER_A), 0.5, 0, 3, 80, po, po, po, po, po, s) == 0
    assert lib.fbbev_history_stream_prologue(P, P, P, P, P, api.f3(DX_A), api.f3(LOWER_A), 0.5, 1, 8193, 80, P, P, P, P, P, s) == E_UNSUPPORTED
    api.sync()
    assert torch.isnan(api.back(out)).all(), 'an empty call wrote something'


# ------------------------------------------------------------------------------------------------------------------ anchor
def anchor_difference():
    """On the two flows and the shape of test_gpu_history.py::test_warp_kernel_vs_reference_grid_sample_and_oracle: the table's warp
    reference against oracle.history_oracle.grid_sample_3d in double on the double grid.  They differ only by what the fp32 coordinate
    chain contributes: |d coordinate| <= c u (|coordinate| + size) on each axis moves a blend by at most sum_axes |d out / d axis| <=
    (max - min of the 8 taps') per unit.  -> (max difference, max of that allowance)"""
    from oracle import history_oracle as H
    g = torch.Generator().manual_seed(2)
    B, CH, Z, Y, X = 2, 37, 8, 50, 60
    hist = torch.randn(B, CH, Z, Y, X, generator=g)
    flows = flows_for(('real_shift', 'real_rot'), (Z, Y, X))
    ref, S = warp_planes_ref(hist.reshape(B, CH, -1), flows, (Z, Y, X))
    grid = H.generate_grid(flows.double(), (Z, Y, X), torch.float64).permute(0, 3, 1, 2, 4)
    exp = H.grid_sample_3d(hist.double(), grid).reshape(B, CH, -1).numpy()
    diff = np.abs(ref - exp).max()
    # 12 roundings on a coordinate of magnitude <= 2 * 60: |d| <= 12 u 120; the blend's slope per axis <= 2 max|a|: three axes
    allow = 12 * U * 120 * 3 * 2 * hist.abs().max().item()
    return diff, allow


# ------------------------------------------------------------------------------------------------------------------ the table's own claims
def table_claims():
    """restates the launch geometry and asserts that every case reaches the path its name claims; -> {case: instantiation launched}"""
    inst = {}
    # ---- planar warp: the U = 4 loop, its tail, a group boundary, a second chunk that is not full
    for name, p in {**WARP_CASES, **WARP_REAL}.items():
        B, CH, grid = len(p['flows']), p['CH'], p['grid']
        zyx = grid[0] * grid[1] * grid[2]
        if p['lds']:
            kinds = lds_geometry(B, CH, grid, [flow_named(f, grid).numpy() for f in p['flows']])
            assert kinds is not None, f'{name}: the brick kernel does not run'
            if 'staged_fallback_empty' in name:
                assert 'staged' in kinds[0] and 'fallback' in kinds[1] and kinds[2] == {'empty'}, (name, kinds)
            inst[name] = f'k_history_warp_lds<{ET[TYPES[p["dt"]]]}>'
            continue
        assert lds_geometry(B, CH, grid, []) is None
        n_chunks, cpb, n_groups = planar_geometry(B, CH, grid)
        assert zyx % 256 != 0 and n_chunks == 2, (name, zyx)                     # a second chunk of 50 / 52 voxels
        assert cpb == 8
        per = [min(cpb, CH - gidx * cpb) for gidx in range(n_groups)]
        want = {1: [1], 3: [3], 4: [4], 9: [8, 1], 37: [8, 8, 8, 8, 5]}[CH]      # U = 4 trips and tails per workgroup
        assert per == want, (name, per)
        inst[name] = f'k_history_warp<{ET[TYPES[p["dt"]]]}>'
    # ---- the 2^k + 1 rule of layer A and the flows: fp32 chain == float64 chain (taps asserts it)
    for grid in (G_A, G_LDS, G_VM80, G_VM16, G_FUSED, (2, 9, 17), (3, 9, 17)):
        assert all(s - 1 == 1 << ((s - 1).bit_length() - 1) for s in grid), grid
        for f in ('shift', 'quarter', 'flipz', 'outside', 'half', 'quarter_int'):
            idx, w, ok = taps(flow_named(f, grid).numpy(), *grid, dyadic=True)
            assert np.array_equal(w * 64, np.round(w * 64))
            if f == 'outside':
                assert not ok.any()
            if f in ('shift', 'quarter'):
                assert ok.any() and not ok.all() and ((w > 0) & (w < 1)).any()   # fractional weights, partial exit
    assert not taps(flow_named('nan', G_A).numpy(), *G_A)[2].any()
    idx, w, ok = taps(flow_named('real_rot_small', G_B).numpy(), *G_B)
    assert ok.any() and not ok.all() and not np.array_equal(w * 64, np.round(w * 64))
    # ---- 16-bit layer A data: the store's rounding is exercised (inexact blends), ties occur, subnormals and +-65504 are there
    for dt in (BF16, F16):
        data = warp_data((2, 3, 330, 16), dt, 5)
        ref, _ = warp_rows_ref(data, flows_for(('shift', 'quarter'), G_VM80), G_VM80, dyadic=True)
        r = to_type(ref, dt).double().numpy()
        inexact = r != ref
        ulp = 2 * ring_half_ulp(np.abs(ref), dt)
        tie = inexact & (np.abs(np.abs(r - ref) - ulp / 2) == 0)
        assert inexact.sum() > 100 and tie.sum() > 10, (dt, inexact.sum(), tie.sum())
        if dt == F16:
            assert (data.float().abs() == 65504).any() and (np.abs(ref) > 2.0 ** 15).any() and ((np.abs(ref) < 2.0 ** -14) & (ref != 0)).any()
    # ---- voxel-major warps
    for name, p in {**WARP_VM_CASES, **WARP_VM_REAL, **WARP_SRC_CASES}.items():
        v = vm_geometry(p['dt'], p['C'], p['T'], p['grid'], p['yb'])
        kern = 'k_history_warp_vm_src' if p['src'] is not None else 'k_history_warp_vm'
        inst[name] = v['instantiation'].replace('k_history_warp_vm', kern)
        if p['C'] == 80 and p['grid'] == G_VM80:
            assert v['items'] == 330 and v['n_xc'] == 2 and v['last_chunk'] == 74, (name, v)     # second x chunk holds 74 items
        if p['grid'] == G_VM16:
            assert v['n_xc'] == (2 if p['dt'] == 'f32' else 1) and v['last_chunk'] == (4 if p['dt'] == 'f32' else 130), (name, v)
        if p['yb'] == 2 and p['grid'][1] == 5:
            assert v['nyb'] == 3 and v['last_band'] == 1, (name, v)                              # the last band overhangs Y by one row
        tu = 4 if p['dt'] == 'f16' else 2
        assert v['TU'] == tu and v['tail_twice'] == (p['T'] % tu != 0)
    for dt, tu in (('f32', 2), ('bf16', 2), ('f16', 4)):                                         # a short, an exact and a clamped batch per type
        ts = sorted(p['T'] for p in WARP_VM_CASES.values() if p['dt'] == dt)
        assert any(t < tu for t in ts) and any(t % tu == 0 for t in ts) and any(t > tu and t % tu for t in ts), (dt, ts)
    assert {f for p in WARP_SRC_CASES.values() for f in p['src']} == {0, 1, 2, 3}
    # ---- frame_vm: every N and C of the list, inner > 1 with an N % 64 tail, all types
    assert {p['N'] for p in FRAME_CASES.values()} == {1, 63, 64, 65, 200} and {p['C'] for p in FRAME_CASES.values()} == {8, 40, 48, 80, 512}
    assert any(p['inner'] > 1 and p['N'] % 64 for p in FRAME_CASES.values())
    for name, p in FRAME_CASES.items():
        inst[name] = f'k_history_frame_vm<{ET[TYPES[p["dt"]]]}>'
    for dt in TYPES:
        assert {p['inner'] > 1 for p in FRAME_CASES.values() if p['dt'] == dt} == {True, False}
    # ---- convolutions: MT in {1, 5} x VM x ET, the generic kernel's three shapes, N on both sides of every tile
    for name, p in CONV_CASES.items():
        inst[name] = conv_instantiation(p)
        tile = 256 if p['route'] == 'x3' else 64
        assert p['N'] in (1, tile - 1, tile, tile + 1, 130), name
    need = {f'k_history_conv_t<{mt}, {mt}, {et}, {vm}>' for mt in (1, 5) for et in (0, 1, 2) for vm in ('false', 'true')}
    need |= {f'k_history_conv_bf16<{mt}, {mt}, {et}, {vm}>' for mt in (1, 5) for et in (0, 1, 2) for vm in ('false', 'true')}
    need |= {f'k_history_conv_bf16x3<{mt}, {mt}, {et}, 2, 8, 1>' for mt in (1, 5) for et in (1, 2)}
    need |= {f'k_history_conv<{et}>' for et in (0, 1, 2)}
    assert need <= set(inst.values()), need - set(inst.values())
    # ---- fused and step entries
    for name, p in {**STEP_CASES, **STEP_REAL}.items():
        s = step_geometry(p)
        if p['entry'] == 'fused' and p['grid'] == G_FUSED:
            assert s['n_xc'] == 2 and s['last_tile'] == 1 and s['YB'] == 14 and s['nyb'] == 2 and s['last_band'] == 3, (name, s)
        if p['entry'] == 'fused_x3' and p['grid'][1:] == (9, 17):
            assert s['n_xt'] == 2 and s['n_yt'] == 2 and s['over_x'] == 1 and s['over_y'] == 1, (name, s)
        if p['entry'] == 'step':
            want = {1: 1, 3: 3, 64: 3, 0: 5}[p['chunks']]
            assert s['chunks'] == want, (name, s)
            assert s['segments'][-1][1] == p['grid'][1] and s['segments'][0][0] == 0
            if p['yb'] == 2:
                assert s['nyb'] * s['YB'] > p['grid'][1]                                         # y1 = yb1 * YB overshoots Y: the clamp matters
            inst[name] = s['instantiation'] + ' + ' + s['conv']
        else:
            inst[name] = s['instantiation']
    need = {f'k_history_fused_bf16<{et}>' for et in (1, 2)} | {f'k_history_fused_x3<{et}>' for et in (1, 2)}
    assert need <= set(inst.values())
    assert any('2, 4, 1>' in v for v in inst.values())                                           # NW = 4: the pipelined step's convolutions
    want_vm = {f'k_history_warp_vm<{et}, {tu}, 1>' for et, tu in ((0, 2), (1, 2), (2, 4))}
    assert want_vm <= set(inst.values())
    # the once-per-process knobs add <2, 2, 1>, NW = 4 in the stand-alone convolution and NW = 8 in the step (KNOB_RUNS)
    for (k, v), runs in KNOB_RUNS.items():
        for kind, case in runs:
            assert case in (WARP_VM_CASES if kind == 'vm' else STEP_CASES if kind == 'step' else CONV_CASES), case
    assert vm_geometry('f16', 80, 3, G_VM80, 2, tu=2)['tail_twice'] and not vm_geometry('f16', 80, 2, G_VM80, 2, tu=2)['tail_twice']
    # ---- every exported entry appears
    import re
    header = open(os.path.join(ROOT, 'include', 'fbbev.h')).read()
    exported = set(re.findall(r'^int (fbbev_history_\w+)\(', header, re.M))
    src = open(os.path.abspath(__file__)).read()
    used = set(re.findall(r"fbbev_history_\w+", src))
    # fbbev_history_warp / fbbev_history_conv are the fp32 shorthands of the _e entries (one line each in capi.hip): check_shorthands
    assert exported <= used, exported - used
    return inst


def check_shorthands(api):
    """fbbev_history_warp and fbbev_history_conv forward to the _e entries with elem_type 0: the same bits"""
    grid, B, CH = G_A, 2, 5
    Z, Y, X = grid
    N = Z * Y * X
    flows = flows_for(('shift', 'quarter'), grid)
    data = warp_data((B, CH, N), F32, 3, ch_axis=1)
    d_out = api.to(torch.full((B, CH, N), float('nan')))
    assert api.call('fbbev_history_warp', api.to(data), 0, api.to(flows), B, CH, Z, Y, X, d_out, 0) == 0
    ref, _ = warp_planes_ref(data, flows, grid, dyadic=True)
    _exact('fbbev_history_warp', 'out', api.back(d_out), to_type(ref, F32))
    x, w1, bias1, w2, bias2 = conv_data(B, 2, 32, 16, 65, F32, 4)
    d_out = api.to(torch.full((B, 16, 65), float('nan')))
    assert api.call('fbbev_history_conv', api.to(x.reshape(B, 64, 65)), 0, api.to(w1), api.to(bias1.reshape(B * 2, 32)), api.to(w2), api.to(bias2),
                    B, 2, 32, 16, 65, d_out, None, 0) == 0
    _exact('fbbev_history_conv', 'out', api.back(d_out), to_type(conv_ref(x, w1, bias1, w2, bias2, 'f32'), F32))
