"""Case tables, input generators, references and bounds for the fused row kernels of the encoder block, shared by the GPU test
(tests/test_gpu_rows_block_kernels.py) and the emulator test (tests/test_emu_rows_block_kernels.py): fbbev_rows_linear_x3_ln,
fbbev_rows_ffn_x3, fbbev_rows_tail_ffn_x3 / _planes, fbbev_rows_linear_x3_planes / _planes_e and fbbev_layernorm (forward) at the
smallest shapes at which each of their code paths exists.  Both adapters call the C ABI itself (fb_bev_amd._capi.lib() on the
device, tests/emu/emu_capi.lib() on the CPU emulator build) through ctypes, so that every row operand can be a strided view and
every `out` a caller-owned, NaN-filled buffer.

Every call: `out` starts as NaN and comes back without one; the padding columns of a strided `out` hold a sentinel (7777) and keep
it; the padding columns of a strided x / residual hold NaN (a read of one poisons the result) and every input has the same bits
afterwards.

Layer A, exact integers.  Activations, weights, biases and residuals are integers in [-4, 4]: exact in bf16, so every lo half is
zero, every product and partial sum is an integer below 2^24 (asserted from the shape) and fp32 addition is exact in any order.
For the FFN the ReLU'd hidden integer is at most 16 I + 4 < 2^16, so bf16 hi + bf16 lo (8 + 8 significant bits) reproduces it,
and max_hidden * 4 * H < 2^24 (asserted).  Entries without a LayerNorm must equal the exact integer result bit for bit (the
reference is an integer matrix product carried in float64, where integers below 2^53 are exact, and compared as int64); 16-bit
planes equal int64 -> float32 -> .to(dtype) word for word.  Entries with a LayerNorm have an exact pre-norm value, so only the
LayerNorm's own roundings remain: the LayerNorm bound below with e = 0.  (The tail kernel: LayerNorm0's input is exact, e0 = 0;
its output is real, so the FFN behind it is bounded as in layer B.)

Layer B, real operands with full mantissas (randn, weights scaled by fan_in^-0.5, LayerNorm weight in [0.5, 1.5]), componentwise
against float64.

Pre-norm bound e of one GEMM, y = x W^T + b + res.  With P = |x| |W|^T and S = P + |b| + |res|:
      e = 4 * 2^-16 * P + (I + 2) * 2^-24 * S
  * bf16 keeps 8 significant bits: v = hi + lo + r with |r| <= 2^-16 |v|; the product (ah + al)(bh + bl) drops al * bl, at most
    2^-16 |a b|: 3 * 2^-16 per product to first order, 4 * 2^-16 with the higher-order terms rounded up (rows_train_cases);
  * an fp32 accumulation of depth n costs at most n * 2^-24 of the sum of magnitudes: I products, the bias add, the residual add.
  The split acts on the products only (bias and residual are added in fp32), so 4 * 2^-16 multiplies P, not S: never more than
  rows_train_cases' c * S with c = linear_c(I) = 4 * 2^-16 + (I + 2) * 2^-24, and much less where the residual dominates.
FFN, y = W2 relu(W1 x + b1) + b2 + res, two GEMMs composed (ReLU is 1-Lipschitz, so the hidden error passes through it):
      A1 = |x| |W1|^T + |b1|                     eh = 4 * 2^-16 * |x| |W1|^T + (I + 2) * 2^-24 * A1  [+ e_x |W1|^T]
      P2 = A1 |W2|^T                              e  = eh |W2|^T + 4 * 2^-16 * P2 + (H + 2) * 2^-24 * (P2 + |b2| + |res|)  [+ e_res]
  (the hidden split hi + lo is the split of GEMM 2's B operand: inside its 4 * 2^-16; H products + b2 + residual: depth H + 2).

LayerNorm bound.  y = the exact pre-norm row, mu = mean(y), sig = sqrt(mean((y - mu)^2) + eps), n = (y - mu) / sig,
exact = gamma n + beta.  The kernels (k_rows_linear_x3<2, true>, k_rows_ffn_x3's epilogue and PRE block, k_layernorm_rows) run one
expression sequence on v = y + err, |err_i| <= e_i:
      s = sum v (per lane (a + b) + (c + d), `s +=` once per 16-output tile, then a shuffle tree); mean = s / O;
      d_i = v_i - mean;  q = sum d_i^2 (same tree);  inv = 1 / sqrtf(q / O + eps);  out_i = d_i * inv * gamma_i + beta_i.
First-order propagation of err:  |d(y_i - mu)| <= e_i + mean(e) =: em_i;  |d sig| <= sum_j |n_j| em_j / O;  hence
      |d n_i| <= em_i / sig + |n_i| sum_j |n_j| em_j / (O sig).
The kernel's own roundings, u = 2^-24, d_s = the depth of the summation tree = 2 (in the lane's float4) + tiles (one `s +=` per
16-output tile: ceil(O / 16)) + 2 shuffles for the MFMA kernels, 2 + 5 shuffles for k_layernorm_rows:
  * the mean: d_s roundings in the sum, one in the division: |mean_hat - mean| <= (d_s + 1) u mean|y|.  It shifts every d_i, so
    in units of sig it costs (d_s + 1) u M with M = mean_j |y_j| / sig.  (The issue wrote this term as |mu| / sig.  The sum of O
    terms errs by d_s u sum|y_j| whatever their mean, so a row with mu = 0 needs mean|y|; |mu| <= mean|y| <= |mu| + sig, the two
    agree on a constant row and on a row with a large mean, the cases the term exists for.)
  * the subtraction: u |n_i|;
  * q: the subtraction's rounding twice in each square, one rounding per square, d_s in the sum, one division, one `+ eps`:
    (d_s + 5) u relative, and the shift of the mean enters q only in second order (sum (y_j - mu) = 0); sqrtf halves that and
    rounds once, the division rounds once (IEEE sqrtf and division: the build sets no fast-math flag): inv errs by
    ((d_s + 5) / 2 + 2) u relative: ((d_s + 5) / 2 + 2) u |n_i|;
  * two multiplications: 2 u |n_i|; the final `+ beta` rounds the result: u |exact_i|, written 2 u |exact_i| below.
  Together u (|n_i| (d_s / 2 + 7.5) + (d_s + 1) M).  Higher-order terms: the shift of the mean enters inv as (shift / sig)^2 / 2
  relative, times |n_i| <= sqrt(O) <= 11.4.  With a := (d_s + 1) u M <= 2^-5 (asserted for every row of every case) that is at most
  a * 11.4 / 64 + a / 64 < 0.25 a: the factor 1.25 on the mean's term.  One constant:
      k = max(d_s / 2 + 7.5, 1.25 (d_s + 1))          (d_s = 9 at O = 80: k = 12.5; d_s = 12 at O = 128: k = 16.25; k_layernorm_rows: k = 11)
      |got - exact|_i <= |gamma_i| (em_i / sig + |n_i| sum_j |n_j| em_j / (O sig) + k u (|n_i| + M)) + 2 u |exact_i|
A contraction of a * b + c into one fma (the device build) removes roundings, never adds one.
fbbev_layernorm: e = 0, or e = 2^-24 (|x| + |r|) with a residual (one fp32 add).
Tail kernel: the bound is applied twice -- LayerNorm0's output bound e1 is the e_x of the FFN composition and, through the
identity add, its e_res; the result is the e of LayerNorm1.

Split-operand evidence: the largest error of every real case is at least 30 times smaller than that of the same composition in
float64 on operands rounded to bf16 (x, W; the hidden rows too), the ratio rows_train_cases and conv_cases use.  A constant row
is left out of both maxima: its error is the rounding of its mean, amplified by 1 / sqrt(eps), with either kind of operand.

Statistics cases, for every entry with a LayerNorm: rows whose pre-norm mean is ~100 against a spread of ~1 (a one-pass variance
E[v^2] - mean^2 loses them), and one constant pre-norm row (var = 0: the M term alone bounds it).

Plain Python and CPU torch only; the adapters import their library on first use.
"""
import contextlib
import ctypes

import torch

from rows_train_cases import EXACT_LIMIT, U16, U24, linear_c, observed

NAN = float('nan')
SENTINEL = 7777.0
EPS = 1e-5
UNSUPPORTED, BADARG = -2, -1
CONST_VALUE = 3.3                         # the constant pre-norm row of the statistics cases (not a dyadic number: its mean rounds)


# ------------------------------------------------------------------------------------------------------------------ adapters
def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ld(t):
    return 0 if t is None else t.stride(0)


class _Calls:
    """the C ABI entries of this family, raw: every method returns the entry's return code"""

    def fragments(self, w):
        """W (O, I) CPU tensor -> (keep-alive buffer, 16-byte aligned pointer) of its split bf16 fragments"""
        O, I = w.shape
        L = self.lib()
        need = L.fbbev_rows_linear_x3_fragment_bytes(I, O)
        buf = torch.zeros(need + 16, dtype=torch.uint8, device=self.device)
        p = ctypes.c_void_p(buf.data_ptr() + (-buf.data_ptr()) % 16)
        wd = self.to(w.contiguous())
        with self.guard():
            code = L.fbbev_rows_linear_x3_fragments(_ptr(wd), I, O, p, need, self.stream())
        assert code == 0, code
        return buf, p

    def linear_ln(self, x, f, b, R, I, O, res, lw, lb, eps, out):
        with self.guard():
            return self.lib().fbbev_rows_linear_x3_ln(_ptr(x), _ld(x), f[1], _ptr(b), R, I, O, _ptr(res), _ld(res), _ptr(lw), _ptr(lb), eps,
                                                      _ptr(out), _ld(out), self.stream())

    def ffn(self, x, f1, b1, f2, b2, R, I, H, O, res, lw, lb, eps, out):
        with self.guard():
            return self.lib().fbbev_rows_ffn_x3(_ptr(x), _ld(x), f1[1], _ptr(b1), f2[1], _ptr(b2), R, I, H, O, _ptr(res), _ld(res), _ptr(lw),
                                                _ptr(lb), eps, _ptr(out), _ld(out), self.stream())

    def tail(self, x, f0, b0, res0, l0w, l0b, eps0, f1, b1, f2, b2, R, E, H, l1w, l1b, eps1, out, S=0):
        with self.guard():
            if S:
                return self.lib().fbbev_rows_tail_ffn_x3_planes(_ptr(x), _ld(x), f0[1], _ptr(b0), _ptr(res0), _ld(res0), _ptr(l0w), _ptr(l0b),
                                                                eps0, f1[1], _ptr(b1), f2[1], _ptr(b2), R, E, H, _ptr(l1w), _ptr(l1b), eps1,
                                                                S, _ptr(out), self.stream())
            return self.lib().fbbev_rows_tail_ffn_x3(_ptr(x), _ld(x), f0[1], _ptr(b0), _ptr(res0), _ld(res0), _ptr(l0w), _ptr(l0b), eps0,
                                                     f1[1], _ptr(b1), f2[1], _ptr(b2), R, E, H, _ptr(l1w), _ptr(l1b), eps1, _ptr(out),
                                                     _ld(out), self.stream())

    def planes(self, x, f, b, R, I, O, S, Dh, out):
        et = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[out.dtype]
        with self.guard():
            if et:
                return self.lib().fbbev_rows_linear_x3_planes_e(_ptr(x), _ld(x), f[1], _ptr(b), R, I, O, S, Dh, et, _ptr(out), self.stream())
            return self.lib().fbbev_rows_linear_x3_planes(_ptr(x), _ld(x), f[1], _ptr(b), R, I, O, S, Dh, _ptr(out), self.stream())

    def layernorm(self, x, r, w, b, eps, rows, C, out):
        with self.guard():
            return self.lib().fbbev_layernorm(_ptr(x), _ptr(r), _ptr(w), _ptr(b), eps, rows, C, _ptr(out), self.stream())

    def full(self, shape, value, dtype=torch.float32):
        return torch.full(shape, value, dtype=dtype, device=self.device)


class GpuApi(_Calls):
    """fb_bev_amd._capi.lib() on cuda:0, on torch's current stream"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi
        self.c = _capi
        self.device = torch.device('cuda:0')

    def lib(self):
        return self.c.lib()

    def guard(self):
        return torch.cuda.device(self.device)

    def stream(self):
        return self.c._stream()

    def to(self, t):
        """CPU tensor or strided CPU view -> the same values with the same strides on the device"""
        if t is None:
            return None
        base = t._base if t._base is not None else t
        d = base.to(self.device)
        return d if t._base is None else d.as_strided(t.shape, t.stride(), t.storage_offset())


class EmuApi(_Calls):
    """tests/emu/emu_capi.lib(): the same entries and kernels compiled for the CPU"""
    name = 'emu'

    def __init__(self):
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
        import emu_capi
        self.E = emu_capi
        self.device = torch.device('cpu')

    def lib(self):
        return self.E.lib()

    def guard(self):
        return contextlib.nullcontext()

    def stream(self):
        return None

    def to(self, t):
        """a copy with the same strides (the caller's tensors stay the reference)"""
        if t is None:
            return None
        if t._base is None:
            return t.clone()
        return t._base.clone().as_strided(t.shape, t.stride(), t.storage_offset())


# ------------------------------------------------------------------------------------------------------------------ helpers
def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _ints(shape, g, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _rows(values, pad):
    """(R, C) values -> a view of a (R, C + pad) tensor whose other columns are NaN (pad = 0: the dense tensor)"""
    if values is None or not pad:
        return values
    R, C = values.shape
    buf = torch.full((R, C + pad), NAN)
    buf[:, :C] = values
    return buf[:, :C]


def _base(t):
    return t._base if t._base is not None else t


class _Frozen:
    """the bits of every input (padding included) before a call; check(): the same bits after it"""

    def __init__(self, *tensors):
        self.t = [t for t in tensors if t is not None]
        self.snap = [_base(t).clone() for t in self.t]

    def check(self):
        for t, s in zip(self.t, self.snap):
            assert torch.equal(_base(t).view(torch.int32), s.view(torch.int32)), 'an input (or its padding) was written'


def _out_rows(api, R, O, pad):
    """-> (view, buffer): `view` (R, O) all NaN, the buffer's other columns the sentinel"""
    buf = api.full((R, O + pad), SENTINEL)
    buf[:, :O] = NAN
    return buf[:, :O], buf


def _out_ok(view, buf):
    O = view.shape[1]
    assert not torch.isnan(view).any(), 'an output element was not written (or is NaN)'
    assert bool((buf[:, O:] == SENTINEL).all()), 'the padding of out was written'
    return view.cpu().double()


def _imm(a, b):
    """integer matrix product a b^T of integer-valued tensors, carried in float64 (exact below 2^53) -> float64"""
    return a.double() @ b.double().t()


def _bf(t):
    return t.float().bfloat16().double()


def ln_ref(y, gamma, beta, eps):
    y = y.double()
    mu = y.mean(-1, keepdim=True)
    sig = ((y - mu).pow(2).mean(-1, keepdim=True) + eps).sqrt()
    return (y - mu) / sig * gamma.double() + beta.double()


def ln_depth(O, mfma=True):
    """d_s of the module docstring: the depth of the kernel's summation tree over a row of O values"""
    return 2 + (O + 15) // 16 + 2 if mfma else 2 + 5


def ln_k(d_s):
    return max(d_s / 2 + 7.5, 1.25 * (d_s + 1))


def ln_bound(y, e, gamma, beta, eps, d_s):
    """the LayerNorm bound of the module docstring -> (exact, bound), float64; e: a tensor like y, or 0"""
    y, gamma, beta = y.double(), gamma.double(), beta.double()
    O = y.shape[-1]
    mu = y.mean(-1, keepdim=True)
    sig = ((y - mu).pow(2).mean(-1, keepdim=True) + eps).sqrt()
    n = (y - mu) / sig
    exact = n * gamma + beta
    e = torch.zeros_like(y) + e
    em = e + e.mean(-1, keepdim=True)
    M = y.abs().mean(-1, keepdim=True) / sig
    assert ((d_s + 1) * U24 * M).max().item() <= 2.0 ** -5, 'the higher-order factor of k needs (d_s + 1) u M <= 2^-5'
    bound = gamma.abs() * (em / sig + n.abs() * (n.abs() * em).sum(-1, keepdim=True) / (O * sig) + ln_k(d_s) * U24 * (n.abs() + M)) \
        + 2 * U24 * exact.abs()
    return exact, bound


def gemm_e(x, w, b, res, e_x=None):
    """pre-norm bound of y = x W^T + b + res (module docstring); float64 in, float64 out"""
    I = w.shape[1]
    P = x.abs() @ w.abs().t()
    S = P + (b.abs() if b is not None else 0) + (res.abs() if res is not None else 0)
    e = 4 * U16 * P + (I + 2) * U24 * S
    return e if e_x is None else e + e_x @ w.abs().t()


def ffn_e(x, w1, b1, w2, b2, res, e_x=None, e_res=None):
    """pre-norm bound of y = W2 relu(W1 x + b1) + b2 + res (module docstring)"""
    H, I = w1.shape
    P1 = x.abs() @ w1.abs().t()
    A1 = P1 + b1.abs()
    eh = 4 * U16 * P1 + (I + 2) * U24 * A1
    if e_x is not None:
        eh = eh + e_x @ w1.abs().t()
    P2 = A1 @ w2.abs().t()
    e = eh @ w2.abs().t() + 4 * U16 * P2 + (H + 2) * U24 * (P2 + b2.abs() + (res.abs() if res is not None else 0))
    return e if e_res is None else e + e_res


def _ffn64(x, w1, b1, w2, b2, res, bf16=False):
    r = _bf if bf16 else (lambda t: t.double())
    h = torch.relu(r(x) @ r(w1).t() + b1.double())
    y = r(h) @ r(w2).t() + b2.double()
    return y if res is None else y + res.double()


def _report(api, entry, name, layer, err, bound, e16=None, keep=None):
    """one [observed] line; asserts err <= bound everywhere and, with e16, the split-operand evidence over the rows `keep`"""
    ratio = (err / bound).max().item()
    text = f'{api.name} {entry} {name} layer {layer}: max|err| = {err.max().item():.3e}, max err / bound = {ratio:.4f}'
    if e16 is not None:
        k = slice(None) if keep is None else keep
        mine, plain = err[k].max().item(), e16[k].max().item()
        text += f'; plain bf16 operands {plain:.3e} = {plain / max(mine, 1e-300):.0f} x'
    observed(text)
    assert ratio <= 1.0, ratio
    if e16 is not None:
        assert mine * 30 < plain, (mine, plain)


# ------------------------------------------------------------------------------------------------------------------ fbbev_rows_linear_x3_ln
def _lc(rows, I, O, res=True, bias=True, pad=True, stats=None, real=True, env=None):
    return dict(rows=rows, I=I, O=O, res=res, bias=bias, pad=pad, stats=stats, real=real, env=env or {})


# rows: the second 16-row tile of a wave (17), the second wave (33), a last tile that is full / short by one / long by one (128 is
# inside 200; 127; 129); O = 4: lanes g > 0 idle; O = 20: the width ends inside tile 1; I = 8 / 80: the cut inside a k-step;
# I = 136: a second K chunk of one piece; I = 320: three chunks
LINEAR_LN_CASES = {
    'r1_i8_o4': _lc(1, 8, 4),
    'r17_i80_o20': _lc(17, 80, 20, res=False),
    'r33_i136_o20': _lc(33, 136, 20),
    'r127_i80_o80': _lc(127, 80, 80),
    'r129_i128_o128': _lc(129, 128, 128, pad=False),
    'r200_i320_o80': _lc(200, 320, 80),
    'r33_i80_o64_nobias': _lc(33, 80, 64, bias=False),
    'r129_i8_o128_nobias_nores': _lc(129, 8, 128, res=False, bias=False),
    'r17_i136_o4': _lc(17, 136, 4, pad=False),
    'r200_i128_o20': _lc(200, 128, 20, res=False),
    'r127_i320_o64': _lc(127, 320, 64, pad=False),
    'r1_i80_o80': _lc(1, 80, 80, res=False, pad=False),
    'r33_i320_o128': _lc(33, 320, 128),
    'r200_i80_o80': _lc(200, 80, 80),
    'r33_i80_o80_mean100': _lc(33, 80, 80, stats='mean'),
    'r17_i80_o20_constant_row': _lc(17, 80, 20, stats='const'),
}
# two row tiles per workgroup (RT = tiles / 1024 = 2 from 2048 tiles on): 2049 tiles, the last workgroup's second tile does not exist
LINEAR_LN_RT2_GPU = _lc(262145, 80, 80, pad=False, real=False)
LINEAR_LN_RT2_EMU = _lc(300, 80, 80, real=False, env={'FBBEV_ROWS_LINEAR_RT': '2'})       # 3 tiles: the same walk


def _stats_rows(stats, res, zero_rows_of, bias_like=()):
    """statistics cases: 'mean' shifts the residual by 100; 'const' makes row R // 2 a constant pre-norm row -> (res, row or None)"""
    if stats == 'mean':
        return res + 100.0, None
    if stats == 'const':
        r = res.shape[0] // 2
        res = res.clone()
        res[r] = CONST_VALUE
        for t in zero_rows_of:
            t[r] = 0.0
        for b in bias_like:
            b.zero_()
        return res, r
    return res, None


def linear_ln_inputs(case, real):
    R, I, O = case['rows'], case['I'], case['O']
    g = _gen(1, R, I, O, real)
    lw, lb = torch.rand(O, generator=g) + 0.5, torch.randn(O, generator=g) * 0.2
    if real:
        x, w, b = torch.randn(R, I, generator=g), torch.randn(O, I, generator=g) / I ** 0.5, torch.randn(O, generator=g) * 0.3
        res = torch.randn(R, O, generator=g)
    else:
        x, w, b, res = _ints((R, I), g), _ints((O, I), g), _ints((O,), g), _ints((R, O), g)
    res, const_row = _stats_rows(case['stats'], res, (x,), (b,))
    pad = case['pad']
    return dict(x=_rows(x, 8 if pad else 0), w=w, b=b if case['bias'] else None, res=_rows(res, 4 if pad else 0) if case['res'] else None,
                lw=lw, lb=lb, const_row=const_row)


def run_linear_ln(api, t, eps=EPS, out_pad=12):
    R, I = t['x'].shape
    O = t['w'].shape[0]
    x, b, res, lw, lb = (api.to(t[k]) for k in ('x', 'b', 'res', 'lw', 'lb'))
    f = api.fragments(t['w'])
    frozen = _Frozen(x, b, res, lw, lb)
    view, buf = _out_rows(api, R, O, out_pad)
    code = api.linear_ln(x, f, b, R, I, O, res, lw, lb, eps, view)
    assert code == 0, code
    got = _out_ok(view, buf)
    frozen.check()
    return got


def check_linear_ln(api, name, case, real):
    assert case['stats'] is None or (real and case['res'] and case['bias'])
    t = linear_ln_inputs(case, real)
    got = run_linear_ln(api, t, out_pad=12 if case['pad'] else 0)
    x, w = t['x'].double(), t['w'].double()
    b = t['b'].double() if t['b'] is not None else None
    res = t['res'].double() if t['res'] is not None else None
    y = x @ w.t() + (b if b is not None else 0) + (res if res is not None else 0)
    if real:
        e = gemm_e(x, w, b, res)
        S = x.abs() @ w.abs().t() + (b.abs() if b is not None else 0) + (res.abs() if res is not None else 0)
        assert bool((e <= linear_c(case['I']) * S * (1 + 1e-12)).all())   # never more than the c * S of rows_train_cases
    else:
        assert (x.abs() @ w.abs().t()).max().item() + 8 < EXACT_LIMIT
        e = 0
    exact, bound = ln_bound(y, e, t['lw'], t['lb'], EPS, ln_depth(case['O']))
    err = (got - exact).abs()
    e16 = keep = None
    if real:
        y16 = _bf(t['x']) @ _bf(t['w']).t() + (b if b is not None else 0) + (res if res is not None else 0)
        e16 = (ln_ref(y16, t['lw'], t['lb'], EPS) - exact).abs()
        keep = [r for r in range(case['rows']) if r != t['const_row']]
    _report(api, 'rows_linear_x3_ln', name, 'B' if real else 'A', err, bound, e16, keep)


def check_linear_ln_refusals(api):
    g = _gen(2)
    R, I = 5, 16
    x = api.to(torch.randn(R, I, generator=g))
    for O, off in ((132, 0), (80, 1)):                    # wider than one workgroup's rows; ln_weight 4 bytes off a 16-byte boundary
        f = api.fragments(torch.randn(O, I, generator=g))
        spare = api.to(torch.ones(O + 4))
        lw, lb, b = spare[off:off + O], api.to(torch.zeros(O)), api.to(torch.zeros(O))
        out = api.full((R, O), NAN)
        assert api.linear_ln(x, f, b, R, I, O, None, lw, lb, EPS, out) == UNSUPPORTED
        assert torch.isnan(out).all(), 'a refused call wrote to out'


# ------------------------------------------------------------------------------------------------------------------ fbbev_rows_ffn_x3
def _fc(rows, I, H, O, ln, res, pad=False, alias=False, stats=None):
    return dict(rows=rows, I=I, H=H, O=O, ln=ln, res=res, pad=pad, alias=alias, stats=stats)


FFN_CASES = {
    'r1_i8_h64_o4_ln_res': _fc(1, 8, 64, 4, True, True),
    'r33_i80_h64_o80_res': _fc(33, 80, 64, 80, False, True, pad=True),
    'r129_i96_h128_o20_ln': _fc(129, 96, 128, 20, True, False, pad=True),
    'r130_i64_h192_o48': _fc(130, 64, 192, 48, False, False),          # W2's second K chunk half filled, the kc2 / ks2 step mid-table
    'r200_i80_h320_o80_ln_res_is_x': _fc(200, 80, 320, 80, True, True, pad=True, alias=True),
    'r40_i80_h1088_o80_ln_res': _fc(40, 80, 1088, 80, True, True),     # b1's LDS tail loop (H > 1024)
    'r40_i80_h1088_o80': _fc(40, 80, 1088, 80, False, False),          # the same without a LayerNorm: layer A is bit for bit
    'r33_i80_h64_o80_mean100': _fc(33, 80, 64, 80, True, True, stats='mean'),
    'r17_i80_h128_o20_constant_row': _fc(17, 80, 128, 20, True, True, stats='const'),
}


def ffn_inputs(case, real):
    R, I, H, O = case['rows'], case['I'], case['H'], case['O']
    g = _gen(3, R, I, H, O, real)
    lw, lb = torch.rand(O, generator=g) + 0.5, torch.randn(O, generator=g) * 0.2
    if real:
        x = torch.randn(R, I, generator=g)
        w1, b1 = torch.randn(H, I, generator=g) / I ** 0.5, torch.randn(H, generator=g) * 0.3
        w2, b2 = torch.randn(O, H, generator=g) / H ** 0.5, torch.randn(O, generator=g) * 0.3
        res = torch.randn(R, O, generator=g)
    else:
        x, w1, b1, w2, b2, res = _ints((R, I), g), _ints((H, I), g), _ints((H,), g), _ints((O, H), g), _ints((O,), g), _ints((R, O), g)
    if case['stats'] == 'const':
        b1 = -b1.abs()                                     # the row with x = 0 has no hidden unit alive: its pre-norm row is b2 + residual
    res, const_row = _stats_rows(case['stats'], res, (x,), (b2,))
    x = _rows(x, 8 if case['pad'] else 0)
    res = (x if case['alias'] else _rows(res, 4 if case['pad'] else 0)) if case['res'] else None
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, res=res, lw=lw if case['ln'] else None, lb=lb if case['ln'] else None, const_row=const_row)


def run_ffn(api, t, out_pad=0):
    R, I = t['x'].shape
    H, O = t['w1'].shape[0], t['w2'].shape[0]
    x, b1, b2, lw, lb = (api.to(t[k]) for k in ('x', 'b1', 'b2', 'lw', 'lb'))
    res = x if t['res'] is t['x'] else api.to(t['res'])                          # rows_ffn_x3(t1, ..., residual=t1)
    f1, f2 = api.fragments(t['w1']), api.fragments(t['w2'])
    frozen = _Frozen(x, b1, b2, res, lw, lb)
    view, buf = _out_rows(api, R, O, out_pad)
    code = api.ffn(x, f1, b1, f2, b2, R, I, H, O, res, lw, lb, EPS, view)
    assert code == 0, code
    got = _out_ok(view, buf)
    frozen.check()
    return got


def check_ffn(api, name, case, real, tag=''):
    assert case['stats'] is None or (real and case['res'] and case['ln'])
    t = ffn_inputs(case, real)
    got = run_ffn(api, t, out_pad=12 if case['pad'] else 0)
    x, w1, b1, w2, b2 = (t[k].double() for k in ('x', 'w1', 'b1', 'w2', 'b2'))
    res = t['res'].double() if t['res'] is not None else None
    y = _ffn64(x, w1, b1, w2, b2, res)
    layer = ('B' if real else 'A') + tag
    if not real:
        hidden = torch.relu(x @ w1.t() + b1)
        max_hidden = 16 * case['I'] + 4
        assert hidden.max().item() <= max_hidden < 2 ** 16 and max_hidden * 4 * case['H'] + 8 < EXACT_LIMIT
        if not case['ln']:
            bad = int((got != y).sum())
            observed(f'{api.name} rows_ffn_x3 {name} layer {layer}: elements that differ from int64 = {bad} of {y.numel()}')
            assert bad == 0 and torch.equal(got.long(), y.long())
            return
    e = ffn_e(x, w1, b1, w2, b2, res) if real else 0
    if case['ln']:
        exact, bound = ln_bound(y, e, t['lw'], t['lb'], EPS, ln_depth(case['O']))
    else:
        exact, bound = y, e
    err = (got - exact).abs()
    e16 = keep = None
    if real:
        y16 = _ffn64(t['x'], t['w1'], b1, t['w2'], b2, res, bf16=True)
        e16 = ((ln_ref(y16, t['lw'], t['lb'], EPS) if case['ln'] else y16) - exact).abs()
        keep = [r for r in range(case['rows']) if r != t['const_row']]
    _report(api, 'rows_ffn_x3', name, layer, err, bound, e16, keep)


def check_ffn_refusals(api):
    g = _gen(4)
    R = 5
    for I, H, O in ((80, 96, 80), (104, 64, 80), (80, 64, 84)):
        x = api.to(torch.randn(R, I, generator=g))
        f1, f2 = api.fragments(torch.randn(H, I, generator=g)), api.fragments(torch.randn(O, H, generator=g))
        out = api.full((R, O), NAN)
        assert api.ffn(x, f1, api.to(torch.zeros(H)), f2, api.to(torch.zeros(O)), R, I, H, O, None, None, None, EPS, out) == UNSUPPORTED
        assert torch.isnan(out).all(), 'a refused call wrote to out'


# ------------------------------------------------------------------------------------------------------------------ fbbev_rows_tail_ffn_x3 / _planes
def _tc(rows, E, H, res0, S, pad=False, stats=None):
    return dict(rows=rows, E=E, H=H, res0=res0, S=S, pad=pad, stats=stats)


TAIL_EPS0, TAIL_EPS1 = 1e-5, 1e-6
# S = tokens per image of the planes form: one image of all rows, 11, 35, 65 (not multiples of 4), 8
TAIL_CASES = {
    'r1_e16_h64': _tc(1, 16, 64, True, 1),
    'r33_e32_h128': _tc(33, 32, 128, False, 11, pad=True),
    'r130_e48_h192': _tc(130, 48, 192, True, 65),
    'r70_e64_h64': _tc(70, 64, 64, False, 35),
    'r200_e80_h320': _tc(200, 80, 320, True, 200, pad=True),
    'r40_e80_h1088': _tc(40, 80, 1088, True, 8),
    'r33_e80_h64_mean100': _tc(33, 80, 64, True, 11, stats='mean'),
    'r17_e32_h128_constant_row': _tc(17, 32, 128, True, 17, stats='const'),
}


def tail_inputs(case, real):
    """layer A: the tail's operands (x, W0, b0, res0) are integers; LayerNorm0's output is real, so the FFN's are real in both layers"""
    R, E, H = case['rows'], case['E'], case['H']
    g = _gen(5, R, E, H, real)
    l0w, l0b = torch.rand(E, generator=g) + 0.5, torch.randn(E, generator=g) * 0.2
    l1w, l1b = torch.rand(E, generator=g) + 0.5, torch.randn(E, generator=g) * 0.2
    w1, b1 = torch.randn(H, E, generator=g) / E ** 0.5, torch.randn(H, generator=g) * 0.3
    w2, b2 = torch.randn(E, H, generator=g) / H ** 0.5, torch.randn(E, generator=g) * 0.3
    if real:
        x, w0, b0 = torch.randn(R, E, generator=g), torch.randn(E, E, generator=g) / E ** 0.5, torch.randn(E, generator=g) * 0.3
        res0 = torch.randn(R, E, generator=g)
    else:
        x, w0, b0, res0 = _ints((R, E), g), _ints((E, E), g), _ints((E,), g), _ints((R, E), g)
    if case['stats'] == 'mean':
        b2 = b2 + 100.0                                     # LayerNorm1's input too: y1 + W2 h + b2
    res0, const_row = _stats_rows(case['stats'], res0, (x,), (b0,))
    return dict(x=_rows(x, 8 if case['pad'] else 0), w0=w0, b0=b0, res0=_rows(res0, 4 if case['pad'] else 0) if case['res0'] else None,
                l0w=l0w, l0b=l0b, w1=w1, b1=b1, w2=w2, b2=b2, l1w=l1w, l1b=l1b, const_row=const_row)


def check_tail(api, name, case, real):
    assert case['stats'] is None or (real and case['res0'])
    R, E, H, S = case['rows'], case['E'], case['H'], case['S']
    t = tail_inputs(case, real)
    names = ('x', 'b0', 'res0', 'l0w', 'l0b', 'b1', 'b2', 'l1w', 'l1b')
    d = {k: api.to(t[k]) for k in names}
    f0, f1, f2 = api.fragments(t['w0']), api.fragments(t['w1']), api.fragments(t['w2'])
    frozen = _Frozen(*d.values())

    def call(out, S=0):
        code = api.tail(d['x'], f0, d['b0'], d['res0'], d['l0w'], d['l0b'], TAIL_EPS0, f1, d['b1'], f2, d['b2'], R, E, H, d['l1w'], d['l1b'],
                        TAIL_EPS1, out, S)
        assert code == 0, code

    view, buf = _out_rows(api, R, E, 12 if case['pad'] else 0)
    call(view)
    got = _out_ok(view, buf)
    # the planes form: (rows / S, E, S), the same words
    planes = api.full((R // S, E, S), NAN)
    call(planes, S)
    assert not torch.isnan(planes).any()
    assert torch.equal(planes, view.reshape(R // S, S, E).transpose(1, 2)), 'the planes form differs from the rows form'
    # the two kernels it replaces: fbbev_rows_linear_x3_ln -> fbbev_rows_ffn_x3(t1, ..., residual = t1)
    t1 = api.full((R, E), NAN)
    assert api.linear_ln(d['x'], f0, d['b0'], R, E, E, d['res0'], d['l0w'], d['l0b'], TAIL_EPS0, t1) == 0
    two = api.full((R, E), NAN)
    assert api.ffn(t1, f1, d['b1'], f2, d['b2'], R, E, H, E, t1, d['l1w'], d['l1b'], TAIL_EPS1, two) == 0
    frozen.check()
    two = two.cpu().double()

    x, w0, b0, w1, b1, w2, b2 = (t[k].double() for k in ('x', 'w0', 'b0', 'w1', 'b1', 'w2', 'b2'))
    res0 = t['res0'].double() if t['res0'] is not None else None
    d_s = ln_depth(E)
    y0 = x @ w0.t() + b0 + (res0 if res0 is not None else 0)
    if real:
        e0 = gemm_e(x, w0, b0, res0)
    else:
        assert (x.abs() @ w0.abs().t()).max().item() + 8 < EXACT_LIMIT
        e0 = 0
    y1, e1 = ln_bound(y0, e0, t['l0w'], t['l0b'], TAIL_EPS0, d_s)
    y = _ffn64(y1, w1, b1, w2, b2, y1)
    e = ffn_e(y1, w1, b1, w2, b2, y1, e_x=e1, e_res=e1)
    exact, bound = ln_bound(y, e, t['l1w'], t['l1b'], TAIL_EPS1, d_s)
    err = (got - exact).abs()
    e16 = keep = None
    if real:
        y0b = _bf(t['x']) @ _bf(t['w0']).t() + b0 + (res0 if res0 is not None else 0)
        y1b = ln_ref(y0b, t['l0w'], t['l0b'], TAIL_EPS0)
        e16 = (ln_ref(_ffn64(y1b, t['w1'], b1, t['w2'], b2, y1b, bf16=True), t['l1w'], t['l1b'], TAIL_EPS1) - exact).abs()
        keep = [r for r in range(R) if r != t['const_row']]
    scale = max(1.0, exact.abs().max().item())
    gap = (got - two).abs().max().item()
    observed(f'{api.name} rows_tail_ffn_x3 {name}: against the two kernels it replaces max|diff| = {gap:.3e} (bar {1e-5 * scale:.3e}), '
             f'bit for bit: {bool(torch.equal(got, two))}; planes form (S = {S}) word for word')
    _report(api, 'rows_tail_ffn_x3', name, 'B' if real else 'A', err, bound, e16, keep)
    assert gap <= 1e-5 * scale, gap


def check_tail_refusals(api):
    g = _gen(6)
    R, H = 6, 64

    def attempt(E, x, S=0, out_shape=None):
        z = lambda n: api.to(torch.zeros(n))  # noqa: E731
        f0, f1, f2 = (api.fragments(torch.randn(*s, generator=g)) for s in ((E, E), (H, E), (E, H)))
        out = api.full(out_shape or (R, E), NAN)
        code = api.tail(x, f0, z(E), None, z(E), z(E), EPS, f1, z(H), f2, z(E), x.shape[0], E, H, z(E), z(E), EPS, out, S)
        assert torch.isnan(out).all(), 'a refused call wrote to out'
        return code

    assert attempt(72, api.to(torch.randn(R, 72, generator=g))) == UNSUPPORTED                 # embed no multiple of 16
    assert attempt(80, api.to(torch.randn(R, 80, generator=g)), S=4, out_shape=(2, 80, 4)) == BADARG   # 6 rows are not whole images of 4
    flat = api.to(torch.randn((R + 1) * 80, generator=g))
    assert attempt(80, flat[2:2 + R * 80].view(R, 80)) == UNSUPPORTED                         # a view 8 bytes off a 16-byte boundary


# ------------------------------------------------------------------------------------------------------------------ fbbev_rows_linear_x3_planes / _planes_e
def _pc(images, S, M, Dh, I, bias=True):
    return dict(images=images, S=S, M=M, Dh=Dh, I=I, bias=bias)


PLANES_CASES = {
    'b3_s7_m2_d10_i80': _pc(3, 7, 2, 10, 80),                 # head_dim no power of two: the reciprocal division
    'b1_s33_m8_d10_i80': _pc(1, 33, 8, 10, 80, bias=False),
    'b2_s5_m4_d2_i8': _pc(2, 5, 4, 2, 8),                      # the smallest head
    'b2_s9_m16_d10_i80': _pc(2, 9, 16, 10, 80),               # O = 160: head 12 = outputs 120-129, across the two output chunks
    'b2_s9_m8_d10_i136': _pc(2, 9, 8, 10, 136),               # two K chunks: the plain kernel's plane epilogue, not the persistent one's
}
PLANES_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def check_planes(api, name, case, real):
    B, S, M, Dh, I = (case[k] for k in ('images', 'S', 'M', 'Dh', 'I'))
    R, O = B * S, M * Dh
    g = _gen(7, B, S, M, Dh, I, real)
    if real:
        x, w, b = torch.randn(R, I, generator=g), torch.randn(O, I, generator=g) / I ** 0.5, torch.randn(O, generator=g) * 0.3
    else:
        x, w, b = _ints((R, I), g), _ints((O, I), g), _ints((O,), g)
        assert 16 * I + 4 < EXACT_LIMIT
    b = b if case['bias'] else None
    dx, db = api.to(_rows(x, 8)), api.to(b)
    f = api.fragments(w)
    frozen = _Frozen(dx, db)
    got = {}
    for dt in PLANES_DTYPES:
        out = api.full((B, M, S, Dh), NAN, dtype=dt)
        assert api.planes(dx, f, db, R, I, O, S, Dh, out) == 0
        assert not torch.isnan(out).any(), dt
        got[dt] = out.cpu()
    frozen.check()
    y = x.double() @ w.double().t() + (b.double() if b is not None else 0)
    as_planes = lambda rows: rows.reshape(B, S, M, Dh).permute(0, 2, 1, 3).contiguous()  # noqa: E731
    exact = as_planes(y)
    word = lambda v: v.view(torch.int16)  # noqa: E731
    if real:
        for dt in PLANES_DTYPES[1:]:                           # one rounding of the same call's f32 planes
            assert torch.equal(word(got[dt]), word(got[torch.float32].to(dt))), dt
        err = (got[torch.float32].double() - exact).abs()
        e16 = (as_planes(_bf(x) @ _bf(w).t() + (b.double() if b is not None else 0)) - exact).abs()
        _report(api, 'rows_linear_x3_planes', name, 'B', err, as_planes(gemm_e(x.double(), w.double(), b.double() if b is not None else None, None)), e16)
        return
    bad = int((got[torch.float32].double() != exact).sum())
    bad16 = sum(int((word(got[dt]) != word(exact.long().float().to(dt))).sum()) for dt in PLANES_DTYPES[1:])
    observed(f'{api.name} rows_linear_x3_planes {name} layer A: elements that differ from int64 = {bad} of {exact.numel()} (f32), '
             f'{bad16} of {2 * exact.numel()} (bf16 and f16 words)')
    assert bad == 0 and bad16 == 0 and torch.equal(got[torch.float32].long(), exact.long())


def check_planes_refusals(api):
    g = _gen(8)
    I = 16
    for R, S, M, Dh, O in ((6, 3, 4, 5, 20), (6, 3, 2, 8, 20), (7, 3, 2, 10, 20)):      # odd head_dim; O % head_dim != 0; rows % S != 0
        x = api.to(torch.randn(R, I, generator=g))
        f = api.fragments(torch.randn(O, I, generator=g))
        for dt in PLANES_DTYPES:
            out = api.full((R * O + 16,), NAN, dtype=dt)
            assert api.planes(x, f, None, R, I, O, S, Dh, out) == UNSUPPORTED
            assert torch.isnan(out).all(), 'a refused call wrote to out'


# ------------------------------------------------------------------------------------------------------------------ fbbev_layernorm
LAYERNORM_ROWS = (1, 7, 8, 9, 37)            # a workgroup is 8 half-waves: a part, a full one, one row into the second, five
LAYERNORM_C = (4, 80, 124, 128)
LAYERNORM_STATS = ('mean', 'const')


def check_layernorm(api, rows, C, with_res, eps, stats=None):
    g = _gen(9, rows, C, with_res, eps > 0)
    x = torch.randn(rows, C, generator=g) * 3 + 1.5
    r = torch.randn(rows, C, generator=g) if with_res else None
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    if stats == 'mean':
        x = torch.randn(rows, C, generator=g) + 100.0
    if stats == 'const':
        x[rows // 2] = CONST_VALUE
        if with_res:
            r[rows // 2] = 0.0
    assert eps > 0 or stats is None                           # eps = 0 only on rows with spread
    dx, dr, dw, db = api.to(x), api.to(r), api.to(w), api.to(b)
    frozen = _Frozen(dx, dr, dw, db)
    out = api.full((rows, C), NAN)
    assert api.layernorm(dx, dr, dw, db, eps, rows, C, out) == 0
    assert not torch.isnan(out).any()
    frozen.check()
    y = x.double() + (r.double() if with_res else 0)
    e = U24 * (x.double().abs() + r.double().abs()) if with_res else 0
    exact, bound = ln_bound(y, e, w, b, eps, ln_depth(C, mfma=False))
    err = (out.cpu().double() - exact).abs()
    observed(f'{api.name} layernorm {rows} x {C} residual {with_res} eps {eps:g}{" " + stats if stats else ""}: '
             f'max|err| = {err.max().item():.3e}, max err / bound = {(err / bound).max().item():.4f}')
    assert (err / bound).max().item() <= 1.0


def check_layernorm_refusals(api):
    for C in (6, 132):
        x, w, b = api.to(torch.randn(8, C)), api.to(torch.ones(C)), api.to(torch.zeros(C))
        out = api.full((8, C), NAN)
        assert api.layernorm(x, None, w, b, EPS, 8, C, out) == UNSUPPORTED
        assert torch.isnan(out).all(), 'a refused call wrote to out'


def run_all_ffn(api, tag=''):
    """every FFN case, both layers (the GPU test's child process under FBBEV_FFN_HC=64) -> the number of checks"""
    n = 0
    for name, case in FFN_CASES.items():
        if case['stats'] is None:
            check_ffn(api, name, case, False, tag)
            n += 1
        check_ffn(api, name, case, True, tag)
        n += 1
    return n
