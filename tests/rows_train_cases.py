"""Case tables, input generators, references and bounds for the training-side row kernels, shared by the GPU test
(tests/test_gpu_rows_train_kernels.py, through fb_bev_amd._capi) and the emulator test (tests/test_emu_rows_train_kernels.py, through
tests/emu/emu_capi.py): fbbev_rows_wgrad_x3, fbbev_rows_linear_x3 / _add / _train, fbbev_softmax_groups / _bwd, fbbev_sum_leading,
fbbev_sum_partials and fbbev_layernorm_bwd at the smallest shapes at which each of their code paths exists.

Two layers of checks for the split-operand MFMA kernels.

Layer A, exact integers.  Every operand is an integer in [-4, 4] (the mask in {-1, 0, 1}): exact in bf16, so the lo halves are zero,
every product and every partial sum is an integer below 2^24 and fp32 addition is exact in ANY order.  The result must equal the
int64 reference bit for bit -- no tolerance, whatever the row count.  A row, column, tile or split that is dropped, duplicated or
misplaced changes an integer.

Layer B, real values with full mantissas.  Componentwise against float64:  |got - exact| <= c * S  with S the same product taken on
absolute values (wgrad: |gy|^T |x|; linear: |x| |W|^T + |b| [+ |residual|]).  c from the arithmetic, not from a measurement:
  * bf16 keeps 8 significant bits: v = hi + lo + e with |e| <= 2^-16 |v| (two roundings of 2^-8 each, a truncating conversion included);
  * the product (ah + al)(bh + bl) drops al * bl, at most 2^-16 |a b|;
  * so the split costs at most 3 * 2^-16 per product to first order: 4 * 2^-16 with the higher-order terms rounded up;
  * an fp32 accumulation of depth n costs at most n * 2^-24 of the sum of magnitudes.
Linear layers: depth I products + the bias add + the residual add  ->  c = 4 * 2^-16 + (I + 2) * 2^-24.
wgrad: a workgroup accumulates kps steps of 32 rows, the fixed-order reduction adds n_split partial results as 8 lane sums and then
the 8 lanes  ->  c = 4 * 2^-16 + (32 * kps + n_split + 8) * 2^-24.  kps and n_split are the literal numbers of the table below (the
plan of wgrad_plan_make in fb_bev_amd/csrc/capi_train.hip under the default knobs); a test checks them against the workspace size the
library reports, which is a function of n_split alone.  The bias gradient has no split error (fp32 adds only): (32 * kps + n_split + 8)
* 2^-24 * sum |gy| covers its 2 * kps adds per thread, the 8 row-pair groups and the reduction.
Each real-valued case also proves that the lo terms are applied: its largest error is at least 30 times smaller than that of the same
product on plain bf16-rounded operands.

Plain Python and CPU torch only; the adapters import their library on first use.
"""
import ctypes

import torch

U16, U24 = 2.0 ** -16, 2.0 ** -24
EXACT_LIMIT = 2 ** 24


# ------------------------------------------------------------------------------------------------------------------ adapters
class GpuApi:
    """fb_bev_amd._capi on cuda:0"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi
        self.c = _capi
        self.device = torch.device('cuda:0')

    def to(self, t):
        """CPU tensor or strided CPU view -> the same values with the same strides on the device"""
        if t is None:
            return None
        base = t._base if t._base is not None else t
        d = base.to(self.device)
        return d if t._base is None else d.as_strided(t.shape, t.stride(), t.storage_offset())

    def empty_rows(self, R, O, pad=0):
        buf = torch.full((R, O + pad), float('nan'), device=self.device)
        return buf[:, :O], buf

    def wgrad(self, gy, x, bias=True, addend=None):
        return self.c.rows_wgrad_x3(gy, x, bias=bias, addend=addend)

    def wgrad_ws_bytes(self, rows, I, O):
        return self.c.lib().fbbev_rows_wgrad_x3_ws_bytes(rows, I, O)

    def linear(self, x, w, b, relu=False, out=None, addend=None):
        return self.c.rows_linear_x3(x, self.c.rows_linear_x3_fragments(w), b, w.shape[0], relu=relu, out=out, addend=addend)

    def linear_train(self, x, w, b, relu=False, addend=None, residual=None, mask=None, out=None):
        return self.c.rows_linear_x3_train(x, self.c.rows_linear_x3_fragments(w), b, w.shape[0], relu=relu, addend=addend,
                                           residual=residual, mask=mask, out=out)

    def softmax(self, x, group, out=None):
        return self.c.softmax_groups(x, group, out=out)

    def softmax_bwd(self, y, gy, group, out=None):
        return self.c.softmax_groups_bwd(y, gy, group, out=out)

    def softmax_code(self, x, n_groups, group, out):
        with torch.cuda.device(self.device):
            return self.c.lib().fbbev_softmax_groups(ctypes.c_void_p(x.data_ptr()), n_groups, group, ctypes.c_void_p(out.data_ptr()),
                                                     self.c._stream())

    def sum_leading(self, x, x2=None):
        return self.c.sum_leading(x, x2)

    def sum_partials(self, part):
        n, ln = part.shape[0], part.numel() // part.shape[0]
        out = torch.full((ln,), float('nan'), device=self.device)
        with torch.cuda.device(self.device):
            code = self.c.lib().fbbev_sum_partials(ctypes.c_void_p(part.data_ptr()), n, ln, ctypes.c_void_p(out.data_ptr()), self.c._stream())
        assert code == 0, code
        return out

    def layernorm_bwd(self, x, gy, w, eps):
        return self.c.layernorm_bwd(x, gy, w, eps)


class EmuApi:
    """tests/emu/emu_capi.py: the same kernels compiled for the CPU"""
    name = 'emu'

    def __init__(self):
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
        import emu_capi
        self.E = emu_capi
        self.device = torch.device('cpu')

    def to(self, t):
        return t

    def empty_rows(self, R, O, pad=0):
        buf = torch.full((R, O + pad), float('nan'))
        return buf[:, :O], buf

    def wgrad(self, gy, x, bias=True, addend=None):
        code, gw, gb = self.E.rows_wgrad_x3(gy, x, with_bias=bias, addend=addend)
        assert code == 0, code
        return gw, gb

    def wgrad_ws_bytes(self, rows, I, O):
        return self.E.lib().fbbev_rows_wgrad_x3_ws_bytes(rows, I, O)

    def linear(self, x, w, b, relu=False, out=None, addend=None):
        code, out = self.E.rows_linear_x3(x, w, b, relu=relu, out=out, addend=addend)
        assert code == 0, code
        return out

    def linear_train(self, x, w, b, relu=False, addend=None, residual=None, mask=None, out=None):
        code, out = self.E.rows_linear_x3_train(x, w, b, relu=relu, addend=addend, residual=residual, mask=mask, out=out)
        assert code == 0, code
        return out

    def softmax(self, x, group, out=None):
        out = torch.full_like(x, float('nan')) if out is None else out
        assert self.softmax_code(x, x.numel() // group, group, out) == 0
        return out

    def softmax_bwd(self, y, gy, group, out=None):
        out = torch.full_like(gy, float('nan')) if out is None else out
        E = self.E
        assert E.lib().fbbev_softmax_groups_bwd(E.p(y), E.p(gy), y.numel() // group, group, E.p(out), None) == 0
        return out

    def softmax_code(self, x, n_groups, group, out):
        return self.E.lib().fbbev_softmax_groups(self.E.p(x), n_groups, group, self.E.p(out), None)

    def sum_leading(self, x, x2=None):
        code, out = self.E.sum_leading(x, x2)
        assert code == 0, code
        return out

    def sum_partials(self, part):
        code, out = self.E.sum_partials(part)
        assert code == 0, code
        return out

    def layernorm_bwd(self, x, gy, w, eps):
        """as fb_bev_amd._capi.layernorm_bwd: the kernel's partial rows summed by fbbev_sum_partials"""
        E = self.E
        C = x.shape[-1]
        rows = x.numel() // C
        n = E.lib().fbbev_layernorm_bwd_partials(rows)
        partial = torch.full((n, 2, C), float('nan'))
        gx = torch.full_like(x, float('nan'))
        E.ok(E.lib().fbbev_layernorm_bwd(E.p(x), E.p(gy), E.p(w), eps, rows, C, E.p(gx), E.p(partial), None))
        s = self.sum_partials(partial).view(2, C)
        return gx, s[0], s[1]


def observed(text):
    print(f'[observed] {text}')


def _ints(shape, g, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _wide(values, pad):
    """(R, C) values -> the same values as a view of a (R, C + pad) tensor whose other columns are NaN (nothing may read them)"""
    R, C = values.shape
    buf = torch.full((R, C + pad), float('nan'))
    buf[:, :C] = values
    return buf[:, :C]


# ------------------------------------------------------------------------------------------------------------------ fbbev_rows_wgrad_x3
# plan columns: the default-knob plan of wgrad_plan_make, as literal numbers (ks = 32-row steps, kps = steps per split)
def _wg(I, O, rows, real, ks, kps, n_split, nti, n_oc, n_ic, amt, period=None, env=None):
    return dict(I=I, O=O, rows=rows, real=real, ks=ks, kps=kps, n_split=n_split, nti=nti, n_oc=n_oc, n_ic=n_ic, amt=amt, period=period,
                env=env or {})


WGRAD_CASES = {
    # NTI = 5; 263 steps in 132 splits of 2, the last split has one step, that step has 7 rows
    'i80_o80_r8391': _wg(80, 80, 8391, False, ks=263, kps=2, n_split=132, nti=5, n_oc=1, n_ic=1, amt=5),
    # four output chunks; 131 steps in 66 splits, the last split has one step (5 rows)
    'i80_o512_r4165': _wg(80, 512, 4165, True, ks=131, kps=2, n_split=66, nti=5, n_oc=4, n_ic=1, amt=8),
    # amt = 2: the narrow-LDS form
    'i80_o32_r77': _wg(80, 32, 77, True, ks=3, kps=1, n_split=3, nti=5, n_oc=1, n_ic=1, amt=2),
    # fewer rows than one step, and an odd count inside a packed (row, row + 1) pair
    'i80_o96_r5': _wg(80, 96, 5, True, ks=1, kps=1, n_split=1, nti=5, n_oc=1, n_ic=1, amt=6),
    'i80_o96_r1': _wg(80, 96, 1, True, ks=1, kps=1, n_split=1, nti=5, n_oc=1, n_ic=1, amt=6),
    # NTI = 8; three input chunks, the last one half filled
    'i320_o80_r257': _wg(320, 80, 257, True, ks=9, kps=1, n_split=9, nti=8, n_oc=1, n_ic=3, amt=5),
    'i512_o80_r2079': _wg(512, 80, 2079, True, ks=65, kps=1, n_split=65, nti=8, n_oc=1, n_ic=4, amt=5),
    # a 4-column last input tile, a 4-output last chunk, three output chunks
    'i132_o260_r40': _wg(132, 260, 40, True, ks=2, kps=1, n_split=2, nti=8, n_oc=3, n_ic=2, amt=8),
    # the smallest legal layer
    'i8_o4_r33': _wg(8, 4, 33, True, ks=2, kps=1, n_split=2, nti=5, n_oc=1, n_ic=1, amt=1),
}
# the periodic addend (x[r] + addend[r % period]); 32 % period != 0 in both
WGRAD_ADDEND_CASES = {
    'i80_o64_r225_p75': _wg(80, 64, 225, True, ks=8, kps=1, n_split=8, nti=5, n_oc=1, n_ic=1, amt=4, period=75),
    'i80_o80_r8391_p2797': _wg(80, 80, 8391, False, ks=263, kps=2, n_split=132, nti=5, n_oc=1, n_ic=1, amt=5, period=2797),
}


def wgrad_c(case):
    return 4 * U16 + (32 * case['kps'] + case['n_split'] + 8) * U24


def wgrad_bias_c(case):
    return (32 * case['kps'] + case['n_split'] + 8) * U24


def wgrad_ws_bytes_expected(case):
    """capi_train.hip: the partial weight gradients and the partial bias gradients of n_split splits, each rounded up to 256 bytes"""
    up = lambda n: (n + 255) // 256 * 256
    return up(case['n_split'] * case['O'] * case['I'] * 4) + up(case['n_split'] * case['O'] * 4)


def wgrad_inputs(case, real, seed=0):
    """-> (gy, x, addend or None): CPU rows as views of wider tensors (row strides O + 4 and I + 8 floats, NaN in the other columns)"""
    I, O, R = case['I'], case['O'], case['rows']
    g = torch.Generator().manual_seed(1000 * seed + R * 7 + I + O + (1 if real else 0))
    if real:
        gy, x = torch.randn(R, O, generator=g), torch.randn(R, I, generator=g) * 2
        add = torch.randn(case['period'], I, generator=g) if case['period'] else None
    else:
        gy, x = _ints((R, O), g), _ints((R, I), g)
        add = _ints((case['period'], I), g) if case['period'] else None
    return _wide(gy, 4), _wide(x, 8), (_wide(add, 8) if add is not None else None)


def _pre_added(x, add):
    R, I = x.shape
    P = add.shape[0]
    return (x.reshape(R // P, P, I) + add[None]).reshape(R, I).contiguous()


def check_wgrad_plan(api, case):
    assert case['ks'] == (case['rows'] + 31) // 32 and case['n_split'] == (case['ks'] + case['kps'] - 1) // case['kps']
    assert api.wgrad_ws_bytes(case['rows'], case['I'], case['O']) == wgrad_ws_bytes_expected(case)


def _wgrad_variants(api, gy, x, add=None):
    """strided run -> (gw, gb); asserts along the way that the dense run, the run without a bias gradient and a second run give the
    same bits, and that a NaN outside the operands' columns is never read"""
    dgy, dx, dadd = api.to(gy), api.to(x), api.to(add)
    gw, gb = api.wgrad(dgy, dx, addend=dadd)
    assert not torch.isnan(gw).any() and not torch.isnan(gb).any()
    gw2, gb2 = api.wgrad(dgy, dx, addend=dadd)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2), 'a second run differs'
    gw3, gb3 = api.wgrad(dgy, dx, bias=False, addend=dadd)
    assert gb3 is None and torch.equal(gw, gw3), 'grad_weight differs without the bias gradient'
    gw4, gb4 = api.wgrad(dgy.contiguous(), dx.contiguous(), addend=dadd.contiguous() if dadd is not None else None)
    assert torch.equal(gw, gw4) and torch.equal(gb, gb4), 'dense rows and strided rows differ'
    return gw.cpu(), gb.cpu()


def check_wgrad_exact(api, name, case):
    """layer A"""
    gy, x, add = wgrad_inputs(case, real=False)
    xs = x if add is None else _pre_added(x, add)
    ew, eb = gy.long().t() @ xs.long(), gy.long().sum(0)
    assert max(ew.abs().max().item(), eb.abs().max().item(), (gy.abs().t() @ xs.abs()).max().item()) < EXACT_LIMIT
    gw, gb = _wgrad_variants(api, gy, x, add)
    bad_w, bad_b = int((gw.double() != ew.double()).sum()), int((gb.double() != eb.double()).sum())
    observed(f'{api.name} rows_wgrad_x3 {name} layer A: elements that differ from int64 = {bad_w} of {ew.numel()} (weight), '
             f'{bad_b} of {eb.numel()} (bias)')
    assert bad_w == 0 and bad_b == 0
    if add is not None:
        pw, pb = api.wgrad(api.to(gy), api.to(xs))
        assert torch.equal(pw.cpu(), gw) and torch.equal(pb.cpu(), gb), 'the addend form differs from the plain entry on pre-added rows'


def check_wgrad_real(api, name, case):
    """layer B"""
    gy, x, add = wgrad_inputs(case, real=True)
    gw, gb = _wgrad_variants(api, gy, x, add)
    xs = x if add is None else _pre_added(x, add)
    if add is not None:
        pw, pb = api.wgrad(api.to(gy), api.to(xs))
        assert torch.equal(pw.cpu(), gw) and torch.equal(pb.cpu(), gb), 'the addend form differs from the plain entry on pre-added rows'
    gd, xd = gy.double(), xs.double()
    ew, eb = gd.t() @ xd, gd.sum(0)
    S, Sb = gd.abs().t() @ xd.abs(), gd.abs().sum(0)
    err, errb = (gw.double() - ew).abs(), (gb.double() - eb).abs()
    ratio, ratiob = (err / (wgrad_c(case) * S)).max().item(), (errb / (wgrad_bias_c(case) * Sb)).max().item()
    e16 = (gy.bfloat16().double().t() @ xs.bfloat16().double() - ew).abs().max().item()
    observed(f'{api.name} rows_wgrad_x3 {name} layer B: max err / (c S) = {ratio:.3f} (weight), {ratiob:.3f} (bias); '
             f'max|err| = {err.max().item():.3e}, plain bf16 operands {e16:.3e}')
    assert ratio <= 1.0 and ratiob <= 1.0
    assert err.max().item() * 30 < e16


# ------------------------------------------------------------------------------------------------------------------ fbbev_rows_linear_x3*
# (rows, I, O, real, period of the addend (rows % period == 0)).  k_rows_linear_x3p (one K chunk, no addend) gives a workgroup every
# n_slots-th tile of 128 rows, n_slots = min(512 / n_oc, tiles) (rows_linear_x3_dispatch in fb_bev_amd/csrc/capi.hip): 65573 rows at two
# output chunks are 513 tiles on 256 slots -- slot 0 walks tiles 0, 256 and 512, and tile 512 has 37 rows.
def _lin(rows, I, O, real, period, env=None):
    return dict(rows=rows, I=I, O=O, real=real, period=period, env=env or {})


LINEAR_CASES = {
    'r150_i80_o160': _lin(150, 80, 160, True, 50),
    'r593_i80_o160': _lin(593, 80, 160, True, 593),
    'r129_i80_o512': _lin(129, 80, 512, True, 43),
    'r257_i128_o96': _lin(257, 128, 96, True, 257),
    'r700_i96_o80': _lin(700, 96, 80, True, 175),
    'r130_i320_o80': _lin(130, 320, 80, True, 65),             # three K chunks
    'r75_i512_o80': _lin(75, 512, 80, True, 25),               # four K chunks
    'r1_i80_o80': _lin(1, 80, 80, True, 1),
    'r127_i80_o80': _lin(127, 80, 80, True, 127),
    'r128_i80_o80': _lin(128, 80, 80, True, 64),
    'r129_i80_o80': _lin(129, 80, 80, True, 43),
    'r65573_i80_o160_three_tiles_per_workgroup': _lin(65573, 80, 160, False, 2851),
}


def linear_c(I):
    return 4 * U16 + (I + 2) * U24


def linear_inputs(case, real):
    """-> dict of CPU tensors: x (row stride I + 8), w, b, res / mask (row stride O + 4), add (period, I)"""
    R, I, O = case['rows'], case['I'], case['O']
    g = torch.Generator().manual_seed(R + 3 * I + 5 * O + (1 if real else 0))
    if real:
        x, w, b = torch.randn(R, I, generator=g) * 2, torch.randn(O, I, generator=g) * 0.2, torch.randn(O, generator=g)
        res, mask, add = torch.randn(R, O, generator=g), torch.randn(R, O, generator=g), torch.randn(case['period'], I, generator=g)
    else:
        x, w, b = _ints((R, I), g), _ints((O, I), g), _ints((O,), g)
        res, mask, add = _ints((R, O), g), _ints((R, O), g, -1, 1), _ints((case['period'], I), g)
    return dict(x=_wide(x, 8), w=w, b=b, res=_wide(res, 4), mask=_wide(mask, 4), add=add)


def _linear_variants(api, t):
    """every epilogue variant -> dict of device tensors.  Asserts what holds for ANY data: NaN outside the operands' columns is never
    read, nothing is written outside `out`, and the training epilogue, the in-place form, the strided form and the addend form are
    the plain product's bits put through the torch expression of the epilogue."""
    d = {k: api.to(v) for k, v in t.items()}
    x, w, b, res, mask, add = d['x'], d['w'], d['b'], d['res'], d['mask'], d['add']
    R, O = res.shape
    res_c, mask_c = res.contiguous(), mask.contiguous()
    zero = torch.zeros((), device=x.device)
    out = {}
    view, buf = api.empty_rows(R, O, pad=4)
    out['plain'] = api.linear(x, w, b, out=view)
    assert out['plain'] is view and not torch.isnan(view).any() and torch.isnan(buf[:, O:]).all()
    out['relu'] = api.linear(x, w, b, relu=True)
    assert torch.equal(out['relu'], out['plain'].relu())
    out['nobias'] = api.linear(x, w, None)
    out['train_plain'] = api.linear_train(x, w, b)
    assert torch.equal(out['train_plain'], out['plain'])
    out['train_relu_nobias'] = api.linear_train(x, w, None, relu=True)
    assert torch.equal(out['train_relu_nobias'], out['nobias'].relu())
    out['mask_res'] = api.linear_train(x, w, b, residual=res_c, mask=mask_c)
    assert torch.equal(out['mask_res'], torch.where(mask_c > 0, out['plain'], zero) + res_c)
    out['res'] = api.linear_train(x, w, b, residual=res_c)
    assert torch.equal(out['res'], out['plain'] + res_c)
    acc = res_c.clone()
    assert api.linear_train(x, w, b, residual=acc, out=acc) is acc                        # residual is out: a running sum
    assert torch.equal(acc, out['res'])
    acc = res_c.clone()
    api.linear_train(x, w, b, relu=True, residual=acc, mask=mask_c, out=acc)
    assert torch.equal(acc, torch.where(mask_c > 0, out['relu'], zero) + res_c)
    view, buf = api.empty_rows(R, O, pad=12)                                               # strided out, residual and mask rows
    api.linear_train(x, w, b, residual=res, mask=mask, out=view)
    assert torch.equal(view, out['mask_res']) and torch.isnan(buf[:, O:]).all()
    summed = _pre_added(x, add)
    out['add'] = api.linear(x, w, b, addend=add)
    assert torch.equal(out['add'], api.linear(summed, w, b)), 'the addend form differs from the plain entry on pre-added rows'
    out['add_res'] = api.linear_train(x, w, b, addend=add, residual=res_c)
    assert torch.equal(out['add_res'], out['add'] + res_c)
    for k, v in out.items():
        assert not torch.isnan(v).any(), k
    return {k: v.cpu() for k, v in out.items()}


def check_linear_exact(api, name, case):
    """layer A: every variant against int64"""
    t = linear_inputs(case, real=False)
    x, w, b, res, mask, add = (t[k].long() for k in ('x', 'w', 'b', 'res', 'mask', 'add'))
    got = _linear_variants(api, t)
    xa = _pre_added(x, add)
    mag = xa.abs() @ w.abs().t() + b.abs() + res.abs()
    assert mag.max().item() < EXACT_LIMIT
    nobias, plain, added = x @ w.t(), x @ w.t() + b, xa @ w.t() + b
    exp = {'plain': plain, 'relu': plain.relu(), 'nobias': nobias, 'train_plain': plain, 'train_relu_nobias': nobias.relu(),
           'mask_res': torch.where(mask > 0, plain, torch.zeros((), dtype=torch.int64)) + res, 'res': plain + res, 'add': added,
           'add_res': added + res}
    bad = {k: int((got[k].double() != exp[k].double()).sum()) for k in exp}
    observed(f'{api.name} rows_linear_x3 {name} layer A: elements that differ from int64 = {sum(bad.values())} of '
             f'{sum(v.numel() for v in exp.values())} in {len(exp)} variants')
    assert not any(bad.values()), bad


def check_linear_real(api, name, case):
    """layer B: the plain product, the addend form and the residual form inside the bound; the epilogues bit for bit (_linear_variants)"""
    t = linear_inputs(case, real=True)
    got = _linear_variants(api, t)
    x, w, b, res, add = (t[k].double() for k in ('x', 'w', 'b', 'res', 'add'))
    c = linear_c(case['I'])
    ratios = {}
    for key, xs, r in (('plain', x, None), ('nobias', x, None), ('add', _pre_added(x, add), None), ('res', x, res)):
        bias = b if key != 'nobias' else torch.zeros_like(b)
        exact = xs @ w.t() + bias + (r if r is not None else 0)
        S = xs.abs() @ w.abs().t() + bias.abs() + (r.abs() if r is not None else 0)
        ratios[key] = ((got[key].double() - exact).abs() / (c * S)).max().item()
    exact = x @ w.t() + b
    err = (got['plain'].double() - exact).abs().max().item()
    e16 = (t['x'].bfloat16().double() @ t['w'].bfloat16().double().t() + b - exact).abs().max().item()
    observed(f'{api.name} rows_linear_x3 {name} layer B: max err / (c S) = ' + ', '.join(f'{v:.3f} ({k})' for k, v in ratios.items()) +
             f'; max|err| = {err:.3e}, plain bf16 operands {e16:.3e}')
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert err * 30 < e16


# ------------------------------------------------------------------------------------------------------------------ softmax over groups
SOFTMAX_GROUPS = (4, 8, 16, 32)
SOFTMAX_COUNTS = (1, 296, 5000)          # one group; a partly filled last wave; a partly filled last workgroup (every group size)
SOFTMAX_BWD_BAR = 1e-6                    # absolute, test_softmax_groups_forward_and_backward_emulated


def check_softmax(api, group, n_groups, fwd_bar):
    """forward and backward against float64, out of place and in place; logits randn * 3, and shifted by +60 / -60"""
    g = torch.Generator().manual_seed(100 * group + n_groups)
    base = torch.randn(n_groups, group, generator=g) * 3
    gy = torch.randn(n_groups, group, generator=g)
    worst_f = worst_b = 0.0
    for shift in (0.0, 60.0, -60.0) if n_groups == 296 else (0.0,):
        x = base + shift
        exp = x.double().softmax(-1)
        dx = api.to(x)
        y = api.softmax(dx, group)
        inplace = dx.clone()
        assert api.softmax(inplace, group, out=inplace) is inplace and torch.equal(inplace, y)
        assert torch.isfinite(y).all()
        worst_f = max(worst_f, (y.cpu().double() - exp).abs().max().item())
        yin = exp.float()                                  # the backward's y does not come from the kernel under test
        yd = yin.double()
        ex = yd * (gy.double() - (yd * gy.double()).sum(-1, keepdim=True))
        dy, dgy = api.to(yin), api.to(gy)
        gx = api.softmax_bwd(dy, dgy, group)
        inplace = dgy.clone()
        assert api.softmax_bwd(dy, inplace, group, out=inplace) is inplace and torch.equal(inplace, gx)
        worst_b = max(worst_b, (gx.cpu().double() - ex).abs().max().item())
    flat = api.to(torch.arange(n_groups, dtype=torch.float32)[:, None].expand(n_groups, group).contiguous() - 7.0)
    assert torch.equal(api.softmax(flat, group), torch.full_like(flat, 1.0 / group)), 'equal logits must give exactly 1 / group'
    observed(f'{api.name} softmax_groups group {group} x {n_groups}: max|err| vs float64 = {worst_f:.3e} forward, {worst_b:.3e} backward')
    assert worst_f < fwd_bar and worst_b < SOFTMAX_BWD_BAR


def check_softmax_rejects_group_12(api):
    x = api.to(torch.zeros(10, 12))
    assert api.softmax_code(x, 10, 12, torch.empty_like(x)) == -2


# ------------------------------------------------------------------------------------------------------------------ fixed-order sums
SUM_LEADING_B = (1, 3, 4)
SUM_LEADING_N = (4, 200, 1028)
SUM_PARTIALS_N = (1, 7, 8, 9, 100, 257)
SUM_PARTIALS_LEN = (8, 40, 256)


def check_sum_leading(api, B, N):
    g = torch.Generator().manual_seed(10 * B + N)
    x, y = api.to(torch.randn(B, N, generator=g)), api.to(torch.randn(B, N, generator=g))
    one, two = x[0], x[0] + y[0]
    for b in range(1, B):
        one = one + x[b]
        two = (two + x[b]) + y[b]
    assert torch.equal(api.sum_leading(x), one)
    assert torch.equal(api.sum_leading(x, y), two)


def check_sum_partials(api, n, ln):
    g = torch.Generator().manual_seed(1000 * n + ln)
    ints = _ints((n, ln), g, -1000, 1000)
    got = api.sum_partials(api.to(ints)).cpu()
    assert torch.equal(got.double(), ints.long().sum(0).double())
    part = torch.randn(n, ln, generator=g)
    dpart = api.to(part)
    got = api.sum_partials(dpart)
    assert torch.equal(got, api.sum_partials(dpart)), 'a second run differs'
    err = (got.cpu().double() - part.double().sum(0)).abs()
    bound = (n + 32) * U24 * part.double().abs().sum(0)
    ratio = (err / bound).max().item()
    observed(f'{api.name} sum_partials n {n} x len {ln}: max err / bound = {ratio:.3f}')
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------ fbbev_layernorm_bwd
LAYERNORM_BWD_CASES = ((1, 4), (5, 4), (37, 80), (8, 128), (3000, 80), (20000, 64))
LAYERNORM_EPS = 1e-5


def layernorm_bwd_ref(x, gy, w, eps):
    """include/fbbev.h in float64: grad_x[row] = inv (g - mean(g) - xhat mean(g xhat)), g = grad_out[row] * weight,
    xhat = (x[row] - mean) inv; grad_weight = column sums of grad_out * xhat, grad_bias = column sums of grad_out"""
    x, gy, w = x.double(), gy.double(), w.double()
    mean = x.mean(-1, keepdim=True)
    inv = 1.0 / ((x - mean).pow(2).mean(-1, keepdim=True) + eps).sqrt()
    xh = (x - mean) * inv
    gg = gy * w
    gx = inv * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    return gx, (gy * xh).sum(0), gy.sum(0)


def check_layernorm_bwd(api, rows, C):
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g) * 3 + 1.5
    w, gy = torch.randn(C, generator=g), torch.randn(rows, C, generator=g)
    ex, ew, eb = layernorm_bwd_ref(x, gy, w, LAYERNORM_EPS)
    gx, gw, gb = (t.cpu().double() for t in api.layernorm_bwd(api.to(x), api.to(gy), api.to(w), LAYERNORM_EPS))
    rx = ((gx - ex).abs() / (3e-6 + 2e-5 * ex.abs())).max().item()
    bw, bb = 2e-5 * max(1.0, ew.abs().max().item()), 2e-5 * max(1.0, eb.abs().max().item())
    observed(f'{api.name} layernorm_bwd {rows} x {C}: max err / bar = {rx:.3f} (grad_x), {(gw - ew).abs().max().item() / bw:.3f} (weight), '
             f'{(gb - eb).abs().max().item() / bb:.3f} (bias)')
    assert torch.allclose(gx, ex, atol=3e-6, rtol=2e-5)
    assert (gw - ew).abs().max().item() <= bw and (gb - eb).abs().max().item() <= bb
