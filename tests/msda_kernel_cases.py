"""Case table, float64 reference, input builders, bounds and adapters for the plain multi-scale deformable attention (MSDA) kernels,
shared by the GPU test (tests/test_gpu_msda_kernels.py, through fb_bev_amd._capi) and the emulator test
(tests/test_emu_msda_kernels.py, through tests/emu/emu_capi.py): fbbev_msda_fwd, fbbev_msda_fwd_fused, fbbev_msda_bwd (global
atomics), fbbev_msda_bwd_ws (band-binned LDS planes) and fbbev_msda_bwd_ex (deterministic fixed-point global scatter), at the smallest
shapes at which each of their code paths exists.  It mirrors tests/da_kernel_cases.py and borrows its bilinear sample.

The reference (`reference`) is written from the contract -- ms_deform_attn_cuda_kernel.cuh semantics as restated in
tests/test_oracle_msda.py::test_msda_edge_semantics -- not from the kernels: im = loc * size - 0.5; a sample is valid for
-1 < h_im < H and -1 < w_im < W; corners outside the level are zero; out[b, q, m, :] = sum over levels and points of
attn * bilinear(value of the level and head).  The fused forward composes loc = ref + offset / (W, H) first.  Vectorised float64
torch, differentiable (the gradients are float64 autograd of it), and it returns S, the same sum on absolute values.

Layer A, exact dyadic inputs (`dyadic_case`).  value is an integer in [-4, 4], the attention weights k/16 in [0, 1] (in [0, 2] where
a case says so), grad_output an integer in [-3, 3].  A level size s = odd * 2^a takes its coordinates from the grid j / 2^(a+2): loc
is then an exact fp32 number and loc * s = odd * j / 4 is an exact quarter pixel (a power-of-two size gets every quarter pixel, an odd
one every odd-th).  The fused forward's reference points sit on the same grid and its offsets are half pixels (a size that is no
power of two: 0, +-s/2, +-s, so that offset / s is exact) -- the DA rule.  `dyadic_case` asserts in fp32 against float64 that every
pixel coordinate is exact.  Every product and partial sum is then a multiple of 2^-9 far below 2^24 quanta (`check_representable`
asserts it from S), so fp32 arithmetic is exact in ANY order and the result must equal float64 bit for bit: out, grad_value,
grad_sampling_loc and grad_attn_weight, on the atomic, band-binned and deterministic routes.  No tolerance.  On the fixed-point routes
every product g * a * w is a multiple of 2^-8 and the plane's scale is 2^(30 - ex) with 2^ex barely above max|g| max(1, max|a|) <= 6
(`check_fixed_point_exact`: 30 - ex - 8 >= 0, and 61 - esum - kq - 8 >= 0 for the deterministic workspace).
The builder plants, and asserts that it did (where the level's size allows the coordinate: h_im = -1 needs loc = -1/(2H) exact):
  samples exactly at h_im = -1, h_im = H, w_im = -1, w_im = W (rejected); in (-1, 0) and (H - 1, H) (partial corners); exactly on a
  grid point; for the band-binned route h_im exactly at r0 - 1, r0, r1 - 1 and r1 - 1/2 of every band of a power-of-two-high level
  (corners on both sides of every band boundary); a query whose samples on one level are all far outside (the 0x00007fff word of
  k_msda_row_ranges); and, with B >= 2, a band that no query of the last sample reaches (its tokens must come back 0 from a
  NaN-prefilled grad_value).

Layer B, real values with full mantissas at sizes that are no powers of two (`real_case`); componentwise against float64.  The
builder keeps every fractional pixel coordinate in [1/8, 7/8] (asserted in float64 on the fp32 inputs), so no rounding moves a
sample into another cell and the one-sided derivative is the derivative.  u = 2^-24; counts from the expressions of k_msda_fwd /
k_msda_bwd (the other kernels evaluate the same expressions; an fma where the compiler contracts one only removes a rounding):
    im = loc * size - 0.5              two roundings: |delta im| <= u (|loc * size| + |im|) (1 + 2^-10)
                                       fused forward, loc = ref + offset / size first: u (|offset| + 2 |loc * size| + |im|) (1 + 2^-10)
    lh = h_im - floor(h_im)            exact for h_im >= 0; in (-1, 0) at most u relative
    hh = 1 - lh                        at most u relative for lh < 1/2, exact else; with lh's error over hh >= 1/8: 4 u
    w_k = hh * hw                      4 + 4 + 1 = 9 u for the worst corner weight
    val = sum_k w_k v_k                9 + 1 (product) + 3 (adds) = 13 u of sum_k |w_k v_k|
  forward       col += val * attn      13 + 1, then L * P adds:                      |err| <= (15 + L P) u S + T
  grad_attn     sum_c top_c val_c      13 + 1, Dh adds (lane or shuffle order), 1 into the word:   (16 + Dh) u S_a + T_a
  grad_loc      sum_c size * gww * tgv gww (signed hh / lh times v, three adds) 4 + 1 + 3, tgv = top * attn 1, two products 2,
                                       Dh adds, 1 into the word:                     (12 + Dh) u S_o + T_o
  grad_value    addend w_k * tgv       9 + 1 + 1 = 11 u each
      atomic route: n fp32 adds into the word in any order (n counted by the reference, + 1 for the prefill):
                                                                                   (11 + n + 1) u S_v + T_v
      LDS-plane route: the addend is rounded once to the plane's grid, the integer sum is exact, one rounding back to fp32:
                                                                                   12 u S_v + T_v + n q / 2
        q = 2^(ex - 30), 2^ex the power of two above max|grad_output| * max(1, max|attn|) over the QUERY SPAN of the token's
        (sample, head, band) workgroup -- not the token's own addends -- the span and n computed by the reference
        (`row_ranges`, `band_spans`) from the contract in the header of msda_bwd_kernels.h.
  S is the gradient's sum on absolute values; T the position term: every addend's derivative with respect to a pixel coordinate in
  absolute value (float64 autograd / the bilinear sample's 'dh', 'dw', 'one' modes: |d w_k / d h_im| = hw or lw, the mixed second
  derivative of a location gradient at most the sum of the four |corners|) times |delta im|.
No constant is taken from the code under test.  No layer B for the deterministic entry (the atomic kernel with fixed-point adds).

Band plan.  `band_plan` restates the rule of msda_bwd_kernels.h (level l is cut into ceil(h / rpb) bands of rpb = max(1, budget / w)
rows) and of the planner (budget = KB * 1024 / (8 Dh) - 16 tokens with KB = 144 or the FBBEV_MSDA_BWD_LDS_KB knob, shrunk by 3/4 while
B * M * bands < 256 and the shrunk budget still holds two rows of the widest level).  Every band-binned case of the table states its
expected bands per level and rows per band; `check_ws` asserts them against the restated rule AND against what the library reports:
fbbev_msda_bwd_ws_bytes = roundup256(4 B L Q) + 8 B n_bands.

Spans.  Forms of k_msda_row_ranges / k_msda_band_queries that keep every gradient but change a query span (no slack, the sampler's own
window, `first < r1 - 1` where no level is one row high) are told apart by `check_ws_poison`: an inf in one grad_output row must make
NaN exactly the planes whose span -- computed here from the contract -- holds that row; `poison_rows` picks a row per such form.
What no output can show: the `o3 >= 0` guard of k_msda_bwd_scatter (t3 = -1 - tok0 is negative anyway), the clamps of loads whose values
are never used (k_msda_bwd_unit's point tail; the scatter kernel's are caught through the +inf `guarded` buffer behind attn), amax
starting at 0 (only a finer grid) and the LDS row padding / padding-workgroup count of k_msda_fwd_unit (a negative count runs no loop).

Plain Python and CPU torch only; the adapters import their library on first use.
"""
import ctypes
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from da_kernel_cases import F32, F64, U24, _bilinear, _pow2, at_float_offset, observed  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3          # include/fbbev.h
FLAG_DETERMINISTIC = 1
UP = U24 * (1 + 2.0 ** -10)


# ------------------------------------------------------------------------------------------------------------------ reference
def geometry(shapes):
    ss = torch.tensor([list(s) for s in shapes], dtype=torch.int64)
    n = ss[:, 0] * ss[:, 1]
    ls = torch.cat([ss.new_zeros(1), n.cumsum(0)[:-1]])
    return ss, ls, int(n.sum())


def compose_loc(ref, offsets, shapes):
    """the fused forward's locations: ref (B, Q, L, 2), offsets (B, Q, M, L, P, 2) -> (B, Q, M, L, P, 2), in the operands' dtype"""
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=offsets.dtype)
    return ref[:, :, None, :, None, :] + offsets / norm[None, None, None, :, None, :]


def pixel_coords(loc, shapes):
    """-> per level (h_im, w_im), each (B, Q, M, P), float64"""
    loc = loc.double()
    return [(loc[:, :, :, l, :, 1] * h - 0.5, loc[:, :, :, l, :, 0] * w - 0.5) for l, (h, w) in enumerate(shapes)]


def _level_bil(value, shapes, pix, mode='val'):
    """per level the bilinear samples (B, M, Q, P, Dh) of value (B, S, M, Dh)"""
    B, S, M, Dh = value.shape
    out, start = [], 0
    for (h, w), (h_im, w_im) in zip(shapes, pix):
        Q, P = h_im.shape[1], h_im.shape[3]
        src = value[:, start:start + h * w].permute(0, 2, 1, 3)
        hi, wi = (t.permute(0, 2, 1, 3).reshape(B, M, Q * P) for t in (h_im, w_im))
        out.append(_bilinear(src, h, w, hi, wi, mode=mode).reshape(B, M, Q, P, Dh))
        start += h * w
    return out


def _combine(bil, attn):
    total = 0
    for l, b in enumerate(bil):
        total = total + (b * attn[:, :, :, l, :].permute(0, 2, 1, 3).unsqueeze(-1)).sum(3)          # (B, M, Q, Dh)
    B, M, Q, Dh = total.shape
    return total.permute(0, 2, 1, 3).reshape(B, Q, M * Dh)


def reference(value, shapes, loc, attn):
    """value (B, S, M, Dh), loc (B, Q, M, L, P, 2), attn (B, Q, M, L, P) -> out (B, Q, M*Dh) in float64 (differentiable in value, loc
    and attn) and S, the same sum on absolute values"""
    value, loc, attn = (t if t.dtype == F64 else t.double() for t in (value, loc, attn))
    out = _combine(_level_bil(value, shapes, pixel_coords(loc, shapes)), attn)
    with torch.no_grad():
        S = _combine(_level_bil(value.detach().abs(), shapes, pixel_coords(loc.detach(), shapes)), attn.detach().abs())
    return out, S


def reference_backward(c):
    """float64 autograd of `reference`: (grad_value, grad_loc, grad_attn)"""
    leaves = [c[k].double().requires_grad_() for k in ('value', 'loc', 'attn')]
    out, _ = reference(leaves[0], c['shapes'], leaves[1], leaves[2])
    return torch.autograd.grad(out, leaves, c['go'].double())


def row_ranges(loc, shapes, slack=True, window='wide'):
    """The contract of k_msda_row_ranges (header of msda_bwd_kernels.h): per (b, level, q) the first and last token row any of the
    M * P samples of the query can touch, one row of slack either side, from the samples with -2 < h_im < H + 1; first > last: none.
    -> (first, last), each (B, L, Q).  slack / window: the variants the poison test tells apart (never the expectation)."""
    B, Q = loc.shape[:2]
    first, last = [], []
    for (h, w), (h_im, _) in zip(shapes, pixel_coords(loc, shapes)):
        h_im = h_im.permute(0, 1, 2, 3).reshape(B, Q, -1)
        ok = (h_im > -2) & (h_im < h + 1) if window == 'wide' else (h_im > -1) & (h_im < h)
        r = torch.floor(h_im)
        lo = torch.where(ok, r - (1 if slack else 0), torch.full_like(r, 1e9)).amin(-1).clamp(min=0)
        hi = torch.where(ok, r + (2 if slack else 1), torch.full_like(r, -1e9)).amax(-1).clamp(max=h - 1)
        first.append(lo)
        last.append(hi)
    return torch.stack(first, 1), torch.stack(last, 1)


def band_plan(B, S, M, Dh, Q, shapes, lds_kb=144):
    """the planner's rule restated (module docstring) -> None (no plan) or (budget, [(level, r0, r1), ...])"""
    if Dh not in (4, 8, 10, 16, 32) or Q <= 0:
        return None
    budget = lds_kb * 1024 // (Dh * 8) - 16
    max_w = max(w for _, w in shapes)
    while True:
        if any(w > budget for _, w in shapes):
            return None
        nb = sum(-(-h // (budget // w)) for h, w in shapes)
        if B * M * nb >= 256 or budget * 3 // 4 < 2 * max_w:
            break
        budget = budget * 3 // 4
    if sum(h * w for h, w in shapes) != S:
        return None
    bands = []
    for l, (h, w) in enumerate(shapes):
        rpb = max(1, budget // w)
        bands += [(l, r0, min(r0 + rpb, h)) for r0 in range(0, h, rpb)]
    return budget, bands


def band_spans(first, last, bands, variant=None):
    """The contract of k_msda_band_queries: [qlo, qhi) of the queries whose row range meets the band; (B, n_bands, 2), (0, 0) if none.
    variant 'r1-1' / 'hi': two off-by-one forms the poison test tells apart (never the expectation)."""
    B, L, Q = first.shape
    out = torch.zeros(B, len(bands), 2, dtype=torch.int64)
    for k, (l, r0, r1) in enumerate(bands):
        meets = (first[:, l] <= last[:, l]) & (first[:, l] < (r1 - 1 if variant == 'r1-1' else r1)) & (last[:, l] >= r0)
        for b in range(B):
            qs = meets[b].nonzero().flatten()
            if len(qs):
                out[b, k, 0], out[b, k, 1] = int(qs[0]), int(qs[-1]) + (0 if variant == 'hi' else 1)
    return out


# ------------------------------------------------------------------------------------------------------------------ input builders
def _grid(size):
    """a size odd * 2^a -> (den = 2^(a+2), odd, jmin, jmax): loc = j / den gives im = odd * j / 4 - 0.5 from about -1.75 to size + 0.75"""
    a = (size & -size).bit_length() - 1
    odd = size >> a
    return 2 ** (a + 2), odd, math.ceil(-1.25 * 4 / odd), math.floor((size + 1.25) * 4 / odd)


def dyadic_case(seed, B, Q, M, Dh, shapes, P, mode='random', attn_max=1, fused=False, bands=None):
    """Layer A inputs (module docstring); asserts what the construction promises.  mode 'raster': query q samples within a few rows of
    the q-th cell of a raster over each level.  bands (the band-binned route): [(level, r0, r1)] for the band-edge plants."""
    g = torch.Generator().manual_seed(seed)
    shapes = tuple(tuple(s) for s in shapes)
    ss, ls, S = geometry(shapes)
    L = len(shapes)
    value = torch.randint(-4, 5, (B, S, M, Dh), generator=g).float()
    attn = torch.randint(0, 16 * attn_max + 1, (B, Q, M, L, P), generator=g).float() / 16
    go = torch.randint(-3, 4, (B, Q, M * Dh), generator=g).float()
    loc = torch.zeros(B, Q, M, L, P, 2)
    qh = max(1, math.isqrt(Q))
    qw = -(-Q // qh)
    for l, (h, w) in enumerate(shapes):
        for xy, size in ((1, h), (0, w)):
            den, odd, jmin, jmax = _grid(size)
            j = torch.randint(jmin, jmax + 1, (B, Q, M, P), generator=g)
            if mode == 'raster':
                cell = (torch.arange(Q) // qw + 0.5) / qh if xy == 1 else (torch.arange(Q) % qw + 0.5) / qw
                spread = max(1, round(6 / odd))
                j = (cell * den).round().long().view(1, Q, 1, 1) + torch.randint(-spread, spread + 1, (B, Q, M, P), generator=g)
            loc[:, :, :, l, :, xy] = j.float() / den
    planted = set()
    lh = next((l for l, (h, w) in enumerate(shapes) if _pow2(h) and h >= 2), None)
    lw = next((l for l, (h, w) in enumerate(shapes) if _pow2(w) and w >= 2), None)
    plants = []                                   # (name, level, x or None, y or None), on (b 0, head 0, point 0) of query number i
    h0, w0 = shapes[0]
    plants += [('h_partial_low', 0, 0.5, 0.0), ('h_partial_high', 0, 0.5, 1.0)]
    if lh is not None:
        h = shapes[lh][0]
        wl = shapes[lh][1]
        plants += [('h_minus_1', lh, 0.5, -0.5 / h), ('h_equals_H', lh, 0.5, (h + 0.5) / h),
                   ('grid_point', lh, 1.5 / wl if _pow2(wl) and wl >= 2 else 0.5, 1.5 / h)]
    if lw is not None:
        w = shapes[lw][1]
        plants += [('w_minus_1', lw, -0.5 / w, 0.5), ('w_equals_W', lw, (w + 0.5) / w, 0.5)]
    for i, (name, l, x, y) in enumerate(plants):
        if i >= Q - 1 and Q > 1 or i >= Q:
            break
        if x is not None:
            loc[0, i, 0, l, 0, 0] = x
        if y is not None:
            loc[0, i, 0, l, 0, 1] = y
        planted.add(name)
    if bands:                                     # band edges on (b 0, head 1 % M, point P - 1), one query each
        slots = [q for q in range(len(plants), Q - 1)] or list(range(Q))
        i = 0
        for l, r0, r1 in bands:
            h = shapes[l][0]
            if not _pow2(h):
                continue
            for him in (r0 - 1, r0, r1 - 1, r1 - 0.5):
                loc[0, slots[i % len(slots)], (1 + i // len(slots)) % M, l, P - 1, 1] = (him + 0.5) / h
                loc[0, slots[i % len(slots)], (1 + i // len(slots)) % M, l, P - 1, 0] = 0.5
                i += 1
            planted.add('band_edges')
        assert i <= len(slots) * M, 'band-edge plants overwrite one another'
    if bands and mode == 'raster' and Q >= 12:    # a bottom query reaches row 0 of level 0 only through a REJECTED sample in the slack window
        den, odd, jmin, jmax = _grid(h0)
        j = next(j for j in range(jmin - 8, 1) if -2 < odd * j / 4 - 0.5 <= -1)
        loc[0, Q - 2, 0, 0, 0, 1], loc[0, Q - 2, 0, 0, 0, 0] = j / den, 0.5
        planted.add('slack_window_only')
    unreached = None
    if bands and B >= 2:                          # the last sample reaches no row of the last band of the first level with >= 3 bands
        for l0 in range(L):
            mine = [bd for bd in bands if bd[0] == l0]
            if len(mine) >= 3 and mine[-1][1] >= 4:
                den, odd, jmin, jmax = _grid(shapes[l0][0])
                jlim = math.ceil((mine[-1][1] - 2 + 0.5) * 4 / odd) - 1          # the largest j with h_im < r0 - 2 is below jlim
                while odd * jlim / 4 - 0.5 >= mine[-1][1] - 2:
                    jlim -= 1
                j = (loc[B - 1, :, :, l0, :, 1] * den).round().long()
                loc[B - 1, :, :, l0, :, 1] = (jmin + (j - jmin) % (jlim - jmin + 1)).float() / den
                unreached = (B - 1, bands.index(mine[-1]))
                planted.add('unreached_band')
                break
    if Q >= 2:                                    # the last query of sample 0 has no sample on the last level
        loc[0, Q - 1, :, L - 1, :, 1] = -2.0
        planted.add('empty_level')
    c = dict(value=value, shapes=shapes, ss=ss, ls=ls, S=S, loc=loc, attn=attn, go=go, planted=planted, unreached=unreached, bands=bands,
             dims=(B, Q, M, Dh, L, P))
    if fused:                                     # loc = ref + offset / size with half-pixel offsets (DA rule where size is no power of two)
        ref = torch.zeros(B, Q, L, 2)
        off = torch.zeros(B, Q, M, L, P, 2)
        for l, (h, w) in enumerate(shapes):
            for xy, size in ((1, h), (0, w)):
                den, odd, jmin, jmax = _grid(size)
                ref[:, :, l, xy] = torch.randint(0, den + 1, (B, Q), generator=g).float() / den
                if _pow2(size):
                    off[:, :, :, l, :, xy] = torch.randint(-4, 5, (B, Q, M, P), generator=g).float() / 2
                else:
                    off[:, :, :, l, :, xy] = torch.randint(-2, 3, (B, Q, M, P), generator=g).float() * (size / 2)
        # the plants of (b 0, head 0, point 0): the offset that lands on the planted location (exact: both on the level's grid)
        loc_f = compose_loc(ref, off, shapes)
        for i, (name, l, x, y) in enumerate(plants):
            if name in planted:
                for xy, t in ((0, x), (1, y)):
                    size = shapes[l][1 - xy]
                    if t is not None:
                        off[0, i, 0, l, 0, xy] = (t - float(ref[0, i, l, xy])) * size
        if 'empty_level' in planted:
            off[0, Q - 1, :, L - 1, :, 1] = (-2.0 - float(ref[0, Q - 1, L - 1, 1])) * shapes[L - 1][0]
        loc_f = compose_loc(ref, off, shapes)
        assert torch.equal(compose_loc(ref.double(), off.double(), shapes), loc_f.double()), 'ref + offset / size is not exact'
        c.update(ref=ref, offsets=off, loc=loc_f)
        loc = loc_f
    # what the construction promises
    pix = pixel_coords(loc, shapes)
    for l, (h, w) in enumerate(shapes):
        h32, w32 = loc[:, :, :, l, :, 1] * h - 0.5, loc[:, :, :, l, :, 0] * w - 0.5
        assert torch.equal(h32.double(), pix[l][0]) and torch.equal(w32.double(), pix[l][1]), 'loc * size is not exact in fp32'
        assert torch.equal(pix[l][0] * 4, (pix[l][0] * 4).round()) and torch.equal(pix[l][1] * 4, (pix[l][1] * 4).round())
    in_w = lambda l: (pix[l][1] > -1) & (pix[l][1] < shapes[l][1])  # noqa: E731
    in_h = lambda l: (pix[l][0] > -1) & (pix[l][0] < shapes[l][0])  # noqa: E731
    checks = {
        'h_partial_low': lambda: (((pix[0][0] > -1) & (pix[0][0] < 0)) & in_w(0)).any(),
        'h_partial_high': lambda: (((pix[0][0] > h0 - 1) & (pix[0][0] < h0)) & in_w(0)).any(),
        'h_minus_1': lambda: ((pix[lh][0] == -1) & in_w(lh)).any(),
        'h_equals_H': lambda: ((pix[lh][0] == shapes[lh][0]) & in_w(lh)).any(),
        'grid_point': lambda: ((pix[lh][0] == pix[lh][0].floor()) & (pix[lh][0] >= 0) & (pix[lh][0] < shapes[lh][0]) & in_w(lh)).any(),
        'w_minus_1': lambda: ((pix[lw][1] == -1) & in_h(lw)).any(),
        'w_equals_W': lambda: ((pix[lw][1] == shapes[lw][1]) & in_h(lw)).any(),
    }
    for name in planted & set(checks):
        assert checks[name](), f'plant {name} is not there'
    first, last = row_ranges(loc, shapes)
    c['ranges'] = (first, last)
    if 'empty_level' in planted:
        assert first[0, L - 1, Q - 1] > last[0, L - 1, Q - 1], 'the last query still has a sample on the last level'
    if bands:
        c['spans'] = band_spans(first, last, bands)
        if 'band_edges' in planted:
            for l, r0, r1 in bands:
                if _pow2(shapes[l][0]):
                    hi = pix[l][0][0][in_w(l)[0]]
                    for him in (r0 - 1, r0, r1 - 1, r1 - 0.5):
                        assert (hi == him).any(), f'no valid sample at h_im = {him} of level {l}'
        if unreached:
            assert c['spans'][unreached[0], unreached[1]].tolist() == [0, 0], 'the unreached band is reached'
    return c


def real_case(seed, B, Q, M, Dh, shapes, P, mode='random', fused=False):
    """Layer B inputs: full-mantissa values; pixel coordinates k + f with f in [0.15, 0.85] from about -0.2 size to 1.2 size (mode
    'raster': within two pixels of the query's raster cell); asserted in float64 on the fp32 operands: every fraction in [1/8, 7/8]"""
    g = torch.Generator().manual_seed(seed)
    shapes = tuple(tuple(s) for s in shapes)
    ss, ls, S = geometry(shapes)
    L = len(shapes)
    value = torch.randn(B, S, M, Dh, generator=g)
    attn = torch.rand(B, Q, M, L, P, generator=g) * 1.5
    go = torch.randn(B, Q, M * Dh, generator=g)
    loc = torch.zeros(B, Q, M, L, P, 2)
    ref = torch.zeros(B, Q, L, 2)
    off = torch.zeros(B, Q, M, L, P, 2)
    qh = max(1, math.isqrt(Q))
    qw = -(-Q // qh)
    for l, (h, w) in enumerate(shapes):
        for xy, size in ((1, h), (0, w)):
            lo, hi = math.floor(-0.2 * size - 0.5), math.ceil(1.2 * size - 0.5)
            k = torch.randint(lo, hi + 1, (B, Q, M, P), generator=g).double()
            if mode == 'raster':
                cell = ((torch.arange(Q) // qw + 0.5) / qh if xy == 1 else (torch.arange(Q) % qw + 0.5) / qw) * size - 0.5
                k = cell.floor().view(1, Q, 1, 1) + torch.randint(-2, 3, (B, Q, M, P), generator=g).double()
            im = k + 0.15 + 0.7 * torch.rand(B, Q, M, P, generator=g, dtype=F64)
            if fused:
                r = torch.rand(B, Q, generator=g).float()
                ref[:, :, l, xy] = r
                off[:, :, :, l, :, xy] = (im + 0.5 - r.double()[:, :, None, None] * size).float()
            else:
                loc[:, :, :, l, :, xy] = ((im + 0.5) / size).float()
    c = dict(value=value, shapes=shapes, ss=ss, ls=ls, S=S, loc=loc, attn=attn, go=go, dims=(B, Q, M, Dh, L, P), bands=None)
    if fused:
        c.update(ref=ref, offsets=off, loc=compose_loc(ref.double(), off.double(), shapes))
    border = 0
    for (h, w), (h_im, w_im) in zip(shapes, pixel_coords(c['loc'], shapes)):
        for t, size in ((h_im, h), (w_im, w)):
            f = t - t.floor()
            assert ((f >= 0.125) & (f <= 0.875)).all()
            border += int((((t > -1) & (t < 0)) | ((t > size - 1) & (t < size))).sum())
    assert border > 0
    c['ranges'] = row_ranges(c['loc'], shapes)
    return c


def check_representable(c, S):
    """Layer A: every partial sum of a quantity is a multiple of its quantum q and the sum of absolute values stays below 2^24 q:
    out and grad_value 2^-8 (corner weights in 1/16, attn in 1/16), grad_loc 2^-6 (an integer size, hh / lh in 1/4, attn in 1/16),
    grad_attn 2^-4"""
    B, Q, M, Dh, L, P = c['dims']
    size = max(max(s) for s in c['shapes'])
    amax = max(1.0, c['attn'].abs().max().item())
    assert S.max().item() / 2.0 ** -8 < 2 ** 24
    assert size * 8.0 * 3 * amax * Dh / 2.0 ** -6 < 2 ** 24          # |gww| <= (hh + lh) * 2 * 4, |tgv| <= 3 amax, Dh channels
    assert 3.0 * 4 * Dh / 2.0 ** -4 < 2 ** 24
    assert (3.0 * amax * Q * P + 2) / 2.0 ** -8 < 2 ** 24             # at most Q * P addends of a head reach one token, + the prefill


def check_fixed_point_exact(c, route):
    """Layer A on the fixed-point routes: every product g * a * w_k is a multiple of 2^-8; it must be an integer at the plane's scale"""
    B, Q, M, Dh, L, P = c['dims']
    gmax, amax = c['go'].abs().max().item(), max(1.0, c['attn'].abs().max().item())
    if route == 'ws':
        ex = math.floor(math.log2(max(gmax * amax, 2.0 ** -90))) + 1
        assert 30 - ex - 8 >= 0
    else:          # fbbev_msda_bwd_ex: scale 2^(61 - ex_g - ex_a - kq), 2^kq >= Q * P adds per word
        esum = sum(math.floor(math.log2(x)) + 1 for x in (gmax, c['attn'].abs().max().item()) if x > 0)
        kq = max(0, math.ceil(math.log2(Q * P)))
        assert 61 - esum - kq - 8 >= 0


# ------------------------------------------------------------------------------------------------------------------ bounds (layer B)
def _deltas(c, fused):
    """per level (|delta h_im|, |delta w_im|), each (B, M, Q, P): the fp32 rounding bound of a pixel coordinate (module docstring)"""
    out = []
    loc = c['loc'].double()
    for l, ((h, w), (h_im, w_im)) in enumerate(zip(c['shapes'], pixel_coords(loc, c['shapes']))):
        d = []
        for xy, size, im in ((1, h, h_im), (0, w, w_im)):
            ls_ = (loc[:, :, :, l, :, xy] * size).abs()
            if fused:
                d.append(UP * (c['offsets'].double()[:, :, :, l, :, xy].abs() + 2 * ls_ + im.abs()))
            else:
                d.append(UP * (ls_ + im.abs()))
        out.append(tuple(t.permute(0, 2, 1, 3) for t in d))
    return out


def forward_bound(c, fused=False):
    B, Q, M, Dh, L, P = c['dims']
    V, A = c['value'].double().abs(), c['attn'].double().abs()
    pix = pixel_coords(c['loc'], c['shapes'])
    bv, bh, bw = (_level_bil(V, c['shapes'], pix, mode=m_) for m_ in ('val', 'dh', 'dw'))
    dl = _deltas(c, fused)
    S = _combine(bv, A)
    T = _combine([bh[l] * dl[l][0].unsqueeze(-1) + bw[l] * dl[l][1].unsqueeze(-1) for l in range(L)], A)
    return (15 + L * P) * U24 * S + T


def backward_bounds(c, route, n_extra=1):
    """per gradient the componentwise bound of the module docstring; route 'atomic' | 'ws'"""
    B, Q, M, Dh, L, P = c['dims']
    shapes = c['shapes']
    V = c['value'].double().abs().requires_grad_()
    A = c['attn'].double().abs()
    G = c['go'].double().abs().view(B, Q, M, Dh).permute(0, 2, 1, 3).unsqueeze(3)                # (B, M, Q, 1, Dh)
    pix = pixel_coords(c['loc'], shapes)
    bv, bh, bw, b1 = (_level_bil(V, shapes, pix, mode=m_) for m_ in ('val', 'dh', 'dw', 'one'))
    dl = _deltas(c, False)
    F_S = F_T = F_n = 0
    S_a, T_a, S_o, T_o = [], [], [], []
    for l, (h, w) in enumerate(shapes):
        a_l = A[:, :, :, l, :].permute(0, 2, 1, 3)                                               # (B, M, Q, P)
        dh_, dw_ = dl[l]
        gb, gh, gw, g1 = ((G * t).sum(-1) for t in (bv[l], bh[l], bw[l], b1[l]))                  # (B, M, Q, P)
        F_S = F_S + (a_l * gb).sum()
        F_T = F_T + (a_l * (gh * dh_ + gw * dw_)).sum()
        F_n = F_n + b1[l].sum()
        with torch.no_grad():
            S_a.append(gb)
            T_a.append(gh * dh_ + gw * dw_)
            S_o.append(torch.stack([w * a_l * gw, h * a_l * gh], -1))
            T_o.append(torch.stack([w * a_l * g1 * dh_, h * a_l * g1 * dw_], -1))
    S_v, = torch.autograd.grad(F_S, V, retain_graph=True)
    T_v, = torch.autograd.grad(F_T, V, retain_graph=True)
    n_v, = torch.autograd.grad(F_n, V)
    lay = lambda ts: torch.stack(ts, 3).permute(0, 2, 1, 3, 4) if ts[0].dim() == 4 else torch.stack(ts, 3).permute(0, 2, 1, 3, 4, 5)  # noqa: E731
    if route == 'atomic':
        b_v = (11 + n_v + n_extra) * U24 * S_v + T_v
    else:
        b_v = 12 * U24 * S_v + T_v + n_v * half_quantum(c).unsqueeze(-1)
    return dict(grad_value=b_v, grad_loc=(12 + Dh) * U24 * lay(S_o) + lay(T_o), grad_attn=(16 + Dh) * U24 * lay(S_a) + lay(T_a))


def half_quantum(c):
    """(B, S, M): half the fixed-point quantum of the plane a token belongs to, from its workgroup's query span (module docstring)"""
    B, Q, M, Dh, L, P = c['dims']
    first, last = c['ranges']
    spans = band_spans(first, last, c['bands'])
    g = c['go'].abs().view(B, Q, M, Dh).amax(-1)
    out = torch.zeros(B, c['S'], M, dtype=F64)
    for k, (l, r0, r1) in enumerate(c['bands']):
        w = c['shapes'][l][1]
        t0 = int(c['ls'][l]) + r0 * w
        for b in range(B):
            qlo, qhi = spans[b, k].tolist()
            if qhi <= qlo:
                continue
            gm = g[b, qlo:qhi].amax(0)                                                             # (M,)
            am = c['attn'][b, qlo:qhi, :, l].abs().amax((0, 2)).clamp(min=1.0)
            prod = (gm * am).double()                                                              # the fp32 product of the two maxima
            hq = torch.where(prod > 0, 2.0 ** (torch.floor(torch.log2(prod.clamp(min=1e-300))) + 1 - 30), torch.zeros_like(prod)) / 2
            out[b, t0:t0 + (r1 - r0) * w] = hq
    return out


# ------------------------------------------------------------------------------------------------------------------ layouts
def pack_rows(value, HS, interleaved=False):
    """(B, S, M, Dh) -> (B, S, M, HS) token rows, NaN in the HS - Dh padding floats; interleaved: [chunk][head][4 floats]"""
    B, S, M, Dh = value.shape
    rows = torch.full((B, S, M, HS), float('nan'))
    rows[..., :Dh] = value
    if interleaved:
        rows = rows.view(B, S, M, HS // 4, 4).permute(0, 1, 3, 2, 4).contiguous().view(B, S, M, HS)
    return rows


def guarded(t, fill, floats=0):
    """the same values as a contiguous view `floats` 4-byte elements into a 64-byte aligned buffer whose other elements hold `fill`"""
    v = at_float_offset(t, floats)
    v._base.fill_(fill)
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------------------------------------ adapters
class _Abi:
    """the C ABI of the MSDA family on one library; tensors go through `to` (CPU views keep their element offset on the device)"""

    def _p(self, t):
        return ctypes.c_void_p(t.data_ptr())

    def fwd(self, c, value=None, loc=None, attn=None):
        B, Q, M, Dh, L, P = c['dims']
        out = self.to(torch.full((B, Q, M * Dh), float('nan')))
        v, lo, a = (self.to(c[k] if t is None else t) for k, t in (('value', value), ('loc', loc), ('attn', attn)))
        ss, ls = self.to(c['ss']), self.to(c['ls'])          # (kept alive until the result is back)
        code = self.lib().fbbev_msda_fwd(self._p(v), self._p(ss), self._p(ls), self._p(lo), self._p(a),
                                         B, c['S'], M, Dh, L, Q, P, self._p(out), self.stream())
        assert code == 0, code
        return self.back(out)

    def fwd_fused(self, c, rows, offsets, attn, Dh, HS, flags):
        """-> (code, out); rows (B, S, M, HS)"""
        B, Q, M, _, L, P = c['dims']
        out = self.to(torch.full((B, Q, M * Dh), float('nan')))
        keep = [self.to(t) for t in (rows, c['ss'], c['ls'], c['ref'], offsets, attn)]
        code = self.lib().fbbev_msda_fwd_fused(*(self._p(t) for t in keep), B, c['S'], M, Dh, L, Q, P, HS, flags, self._p(out), self.stream())
        return code, self.back(out)

    def ws_bytes(self, B, S, M, Dh, L, Q, P, level_hw):
        flat = [int(x) for hw in level_hw for x in hw]
        return self.lib().fbbev_msda_bwd_ws_bytes(B, S, M, Dh, L, Q, P, (ctypes.c_int32 * len(flat))(*flat))

    def bwd(self, entry, c, prefill, value=None, loc=None, attn=None, go=None, ws_short=0, S=None):
        """entry 'atomic' | 'ws' | 'det'; prefill: (grad_value, grad_loc, grad_attn) CPU tensors -> (code, gv, gl, ga)"""
        B, Q, M, Dh, L, P = c['dims']
        S = c['S'] if S is None else S
        keep = [self.to(c[k] if t is None else t) for k, t in (('value', value), ('ss', None), ('ls', None), ('loc', loc), ('attn', attn),
                                                                ('go', go))]
        outs = [self.to(t.clone()) for t in prefill]
        args = [self._p(t) for t in keep] + [B, S, M, Dh, L, Q, P] + [self._p(t) for t in outs]
        if entry == 'atomic':
            code = self.lib().fbbev_msda_bwd(*args, self.stream())
        elif entry == 'ws':
            flat = [int(x) for hw in c['shapes'] for x in hw]
            arr = (ctypes.c_int32 * len(flat))(*flat)
            need = self.lib().fbbev_msda_bwd_ws_bytes(B, S, M, Dh, L, Q, P, arr)
            ws = self.to(torch.zeros(max(need, 16), dtype=torch.uint8))
            code = self.lib().fbbev_msda_bwd_ws(*args, arr, self._p(ws), need, self.stream())
        else:
            need = self.lib().fbbev_msda_bwd_det_ws_bytes(B, S, M, Dh)
            ws = self.to(torch.zeros(need + 64, dtype=torch.uint8))
            code = self.lib().fbbev_msda_bwd_ex(*args, FLAG_DETERMINISTIC, self._p(ws), need - ws_short, self.stream())
        return (code,) + tuple(self.back(t) for t in outs)


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

    def to(self, t):
        base = t._base if t._base is not None else t
        d = base.to(self.device)
        return d if t._base is None else d.as_strided(t.shape, t.stride(), t.storage_offset())

    def back(self, t):
        torch.cuda.synchronize()
        return t.cpu().contiguous()


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

    def to(self, t):
        return t

    def back(self, t):
        return t


# ------------------------------------------------------------------------------------------------------------------ case table
def _c(B, Q, M, Dh, shapes, P, **kw):
    return dict(B=B, Q=Q, M=M, Dh=Dh, shapes=tuple(tuple(s) for s in shapes), P=P, seed=kw.pop('seed', 0), **kw)


FWD_CASES = {
    'fwd_dh10_two_levels': _c(2, 37, 3, 10, [[6, 9], [3, 5]], 4),
    'fwd_dh59_one_point': _c(1, 5, 1, 59, [[8, 11]], 1),
    'fwd_dh4_three_levels_two_blocks': _c(1, 300, 2, 4, [[4, 4], [2, 2], [1, 1]], 2),
    # an all-power-of-two pyramid: the only sizes at which every border plant is an exact fp32 location
    'fwd_dh10_pow2_plants': _c(2, 37, 3, 10, [[8, 16], [4, 8]], 4, seed=1),
}
# 32 769 * 8 * 64 = 16 777 728 outputs = 65 536 * 256 + 512: every thread of the capped grid takes a second trip for the last query only
FWD_GRID_STRIDE = _c(1, 32769, 8, 64, [[2, 2]], 1, seed=2)


def _fu(Dh, HS, L, P, form, Q=25, M=4, B=1, head_minor=False, seed=0):
    shapes = ((8, 16), (3, 5))[:L]
    return _c(B, Q, M, Dh, shapes, P, HS=HS, form=form, head_minor=head_minor, seed=seed)


FUSED_CASES = {                                   # 100 units unless a case says otherwise; LP = 4 is staged
    'fused_dh10_narrow': _fu(10, 10, 2, 2, 'narrow'),
    'fused_dh10_wide': _fu(10, 12, 2, 2, 'wide'),
    'fused_dh10_interleaved': _fu(10, 12, 2, 2, 'interleaved'),
    'fused_dh10_narrow_head_minor': _fu(10, 10, 2, 2, 'narrow', head_minor=True, seed=1),
    'fused_dh10_wide_lp8_head_minor': _fu(10, 12, 2, 4, 'wide', head_minor=True, seed=2),
    'fused_dh10_interleaved_lp36': _fu(10, 12, 1, 36, 'interleaved', seed=3),
    'fused_dh10_wide_lp6_unstaged': _fu(10, 12, 2, 3, 'wide', seed=4),
    'fused_dh10_interleaved_lp40_unstaged_head_minor': _fu(10, 12, 2, 20, 'interleaved', head_minor=True, seed=5),
    'fused_dh10_narrow_lp6_unstaged': _fu(10, 10, 2, 3, 'narrow', seed=6),
    # 256 * 9 + 17 units: ten workgroups of units in a grid of sixteen -- a partial workgroup, and padding workgroups on the last XCD
    'fused_dh10_interleaved_2321_units': _fu(10, 12, 1, 4, 'interleaved', Q=211, M=11, seed=7),
    'fused_dh8_wide_2321_units_head_minor': _fu(8, 8, 2, 2, 'wide', Q=211, M=11, head_minor=True, seed=8),
    'fused_dh10_wide_2321_units_unstaged': _fu(10, 12, 2, 3, 'wide', Q=211, M=11, seed=9),
}
for _dh in (4, 8, 16, 32):
    FUSED_CASES[f'fused_dh{_dh}_wide'] = _fu(_dh, _dh, 2, 2, 'wide', seed=10 + _dh)
    FUSED_CASES[f'fused_dh{_dh}_interleaved'] = _fu(_dh, _dh, 1, 4, 'interleaved', head_minor=_dh in (4, 16), seed=20 + _dh)
FUSED_REAL = ['fused_dh10_narrow', 'fused_dh10_wide', 'fused_dh10_interleaved_lp36', 'fused_dh10_wide_lp6_unstaged', 'fused_dh4_wide',
              'fused_dh8_wide_2321_units_head_minor', 'fused_dh16_interleaved', 'fused_dh32_wide']

ATOMIC_CASES = {                                  # units: 222 (no multiple of 16), 42 (of 8), 5 and 6 (of 4)
    'atomic16_dh3': _c(2, 37, 3, 3, [[6, 9], [3, 5]], 4),
    'atomic16_dh10': _c(2, 37, 3, 10, [[8, 16], [4, 8]], 4, seed=1),
    'atomic32_dh24': _c(2, 7, 3, 24, [[8, 16], [3, 5]], 3, seed=2),
    'atomic64_dh59': _c(1, 5, 1, 59, [[8, 11]], 1, seed=3),
    'atomic64_dh80_two_channel_trips': _c(1, 3, 2, 80, [[4, 4], [2, 2], [1, 1]], 2, seed=4),
}
DET_CASES = {
    'det16_dh10': _c(2, 37, 3, 10, [[8, 16], [4, 8]], 4, seed=5),
    'det32_dh24': _c(2, 7, 3, 24, [[8, 16], [3, 5]], 3, seed=6),
    'det64_dh59': _c(1, 5, 1, 59, [[8, 11]], 1, seed=7),
}

L2, L4, L1 = [[7, 9], [3, 5]], [[16, 44], [8, 22], [4, 11], [1, 1]], [[24, 20]]


def _ws(B, Q, M, Dh, shapes, P, bands, rows, mode='random', unit='lane', misalign=None, attn_max=1, seed=0, real=True):
    """bands: expected bands per level; rows: expected rows of a level's full bands (the last band may be shorter)"""
    return _c(B, Q, M, Dh, shapes, P, bands=bands, rows=rows, mode=mode, unit=unit, misalign=misalign, attn_max=attn_max, seed=seed, real=real)


WS_CASES = {
    # ---- lane-per-unit kernel, Dh 4 / 8 / 10 / 16; [[7, 9], [3, 5]]: budget 23 -> 2-row bands (last one short), 4-row band
    'ws_dh4_l2': _ws(2, 37, 3, 4, L2, 4, (4, 1), (2, 3)),
    'ws_dh8_l2_p3': _ws(2, 37, 3, 8, L2, 3, (4, 1), (2, 3), seed=1),
    'ws_dh10_l2_p5': _ws(2, 37, 3, 10, L2, 5, (4, 1), (2, 3), seed=2),
    'ws_dh16_l2_p1': _ws(2, 37, 3, 16, L2, 1, (4, 1), (2, 3), seed=3),
    # ---- the shipped pyramid plus a level of height 1: eight 2-row bands on level 0
    'ws_dh10_l4_q2100_raster': _ws(2, 2100, 2, 10, L4, 4, (8, 2, 1, 1), (2, 4, 4, 1), mode='raster', seed=4),
    'ws_dh10_l4_q2100_random_span_over_512': _ws(1, 2100, 2, 10, L4, 4, (8, 2, 1, 1), (2, 4, 4, 1), seed=5, real=False),
    'ws_dh8_l4_q300_p8_raster_weights_to_2': _ws(2, 300, 2, 8, L4, 8, (8, 2, 1, 1), (2, 4, 4, 1), mode='raster', attn_max=2, seed=6),
    'ws_dh10_l4_q37_p3': _ws(2, 37, 2, 10, L4, 3, (8, 2, 1, 1), (2, 4, 4, 1), seed=7),
    # ---- one level 24 x 20: twelve 2-row bands
    'ws_dh10_l1_q300_p4_raster': _ws(2, 300, 4, 10, L1, 4, (12,), (2,), mode='raster', seed=8),
    'ws_dh4_l1_q1_p8': _ws(1, 1, 2, 4, L1, 8, (12,), (2,), seed=9, real=False),
    'ws_dh16_l1_q37_p5': _ws(2, 37, 2, 16, L1, 5, (12,), (2,), seed=10),
    # ---- power-of-two heights: every band-edge plant exists; eight 2-row bands of the 16 x 8 level, two 4-row bands of the 8 x 4 level
    'ws_dh10_pow2_q300_raster': _ws(2, 300, 2, 10, [[16, 8], [8, 4]], 4, (8, 2), (2, 4), mode='raster', seed=11),
    'ws_dh8_pow2_q37': _ws(2, 37, 3, 8, [[16, 8], [8, 4]], 4, (8, 2), (2, 4), seed=12),
    # ---- the lane-group fallback k_msda_bwd<16, false>: an operand 4 bytes off an 8-byte boundary
    'ws_dh10_value_at_4_bytes': _ws(2, 37, 3, 10, [[16, 8], [8, 4]], 4, (8, 2), (2, 4), unit='group', misalign='value', seed=13),
    'ws_dh10_grad_output_at_4_bytes': _ws(2, 37, 3, 10, L2, 4, (4, 1), (2, 3), unit='group', misalign='go', seed=14),
    'ws_dh10_loc_at_4_bytes': _ws(2, 37, 3, 10, L2, 4, (4, 1), (2, 3), unit='group', misalign='loc', seed=15),
    # ---- Dh = 32: k_msda_bwd<32, false> and k_msda_bwd_scatter<512, 32>
    'ws_dh32_pow2': _ws(2, 37, 2, 32, [[16, 8], [8, 4]], 4, (8, 2), (2, 4), unit='group', seed=16),
    'ws_dh32_l4_p3': _ws(1, 300, 2, 32, L4, 3, (8, 2, 1, 1), (2, 4, 4, 1), unit='group', mode='raster', seed=17),
}
WS_POISON = ['ws_dh10_l4_q2100_raster', 'ws_dh10_pow2_q300_raster', 'ws_dh10_l1_q300_p4_raster', 'ws_dh8_pow2_q37']

# shapes the planner declines (fbbev_msda_bwd_ws_bytes == 0): the entry and the wrapper accumulate through the atomic kernel
NO_PLAN_CASES = {
    'no_plan_dh59': _c(1, 5, 1, 59, [[8, 11]], 1, seed=3),
    'no_plan_level_tokens_differ_from_S': _c(2, 37, 3, 10, [[8, 16], [4, 8]], 4, seed=1, extra_tokens=3),
    'no_plan_level_wider_than_budget': _c(1, 9, 1, 32, [[1, 600]], 2, seed=8),          # 144 KB / (32 * 8 B) - 16 = 560 tokens
}

# FBBEV_MSDA_BWD_LDS_KB, read once per process: expected bands per level under the setting (None: no plan, the atomic kernel)
KNOB = 'FBBEV_MSDA_BWD_LDS_KB'
_P2, _P3, _P4 = ((4, 1), (2, 3)), ((16, 3, 1, 1), (1, 3, 4, 1)), ((12,), (2,))
KNOB_RUNS = {
    # 8 KB: 8192 / 80 - 16 = 86 tokens at Dh = 10 -- ONE-ROW bands at w = 44 (sixteen of them) and 3-row bands at w = 22; 240 tokens at
    # Dh = 4, 112 at Dh = 8, 48 at Dh = 16 (all shrunk by 3/4 down to two rows of the widest level, as at 144 KB); 16 tokens at Dh = 32:
    # two rows at w = 8, no plan at w = 44
    '8': {'ws_dh4_l2': _P2, 'ws_dh8_l2_p3': _P2, 'ws_dh10_l2_p5': _P2, 'ws_dh16_l2_p1': _P2,
          'ws_dh10_l4_q2100_raster': _P3, 'ws_dh10_l4_q2100_random_span_over_512': _P3,
          'ws_dh8_l4_q300_p8_raster_weights_to_2': ((8, 2, 1, 1), (2, 5, 4, 1)), 'ws_dh10_l4_q37_p3': _P3,
          'ws_dh10_l1_q300_p4_raster': _P4, 'ws_dh4_l1_q1_p8': _P4, 'ws_dh16_l1_q37_p5': _P4,
          'ws_dh10_pow2_q300_raster': ((8, 2), (2, 5)), 'ws_dh8_pow2_q37': ((8, 2), (2, 4)), 'ws_dh10_value_at_4_bytes': ((8, 2), (2, 5)),
          'ws_dh10_grad_output_at_4_bytes': _P2, 'ws_dh10_loc_at_4_bytes': _P2, 'ws_dh32_pow2': ((8, 2), (2, 4)), 'ws_dh32_l4_p3': None},
    # 1 KB: 1024 / 32 - 16 = 16 tokens at Dh = 4 -- one-row bands at w = 9, no plan at w = 20; 0 tokens at Dh = 8 and a negative budget
    # from Dh = 10 up: no plan at any width, Dh = 32 included
    '1': dict({name: None for name in WS_CASES}, ws_dh4_l2=((7, 1), (1, 3))),
}
assert all(set(v) == set(WS_CASES) for v in KNOB_RUNS.values())

_CACHE = {}


def _build(kind, p, real=False, **kw):
    key = (kind, real, tuple(sorted((k, str(v)) for k, v in p.items())), tuple(sorted(kw.items())))
    if key not in _CACHE:
        mk = real_case if real else dyadic_case
        _CACHE[key] = mk(p['seed'] + (100 if real else 0), p['B'], p['Q'], p['M'], p['Dh'], p['shapes'], p['P'], **kw)
    return _CACHE[key]


def _ref(c):
    if 'ref_out' not in c:
        with torch.no_grad():
            c['ref_out'] = reference(c['value'], c['shapes'], c['loc'], c['attn'])
    return c['ref_out']


def _grads(c):
    if 'grads' not in c:
        c['grads'] = reference_backward(c)
    return c['grads']


def _exact(tag, what, got, exp):
    assert not torch.isnan(got).any(), f'{tag}: NaN left in {what}'
    bad = (got.double() != exp).sum().item()
    assert bad == 0, f'{tag}: {bad} of {exp.numel()} words of {what} differ from float64, max|diff| = {(got.double() - exp).abs().max().item():.3e}'


def _inside(tag, what, got, exp, bound):
    assert not torch.isnan(got).any(), f'{tag}: NaN left in {what}'
    assert bound.shape == exp.shape, (what, bound.shape, exp.shape)
    err = (got.double() - exp).abs()
    return (err / bound.clamp(min=1e-300)).max().item(), err.max().item()


# ---- fbbev_msda_fwd
def check_fwd(api, name, real=False):
    p = FWD_CASES[name]
    c = _build('fwd', p, real)
    tag = f'msda_fwd {name} [{api.name}]'
    got = api.fwd(c)
    exp, S = _ref(c)
    if not real:
        check_representable(c, S)
        _exact(tag, 'out', got, exp)
        observed(f'{tag}: layer A, {exp.numel()} outputs exact; planted {sorted(c["planted"])}')
        return
    ratio, err = _inside(tag, 'out', got, exp, forward_bound(c))
    observed(f'{tag}: layer B max err/bound = {ratio:.3f} (max|err| = {err:.3e})')
    assert ratio <= 1.0, ratio


def check_fwd_grid_stride(api):
    """the capped grid's second trip: a strided subset of the queries and the last one (the last 512 outputs) against float64"""
    p = FWD_GRID_STRIDE
    g = torch.Generator().manual_seed(p['seed'])
    B, Q, M, Dh, P = p['B'], p['Q'], p['M'], p['Dh'], p['P']
    assert B * Q * M * Dh > 65536 * 256 and B * Q * M * Dh - 65536 * 256 == M * Dh
    ss, ls, S = geometry(p['shapes'])
    value = torch.randint(-4, 5, (B, S, M, Dh), generator=g).float()
    loc = torch.randint(-1, 6, (B, Q, M, 1, P, 2), generator=g).float() / 4          # h = w = 2: im = loc * 2 - 0.5 in half pixels
    attn = torch.randint(0, 17, (B, Q, M, 1, P), generator=g).float() / 16
    c = dict(value=value, shapes=p['shapes'], ss=ss, ls=ls, S=S, loc=loc, attn=attn, dims=(B, Q, M, Dh, 1, P))
    got = api.fwd(c).view(Q, M * Dh)
    pick = torch.cat([torch.arange(0, Q, 97), torch.arange(Q - 8, Q)]).unique()
    with torch.no_grad():
        exp, _ = reference(value, p['shapes'], loc[:, pick], attn[:, pick])
    assert Q - 1 in pick.tolist()
    _exact('msda_fwd grid stride', 'out', got[pick], exp[0])
    assert not torch.isnan(got).any()
    observed(f'msda_fwd fwd_grid_stride [{api.name}]: layer A, {exp.numel()} of {got.numel()} outputs exact, the last 512 among them')


# ---- fbbev_msda_fwd_fused
def fused_form(p, attn_aligned=True):
    """the kernel form the table expects, restated from the launcher's documented conditions: (row form, staged weights).  The library
    reports neither, and every form computes the same bits: this keeps the table consistent with itself, it is no route assertion."""
    HS, Dh = p['HS'], p['Dh']
    wide = HS % 4 == 0 and HS >= (Dh + 3) // 4 * 4
    LP = len(p['shapes']) * p['P']
    return ('interleaved' if p['form'] == 'interleaved' else 'wide' if wide else 'narrow'), LP % 4 == 0 and LP <= 36 and attn_aligned


def check_fused(api, name, real=False):
    p = FUSED_CASES[name]
    c = _build('fused', p, real, fused=True)
    form, staged = fused_form(p)
    assert form == p['form'] and staged == ('unstaged' not in name), name
    B, Q, M, Dh, L, P = c['dims']
    units = B * Q * M
    n_wg = -(-units // 256)
    assert units in (100, 2321) and (units == 100 or (n_wg == 10 and (n_wg + 7) // 8 * 8 > n_wg and units % 256))
    rows = pack_rows(c['value'], p['HS'], interleaved=form == 'interleaved')
    off = c['offsets'].permute(0, 1, 3, 4, 2, 5).contiguous() if p['head_minor'] else c['offsets']
    flags = (1 if p['head_minor'] else 0) | (4 if form == 'interleaved' else 0)
    code, got = api.fwd_fused(c, rows, off, c['attn'], Dh, p['HS'], flags)
    assert code == 0, code
    tag = f'msda_fwd_fused {name} [{api.name}]'
    exp, S = _ref(c)
    if real:
        ratio, err = _inside(tag, 'out', got, exp, forward_bound(c, fused=True))
        observed(f'{tag}: layer B max err/bound = {ratio:.3f} (max|err| = {err:.3e}; {form}, {"staged" if staged else "unstaged"})')
        assert ratio <= 1.0, ratio
        return
    check_representable(c, S)
    _exact(tag, 'out', got, exp)
    composed = api.fwd(c)                          # fbbev_msda_fwd on the composed locations: the same bits
    assert torch.equal(got, composed), f'{tag}: differs from fbbev_msda_fwd on the composed locations'
    observed(f'{tag}: layer A, {exp.numel()} outputs exact and bit-equal to msda_fwd ({form}, {"staged" if staged else "unstaged"}, '
             f'{units} units); planted {sorted(c["planted"])}')


def check_fused_codes(api):
    p = FUSED_CASES['fused_dh10_wide']
    c = _build('fused', p, False, fused=True)
    rows = pack_rows(c['value'], 12)
    assert api.fwd_fused(c, rows, c['offsets'], c['attn'], 10, 12, 0)[0] == 0
    assert api.fwd_fused(c, rows, guarded(c['offsets'], 0.0, floats=1), c['attn'], 10, 12, 0)[0] == E_UNSUPPORTED
    assert api.fwd_fused(c, rows, c['offsets'], c['attn'], 10, 8, 0)[0] == E_BADARG                  # head_stride < channels
    c12 = dict(c, dims=(c['dims'][0], c['dims'][1], c['dims'][2], 12, c['dims'][4], c['dims'][5]))
    assert api.fwd_fused(c12, rows, c['offsets'], c['attn'], 12, 12, 0)[0] == E_UNSUPPORTED          # Dh = 12: no kernel
    observed(f'msda_fwd_fused codes [{api.name}]: Dh 12 and offsets at 4 bytes unsupported, head_stride < channels a bad argument')


# ---- backward: shared
def _prefill(c, g, nan_value=False):
    """dyadic prefills: the contract of the atomic and deterministic entries is 'accumulated into'"""
    pv = torch.full_like(c['value'], float('nan')) if nan_value else torch.randint(-2, 3, c['value'].shape, generator=g).float()
    return pv, torch.randint(-2, 3, c['loc'].shape, generator=g).float() / 2, torch.randint(-2, 3, c['attn'].shape, generator=g).float()


def _check_grads_exact(tag, c, got, prefill, written):
    gv, gl, ga = _grads(c)
    _exact(tag, 'grad_value', got[0], gv if written else gv + prefill[0].double())
    _exact(tag, 'grad_sampling_loc', got[1], gl + prefill[1].double())
    _exact(tag, 'grad_attn_weight', got[2], ga + prefill[2].double())


def _check_grads_real(tag, c, got, route, extra=''):
    bounds = backward_bounds(c, route)
    worst = {}
    for what, g_, e_ in zip(('grad_value', 'grad_loc', 'grad_attn'), got, _grads(c)):
        worst[what], _ = _inside(tag, what, g_, e_, bounds[what])
    observed(f'{tag}: layer B max err/bound ' + ', '.join(f'{k[5:]} = {v:.4f}' for k, v in worst.items()) + extra)
    for what, r in worst.items():
        assert r <= 1.0, f'{tag}: {what} err/bound = {r:.3f}'


def check_atomic(api, name, real=False):
    p = ATOMIC_CASES[name]
    c = _build('bwd', p, real)
    gw = 16 if p['Dh'] <= 16 else 32 if p['Dh'] <= 32 else 64
    assert name.startswith(f'atomic{gw}_') and (p['B'] * p['Q'] * p['M']) % (256 // gw) != 0, name
    tag = f'msda_bwd {name} [{api.name}]'
    g = torch.Generator().manual_seed(77)
    pre = [torch.zeros_like(t) for t in (c['value'], c['loc'], c['attn'])] if real else _prefill(c, g)
    code, *got = api.bwd('atomic', c, pre)
    assert code == 0, code
    if real:
        return _check_grads_real(tag, c, got, 'atomic')
    check_representable(c, _ref(c)[1])
    _check_grads_exact(tag, c, got, pre, written=False)
    observed(f'{tag}: layer A, three gradients exact on dyadic prefills (lane groups of {gw}); planted {sorted(c["planted"])}')


def check_det(api, name):
    p = DET_CASES[name]
    c = _build('bwd', p, False)
    check_fixed_point_exact(c, 'det')
    tag = f'msda_bwd_ex {name} [{api.name}]'
    g = torch.Generator().manual_seed(78)
    pre = _prefill(c, g)
    code, *got = api.bwd('det', c, pre)
    assert code == 0, code
    _check_grads_exact(tag, c, got, pre, written=False)
    code, *again = api.bwd('det', c, pre)
    assert code == 0 and all(torch.equal(a, b) for a, b in zip(got, again)), f'{tag}: two runs differ'
    code, gv0, _, _ = api.bwd('det', c, pre, go=torch.zeros_like(c['go']))
    assert code == 0 and torch.equal(gv0, pre[0]), f'{tag}: an all-zero grad_output changed grad_value'
    assert api.bwd('det', c, pre, ws_short=1)[0] == E_WORKSPACE
    observed(f'{tag}: layer A, three gradients exact and ADDED to dyadic prefills, two runs equal, zero grad_output leaves grad_value, '
             f'a workspace one byte short is refused')


# ---- fbbev_msda_bwd_ws
def expected_bands(p, lds_kb=144):
    plan = band_plan(p['B'], sum(h * w for h, w in p['shapes']), p['M'], p['Dh'], p['Q'], p['shapes'], lds_kb)
    return plan[1] if plan else None


def _assert_plan(api, p, bands, stated):
    """the table's statement == the restated rule == what the library reports through its workspace size"""
    B, Q, M, Dh, P, shapes = p['B'], p['Q'], p['M'], p['Dh'], p['P'], p['shapes']
    L, S = len(shapes), sum(h * w for h, w in shapes)
    ws = api.ws_bytes(B, S, M, Dh, L, Q, P, shapes)
    if stated is None:
        assert bands is None and ws == 0, (bands, ws)
        return
    per_level, rows = stated
    assert bands is not None, 'the restated rule plans nothing'
    assert tuple(sum(1 for bd in bands if bd[0] == l) for l in range(L)) == tuple(per_level), bands
    for l in range(L):
        mine = [r1 - r0 for ll, r0, r1 in bands if ll == l]
        assert all(r == rows[l] for r in mine[:-1]) and 0 < mine[-1] <= rows[l] and (len(mine) > 1 or mine[0] == min(rows[l], shapes[l][0])), (l, mine)
    assert ws == -(-4 * B * L * Q // 256) * 256 + 8 * B * len(bands), (ws, len(bands))


def _ws_operands(c, p):
    """operands of a band-binned launch: attn sits in a buffer with +inf around it (a read past a unit's P weights that reaches the
    buffer's end poisons its plane); one operand 4 bytes off an 8-byte boundary where the case says so"""
    ops = dict(attn=guarded(c['attn'], float('inf')))
    if p.get('misalign'):
        k = p['misalign']
        ops[k] = guarded(c[k], 0.0, floats=1)
        assert ops[k].data_ptr() % 8 == 4
    return ops


def check_ws(api, name, real=False, lds_kb=144, stated='table'):
    p = WS_CASES[name]
    stated = (p['bands'], p['rows']) if stated == 'table' else stated
    bands = expected_bands(p, lds_kb)
    _assert_plan(api, p, bands, stated)
    lane = p['Dh'] % 2 == 0 and p['Dh'] in (4, 8, 10, 16) and not p['misalign']
    assert lane == (p['unit'] == 'lane'), name
    tag = f'msda_bwd_ws {name} [{api.name}]' + (f' at {lds_kb} KB' if lds_kb != 144 else '')
    kw = dict(mode=p['mode']) if real else dict(mode=p['mode'], attn_max=p['attn_max'], bands=tuple(expected_bands(p) or ()))
    c = _build('ws', p, real, **kw)
    g = torch.Generator().manual_seed(79)
    if bands is None:                              # no plan under this setting: the entry accumulates through the atomic kernel
        pre = _prefill(c, g)
        code, *got = api.bwd('ws', c, pre, **_ws_operands(c, p))
        assert code == 0, code
        _check_grads_exact(tag, c, got, pre, written=False)
        observed(f'{tag}: layer A, no plan -- three gradients exact and accumulated (atomic kernel)')
        return
    c = dict(c, bands=bands, default_bands=c['bands'])
    if real:
        pre = [torch.full_like(c['value'], float('nan')), torch.zeros_like(c['loc']), torch.zeros_like(c['attn'])]
        code, *got = api.bwd('ws', c, pre, **_ws_operands(c, p))
        assert code == 0, code
        return _check_grads_real(tag, c, got, 'ws', extra=f' ({len(bands)} bands, {p["unit"]} units)')
    check_representable(c, _ref(c)[1])
    check_fixed_point_exact(c, 'ws')
    pre = _prefill(c, g, nan_value=True)
    code, *got = api.bwd('ws', c, pre, **_ws_operands(c, p))
    assert code == 0, code
    _check_grads_exact(tag, c, got, pre, written=True)          # every token written exactly once: no NaN left, none added twice
    if c['unreached']:                             # (under any plan: no corner of that sample lies in those rows)
        b, k = c['unreached']
        l, r0, r1 = c['default_bands'][k]
        t0 = int(c['ls'][l]) + r0 * p['shapes'][l][1]
        assert (got[0][b, t0:t0 + (r1 - r0) * p['shapes'][l][1]] == 0).all()
    code, *again = api.bwd('ws', c, pre, **_ws_operands(c, p))
    assert code == 0 and all(torch.equal(a, b) for a, b in zip(got, again)), f'{tag}: two runs differ'
    spans = band_spans(*c['ranges'], bands)
    longest = int((spans[..., 1] - spans[..., 0]).max())
    if 'span_over_512' in name or 'q2100' in name:
        assert longest > 512, longest
    observed(f'{tag}: layer A, three gradients exact from a NaN grad_value, two runs equal ({len(bands)} bands {stated[0]} of {stated[1]} rows, '
             f'{p["unit"]} units, longest span {longest}); planted {sorted(c["planted"])}')


POISON_VARIANTS = {          # forms of the two index kernels that give the same gradients but other query spans
    'no_slack': dict(slack=False), 'sampler_window': dict(window='own'), 'first_below_r1_minus_1': dict(variant='r1-1'), 'last_query_dropped': dict(variant='hi')}


def poison_rows(c, bands):
    """per variant a (b, q) that the contract's spans hold and the variant's do not (None where the case has none)"""
    first, last = c['ranges']
    spans = band_spans(first, last, bands)
    out = {}
    for key, kw in POISON_VARIANTS.items():
        rk = {k: v for k, v in kw.items() if k != 'variant'}
        f2, l2 = row_ranges(c['loc'], c['shapes'], **rk) if rk else (first, last)
        other = band_spans(f2, l2, bands, variant=kw.get('variant'))
        out[key] = None
        for b in range(spans.shape[0]):
            for k in range(len(bands)):
                (lo, hi), (lo2, hi2) = spans[b, k].tolist(), other[b, k].tolist()
                if hi > lo and out[key] is None:
                    if hi2 <= lo2 or lo2 > lo:
                        out[key] = (b, lo)
                    elif hi2 < hi:
                        out[key] = (b, hi - 1)
    return out


def check_ws_poison(api, name):
    """an inf in one grad_output row makes NaN exactly the tokens of the (sample, head, band) workgroups whose query span holds that row
    (spans from the reference's row ranges); every other token equals the clean run bit for bit"""
    p = WS_CASES[name]
    bands = expected_bands(p)
    c = dict(_build('ws', p, False, mode=p['mode'], attn_max=p['attn_max'], bands=tuple(bands)), bands=bands)
    B, Q, M, Dh, L, P = c['dims']
    g = torch.Generator().manual_seed(79)
    pre = _prefill(c, g, nan_value=True)
    ops = _ws_operands(c, p)
    code, clean, _, _ = api.bwd('ws', c, pre, **ops)
    assert code == 0 and not torch.isnan(clean).any()
    spans = band_spans(*c['ranges'], bands)
    rows = poison_rows(c, bands)
    seen = []
    for key, bq in rows.items():
        if bq is None:
            continue
        b, q = bq
        m = (q + b) % M
        go = c['go'].clone()
        go[b, q, m * Dh + (q % Dh)] = float('inf')
        code, gv, _, _ = api.bwd('ws', c, pre, go=go, **{k: v for k, v in ops.items() if k != 'go'})
        assert code == 0
        want = torch.zeros(B, c['S'], M, dtype=torch.bool)
        for k, (l, r0, r1) in enumerate(bands):
            lo, hi = spans[b, k].tolist()
            if lo <= q < hi:
                w = p['shapes'][l][1]
                t0 = int(c['ls'][l]) + r0 * w
                want[b, t0:t0 + (r1 - r0) * w, m] = True
        nan = torch.isnan(gv).all(-1)
        assert torch.equal(torch.isnan(gv).any(-1), nan), f'{name}/{key}: a token is NaN in part'
        assert torch.equal(nan, want), f'{name}/{key}: row (b {b}, q {q}, head {m}) poisons {int(nan.sum())} tokens, the spans say {int(want.sum())}'
        assert torch.equal(gv[~nan], clean[~nan]), f'{name}/{key}: a token outside the poisoned planes changed'
        seen.append(key)
    observed(f'msda_bwd_ws poison {name} [{api.name}]: NaN exactly on the planes whose span holds the row, for rows that tell apart {seen}')
    return seen


def check_no_plan(api, name):
    """the planner declines: fbbev_msda_bwd_ws_bytes == 0 and fbbev_msda_bwd_ws accumulates through the atomic kernel"""
    p = NO_PLAN_CASES[name]
    c = _build('bwd', p, False)
    B, Q, M, Dh, L, P = c['dims']
    extra = p.get('extra_tokens', 0)
    S = c['S'] + extra
    value = torch.cat([c['value'], torch.full((B, extra, M, Dh), float('nan'))], 1) if extra else c['value']
    assert api.ws_bytes(B, S, M, Dh, L, Q, P, p['shapes']) == 0, name
    g = torch.Generator().manual_seed(80)
    pre = list(_prefill(c, g))
    pre_v = torch.cat([pre[0], torch.ones(B, extra, M, Dh)], 1) if extra else pre[0]
    code, gv, gl, ga = api.bwd('ws', c, (pre_v, pre[1], pre[2]), value=value, S=S)
    assert code == 0, code
    tag = f'msda_bwd_ws {name} [{api.name}]'
    _check_grads_exact(tag, c, (gv[:, :c['S']], gl, ga), pre, written=False)
    assert (gv[:, c['S']:] == 1).all()
    observed(f'{tag}: layer A, ws_bytes = 0 and three gradients exact, accumulated through the atomic kernel')


def run_knob(api, kb):
    """the band-binned layer-A cases of one FBBEV_MSDA_BWD_LDS_KB setting; the caller has set the environment"""
    assert os.environ.get(KNOB) == kb, os.environ.get(KNOB)
    for name, stated in KNOB_RUNS[kb].items():
        check_ws(api, name, lds_kb=int(kb), stated=stated)
    if kb == '8':
        bands = expected_bands(WS_CASES['ws_dh10_l4_q2100_raster'], 8)
        assert all(r1 - r0 == 1 for l, r0, r1 in bands if l == 0) and sum(1 for bd in bands if bd[0] == 0) == 16
    else:
        assert expected_bands(WS_CASES['ws_dh32_pow2'], 1) is None and expected_bands(WS_CASES['ws_dh10_l4_q37_p3'], 1) is None
        assert band_plan(1, 1, 1, 32, 1, ((1, 1),), 1) is None          # Dh = 32: no plan at any width
    return len(KNOB_RUNS[kb])


def table_claims():
    """what the table promises as a whole (checked once, without any library)"""
    full = {'h_minus_1', 'h_equals_H', 'w_minus_1', 'w_equals_W', 'h_partial_low', 'h_partial_high', 'grid_point', 'empty_level'}
    for kind, cases, kw in (('fwd', FWD_CASES, {}), ('fused', FUSED_CASES, dict(fused=True)), ('bwd', ATOMIC_CASES, {}), ('bwd', DET_CASES, {})):
        got = set()
        for name, p in cases.items():
            got |= _build(kind, p, False, **kw)['planted']
        assert full <= got, (kind, full - got)
    got, short, one_high, four = set(), False, False, False
    for name, p in WS_CASES.items():
        bands = expected_bands(p)
        got |= _build('ws', p, False, mode=p['mode'], attn_max=p['attn_max'], bands=tuple(bands))['planted']
        for l, (h, w) in enumerate(p['shapes']):
            mine = [r1 - r0 for ll, r0, r1 in bands if ll == l]
            short |= len(mine) > 1 and mine[-1] < mine[0]
            one_high |= h == 1
            four |= len(mine) >= 4
    assert full | {'band_edges', 'unreached_band'} <= got, full - got
    assert short and one_high and four
    assert {p['P'] for p in WS_CASES.values()} >= {1, 3, 4, 5, 8} and {p['Q'] for p in WS_CASES.values()} >= {1, 37, 300, 2100}
    assert {p['Dh'] for p in WS_CASES.values()} == {4, 8, 10, 16, 32}
    assert {len(p['shapes']) for p in WS_CASES.values()} >= {1, 2, 4}
    assert {p['misalign'] for p in WS_CASES.values()} >= {'value', 'go', 'loc'}


# ------------------------------------------------------------------------------------------------------------------ the Python wrappers (GPU only)
def _dev_case(api, c, value=None):
    return [api.to(t) for t in (c['value'] if value is None else value, c['ss'], c['ls'], c['loc'], c['attn'], c['go'])]


def check_capi_no_plan(api, name):
    """_capi.msda_bwd with level_hw on a shape the planner declines: accumulated through the atomic kernel"""
    p = NO_PLAN_CASES[name]
    c = _build('bwd', p, False)
    B, Q, M, Dh, L, P = c['dims']
    extra = p.get('extra_tokens', 0)
    value = torch.cat([c['value'], torch.full((B, extra, M, Dh), float('nan'))], 1) if extra else c['value']
    assert api.c.msda_bwd_ws_bytes(B, c['S'] + extra, M, Dh, L, Q, P, p['shapes']) == 0
    pre = list(_prefill(c, torch.Generator().manual_seed(80)))
    pre_v = torch.cat([pre[0], torch.ones(B, extra, M, Dh)], 1) if extra else pre[0]
    outs = [api.to(t.clone()) for t in (pre_v, pre[1], pre[2])]
    api.c.msda_bwd(*_dev_case(api, c, value), *outs, level_hw=p['shapes'])
    gv, gl, ga = (api.back(t) for t in outs)
    tag = f'_capi.msda_bwd {name} [{api.name}]'
    _check_grads_exact(tag, c, (gv[:, :c['S']], gl, ga), pre, written=False)
    assert (gv[:, c['S']:] == 1).all()
    observed(f'{tag}: layer A, no plan -- three gradients exact, accumulated')


def check_deterministic_wrapper(api):
    """fb_bev_amd.set_deterministic(True): both contracts of _capi._msda_bwd_det, and its fixed-point global scatter where no plan exists"""
    import fb_bev_amd
    p = WS_CASES['ws_dh8_pow2_q37']
    c = _build('ws', p, False, mode=p['mode'], attn_max=p['attn_max'], bands=tuple(expected_bands(p)))
    pd = DET_CASES['det64_dh59']
    cd = _build('bwd', pd, False)
    g = torch.Generator().manual_seed(81)
    fb_bev_amd.set_deterministic(True)
    try:
        pre = _prefill(c, g, nan_value=True)                    # with level_hw: grad_value is written
        outs = [api.to(t.clone()) for t in pre]
        api.c.msda_bwd(*_dev_case(api, c), *outs, level_hw=p['shapes'])
        _check_grads_exact('det wrapper, level_hw', c, [api.back(t) for t in outs], pre, written=True)
        pre = _prefill(c, g)                                    # without: the result is added after the host read
        outs = [api.to(t.clone()) for t in pre]
        api.c.msda_bwd(*_dev_case(api, c), *outs)
        _check_grads_exact('det wrapper, host read', c, [api.back(t) for t in outs], pre, written=False)
        pre = _prefill(cd, g)                                   # no plan at Dh = 59: fbbev_msda_bwd_ex, accumulated
        outs = [api.to(t.clone()) for t in pre]
        api.c.msda_bwd(*_dev_case(api, cd), *outs, level_hw=pd['shapes'])
        _check_grads_exact('det wrapper, no plan', cd, [api.back(t) for t in outs], pre, written=False)
    finally:
        fb_bev_amd.set_deterministic(None)
    observed(f'deterministic wrapper [{api.name}]: layer A, written with level_hw, added without it, fbbev_msda_bwd_ex where no plan exists')


def check_autograd_function(api, name='ws_dh10_pow2_q300_raster'):
    """MultiScaleDeformableAttnFunction_fp32: const_tensor shapes take the band-binned route, plain tensors the atomic one"""
    from fb_bev_amd.backward_projection import const_tensor
    from fb_bev_amd.ms_deform_attn import MultiScaleDeformableAttnFunction_fp32 as Fn
    p = WS_CASES[name]
    bands = expected_bands(p)
    c = _build('ws', p, False, mode=p['mode'], attn_max=p['attn_max'], bands=tuple(bands))
    pre = [torch.full_like(c['value'], float('nan')), torch.zeros_like(c['loc']), torch.zeros_like(c['attn'])]
    code, *ws = api.bwd('ws', dict(c, bands=bands), pre)
    assert code == 0
    for route in ('band-binned', 'atomic'):
        if route == 'band-binned':
            ss = const_tensor([list(s) for s in p['shapes']], api.device)
            ls = const_tensor([int(x) for x in c['ls']], api.device)
        else:
            ss, ls = api.to(c['ss']), api.to(c['ls'])
        leaves = [api.to(c[k]).requires_grad_() for k in ('value', 'loc', 'attn')]
        out = Fn.apply(leaves[0], ss, ls, leaves[1], leaves[2], 64)
        _exact(f'Function_fp32 {route}', 'out', api.back(out.detach()), _ref(c)[0])
        out.backward(api.to(c['go']))
        got = [api.back(t.grad) for t in leaves]
        _check_grads_exact(f'Function_fp32 {route}', c, got, [torch.zeros_like(t) for t in pre], written=True)
        assert all(torch.equal(a, b) for a, b in zip(got, ws)), route
    observed(f'MultiScaleDeformableAttnFunction_fp32 {name} [{api.name}]: layer A, output and three gradients exact on both routes')
