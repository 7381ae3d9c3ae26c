"""Case tables, input generators, float64 references and bounds for the convolution kernels of fb_bev_amd/csrc/conv3d_kernels.h, shared
by the GPU test (tests/test_gpu_conv_kernels.py, through fb_bev_amd._capi) and the emulator test (tests/test_emu_conv_kernels.py,
through tests/emu/emu_capi.py): fbbev_conv3d_ndhwc (plain and transposed), fbbev_conv2d_nhwc, fbbev_conv3d_ndhwc_bf16,
fbbev_conv3d_k3s1_tiled_bf16, fbbev_conv3d_dgrad_ndhwc, fbbev_conv3d_wgrad_ndhwc / _ex and fbbev_blend_levels_ndhwc at the smallest
shapes at which each of their code paths exists.  Every output buffer starts as NaN and must come back without one; dw alone starts
as zero, which is its contract (the deterministic route's chunk workspace starts as NaN).

Layer A, exact integers.  Activations, weights, bias, residual and dy are integers in [-4, 4]: exact in bf16 and in fp32, every
product and every partial sum is an integer below 2^24 (asserted from taps * Cin * 16 + 8, and from nvox * 16 for the weight
gradient), so fp32 addition is exact in ANY order.  The result must equal the float64 reference under torch.equal -- no tolerance.
A tap, channel group, tile, chunk or voxel that is dropped, duplicated or misplaced changes an integer.  This holds for the fp32, bf16,
tiled, transposed, data-gradient and both weight-gradient routes; the tiled kernel must also equal the direct bf16 kernel, and the
atomic weight gradient the deterministic one.

Layer B, real values with full mantissas (randn; weights scaled by (Cin * taps)^-0.5).  Componentwise against float64
(F.conv3d / F.conv_transpose3d / autograd in float64):  |got - exact| <= c * S  with S the same operation on absolute values:
conv(|x|, |w|) + |b| + |residual|, for the weight gradient sum_v |dy| |x|.  ReLU needs no mask: |relu a - relu b| <= |a - b|.
c from the arithmetic, not from a run:
  * an fp32 MFMA is a k-ordered fmaf chain with one rounding per product, so a chain of n products is within n * 2^-24 of the sum
    of magnitudes (first order; the factor 1.001 covers the higher-order terms up to n = 2^13);
  * forward, transposed, data gradient: one chain of n = taps * Cin products (transposed: every output voxel sees ONE tap, n = Cin;
    data gradient: the chain runs over dy's channels, n = taps * Cout), then the bias add and the residual add:
        c = (n + 3) * 2^-24 * 1.001
  * weight gradient: one chain over the `chunk` voxels of a chunk, then n_chunks adds (atomic, in any order, in the default route; in
    chunk order starting from zero, plus the add into dw, in the deterministic route):
        c = (chunk + n_chunks + 2) * 2^-24 * 1.001
    chunk and n_chunks are literal numbers in the table (conv3d_wgrad_chunk in fb_bev_amd/csrc/capi.hip); a test checks them against
    fbbev_conv3d_wgrad_ws_bytes = n_chunks * taps * Cout * Cin * 4;
  * bf16 kernels: the reference is the float64 convolution of the operands rounded to bf16 with round to nearest even (what
    fbbev_cvt_bf16x8 and weight_fragments_bf16 do).  One variant feeds activations that are bf16-representable already, one feeds
    full mantissas and rounds them in the reference only.  A product of two bf16 values is exact in fp32 and the accumulation follows
    the model tests/rows_train_cases.py uses for the bf16 MFMA, n * 2^-24 of the sum of magnitudes: c as for fp32.
Each real-valued fp32 case also shows that no operand is rounded on the way: its largest error is at least 30 times smaller than that
of the same convolution on bf16-rounded operands (a worst-case bound at n = 2592 cannot see that; this ratio can).

Level blend.  Layer A: dyadic ratios (2x, 4x, coarse extents of 1 included), small integers, wsoft in multiples of 1/8: source
indices, interpolation weights, products and sums are exact, so the result equals the float64 F.interpolate(trilinear,
align_corners=False) composite bit for bit.  Layer B: non-dyadic ratios (10 from 3, 6 from 4, 6 and 10 from 1):
    |got - exact| <= eps * sum_k |w_k| * max|f_k|,   eps = (9 * max_in_size + 16) * 2^-24
three roundings in the source index scale * (dst + 0.5) - 0.5 (the quotient, the product, the subtraction; |index| <= in_size) put at
most 3 * in_size * 2^-24 on an interpolation weight, over three axes 9 * in_size * 2^-24; the interpolation is continuous in the index,
so a floor that lands on the other side of an integer costs nothing more; 16 roundings cover the lerps and the level sum.
wsoft has more columns than levels (K > n_coarse + 1) and the unused ones hold NaN.

Plain Python and CPU torch only; the adapters import their library on first use.
"""
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
EXACT_LIMIT = 2 ** 24
NAN = float('nan')


def observed(text):
    print(f'[observed] {text}')


def out_dims(dims, k, s, p, planar=False):
    f = lambda n: (n + 2 * p - k) // s + 1  # noqa: E731
    return (1 if planar else f(dims[0]), f(dims[1]), f(dims[2]))


def pad16(b):
    return F.pad(b, (0, (-b.numel()) % 16)).contiguous()


# ------------------------------------------------------------------------------------------------------------------ adapters
# Both take and return CPU tensors: activations NDHWC f32, weights in torch's layout (Cout, Cin, k, k, k) [transposed: (Cin, Cout, 2, 2,
# 2); 2-D: (Cout, Cin, k, k)], bias of Cout floats (padded here), dw as (k^3, Cout, Cin).
class GpuApi:
    """fb_bev_amd._capi on cuda:0, weights through fb_bev_amd.mfma_conv3d.weight_fragments / weight_fragments_bf16"""
    name = 'gpu'

    def __init__(self):
        from fb_bev_amd import _capi, mfma_conv3d
        self.c, self.M = _capi, mfma_conv3d
        self.device = torch.device('cuda:0')

    def _d(self, t):
        return None if t is None else t.contiguous().to(self.device)

    def _nan(self, *shape):
        return torch.full(shape, NAN, device=self.device)

    def conv(self, x, w, b, k, s, p, relu=False, res=None):
        out = self._nan(x.shape[0], *out_dims(x.shape[1:4], k, s, p), w.shape[0])
        return self.c.conv3d_ndhwc(self._d(x), self._d(self.M.weight_fragments(w)), self._d(pad16(b)), out, w.shape[0], ksize=k, stride=s,
                                   pad=p, relu=relu, residual=self._d(res)).cpu()

    def conv_transposed(self, x, w, b, relu=False):
        B, D, H, W, _ = x.shape
        out = self._nan(B, 2 * D, 2 * H, 2 * W, w.shape[1])
        return self.c.conv3d_ndhwc(self._d(x), self._d(self.M.weight_fragments(w, transposed=True)), self._d(pad16(b)), out, w.shape[1],
                                   relu=relu, transposed=True).cpu()

    def conv2d(self, x, w, b, k, s, p, relu=False, res=None):
        out = self._nan(x.shape[0], *out_dims((1, *x.shape[1:3]), k, s, p)[1:], w.shape[0])
        return self.c.conv2d_nhwc(self._d(x), self._d(self.M.weight_fragments(w[:, :, None])), self._d(pad16(b)), out, w.shape[0], ksize=k,
                                  stride=s, pad=p, relu=relu, residual=self._d(res)).cpu()

    def conv_bf16(self, x, w, b, k, s, p, relu=False, res=None, planar=False):
        out = self._nan(x.shape[0], *out_dims(x.shape[1:4], k, s, p, planar), w.shape[0])
        return self.c.conv3d_ndhwc_bf16(self._d(x), self._d(self.M.weight_fragments_bf16(w)), self._d(pad16(b)), out, w.shape[0], ksize=k,
                                        stride=s, pad=p, relu=relu, residual=self._d(res), planar=planar).cpu()

    def conv_transposed_bf16(self, x, w, b, relu=False):
        B, D, H, W, _ = x.shape
        out = self._nan(B, 2 * D, 2 * H, 2 * W, w.shape[1])
        return self.c.conv3d_ndhwc_bf16(self._d(x), self._d(self.M.weight_fragments_bf16(w, transposed=True)), self._d(pad16(b)), out,
                                        w.shape[1], relu=relu, transposed=True).cpu()

    def conv_tiled(self, x, w, b, relu=False, res=None):
        out = self._nan(*x.shape[:4], w.shape[0])
        return self.c.conv3d_k3s1_tiled_bf16(self._d(x), self._d(self.M.weight_fragments_bf16(w)), self._d(pad16(b)), out, w.shape[0],
                                             relu=relu, residual=self._d(res)).cpu()

    def dgrad(self, dy, w, in_dims, k, s, p):
        dx = self._nan(dy.shape[0], *in_dims, w.shape[1])
        return self.c.conv3d_dgrad_ndhwc(self._d(dy), self._d(self.M.weight_fragments(w.transpose(0, 1))), dx, ksize=k, stride=s, pad=p).cpu()

    def wgrad_ws_bytes(self, B, Do, Ho, Wo, Cin, Cout, k):
        return self.c.lib().fbbev_conv3d_wgrad_ws_bytes(B, Do, Ho, Wo, Cin, Cout, k, self.c.FLAG_DETERMINISTIC)

    def wgrad(self, x, dy, k, s, p, deterministic):
        """the C entries themselves, so that the route does not depend on the process-wide deterministic switch"""
        c, p_ = self.c, ctypes.c_void_p
        B, Di, Hi, Wi, Cin = x.shape
        _, Do, Ho, Wo, Cout = dy.shape
        dx, ddy = self._d(x), self._d(dy)
        dw = torch.zeros(k ** 3, Cout, Cin, device=self.device)
        with torch.cuda.device(self.device):
            if deterministic:
                need = self.wgrad_ws_bytes(B, Do, Ho, Wo, Cin, Cout, k)
                ws = self._nan(need // 4)
                code = c.lib().fbbev_conv3d_wgrad_ndhwc_ex(p_(dx.data_ptr()), p_(ddy.data_ptr()), B, Di, Hi, Wi, Cin, Do, Ho, Wo, Cout, k, s, p,
                                                           p_(dw.data_ptr()), c.FLAG_DETERMINISTIC, p_(ws.data_ptr()), need, c._stream())
            else:
                code = c.lib().fbbev_conv3d_wgrad_ndhwc(p_(dx.data_ptr()), p_(ddy.data_ptr()), B, Di, Hi, Wi, Cin, Do, Ho, Wo, Cout, k, s, p,
                                                        p_(dw.data_ptr()), c._stream())
        assert code == 0, code
        return dw.cpu()

    def blend(self, level0, coarse, wsoft):
        return self.c.blend_levels_ndhwc(self._d(level0), [self._d(t) for t in coarse], self._d(wsoft), self._nan(*level0.shape)).cpu()


class EmuApi:
    """tests/emu/emu_capi.py: the same kernels compiled for the CPU (its wrappers fill every output with NaN)"""
    name = 'emu'

    def __init__(self):
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
        import emu_capi
        from fb_bev_amd import mfma_conv3d
        self.E, self.M = emu_capi, mfma_conv3d

    @staticmethod
    def _ok(pair):
        code, out = pair
        assert code == 0, code
        return out

    @staticmethod
    def _c(t):
        return None if t is None else t.contiguous()

    def conv(self, x, w, b, k, s, p, relu=False, res=None):
        return self._ok(self.E.conv3d_ndhwc(self._c(x), self.M.weight_fragments(w), pad16(b), w.shape[0], ksize=k, stride=s, pad=p, relu=relu,
                                            residual=self._c(res)))

    def conv_transposed(self, x, w, b, relu=False):
        return self._ok(self.E.conv3d_ndhwc(self._c(x), self.M.weight_fragments(w, transposed=True), pad16(b), w.shape[1], relu=relu,
                                            transposed=True))

    def conv2d(self, x, w, b, k, s, p, relu=False, res=None):
        return self._ok(self.E.conv2d_nhwc(self._c(x), self.M.weight_fragments(w[:, :, None]), pad16(b), w.shape[0], ksize=k, stride=s, pad=p,
                                           relu=relu, residual=self._c(res)))

    def conv_bf16(self, x, w, b, k, s, p, relu=False, res=None, planar=False):
        return self._ok(self.E.conv3d_ndhwc_bf16(self._c(x), self.M.weight_fragments_bf16(w), pad16(b), w.shape[0], ksize=k, stride=s, pad=p,
                                                 relu=relu, residual=self._c(res), planar=planar))

    def conv_transposed_bf16(self, x, w, b, relu=False):
        return self._ok(self.E.conv3d_ndhwc_bf16(self._c(x), self.M.weight_fragments_bf16(w, transposed=True), pad16(b), w.shape[1], relu=relu,
                                                 transposed=True))

    def conv_tiled(self, x, w, b, relu=False, res=None):
        return self._ok(self.E.conv3d_k3s1_tiled_bf16(self._c(x), self.M.weight_fragments_bf16(w), pad16(b), w.shape[0], relu=relu,
                                                      residual=self._c(res)))

    def dgrad(self, dy, w, in_dims, k, s, p):
        return self._ok(self.E.conv3d_dgrad_ndhwc(self._c(dy), self.M.weight_fragments(w.transpose(0, 1)), tuple(in_dims), w.shape[1], ksize=k,
                                                  stride=s, pad=p))

    def wgrad_ws_bytes(self, B, Do, Ho, Wo, Cin, Cout, k):
        return self.E.conv3d_wgrad_ws_bytes(B, Do, Ho, Wo, Cin, Cout, k)

    def wgrad(self, x, dy, k, s, p, deterministic):
        if deterministic:
            return self._ok(self.E.conv3d_wgrad_ndhwc_ex(self._c(x), self._c(dy), ksize=k, stride=s, pad=p))
        return self._ok(self.E.conv3d_wgrad_ndhwc(self._c(x), self._c(dy), ksize=k, stride=s, pad=p))

    def blend(self, level0, coarse, wsoft):
        return self._ok(self.E.blend_levels_ndhwc(self._c(level0), [self._c(t) for t in coarse], self._c(wsoft)))


# ------------------------------------------------------------------------------------------------------------------ case tables
def _cv(B, dims, Cin, Cout, k=3, s=1, p=1, relu=False, res=False, planar=False):
    return dict(B=B, dims=tuple(dims), Cin=Cin, Cout=Cout, k=k, s=s, p=p, relu=relu, res=res, planar=planar)


# fbbev_conv3d_ndhwc, fp32.  A wave owns 64 output voxels (4 tiles of 16) x MT cout tiles, a workgroup 4 waves; J = Cin / 16 channel
# groups per tap walked in ping-pong pairs; MT = 4 / 2 / 1 by the divisibility of ceil(Cout / 16), gy = ceil(Cout / 16) / MT.
FORWARD_CASES = {
    # 30 voxels: one live wave, one partial tile, two dead tiles; J = 1 (the second block of the pair runs on zeros); c0 >= Cout skipped
    'b1_3x5x2_i16_o4_k1_res': _cv(1, (3, 5, 2), 16, 4, 1, 1, 0, False, True),
    # odd J at k = 3, MT = 2 with a padded cout tile and the scalar store path
    'b1_3x5x2_i48_o19_k3': _cv(1, (3, 5, 2), 48, 19, 3, 1, 1, False, False),
    # 45 voxels per sample: tile 2 straddles the two samples; MT = 1, gy = 3
    'b2_3x3x5_i16_o48_k3_relu_res': _cv(2, (3, 3, 5), 16, 48, 3, 1, 1, True, True),
    # 288 voxels: the second workgroup has one live wave and that wave is half full (trailing waves exit at base >= nvox); MT = 2, gy = 3
    'b1_4x9x8_i32_o96_k3_relu': _cv(1, (4, 9, 8), 32, 96, 3, 1, 1, True, False),
    # stride 2 on odd and even extents, J = 5, MT = 4
    'b2_5x6x3_i80_o64_k3s2_relu': _cv(2, (5, 6, 3), 80, 64, 3, 2, 1, True, False),
    # gy = 5
    'b1_6x6x4_i16_o80_k1s2': _cv(1, (6, 6, 4), 16, 80, 1, 2, 0, False, False),
    # k = 2, MT = 4, gy = 2
    'b1_4x4x2_i32_o128_k2s2': _cv(1, (4, 4, 2), 32, 128, 2, 2, 0, False, False),
}
# fbbev_conv2d_nhwc: dims = (1, H, W), the planar instantiation (one tap along the plane axis, no padding along it)
FORWARD_2D_CASES = {
    'b2_9x7_i16_o32_k3_relu_res': _cv(2, (1, 9, 7), 16, 32, 3, 1, 1, True, True, planar=True),
    'b1_8x11_i48_o19_k3s2': _cv(1, (1, 8, 11), 48, 19, 3, 2, 1, False, False, planar=True),
    'b2_6x6_i16_o48_k1s2': _cv(2, (1, 6, 6), 16, 48, 1, 2, 0, False, False, planar=True),
}
# ConvTranspose3d kernel 2 stride 2, fp32 and bf16 (the bf16 kernel needs Cin % 32): dims = the input, the output is twice that
TRANSPOSED_CASES = {
    'b2_3x4x2_i32_o24': _cv(2, (3, 4, 2), 32, 24, 2, 2, 0, True, False),
    'b1_2x2x3_i64_o128': _cv(1, (2, 2, 3), 64, 128, 2, 2, 0, False, False),
}
# fbbev_conv3d_ndhwc_bf16: J = Cin / 32
BF16_CASES = {
    'b1_5x6x3_i32_o16_k3': _cv(1, (5, 6, 3), 32, 16, 3, 1, 1),                                    # J = 1
    'b2_5x6x3_i96_o64_k3s2_relu_res': _cv(2, (5, 6, 3), 96, 64, 3, 2, 1, True, True),             # J = 3
    'b1_3x5x2_i64_o19_k1': _cv(1, (3, 5, 2), 64, 19, 1, 1, 0),
    'planar_b2_8x6_i64_o48_k3': _cv(2, (1, 8, 6), 64, 48, 3, 1, 1, planar=True),
    'planar_b1_8x6_i32_o80_k1s2_res': _cv(1, (1, 8, 6), 32, 80, 1, 2, 0, False, True, planar=True),
}
# fbbev_conv3d_k3s1_tiled_bf16: a workgroup owns a 4 x 8 x 8 tile, the grid is whole groups of 8 tiles x gy
TILED_CASES = {
    'b1_4x8x8_i32_o16': _cv(1, (4, 8, 8), 32, 16, relu=False, res=False),          # one exact tile, 7 idle workgroups; one stage
    'b1_5x9x9_i96_o19_relu_res': _cv(1, (5, 9, 9), 96, 19, relu=True, res=True),   # 8 tiles with 1-thick partial edges; J = 3; scalar tail
    'b1_3x7x5_i64_o80_relu': _cv(1, (3, 7, 5), 64, 80, relu=True, res=False),      # smaller than a tile; gy = 5
    'b3_5x9x9_i32_o128_res': _cv(3, (5, 9, 9), 32, 128, relu=False, res=True),     # 24 tiles, gy = 2
    'b2_4x9x8_i64_o64_relu': _cv(2, (4, 9, 8), 64, 64, relu=True, res=False),      # 4 tiles padded to 8
}
# fbbev_conv3d_dgrad_ndhwc: dims = the forward input = dx
DGRAD_CASES = {
    'b1_5x6x3_i16_o16_k3': _cv(1, (5, 6, 3), 16, 16, 3, 1, 1),
    'b2_6x6x4_i16_o32_k3s2': _cv(2, (6, 6, 4), 16, 32, 3, 2, 1),
    'b1_5x7x3_i32_o48_k3s2': _cv(1, (5, 7, 3), 32, 48, 3, 2, 1),
    'b1_6x4x4_i16_o80_k1s2': _cv(1, (6, 4, 4), 16, 80, 1, 2, 0),
    'b2_4x4x2_i16_o32_k2s2': _cv(2, (4, 4, 2), 16, 32, 2, 2, 0),
}


def _wg(B, dims, Cin, Cout, k, s, p, chunk, n_chunks):
    return dict(B=B, dims=tuple(dims), Cin=Cin, Cout=Cout, k=k, s=s, p=p, chunk=chunk, n_chunks=n_chunks, relu=False, res=False, planar=False)


# fbbev_conv3d_wgrad_ndhwc / _ex: a wave owns (chunk, 64 couts, 64 cins, tap) and walks its chunk 16 voxels per iteration in ping-pong
# pairs, carrying (b, d, h, w) by 4 voxels per k-step.  chunk / n_chunks: the plan, as literal numbers.
WGRAD_CASES = {
    # 1440 voxels: 6 chunks of 256, the last of 160; Cin and Cout tails
    'b2_12x10x6_i20_o80_k3': _wg(2, (12, 10, 6), 20, 80, 3, 1, 1, 256, 6),
    # Wo = 3; the second cin block has 4 live channels; a_ok is mostly false
    'b1_5x7x5_i68_o4_k3s2': _wg(1, (5, 7, 5), 68, 4, 3, 2, 1, 256, 1),
    # 17 576 voxels: chunk 288, 62 chunks, the last of 8 voxels
    'b1_26x26x26_i4_o8_k1': _wg(1, (26, 26, 26), 4, 8, 1, 1, 0, 288, 62),
    'b1_9x5x7_i16_o16_k3': _wg(1, (9, 5, 7), 16, 16, 3, 1, 1, 256, 2),              # Wo = 7
    'b2_4x6x10_i8_o12_k1s2': _wg(2, (4, 6, 10), 8, 12, 1, 2, 0, 256, 1),            # Wo = 5
    'b9_1x1x1_i4_o4_k1': _wg(9, (1, 1, 1), 4, 4, 1, 1, 0, 256, 1),                  # every step carries through all four digits
    'b5_1x2x1_i8_o4_k1': _wg(5, (1, 2, 1), 8, 4, 1, 1, 0, 256, 1),
    'b2_3x1x2_i4_o4_k1': _wg(2, (3, 1, 2), 4, 4, 1, 1, 0, 256, 1),
    'b2_4x4x2_i16_o32_k2s2': _wg(2, (4, 4, 2), 16, 32, 2, 2, 0, 256, 1),
    # 68 voxels, 5 iterations of 16: the masked second half of the last ping-pong pair
    'b1_4x17x1_i4_o4_k1': _wg(1, (4, 17, 1), 4, 4, 1, 1, 0, 256, 1),
}


def taps_of(case):
    return case['k'] ** (2 if case['planar'] else 3)


def forward_c(n):
    return (n + 3) * U24 * 1.001


def wgrad_c(case):
    return (case['chunk'] + case['n_chunks'] + 2) * U24 * 1.001


def check_tables_stay_exact():
    """layer A's premise, from the table alone: |operand| <= 4, so a sum of n products is at most 16 n (+ 4 + 4 for bias and residual)"""
    for table in (FORWARD_CASES, FORWARD_2D_CASES, TRANSPOSED_CASES, BF16_CASES, TILED_CASES):
        for name, c in table.items():
            assert taps_of(c) * c['Cin'] * 16 + 8 < EXACT_LIMIT, name
    for name, c in DGRAD_CASES.items():
        assert taps_of(c) * c['Cout'] * 16 < EXACT_LIMIT, name
    for name, c in WGRAD_CASES.items():
        nvox = c['B'] * _prod(out_dims(c['dims'], c['k'], c['s'], c['p']))
        assert nvox * 16 < EXACT_LIMIT, name
        assert c['n_chunks'] == (nvox + c['chunk'] - 1) // c['chunk'] and c['chunk'] % 16 == 0 and c['chunk'] >= 256, name


def _prod(v):
    r = 1
    for n in v:
        r *= n
    return r


# ------------------------------------------------------------------------------------------------------------------ inputs and references
def _ints(shape, g):
    return torch.randint(-4, 5, tuple(shape), generator=g).float()


def _seed(case, real, extra=0):
    return sum(case['dims']) * 131 + case['B'] * 17 + case['Cin'] * 7 + case['Cout'] * 3 + case['k'] + case['s'] * 1009 + (5000 if real else 0) + extra


def conv_inputs(case, real, transposed=False):
    """-> x (B, D, H, W, Cin), w (torch layout, 5-D; planar: one tap along the plane axis), b (Cout), res (like the output) or None"""
    g = torch.Generator().manual_seed(_seed(case, real, 77 if transposed else 0))
    B, dims, Cin, Cout, k = case['B'], case['dims'], case['Cin'], case['Cout'], case['k']
    wshape = (Cin, Cout, 2, 2, 2) if transposed else (Cout, Cin, 1 if case['planar'] else k, k, k)
    odims = tuple(2 * d for d in dims) if transposed else out_dims(dims, k, case['s'], case['p'], case['planar'])
    n = Cin if transposed else Cin * taps_of(case)
    if real:
        x, w, b = torch.randn(B, *dims, Cin, generator=g), torch.randn(wshape, generator=g) * n ** -0.5, torch.randn(Cout, generator=g)
        res = torch.randn(B, *odims, Cout, generator=g) if case['res'] else None
    else:
        x, w, b = _ints((B, *dims, Cin), g), _ints(wshape, g), _ints((Cout,), g)
        res = _ints((B, *odims, Cout), g) if case['res'] else None
    return x, w, b, res


def conv_ref(case, x, w, b, res, transposed=False, relu=None):
    """float64, NDHWC in and out; relu=False for the magnitude sum S"""
    xn = x.double().permute(0, 4, 1, 2, 3)
    if transposed:
        y = F.conv_transpose3d(xn, w.double(), b.double(), stride=2)
    else:
        s, p = case['s'], case['p']
        y = F.conv3d(xn, w.double(), b.double(), stride=(1, s, s) if case['planar'] else s, padding=(0, p, p) if case['planar'] else p)
    y = y.permute(0, 2, 3, 4, 1)
    if res is not None:
        y = y + res.double()
    return y.relu() if (case['relu'] if relu is None else relu) else y.contiguous()


def _magnitudes(case, x, w, b, res, transposed=False):
    return conv_ref(case, x.abs(), w.abs(), b.abs(), None if res is None else res.abs(), transposed, relu=False)


def _rb(t):
    """round to bf16, nearest even"""
    return t.bfloat16().float()


def _no_nan(t, what):
    assert not torch.isnan(t).any(), f'{what}: NaN left in the output'
    return t


def _inside(err, bound):
    """componentwise err <= bound (where the bound is zero the result must be exact) -> the largest err / bound"""
    assert (err <= bound).all(), f'max err / bound = {(err / bound)[bound > 0].max().item():.3f}; ' \
                                 f'{int((err > bound).sum())} of {err.numel()} elements outside'
    pos = bound > 0
    return (err[pos] / bound[pos]).max().item() if pos.any() else 0.0


def _run_f32(api, kind, case, x, w, b, res):
    k, s, p, relu = case['k'], case['s'], case['p'], case['relu']
    if kind == 'f32':
        return api.conv(x, w, b, k, s, p, relu=relu, res=res)
    if kind == '2d':
        return api.conv2d(x[:, 0], w[:, :, 0], b, k, s, p, relu=relu, res=None if res is None else res[:, 0])[:, None]
    assert kind == 'transposed'
    return api.conv_transposed(x, w, b, relu=relu)


def _run_bf16(api, kind, case, x, w, b, res):
    k, s, p, relu = case['k'], case['s'], case['p'], case['relu']
    if kind == 'bf16':
        return api.conv_bf16(x, w, b, k, s, p, relu=relu, res=res, planar=case['planar'])
    if kind == 'tiled':
        return api.conv_tiled(x, w, b, relu=relu, res=res)
    assert kind == 'transposed_bf16'
    return api.conv_transposed_bf16(x, w, b, relu=relu)


# ------------------------------------------------------------------------------------------------------------------ forward checks
def check_conv_exact(api, kind, name, case):
    """layer A for every forward kernel; `tiled` also against the direct bf16 kernel"""
    T = kind.startswith('transposed')
    x, w, b, res = conv_inputs(case, real=False, transposed=T)
    exp = conv_ref(case, x, w, b, res, T)
    assert _magnitudes(case, x, w, b, res, T).max().item() < EXACT_LIMIT
    run = _run_f32 if kind in ('f32', '2d', 'transposed') else _run_bf16
    got = _no_nan(run(api, kind, case, x, w, b, res), name)
    assert got.shape == exp.shape
    bad = int((got.double() != exp).sum())
    observed(f'{api.name} conv {kind} {name} layer A: elements that differ from float64 = {bad} of {exp.numel()}')
    assert torch.equal(got.double(), exp)
    if kind == 'tiled':
        direct = _no_nan(api.conv_bf16(x, w, b, 3, 1, 1, relu=case['relu'], res=res), name)
        assert torch.equal(got, direct), 'the tiled kernel differs from the direct bf16 kernel'


def check_conv_real_f32(api, kind, name, case):
    """layer B for fbbev_conv3d_ndhwc (plain, transposed) and fbbev_conv2d_nhwc"""
    T = kind == 'transposed'
    x, w, b, res = conv_inputs(case, real=True, transposed=T)
    exact, S = conv_ref(case, x, w, b, res, T), _magnitudes(case, x, w, b, res, T)
    got = _no_nan(_run_f32(api, kind, case, x, w, b, res), name).double()
    assert got.shape == exact.shape
    n = case['Cin'] if T else taps_of(case) * case['Cin']
    err = (got - exact).abs()
    e16 = (conv_ref(case, _rb(x), _rb(w), b, res, T) - exact).abs().max().item()
    bound = forward_c(n) * S
    worst = (err / bound).max().item()
    observed(f'{api.name} conv {kind} {name} layer B: max err / (c S) = {worst:.4f} (n = {n}, c = {forward_c(n):.3e}); max|err| = '
             f'{err.max().item():.3e}, bf16-rounded operands {e16:.3e} (ratio {e16 / max(err.max().item(), 1e-300):.0f})')
    _inside(err, bound)
    assert err.max().item() * 30 < e16


def check_conv_real_bf16(api, kind, name, case):
    """layer B for the bf16 kernels: activations that are bf16 values already, and full mantissas rounded in the reference only"""
    T = kind == 'transposed_bf16'
    x, w, b, res = conv_inputs(case, real=True, transposed=T)
    n = case['Cin'] if T else taps_of(case) * case['Cin']
    worst = {}
    for variant, xin in (('representable', _rb(x)), ('full mantissa', x)):
        exact, S = conv_ref(case, _rb(xin), _rb(w), b, res, T), _magnitudes(case, _rb(xin), _rb(w), b, res, T)
        got = _no_nan(_run_bf16(api, kind, case, xin, w, b, res), name).double()
        assert got.shape == exact.shape
        err, bound = (got - exact).abs(), forward_c(n) * S
        worst[variant] = ((err / bound).max().item(), err.max().item())
    observed(f'{api.name} conv {kind} {name} layer B: max err / (c S) = ' +
             ', '.join(f'{v[0]:.4f} ({k}, max|err| {v[1]:.3e})' for k, v in worst.items()) + f' (n = {n}, c = {forward_c(n):.3e})')
    assert all(v[0] <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------------------------ gradients
def grad_inputs(case, real):
    """-> x (B, D, H, W, Cin), w (Cout, Cin, k, k, k), dy (B, Do, Ho, Wo, Cout)"""
    g = torch.Generator().manual_seed(_seed(case, real, 31))
    B, dims, Cin, Cout, k = case['B'], case['dims'], case['Cin'], case['Cout'], case['k']
    od = out_dims(dims, k, case['s'], case['p'])
    if real:
        return (torch.randn(B, *dims, Cin, generator=g), torch.randn(Cout, Cin, k, k, k, generator=g) * (Cout * k ** 3) ** -0.5,
                torch.randn(B, *od, Cout, generator=g))
    return _ints((B, *dims, Cin), g), _ints((Cout, Cin, k, k, k), g), _ints((B, *od, Cout), g)


def grad_ref(case, x, w, dy):
    """float64 autograd -> dx (B, D, H, W, Cin), dw (k^3, Cout, Cin)"""
    xn = x.double().permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
    wd = w.double().clone().requires_grad_()
    F.conv3d(xn, wd, None, stride=case['s'], padding=case['p']).backward(dy.double().permute(0, 4, 1, 2, 3).contiguous())
    k = case['k']
    return xn.grad.permute(0, 2, 3, 4, 1).contiguous(), wd.grad.permute(2, 3, 4, 0, 1).reshape(k ** 3, case['Cout'], case['Cin']).contiguous()


def check_dgrad_exact(api, name, case):
    x, w, dy = grad_inputs(case, real=False)
    exp = grad_ref(case, x, w, dy)[0]
    got = _no_nan(api.dgrad(dy, w, case['dims'], case['k'], case['s'], case['p']), name)
    bad = int((got.double() != exp).sum())
    observed(f'{api.name} conv dgrad {name} layer A: elements that differ from float64 = {bad} of {exp.numel()}')
    assert got.shape == exp.shape and torch.equal(got.double(), exp)


def check_dgrad_real(api, name, case):
    x, w, dy = grad_inputs(case, real=True)
    exact, S = grad_ref(case, x, w, dy)[0], grad_ref(case, x, w.abs(), dy.abs())[0]
    got = _no_nan(api.dgrad(dy, w, case['dims'], case['k'], case['s'], case['p']), name).double()
    n = case['k'] ** 3 * case['Cout']
    err = (got - exact).abs()
    e16 = (grad_ref(case, x, _rb(w), _rb(dy))[0] - exact).abs().max().item()
    worst = _inside(err, forward_c(n) * S)
    observed(f'{api.name} conv dgrad {name} layer B: max err / (c S) = {worst:.4f} (n = {n}, c = {forward_c(n):.3e}); max|err| = '
             f'{err.max().item():.3e}, bf16-rounded operands {e16:.3e} (ratio {e16 / max(err.max().item(), 1e-300):.0f})')
    assert err.max().item() * 30 < e16


def check_wgrad_plan(api, case):
    od = out_dims(case['dims'], case['k'], case['s'], case['p'])
    assert api.wgrad_ws_bytes(case['B'], *od, case['Cin'], case['Cout'], case['k']) == \
        case['n_chunks'] * case['k'] ** 3 * case['Cout'] * case['Cin'] * 4


def check_wgrad_exact(api, name, case):
    """layer A for both routes, which must also equal each other"""
    x, w, dy = grad_inputs(case, real=False)
    k, s, p = case['k'], case['s'], case['p']
    exp = grad_ref(case, x, w, dy)[1]
    assert grad_ref(case, x.abs(), w, dy.abs())[1].max().item() < EXACT_LIMIT
    atomic = _no_nan(api.wgrad(x, dy, k, s, p, deterministic=False), name)
    det = _no_nan(api.wgrad(x, dy, k, s, p, deterministic=True), name)
    bad = (int((atomic.double() != exp).sum()), int((det.double() != exp).sum()))
    observed(f'{api.name} conv wgrad {name} layer A: elements that differ from float64 = {bad[0]} (atomic), {bad[1]} (deterministic) '
             f'of {exp.numel()}')
    assert atomic.shape == exp.shape and torch.equal(atomic.double(), exp)
    assert torch.equal(det.double(), exp)
    assert torch.equal(atomic, det), 'the atomic and the deterministic route differ'


def check_wgrad_real(api, name, case):
    """layer B for both routes; the deterministic route bit-stable over three calls"""
    x, w, dy = grad_inputs(case, real=True)
    k, s, p = case['k'], case['s'], case['p']
    exact, S = grad_ref(case, x, w, dy)[1], grad_ref(case, x.abs(), w, dy.abs())[1]
    e16 = (grad_ref(case, _rb(x), w, _rb(dy))[1] - exact).abs().max().item()
    atomic = _no_nan(api.wgrad(x, dy, k, s, p, deterministic=False), name)
    det = [_no_nan(api.wgrad(x, dy, k, s, p, deterministic=True), name) for _ in range(3)]
    assert torch.equal(det[0], det[1]) and torch.equal(det[0], det[2]), 'the deterministic route is not bit-stable'
    c = wgrad_c(case)
    for route, got in (('atomic', atomic), ('deterministic', det[0])):
        err = (got.double() - exact).abs()
        worst = _inside(err, c * S)
        observed(f'{api.name} conv wgrad {name} layer B {route}: max err / (c S) = {worst:.4f} (chunk {case["chunk"]} x {case["n_chunks"]}, '
                 f'c = {c:.3e}); max|err| = {err.max().item():.3e}, bf16-rounded operands {e16:.3e} '
                 f'(ratio {e16 / max(err.max().item(), 1e-300):.0f})')
        assert err.max().item() * 30 < e16


# ------------------------------------------------------------------------------------------------------------------ level blend
def _bl(B, dims, coarse, C, K):
    return dict(B=B, dims=tuple(dims), coarse=[tuple(c) for c in coarse], C=C, K=K)


# n_coarse over 0..3, K > n_coarse + 1, C 4 or 20.  Exact: ratios 2 and 4 on every axis, coarse extents of 1 included.
BLEND_EXACT_CASES = {
    'n0_c4': _bl(2, (4, 8, 2), [], 4, 3),
    'n1_c20': _bl(2, (4, 8, 2), [(2, 4, 1)], 20, 3),
    'n2_c4': _bl(1, (4, 8, 2), [(2, 4, 1), (1, 2, 1)], 4, 4),
    'n3_c20': _bl(2, (4, 8, 2), [(2, 4, 1), (1, 2, 1), (2, 2, 1)], 20, 6),
}
# Real: 10 from 3, 6 from 4, and extents of 1
BLEND_REAL_CASES = {
    'n0_c20': _bl(1, (6, 10, 6), [], 20, 2),
    'n1_c4': _bl(2, (6, 10, 6), [(4, 3, 4)], 4, 3),
    'n2_c20': _bl(1, (6, 10, 6), [(4, 3, 4), (4, 3, 1)], 20, 4),
    'n3_c4': _bl(2, (6, 10, 6), [(4, 3, 4), (1, 3, 4), (4, 1, 1)], 4, 5),
}


def blend_inputs(case, real):
    g = torch.Generator().manual_seed(sum(case['dims']) + 10 * len(case['coarse']) + case['C'] + (500 if real else 0))
    B, dims, C, K, n = case['B'], case['dims'], case['C'], case['K'], len(case['coarse'])
    wsoft = torch.full((B, *dims, K), NAN)
    if real:
        level0, coarse = torch.randn(B, *dims, C, generator=g), [torch.randn(B, *d, C, generator=g) for d in case['coarse']]
        wsoft[..., :n + 1] = torch.randn(B, *dims, n + 2, generator=g).softmax(-1)[..., :n + 1]
    else:
        level0, coarse = _ints((B, *dims, C), g), [_ints((B, *d, C), g) for d in case['coarse']]
        wsoft[..., :n + 1] = torch.randint(-8, 9, (B, *dims, n + 1), generator=g).float() / 8
    return level0, coarse, wsoft


def blend_ref(case, level0, coarse, wsoft):
    """float64 composite -> (result, sum_k |w_k| max|f_k|)"""
    ws = wsoft.double()
    out = level0.double() * ws[..., 0:1]
    mag = ws[..., 0:1].abs() * level0.abs().max().item()
    for k, f in enumerate(coarse):
        up = F.interpolate(f.double().permute(0, 4, 1, 2, 3), size=list(case['dims']), mode='trilinear', align_corners=False)
        out = out + up.permute(0, 2, 3, 4, 1) * ws[..., k + 1:k + 2]
        mag = mag + ws[..., k + 1:k + 2].abs() * f.abs().max().item()
    return out, mag.expand_as(out)


def check_blend_exact(api, name, case):
    level0, coarse, wsoft = blend_inputs(case, real=False)
    exp = blend_ref(case, level0, coarse, wsoft)[0]
    got = _no_nan(api.blend(level0, coarse, wsoft), name)
    bad = int((got.double() != exp).sum())
    observed(f'{api.name} blend {name} layer A: elements that differ from float64 = {bad} of {exp.numel()}')
    assert got.shape == exp.shape and torch.equal(got.double(), exp)


def check_blend_real(api, name, case):
    level0, coarse, wsoft = blend_inputs(case, real=True)
    exact, mag = blend_ref(case, level0, coarse, wsoft)
    got = _no_nan(api.blend(level0, coarse, wsoft), name).double()
    eps = (9 * max([1] + [max(d) for d in case['coarse']]) + 16) * U24
    err = (got - exact).abs()
    worst = _inside(err, eps * mag)
    observed(f'{api.name} blend {name} layer B: max err / bound = {worst:.4f} (eps = {eps:.3e}); max|err| = {err.max().item():.3e}')


# ------------------------------------------------------------------------------------------------------------------ bias guard
def check_bias_guard():
    """the four forward wrappers of fb_bev_amd._capi refuse a bias shorter than 16 * ceil(Cout / 16) before they look at the device:
    CPU tensors reach the guard, and with a padded bias the same call gets as far as the device check"""
    import pytest
    from fb_bev_amd import _capi
    x, x2 = torch.zeros(1, 4, 8, 8, 32), torch.zeros(1, 8, 8, 32)
    wf, wfb = torch.zeros(27 * 2 * 2 * 256), torch.zeros(27 * 2 * 512, dtype=torch.bfloat16)
    out, out2 = torch.zeros(1, 4, 8, 8, 19), torch.zeros(1, 8, 8, 19)
    calls = {
        'conv3d_ndhwc': lambda b: _capi.conv3d_ndhwc(x, wf, b, out, 19),
        'conv2d_nhwc': lambda b: _capi.conv2d_nhwc(x2, wf, b, out2, 19),
        'conv3d_ndhwc_bf16': lambda b: _capi.conv3d_ndhwc_bf16(x, wfb, b, out, 19),
        'conv3d_k3s1_tiled_bf16': lambda b: _capi.conv3d_k3s1_tiled_bf16(x, wfb, b, out, 19),
    }
    for what, call in calls.items():
        for short in (torch.zeros(19), torch.zeros(31), torch.zeros(0), None):
            with pytest.raises(_capi.FbbevError, match=f'{what}: bias must be zero-padded to 32 floats'):
                call(short)
        with pytest.raises(_capi.FbbevError, match='GPU tensor'):
            call(torch.zeros(32))
    with pytest.raises(_capi.FbbevError, match='zero-padded to 16 floats'):
        _capi.conv3d_ndhwc(x, wf, torch.zeros(4), torch.zeros(1, 4, 8, 8, 4), 4)
