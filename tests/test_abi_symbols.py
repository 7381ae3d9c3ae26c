"""CPU-side checks of the drop-in boundary: libfbbev_hip.so loads and exports every symbol that
include/fbbev.h declares; the Python signature table matches the header; the product refuses CPU
tensors (no fallback).  No compute calls are made (no GPU here)."""
import ctypes
import os
import re

import pytest
import torch

from fb_bev_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, 'include', 'fbbev.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return {m.group(2): m.group(3) for m in
            re.finditer(r'\b(int|size_t)\s+(fbbev_\w+)\s*\(([^;]*?)\)\s*;', src, flags=re.S)}


def test_header_and_signature_table_agree():
    decl = header_functions()
    assert set(decl) == set(_capi.SIGNATURES), set(decl) ^ set(_capi.SIGNATURES)
    for name, args in decl.items():
        n = 0 if args.strip() in ('void', '') else len(args.split(','))
        assert n == len(_capi.SIGNATURES[name][1]), name


def test_library_exports_every_symbol():
    assert os.path.exists(_capi.LIB_PATH), 'run `python -m fb_bev_amd.build` (or __graft_entry__.build())'
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in header_functions():
        assert hasattr(lib, name), name
    _capi.declare(lib)
    assert lib.fbbev_version() >= 100


def test_no_cpu_fallback():
    from fb_bev_amd import bev_pool_v2_ext, ms_deform_attn
    x = torch.zeros(1, 1, 2, 2, 2)
    i = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_capi.FbbevError):
        bev_pool_v2_ext.bev_pool_v2_forward(x, x, x.clone(), i, i, i, i, i)
    with pytest.raises(_capi.FbbevError):
        ms_deform_attn.ms_deform_attn_forward(torch.zeros(1, 4, 1, 1), torch.tensor([[2, 2]]), torch.tensor([0]),
                                              torch.zeros(1, 1, 1, 1, 1, 2), torch.zeros(1, 1, 1, 1, 1))


def test_compat_install_binds_reference_names():
    import sys
    from fb_bev_amd import compat
    ext = compat.install(force=True)
    assert sys.modules['mmdet3d.ops.bev_pool_v2.bev_pool_v2_ext'].bev_pool_v2_forward
    assert callable(ext.ms_deform_attn_forward) and callable(ext.ms_deform_attn_backward)
    del sys.modules['mmdet3d.ops.bev_pool_v2.bev_pool_v2_ext']


def test_invalid_arguments_return_error_codes_without_touching_the_gpu():
    """Error convention of include/fbbev.h: <0 for invalid arguments, never an exception across the ABI.
    Every call below is rejected by the argument checks BEFORE any launch, so this runs without a GPU."""
    lib = _capi.declare(ctypes.CDLL(_capi.LIB_PATH))
    NULL = ctypes.c_void_p(0)
    P = ctypes.c_void_p(0x1000)          # non-null dummy; never dereferenced on these paths
    assert lib.fbbev_bev_pool_v2_fwd(0, 4, P, P, P, P, P, P, P, P, NULL) == -1          # c <= 0
    assert lib.fbbev_bev_pool_v2_fwd(80, -1, P, P, P, P, P, P, P, P, NULL) == -1        # n_intervals < 0
    assert lib.fbbev_bev_pool_v2_fwd(80, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0   # empty: no-op
    assert lib.fbbev_bev_pool_v2_fwd(80, 4, NULL, P, P, P, P, P, P, P, NULL) == -1      # null depth
    assert lib.fbbev_bev_pool_v2_bwd(300, 4, P, P, P, P, P, P, P, P, P, P, NULL) == -2  # c > 256 unsupported
    assert lib.fbbev_lidar_coor(P, P, P, P, P, P, P, P, P, 0, 6, 8, 4, 6, P, NULL) == -1
    assert lib.fbbev_rank_build(NULL, 1, 6, 8, 4, 6, P, P, P, P, P, P, P, P, P, P, P, 1 << 30, NULL) == -1
    assert lib.fbbev_rank_build(P, 1, 6, 8, 4, 6, P, P, P, P, P, P, P, P, P, P, P, 16, NULL) == -3      # workspace too small
    assert lib.fbbev_pool_tile_index(P, P, P, 10, 1, 16, 200, 200, 128, 0, P, 8, NULL) == -3
    assert lib.fbbev_bev_pool_v2_dense_fwd(P, P, P, P, P, P, P, 1, 6, 4, 16, 16, P, 0, 0, P, 1 << 20, 128, 0, NULL) == -2  # C % 4
    assert lib.fbbev_bev_pool_v2_dense_fwd(P, P, P, P, P, P, P, 1, 8, 4, 16, 16, P, 0, 17, P, 1 << 20, 128, 0, NULL) == -1  # bad stride
    assert lib.fbbev_msda_fwd(P, P, P, P, P, 1, 0, 8, 10, 1, 5, 4, P, NULL) == -1       # spatial_size <= 0
    assert lib.fbbev_msda_fwd(P, P, P, P, P, 0, 704, 8, 10, 1, 5, 4, P, NULL) == 0      # empty batch: no-op
    assert lib.fbbev_da_cross_attn_fwd(P, P, P, P, P, P, P, P, P, 1, 6, 704, 8, 10, 1, 100, 8, 16, 80, 2.0, 0.5, 0, 0, P, NULL) == -2  # Za > 8
    assert lib.fbbev_da_cross_attn_fwd(P, P, P, P, P, P, P, P, P, 1, 6, 704, 8, 10, 1, 100, 8, 4, 80, 2.0, 0.0, 0, 0, P, NULL) == -1   # dstep == 0
    # temporal history fusion: the reference-layout entries and the voxel-major ring
    P16, P8 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)     # 16-byte aligned / not
    assert lib.fbbev_history_warp_e(P, 0, P, 1, 80, 1, 8, 8, P, 0, 0, NULL) == -1          # Z < 2 (the reference divides by Z - 1)
    assert lib.fbbev_history_warp_e(P, 0, P, 0, 80, 8, 8, 8, P, 0, 0, NULL) == 0           # empty batch: no-op
    assert lib.fbbev_history_warp_vm(P16, 0, P, 1, 16, 80, 8, 8, 8, P16, 0, 3, NULL) == -1  # elem_type
    assert lib.fbbev_history_warp_vm(P16, 0, P, 1, 16, 84, 8, 8, 8, P16, 0, 2, NULL) == -2  # C % 8 (16-bit row pieces)
    assert lib.fbbev_history_warp_vm(P16, 0, P, 1, 16, 80, 8, 8, 8, P8, 0, 2, NULL) == -2   # out not 16-byte aligned
    assert lib.fbbev_history_warp_vm(P16, 100, P, 1, 16, 80, 8, 8, 8, P16, 0, 2, NULL) == -1    # batch stride < T*N*C
    assert lib.fbbev_history_warp_vm(P16, 0, P, 1, 0, 80, 8, 8, 8, P16, 0, 2, NULL) == 0    # no frames: no-op
    assert lib.fbbev_history_frame_vm(P, 1, 80, 512, 3, P16, 0, 2, NULL) == -1              # N % inner
    assert lib.fbbev_history_frame_vm(P, 1, 82, 512, 1, P16, 0, 2, NULL) == -2              # C % 8
    assert lib.fbbev_history_conv_bf16(P16, 0, P16, P16, P16, P16, 1, 17, 32, 32, 64, P16, P16, 1 << 20, 0, 1, NULL) == -2   # C in {16, 80}
    assert lib.fbbev_history_conv_bf16(P16, 0, P16, P16, P16, P16, 1, 17, 80, 80, 64, P16, P16, 16, 0, 1, NULL) == -3        # workspace
    assert lib.fbbev_history_conv_bf16(P16, 0, P16, P16, P16, P16, 1, 17, 80, 80, 64, P16, P16, 1 << 20, 2, 1, NULL) == -1   # layout flag
    assert lib.fbbev_history_conv_bf16(P8, 0, P16, P16, P16, P16, 1, 17, 80, 80, 64, P16, P16, 1 << 20, 1, 1, NULL) == -2    # rows not aligned
    assert lib.fbbev_history_conv_vm(P16, 0, P16, P16, P16, P16, 1, 17, 80, 80, 64, P16, NULL, 0, 1, NULL) == -3             # workspace required
    assert lib.fbbev_history_conv_vm(P16, 0, P16, P16, P16, P16, 1, 17, 48, 48, 64, P16, P16, 1 << 20, 1, NULL) == -2
    assert lib.fbbev_history_conv_e(P16, 0, P16, P8, P16, P16, 1, 17, 80, 80, 64, P16, P16, 1 << 20, 1, NULL) == -2          # bias rows are 16-byte loads
    assert lib.fbbev_rank_workspace_bytes(0) == 256 and lib.fbbev_pool_dense_workspace_bytes(0, 1, 1, 1) == 256
    # row operands of the row-wise linear family (256 rows, 80 -> 80 features, hidden 320): a row stride below the width is -1, a
    # stride that is no multiple of 4 floats or a pointer off a 16-byte boundary is -2; where two defects coincide the code is
    # that of the check the entry makes first
    for fam in ('x3', 'f32'):
        lin, add, ln = (getattr(lib, f'fbbev_rows_linear_{fam}{s}') for s in ('', '_add', '_ln'))
        assert lin(P16, 40, P16, P16, 256, 80, 80, 0, P16, 0, NULL) == -1                   # x stride < in_features
        assert lin(P16, 0, P16, P16, 256, 80, 80, 0, P16, 82, NULL) == -2                   # out stride % 4
        assert lin(P8, 0, P16, P16, 256, 80, 80, 0, P16, 0, NULL) == -2                     # x misaligned
        assert lin(P8, 0, P16, P16, 256, 80, 80, 0, P16, 40, NULL) == -1                    # ... and out stride < out_features
        assert lin(P16, 82, P16, P16, 256, 80, 80, 0, P16, 40, NULL) == -1                  # x stride % 4, out stride too short
        assert lin(P16, 82, P8, P16, -1, 80, 80, 0, P16, 0, NULL) == -1                     # rows < 0 comes before both
        assert add(P16, 0, P16, 40, 1, P16, P16, 256, 80, 80, 0, P16, 0, NULL) == -1        # addend stride < in_features
        assert add(P16, 0, P16, 82, 1, P16, P16, 256, 80, 80, 0, P16, 0, NULL) == -2        # addend stride % 4
        assert add(P16, 0, P8, 0, 1, P16, P16, 256, 80, 80, 0, P16, 0, NULL) == -2          # addend misaligned
        assert add(P16, 0, P8, 0, 1, P16, P16, -1, 80, 80, 0, P16, 0, NULL) == -2           # ... checked before rows < 0
        assert add(P16, 40, P16, 82, 1, P16, P16, 256, 80, 80, 0, P16, 0, NULL) == -2       # ... and before x's stride
        assert add(P8, 0, P16, 40, 1, P16, P16, 256, 80, 80, 0, P16, 0, NULL) == -1         # short addend rows, x misaligned
        assert add(P16, 0, P8, 40, 0, P16, P16, 256, 80, 80, 0, P16, 0, NULL) == -1         # period <= 0 comes first
        assert ln(P16, 0, P16, P16, 256, 80, 80, P16, 40, P16, P16, 1e-5, P16, 0, NULL) == -1   # residual stride < out_features
        assert ln(P16, 0, P16, P16, 256, 80, 80, P8, 0, P16, P16, 1e-5, P16, 0, NULL) == -2     # residual misaligned
        assert ln(P16, 40, P16, P16, 256, 80, 80, P8, 0, P16, P16, 1e-5, P16, 0, NULL) == -2    # ... checked before x's stride
        assert ln(P16, 0, P16, P16, 256, 80, 80, P16, 40, P8, P16, 1e-5, P16, 0, NULL) == -1    # short residual rows, ln_weight misaligned
        assert ln(P16, 0, P16, P16, 256, 80, 80, NULL, 40, P16, P16, 1e-5, P8, 0, NULL) == -2   # no residual: its stride is not looked at
    train = lib.fbbev_rows_linear_x3_train
    assert train(P16, 0, NULL, 0, 0, P16, P16, 256, 80, 80, 0, P16, 40, P16, 0, P16, 0, NULL) == -1     # residual stride < out_features
    assert train(P16, 0, NULL, 0, 0, P16, P16, 256, 80, 80, 0, P16, 0, P16, 82, P16, 0, NULL) == -2     # mask stride % 4
    assert train(P16, 0, NULL, 0, 0, P16, P16, 256, 80, 80, 0, P16, 0, P8, 0, P16, 0, NULL) == -2       # mask misaligned
    assert train(P16, 0, P16, 40, 1, P16, P16, 256, 80, 80, 0, P16, 0, P16, 0, P16, 0, NULL) == -1      # addend stride < in_features
    assert train(P16, 0, NULL, 0, 0, P16, P16, 256, 80, 80, 0, P8, 0, P16, 40, P16, 0, NULL) == -2      # residual (misaligned) before mask (short)
    assert train(P16, 0, P16, 82, 1, P16, P16, 256, 80, 80, 0, P16, 40, P16, 0, P16, 0, NULL) == -2     # addend (% 4) before residual (short)
    assert train(P16, 0, NULL, 0, 0, P16, P16, -1, 80, 80, 0, P16, 0, P16, 40, P16, 0, NULL) == -1      # mask (short) before rows < 0
    assert train(P8, 0, NULL, 0, 0, P16, P16, 256, 80, 80, 0, P16, 0, P16, 0, P16, 40, NULL) == -1      # x misaligned, out rows short
    planes, planes_e = lib.fbbev_rows_linear_x3_planes, lib.fbbev_rows_linear_x3_planes_e
    assert planes(P16, 40, P16, P16, 256, 80, 80, 128, 10, P16, NULL) == -1                 # x stride < in_features
    assert planes(P8, 0, P16, P16, 256, 80, 80, 128, 10, P16, NULL) == -2                   # x misaligned
    assert planes(P16, 40, P8, P16, 256, 80, 80, 128, 10, P16, NULL) == -1                  # short x rows, fragments misaligned
    assert planes(P16, 40, P16, P16, 256, 80, 80, 128, 10, ctypes.c_void_p(0x1004), NULL) == -2      # out off 8 bytes comes first
    assert planes_e(P16, 40, P16, P16, 256, 80, 80, 128, 10, 1, P16, NULL) == -1
    assert planes_e(P16, 82, P16, P16, 256, 80, 80, 128, 10, 1, P16, NULL) == -2            # x stride % 4
    assert planes_e(P8, 0, P16, P16, 256, 80, 80, 128, 10, 2, P16, NULL) == -2
    assert planes_e(P16, 40, P16, P8, 256, 80, 80, 128, 10, 1, P16, NULL) == -1             # short x rows, bias misaligned
    assert planes_e(P16, 40, P16, P16, 256, 80, 80, 128, 10, 1, P8, NULL) == -2             # out off 16 bytes comes first
    ffn = lib.fbbev_rows_ffn_x3
    assert ffn(P16, 40, P16, P16, P16, P16, 256, 80, 320, 80, NULL, 0, NULL, NULL, 0.0, P16, 0, NULL) == -1      # x stride
    assert ffn(P16, 0, P16, P16, P16, P16, 256, 80, 320, 80, P16, 40, NULL, NULL, 0.0, P16, 0, NULL) == -1       # residual stride
    assert ffn(P16, 0, P16, P16, P16, P16, 256, 80, 320, 80, P16, 82, NULL, NULL, 0.0, P16, 0, NULL) == -2       # residual stride % 4
    assert ffn(P16, 0, P16, P16, P16, P16, 256, 80, 320, 80, P8, 0, NULL, NULL, 0.0, P16, 0, NULL) == -2         # residual misaligned
    assert ffn(P8, 0, P16, P16, P16, P16, 256, 80, 320, 80, P16, 40, NULL, NULL, 0.0, P16, 0, NULL) == -1        # ... x misaligned as well
    assert ffn(P16, 82, P16, P16, P16, P16, 256, 80, 320, 80, NULL, 0, NULL, NULL, 0.0, P16, 40, NULL) == -1     # x % 4, out short
    tail, tail_planes = lib.fbbev_rows_tail_ffn_x3, lib.fbbev_rows_tail_ffn_x3_planes
    W = (P16, P16, P16, P16)                                                                 # w1 fragments, b1, w2 fragments, b2
    assert tail(P16, 40, P16, P16, NULL, 0, P16, P16, 1e-5, *W, 256, 80, 320, P16, P16, 1e-5, P16, 0, NULL) == -1    # x stride
    assert tail(P16, 0, P16, P16, P16, 40, P16, P16, 1e-5, *W, 256, 80, 320, P16, P16, 1e-5, P16, 0, NULL) == -1     # residual0 stride
    assert tail(P16, 0, P16, P16, P8, 0, P16, P16, 1e-5, *W, 256, 80, 320, P16, P16, 1e-5, P16, 0, NULL) == -2       # residual0 misaligned
    assert tail(P16, 0, P16, P16, P16, 0, P16, P16, 1e-5, *W, 256, 80, 320, P16, P16, 1e-5, P16, 82, NULL) == -2     # out stride % 4
    assert tail(P8, 0, P16, P16, P16, 0, P16, P16, 1e-5, *W, 256, 80, 320, P16, P16, 1e-5, P16, 40, NULL) == -1      # x misaligned, out short
    assert tail(P16, 0, P16, P16, P8, 40, P16, P16, 1e-5, *W, 256, 80, 320, P16, P16, 1e-5, P16, 0, NULL) == -1      # residual0 short and misaligned
    assert tail_planes(P16, 40, P16, P16, NULL, 0, P16, P16, 1e-5, *W, 256, 80, 320, P16, P16, 1e-5, 128, P16, NULL) == -1
    assert tail_planes(P8, 0, P16, P16, NULL, 0, P16, P16, 1e-5, *W, 256, 80, 320, P16, P16, 1e-5, 128, P16, NULL) == -2
    assert tail_planes(P16, 0, P16, P16, P16, 82, P16, P16, 1e-5, *W, 256, 80, 320, P16, P16, 1e-5, 128, P16, NULL) == -2
    assert tail_planes(P16, 0, P16, P16, P16, 40, P16, P16, 1e-5, *W, 256, 80, 320, P16, P16, 1e-5, 128, P8, NULL) == -1   # residual0 short, out misaligned
    wgrad = lib.fbbev_rows_wgrad_x3
    assert wgrad(P16, 0, P16, 0, P16, 40, 1, 256, 80, 80, P16, P16, P16, 1 << 30, NULL) == -1      # addend stride < in_features
    assert wgrad(P16, 0, P16, 0, P16, 82, 1, 256, 80, 80, P16, P16, P16, 1 << 30, NULL) == -2      # addend stride % 4
    assert wgrad(P16, 0, P16, 0, P8, 0, 1, 256, 80, 80, P16, P16, P16, 1 << 30, NULL) == -2        # addend misaligned
    assert wgrad(P16, 40, P16, 0, P16, 0, 1, 256, 80, 80, P16, P16, P16, 1 << 30, NULL) == -1      # grad_out stride < out_features
    assert wgrad(P16, 0, P16, 82, NULL, 0, 0, 256, 80, 80, P16, P16, P16, 1 << 30, NULL) == -2     # x stride % 4
    assert wgrad(P8, 0, P16, 0, NULL, 0, 0, 256, 80, 80, P16, P16, P16, 1 << 30, NULL) == -2       # grad_out misaligned
    assert wgrad(P16, 40, P16, 0, P16, 82, 1, 256, 80, 80, P16, P16, P16, 1 << 30, NULL) == -1     # short grad_out rows before the addend
    assert wgrad(P16, 82, P16, 0, P16, 40, 1, 256, 80, 80, P16, P16, P16, 1 << 30, NULL) == -1     # short addend rows before grad_out % 4
    assert wgrad(P16, 0, P16, 0, P8, 0, 1, 256, 80, 80, P16, P16, NULL, 0, NULL) == -2             # addend before the workspace (-3)
    assert wgrad(P16, 0, P8, 0, NULL, 0, 0, 256, 80, 80, P16, P16, NULL, 0, NULL) == -2            # x before the workspace


# ---- the depth-aware cross-attention family: one table per entry, recorded on the launchers before they shared an argument record
DA_NULL = ctypes.c_void_p(0)
DA_P16, DA_P8, DA_P4 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008), ctypes.c_void_p(0x1004)   # 16-byte aligned / 8 / 4
DA_GEOMETRY = ['spatial_shapes', 'level_start_index', 'pred_depth', 'ref_cam', 'mask', 'qdepth']
DA_DIMS = ['B', 'Ncam', 'S', 'M', 'Dh', 'L', 'Q', 'P', 'Za', 'DC']
DA_FWD = ['value'] + DA_GEOMETRY + ['offsets', 'attn'] + DA_DIMS + ['d0', 'dstep', 'head_minor']
DA_BWD = (['value'] + DA_GEOMETRY + ['offsets', 'attn', 'grad_slots'] + DA_DIMS + ['d0', 'dstep', 'head_minor', 'head_stride'] +
          ['grad_value', 'grad_pred_depth', 'grad_offsets', 'grad_attn'])
DA_FUSED = (DA_GEOMETRY + ['query', 'query_row_stride', 'addend', 'addend_row_stride', 'addend_period', 'offsets_fragments',
                           'offsets_bias', 'attn_fragments', 'attn_bias'])
DA_FUSED_TAIL = DA_DIMS + ['d0', 'dstep', 'bev_w', 'min_level_width', 'slots', 'stream']
DA_LN = ['out_fragments', 'out_bias', 'residual', 'residual_row_stride', 'ln_weight', 'ln_bias', 'ln_eps']
DA_PARAMS = {
    'fwd': DA_FWD + ['head_stride', 'slots', 'stream'],
    'fwd_e': DA_FWD + ['head_stride', 'elem_type', 'slots', 'stream'],
    'fwd_zt': DA_FWD + ['head_stride', 'bev_w', 'slots', 'stream'],
    'fwd_planes': DA_FWD + ['bev_w', 'min_level_width', 'slots', 'stream'],
    'fused': ['value'] + DA_FUSED + DA_FUSED_TAIL,
    'fused_e': ['value', 'elem_type'] + DA_FUSED + DA_FUSED_TAIL,
    'fused_ln': ['value'] + DA_FUSED + DA_LN + DA_FUSED_TAIL,
    'bwd': DA_BWD + ['stream'],
    'bwd_ex': DA_BWD + ['H0', 'W0', 'flags', 'det_ws', 'det_ws_bytes', 'stream'],
    'bwd_ws': DA_BWD + ['level_hw', 'ws', 'ws_bytes', 'stream'],
    'bwd_ws_grid': DA_BWD + ['level_hw', 'ws', 'ws_bytes', 'bev_w', 'stream'],
    'bwd_ws_grid_ex': DA_BWD + ['level_hw', 'ws', 'ws_bytes', 'bev_w', 'flags', 'det_ws', 'det_ws_bytes', 'stream'],
    'bwd_planes': DA_BWD + ['level_hw', 'ws', 'ws_bytes', 'bev_w', 'stream'],
    'bwd_planes_ex': DA_BWD + ['level_hw', 'ws', 'ws_bytes', 'bev_w', 'flags', 'det_ws', 'det_ws_bytes', 'stream'],
}
# a call that would LAUNCH (so no row below is this alone): one sample, 6 cameras, one 22 x 32 level, 8 heads of 10 channels,
# 100 queries on a 10-wide grid, 8 points on 4 anchors, 80 depth bins; every pointer non-null and 16-byte aligned
DA_BASE = dict(B=1, Ncam=6, S=704, M=8, Dh=10, L=1, Q=100, P=8, Za=4, DC=80, d0=2.0, dstep=0.5, head_minor=0, head_stride=0,
               elem_type=1, bev_w=10, min_level_width=2, query_row_stride=0, addend=DA_NULL, addend_row_stride=0, addend_period=0,
               residual=DA_NULL, residual_row_stride=0, ln_eps=1e-5, H0=22, W0=32, flags=1, det_ws_bytes=1 << 40, level_hw=DA_NULL,
               ws_bytes=1 << 40, stream=DA_NULL)
DA_INTS = set(DA_DIMS) | {'head_minor', 'head_stride', 'elem_type', 'bev_w', 'min_level_width', 'query_row_stride',
                          'addend_row_stride', 'addend_period', 'residual_row_stride', 'H0', 'W0', 'flags', 'det_ws_bytes', 'ws_bytes'}


def da_call(lib, entry, case):
    """`entry` with DA_BASE's operands, `case` on top of them; 'null': every pointer the entry takes is null unless `case` names it"""
    case = dict(case)
    null = case.pop('null', False)
    args = []
    for name in DA_PARAMS[entry]:
        if name in case:
            args.append(case.pop(name))
        elif name in DA_BASE and (name in DA_INTS or name in ('d0', 'dstep', 'ln_eps') or not null):
            args.append(DA_BASE[name])
        else:
            args.append(DA_NULL if null else DA_P16)
    assert not case, (entry, 'operands the entry does not take', case)
    return getattr(lib, 'fbbev_da_cross_attn_' + entry)(*args)


def test_da_cross_attn_entries_keep_their_error_codes_and_plan_sizes():
    """Every entry of the depth-aware cross-attention family: the code of each argument check, and which code wins where two
    defects coincide (the order of an entry's checks is part of the ABI).  Every row returns BEFORE any runtime call, so this
    runs without a GPU.  Below the table, the pure host functions (probes, workspace sizes) as the numbers they returned when
    the table was recorded."""
    lib = _capi.declare(ctypes.CDLL(_capi.LIB_PATH))
    NULL, P16, P8, P4 = DA_NULL, DA_P16, DA_P8, DA_P4
    LOGITS = 0x10                                                    # FBBEV_DA_ATTN_LOGITS
    hw_22x32 = (ctypes.c_int32 * 2)(22, 32)
    hw_2x2 = (ctypes.c_int32 * 2)(2, 2)
    hw_bad = (ctypes.c_int32 * 2)(0, 32)
    small_det = dict(level_hw=hw_22x32, det_ws_bytes=16)
    # the smallest shape fbbev_da_cross_attn_bwd_planes_supported takes with the knobs unset: 256 (sample, camera, head) planes of
    # one 2 x 2 level, rows padded to 12 floats
    planes_ok = dict(B=4, Ncam=8, S=4, Q=64, bev_w=8, head_stride=12, level_hw=hw_2x2)
    assert lib.fbbev_da_cross_attn_bwd_planes_supported(4, 8, 4, 8, 10, 1, 64, 8, 4, 12, hw_2x2, 8) == 1
    assert lib.fbbev_da_cross_attn_bwd_planes_supported(4, 7, 4, 8, 10, 1, 64, 8, 4, 12, hw_2x2, 8) == 0      # 224 planes
    table = [
        # ---- fbbev_da_cross_attn_fwd: dimensions, Za / P % Za (-2), dstep (-1), empty (0), null pointers, row layout
        ('fwd', dict(B=0), -1),
        ('fwd', dict(DC=0), -1),
        ('fwd', dict(Q=-1), -1),
        ('fwd', dict(Q=0, null=True), 0),
        ('fwd', dict(slots=NULL), -1),
        ('fwd', dict(value=NULL), -1),
        ('fwd', dict(Za=16), -2),
        ('fwd', dict(P=6), -2),
        ('fwd', dict(dstep=0.0), -1),
        ('fwd', dict(Za=16, dstep=0.0), -2),
        ('fwd', dict(Za=16, B=0), -1),
        ('fwd', dict(Za=16, Q=0, null=True), -2),
        ('fwd', dict(Q=0, dstep=0.0, null=True), -1),
        ('fwd', dict(Za=16, mask=NULL), -2),
        ('fwd', dict(head_stride=8), -1),
        ('fwd', dict(head_stride=8, attn=NULL), -1),
        ('fwd', dict(head_minor=4, head_stride=10), -2),
        ('fwd', dict(head_minor=4, head_stride=8), -1),
        ('fwd', dict(head_minor=4, head_stride=12, value=P8), -2),
        ('fwd', dict(head_minor=4, head_stride=12, B=3000), -2),                   # chunk-major rows past 32-bit byte offsets
        # ---- fbbev_da_cross_attn_fwd_e: the element type first, then fwd's order; 16-bit rows are chunk-major pieces of 8
        ('fwd_e', dict(elem_type=3), -1),
        ('fwd_e', dict(elem_type=-1, Za=16), -1),
        ('fwd_e', dict(elem_type=0, Za=16), -2),
        ('fwd_e', dict(elem_type=0, head_stride=8), -1),
        ('fwd_e', dict(elem_type=0, Q=0, null=True), 0),
        ('fwd_e', dict(B=0), -1),
        ('fwd_e', dict(Q=0, null=True), 0),
        ('fwd_e', dict(elem_type=2, Q=0, null=True), 0),
        ('fwd_e', dict(attn=NULL), -1),
        ('fwd_e', dict(Za=16), -2),
        ('fwd_e', dict(dstep=0.0), -1),
        ('fwd_e', dict(Za=16, dstep=0.0), -2),
        ('fwd_e', dict(Q=0, dstep=0.0, null=True), -1),
        ('fwd_e', dict(head_minor=0, head_stride=16), -2),
        ('fwd_e', dict(head_minor=0, head_stride=16, slots=NULL), -1),
        ('fwd_e', dict(head_minor=4, head_stride=16, Dh=12), -2),
        ('fwd_e', dict(head_minor=4, head_stride=8), -2),                          # a row of 8 does not hold Dh = 10
        ('fwd_e', dict(head_minor=4, head_stride=0, Dh=8), -2),                    # 16-bit rows: 0 is no stride (not "dense")
        ('fwd_e', dict(head_minor=4, head_stride=16, slots=P4), -2),
        ('fwd_e', dict(head_minor=4, head_stride=16, value=P8), -2),
        # ---- fbbev_da_cross_attn_fwd_zt: its own dimensions (with bev_w), then the pipelined kernel or fwd's checks
        ('fwd_zt', dict(bev_w=-1), -1),
        ('fwd_zt', dict(B=0), -1),
        ('fwd_zt', dict(Q=0, null=True), 0),
        ('fwd_zt', dict(head_minor=LOGITS), -2),
        ('fwd_zt', dict(head_minor=LOGITS | 5, head_stride=12, Za=2), -2),         # the pipelined kernel takes 4 anchors
        ('fwd_zt', dict(head_minor=LOGITS, B=0), -1),
        ('fwd_zt', dict(head_minor=LOGITS, dstep=0.0), -2),
        ('fwd_zt', dict(head_minor=LOGITS, slots=NULL), -2),
        ('fwd_zt', dict(Za=16), -2),
        ('fwd_zt', dict(dstep=0.0), -1),
        ('fwd_zt', dict(Za=16, dstep=0.0), -2),
        ('fwd_zt', dict(slots=NULL), -1),
        ('fwd_zt', dict(head_stride=8), -1),
        ('fwd_zt', dict(head_minor=5, head_stride=12, spatial_shapes=NULL), -1),   # a shape the pipelined kernel takes
        ('fwd_zt', dict(head_minor=5, head_stride=12, qdepth=NULL), -1),
        # ---- fbbev_da_cross_attn_fwd_planes: dimensions, empty (0) BEFORE dstep, null pointers / dstep, shape and alignment
        ('fwd_planes', dict(B=0), -1),
        ('fwd_planes', dict(bev_w=-1), -1),
        ('fwd_planes', dict(Q=0, null=True), 0),
        ('fwd_planes', dict(Q=0, dstep=0.0, null=True), 0),
        ('fwd_planes', dict(dstep=0.0), -1),
        ('fwd_planes', dict(value=NULL), -1),
        ('fwd_planes', dict(value=NULL, M=4), -1),
        ('fwd_planes', dict(M=4), -2),
        ('fwd_planes', dict(M=4, dstep=0.0), -1),
        ('fwd_planes', dict(Za=8), -2),
        ('fwd_planes', dict(min_level_width=1), -2),
        ('fwd_planes', dict(offsets=P4), -2),
        ('fwd_planes', dict(slots=P4), -2),
        ('fwd_planes', dict(ref_cam=P8), -2),
        ('fwd_planes', dict(mask=ctypes.c_void_p(0x1002)), -2),
        # ---- fbbev_da_cross_attn_fused / _e / _ln
        ('fused', dict(B=0), -1),
        ('fused', dict(bev_w=-1), -1),
        ('fused', dict(Q=0, null=True), 0),
        ('fused', dict(Q=0, dstep=0.0, null=True), 0),
        ('fused', dict(query=NULL), -1),
        ('fused', dict(value=NULL), -1),
        ('fused', dict(dstep=0.0), -1),
        ('fused', dict(query_row_stride=40), -1),
        ('fused', dict(query_row_stride=82), -2),
        ('fused', dict(addend=P16, addend_period=0), -1),
        ('fused', dict(addend=P16, addend_period=1, addend_row_stride=40), -1),
        ('fused', dict(addend=P16, addend_period=1, addend_row_stride=82), -2),
        ('fused', dict(addend=P8, addend_period=1), -2),
        ('fused', dict(min_level_width=1), -2),
        ('fused', dict(M=4), -2),
        ('fused', dict(bev_w=0), -2),
        ('fused', dict(bev_w=7), -2),
        ('fused', dict(Ncam=33), -2),
        ('fused', dict(value=P4), -2),
        ('fused', dict(slots=P4), -2),
        ('fused', dict(M=4, query_row_stride=20), -1),
        ('fused', dict(min_level_width=1, addend=P16, addend_period=0), -1),
        ('fused', dict(M=4, query=NULL), -1),
        ('fused_e', dict(elem_type=3), -1),
        ('fused_e', dict(elem_type=3, Q=0, null=True), -1),
        ('fused_e', dict(elem_type=0, M=4), -2),
        ('fused_e', dict(Q=0, null=True), 0),
        ('fused_e', dict(query_row_stride=40), -1),
        ('fused_e', dict(query_row_stride=82), -2),
        ('fused_e', dict(elem_type=2, addend=P16, addend_period=0), -1),
        ('fused_e', dict(elem_type=2, min_level_width=1), -2),
        # (_ln: the tail's own checks come first)
        ('fused_ln', dict(out_bias=NULL), -1),
        ('fused_ln', dict(ln_eps=-1.0), -1),
        ('fused_ln', dict(M=0, out_fragments=P8), -1),
        ('fused_ln', dict(residual=P8, B=0), -2),
        ('fused_ln', dict(residual=P16, residual_row_stride=40), -1),
        ('fused_ln', dict(residual=P16, residual_row_stride=82), -2),
        ('fused_ln', dict(residual=P16, residual_row_stride=40, ln_bias=P8), -1),
        ('fused_ln', dict(Dh=9), -2),                                              # E % 16
        ('fused_ln', dict(slots=P8), -2),
        ('fused_ln', dict(slots=P8, out_bias=NULL), -1),
        ('fused_ln', dict(B=0), -1),
        ('fused_ln', dict(query=NULL), -1),
        ('fused_ln', dict(query_row_stride=40), -1),
        ('fused_ln', dict(query_row_stride=82), -2),
        ('fused_ln', dict(addend=P16, addend_period=0), -1),
        ('fused_ln', dict(min_level_width=1), -2),
        # ---- fbbev_da_cross_attn_bwd: fwd's order, then Dh > 32 (-2), the row stride (-1), chunk-major rows (-2)
        ('bwd', dict(B=0), -1),
        ('bwd', dict(Q=0, null=True), 0),
        ('bwd', dict(grad_attn=NULL), -1),
        ('bwd', dict(grad_slots=NULL), -1),
        ('bwd', dict(Za=16), -2),
        ('bwd', dict(P=6), -2),
        ('bwd', dict(dstep=0.0), -1),
        ('bwd', dict(Za=16, dstep=0.0), -2),
        ('bwd', dict(Q=0, dstep=0.0, null=True), -1),
        ('bwd', dict(Za=16, grad_value=NULL), -2),
        ('bwd', dict(Dh=40), -2),
        ('bwd', dict(Dh=40, grad_attn=NULL), -1),
        ('bwd', dict(head_stride=8), -1),
        ('bwd', dict(Dh=40, head_stride=8), -2),
        ('bwd', dict(head_minor=4, head_stride=10), -2),
        ('bwd', dict(head_minor=4, head_stride=8), -1),
        ('bwd', dict(B=1 << 15, Q=1 << 16), -2),                                   # more workgroups than a grid holds
        # ---- fbbev_da_cross_attn_bwd_ex: without the flag it is bwd; with it H0 / W0 join the dimensions, det_ws the pointers
        ('bwd_ex', dict(flags=0, Za=16), -2),
        ('bwd_ex', dict(flags=0, H0=0, Dh=40), -2),
        ('bwd_ex', dict(flags=0, det_ws=NULL, grad_attn=NULL), -1),
        ('bwd_ex', dict(flags=0, Q=0, null=True), 0),
        ('bwd_ex', dict(H0=0), -1),
        ('bwd_ex', dict(W0=0, Za=16), -1),
        ('bwd_ex', dict(B=0), -1),
        ('bwd_ex', dict(Za=16), -2),
        ('bwd_ex', dict(dstep=0.0), -1),
        ('bwd_ex', dict(Za=16, dstep=0.0), -2),
        ('bwd_ex', dict(Q=0, null=True), 0),
        ('bwd_ex', dict(det_ws=NULL), -1),
        ('bwd_ex', dict(grad_offsets=NULL), -1),
        ('bwd_ex', dict(Dh=40), -2),
        ('bwd_ex', dict(Dh=40, det_ws=NULL), -1),
        ('bwd_ex', dict(head_stride=8), -1),
        ('bwd_ex', dict(head_minor=4, head_stride=10), -2),
        ('bwd_ex', dict(det_ws_bytes=16), -3),
        ('bwd_ex', dict(det_ws=P8), -3),                                           # enough bytes, 8-byte aligned only
        ('bwd_ex', dict(head_minor=4, head_stride=10, det_ws_bytes=16), -2),
        ('bwd_ex', dict(head_stride=8, det_ws_bytes=16), -1),
        # ---- fbbev_da_cross_attn_bwd_ws / _ws_grid without a workspace (or with one too small for either plan): bwd's checks
        ('bwd_ws', dict(ws=NULL, B=0), -1),
        ('bwd_ws', dict(ws=NULL, Q=0, null=True), 0),
        ('bwd_ws', dict(ws=NULL, Za=16), -2),
        ('bwd_ws', dict(ws=NULL, dstep=0.0), -1),
        ('bwd_ws', dict(ws=NULL, Za=16, dstep=0.0), -2),
        ('bwd_ws', dict(ws=NULL, grad_attn=NULL), -1),
        ('bwd_ws', dict(ws=NULL, Dh=40), -2),
        ('bwd_ws', dict(ws=NULL, head_stride=8), -1),
        ('bwd_ws', dict(ws_bytes=16, dstep=0.0), -1),
        ('bwd_ws', dict(ws_bytes=16, Za=16, level_hw=hw_22x32), -2),
        ('bwd_ws', dict(ws=P8, Dh=40), -2),
        ('bwd_ws_grid', dict(ws=NULL, bev_w=-1), -1),
        ('bwd_ws_grid', dict(ws=NULL, bev_w=-1, Za=16), -1),
        ('bwd_ws_grid', dict(ws=NULL, B=0), -1),
        ('bwd_ws_grid', dict(ws=NULL, Q=0, null=True), 0),
        ('bwd_ws_grid', dict(ws=NULL, Za=16), -2),
        ('bwd_ws_grid', dict(ws=NULL, dstep=0.0), -1),
        ('bwd_ws_grid', dict(ws=NULL, value=NULL), -1),
        ('bwd_ws_grid', dict(ws_bytes=16, level_hw=hw_22x32, dstep=0.0), -1),
        # ---- _bwd_ws_grid_ex / _bwd_planes_ex: without the flag the plain entry; with it the deterministic wrapper's checks first
        # (no row passes them: the next thing it does is a runtime memset)
        ('bwd_ws_grid_ex', dict(flags=0, ws=NULL, Za=16), -2),
        ('bwd_ws_grid_ex', dict(flags=0, ws=NULL, bev_w=-1), -1),
        ('bwd_ws_grid_ex', dict(flags=0, ws=NULL, dstep=0.0, det_ws=NULL), -1),
        ('bwd_ws_grid_ex', dict(flags=0, ws=NULL, Q=0, null=True), 0),
        ('bwd_ws_grid_ex', dict(), -1),                                            # level_hw_host is required
        ('bwd_ws_grid_ex', dict(M=3), -1),
        ('bwd_ws_grid_ex', dict(level_hw=hw_22x32, M=3), -2),
        ('bwd_ws_grid_ex', dict(level_hw=hw_22x32, M=128), -2),
        ('bwd_ws_grid_ex', dict(level_hw=hw_22x32, det_ws=NULL), -1),
        ('bwd_ws_grid_ex', dict(level_hw=hw_22x32, grad_pred_depth=NULL), -1),
        ('bwd_ws_grid_ex', dict(level_hw=hw_22x32, B=0), -1),
        ('bwd_ws_grid_ex', dict(level_hw=hw_22x32, Q=0), -1),                      # (no empty case on this route)
        ('bwd_ws_grid_ex', dict(level_hw=hw_22x32, dstep=0.0, M=3), -1),
        ('bwd_ws_grid_ex', dict(level_hw=hw_bad), -1),
        ('bwd_ws_grid_ex', dict(level_hw=hw_bad, M=3), -2),
        ('bwd_ws_grid_ex', small_det, -3),
        ('bwd_ws_grid_ex', dict(small_det, M=3), -2),
        ('bwd_ws_grid_ex', dict(level_hw=hw_22x32, det_ws=P8), -3),
        ('bwd_planes_ex', dict(flags=0, ws=NULL), -1),
        ('bwd_planes_ex', dict(flags=0, Za=8), -2),
        ('bwd_planes_ex', dict(flags=0, bev_w=0), -1),
        ('bwd_planes_ex', dict(flags=0, ws_bytes=16, **planes_ok), -3),
        ('bwd_planes_ex', dict(), -1),
        ('bwd_planes_ex', dict(level_hw=hw_22x32, M=3), -2),
        ('bwd_planes_ex', dict(level_hw=hw_22x32, qdepth=NULL), -1),
        ('bwd_planes_ex', dict(level_hw=hw_22x32, Q=0), -1),
        ('bwd_planes_ex', small_det, -3),
        ('bwd_planes_ex', dict(small_det, M=3), -2),
        ('bwd_planes_ex', dict(level_hw=hw_22x32, det_ws=P8), -3),
        # ---- fbbev_da_cross_attn_bwd_planes: dimensions (Q and bev_w positive), pointers, dstep, the route's shape (-2),
        # alignment (-2), workspace (-3)
        ('bwd_planes', dict(level_hw=hw_22x32, bev_w=0), -1),
        ('bwd_planes', dict(level_hw=hw_22x32, Q=0, null=True), -1),
        ('bwd_planes', dict(level_hw=hw_22x32, ws=NULL), -1),
        ('bwd_planes', dict(level_hw=hw_22x32, value=NULL), -1),
        ('bwd_planes', dict(level_hw=hw_22x32, dstep=0.0), -1),
        ('bwd_planes', dict(level_hw=hw_22x32, Za=8), -2),
        ('bwd_planes', dict(level_hw=hw_22x32, Za=8, dstep=0.0), -1),
        ('bwd_planes', dict(level_hw=hw_22x32, Za=8, ws=NULL), -1),
        ('bwd_planes', dict(level_hw=hw_22x32, head_stride=8), -2),                # (a short row stride is -2 on this route)
        ('bwd_planes', dict(level_hw=hw_22x32, bev_w=7), -2),
        ('bwd_planes', dict(head_stride=12), -2),                                  # no host level shapes: no head-plane route
        ('bwd_planes', dict(ws_bytes=16, **planes_ok), -3),
        ('bwd_planes', dict(grad_value=P8, **planes_ok), -2),
        ('bwd_planes', dict(grad_value=P8, ws_bytes=16, **planes_ok), -2),
        ('bwd_planes', dict(grad_slots=P4, **planes_ok), -2),
        ('bwd_planes', dict(ws=P8, **planes_ok), -2),
    ]
    got = [(entry, {k: (v.value if isinstance(v, ctypes.c_void_p) else v) for k, v in case.items() if k != 'level_hw'},
            da_call(lib, entry, case)) for entry, case, _ in table]
    want = [(entry, {k: (v.value if isinstance(v, ctypes.c_void_p) else v) for k, v in case.items() if k != 'level_hw'}, code)
            for entry, case, code in table]
    assert got == want, [(g, w[2]) for g, w in zip(got, want) if g != w]
    # ---- the pure host functions: every one goes through a plan or a shape check of this family
    pyramid = (ctypes.c_int32 * 8)(16, 44, 32, 88, 8, 22, 4, 11)
    shapes = {
        # BASELINE configs[2]: 4 samples, 6 cameras, the 4-level pyramid, 8 heads of 10 channels in rows of 12, 200 x 200 queries
        'configs2': dict(B=4, Ncam=6, S=3740, M=8, Dh=10, L=4, Q=40000, P=8, Za=4, DC=59, HS=12, bev_w=200, hw=pyramid, H0=16, W0=44),
        'one 2 x 2 level': dict(B=1, Ncam=2, S=4, M=8, Dh=10, L=1, Q=16, P=8, Za=4, DC=8, HS=12, bev_w=4, hw=hw_2x2, H0=2, W0=2),
        'one level, no host shapes': dict(B=2, Ncam=6, S=704, M=8, Dh=8, L=1, Q=2500, P=8, Za=4, DC=59, HS=0, bev_w=50, hw=NULL,
                                          H0=22, W0=32),
        '33 cameras': dict(B=4, Ncam=33, S=3740, M=8, Dh=10, L=4, Q=40000, P=8, Za=4, DC=59, HS=12, bev_w=200, hw=pyramid, H0=16, W0=44),
        '4 heads': dict(B=4, Ncam=6, S=3740, M=4, Dh=10, L=4, Q=40000, P=8, Za=4, DC=59, HS=12, bev_w=200, hw=pyramid, H0=16, W0=44),
        '2 anchors': dict(B=4, Ncam=6, S=3740, M=8, Dh=10, L=4, Q=40000, P=8, Za=2, DC=59, HS=12, bev_w=200, hw=pyramid, H0=16, W0=44),
        'no samples': dict(B=0, Ncam=6, S=3740, M=8, Dh=10, L=4, Q=40000, P=8, Za=4, DC=59, HS=12, bev_w=200, hw=pyramid, H0=16, W0=44),
        'no queries': dict(B=4, Ncam=6, S=3740, M=8, Dh=10, L=4, Q=0, P=8, Za=4, DC=59, HS=12, bev_w=200, hw=pyramid, H0=16, W0=44),
        'rows shorter than a head': dict(B=4, Ncam=6, S=3740, M=8, Dh=10, L=4, Q=40000, P=8, Za=4, DC=59, HS=8, bev_w=200, hw=pyramid,
                                         H0=16, W0=44),
        'queries off the grid': dict(B=4, Ncam=6, S=3740, M=8, Dh=10, L=4, Q=40000, P=8, Za=4, DC=59, HS=12, bev_w=199, hw=pyramid,
                                     H0=16, W0=44),
    }
    functions = {
        'bwd_ws_bytes': ('B', 'Ncam', 'S', 'M', 'Dh', 'Q', 'HS', 'L', 'P', 'hw'),
        'bwd_ws_bytes_za': ('B', 'Ncam', 'S', 'M', 'Dh', 'Q', 'HS', 'L', 'P', 'Za', 'hw'),
        'bwd_det_ws_bytes': ('B', 'Ncam', 'S', 'M', 'HS', 'Q', 'Za', 'DC', 'H0', 'W0'),
        'fused_supported': ('B', 'Ncam', 'S', 'M', 'Dh', 'L', 'Q', 'P', 'Za', 'bev_w'),
        'fwd_planes_supported': ('B', 'Ncam', 'S', 'M', 'Dh', 'L', 'Q', 'P', 'Za'),
        'bwd_planes_supported': ('B', 'Ncam', 'S', 'M', 'Dh', 'L', 'Q', 'P', 'Za', 'HS', 'hw', 'bev_w'),
        'fwd_zt_fuses_softmax': ('B', 'Ncam', 'S', 'M', 'Dh', 'L', 'Q', 'P', 'Za', 'head_minor', 'HS'),
    }
    # columns: the seven functions above in order, then fbbev_da_bwd_det_ws_bytes and fbbev_da_depth_taps_det_ws_bytes
    recorded = {
        'configs2': (582205440, 90163712, 215151104, 1, 1, 1, 1, 23335168, 7975168),
        'one 2 x 2 level': (3072, 3072, 11776, 1, 1, 0, 1, 1280, 768),
        'one level, no host shapes': (21626880, 21626880, 0, 1, 1, 0, 1, 4467712, 3987712),
        '33 cameras': (3202129920, 337921024, 1183328768, 0, 1, 0, 1, 128342272, 43862272),
        '4 heads': (496035840, 61440512, 119243264, 0, 0, 0, 1, 23335168, 7975168),
        '2 anchors': (582205440, 90163712, 146031104, 0, 0, 0, 0, 15655168, 7975168),
        'no samples': (0, 0, 0, 0, 0, 0, 0, 0, 0),
        'no queries': (0, 0, 76911104, 0, 0, 0, 0, 0, 7975168),
        'rows shorter than a head': (0, 0, 192172544, 1, 1, 0, 0, 23335168, 7975168),
        'queries off the grid': (582205440, 90163712, 215151104, 0, 1, 0, 1, 23335168, 7975168),
    }
    for name, s in shapes.items():
        s = dict(s, head_minor=5)
        row = tuple(getattr(lib, 'fbbev_da_cross_attn_' + f)(*(s[k] for k in keys)) for f, keys in functions.items())
        row += (lib.fbbev_da_bwd_det_ws_bytes(*(s[k] for k in ('B', 'Ncam', 'Q', 'Za', 'DC', 'H0', 'W0'))),
                lib.fbbev_da_depth_taps_det_ws_bytes(*(s[k] for k in ('B', 'Ncam', 'DC', 'H0', 'W0'))))
        assert row == recorded[name], (name, row)
    # the pipelined forward takes head-minor offsets on chunk-major rows only
    s = shapes['configs2']
    assert lib.fbbev_da_cross_attn_fwd_zt_fuses_softmax(*(s[k] for k in functions['fwd_zt_fuses_softmax'][:9]), 1, 12) == 0
    assert lib.fbbev_da_cross_attn_fwd_zt_fuses_softmax(*(s[k] for k in functions['fwd_zt_fuses_softmax'][:9]), 5, 0) == 0


# ---- the temporal-history family (and the three LayerNorm entries that share its region): one table per entry, recorded on the
# launchers before they shared a ring record
H_RING = ['history', 'history_stride_b', 'rt_flow', 'B']
H_CONV = ['feats', 'feats_stride_b', 'w1', 'bias1', 'w2', 'bias2', 'B', 'T1', 'C', 'Cout', 'N', 'out', 'workspace', 'workspace_bytes']
H_STEP = ['history', 'history_stride_b', 'next', 'next_stride_b', 'rt_flow', 'w1', 'bias1', 'w2', 'bias2', 'B', 'T', 'C', 'Cout',
          'Z', 'Y', 'X', 'out', 'workspace', 'workspace_bytes', 'elem_type']
H_PARAMS = {
    'history_flow': ['history_forward_augs', 'curr_to_prev_ego_rt', 'bda', 'dx3', 'lower3', 'B', 'rt_flow', 'stream'],
    'history_stream_prologue': ['flags', 'curr_to_prev_ego_rt', 'bda', 'b1', 'wt', 'dx3', 'lower3', 'freq', 'B', 'T', 'C',
                                'history_forward_augs', 'sweep_time', 'flow_augs', 'rt_flow', 'bias1', 'stream'],
    'history_warp': H_RING + ['CH', 'Z', 'Y', 'X', 'out', 'out_stride_b', 'stream'],
    'history_warp_e': H_RING + ['CH', 'Z', 'Y', 'X', 'out', 'out_stride_b', 'elem_type', 'stream'],
    'history_warp_vm': H_RING + ['T', 'C', 'Z', 'Y', 'X', 'out', 'out_stride_b', 'elem_type', 'stream'],
    'history_warp_vm_src': ['history', 'history_stride_b', 'curr', 'curr_stride_b', 'flags', 'rt_flow', 'B', 'T', 'C', 'Z', 'Y', 'X',
                            'out', 'out_stride_b', 'elem_type', 'stream'],
    'history_frame_vm': ['curr', 'B', 'C', 'N', 'inner', 'out', 'out_stride_b', 'elem_type', 'stream'],
    'history_conv': H_CONV + ['stream'],
    'history_conv_e': H_CONV + ['elem_type', 'stream'],
    'history_conv_vm': H_CONV + ['elem_type', 'stream'],
    'history_conv_bf16': H_CONV + ['voxel_major', 'elem_type', 'stream'],
    'history_conv_bf16x3': H_CONV + ['elem_type', 'stream'],
    'history_fused_x3_vm': H_STEP + ['stream'],
    'history_step_x3_vm': H_STEP + ['chunks', 'stream'],
    'history_fused_vm': H_STEP + ['stream'],
    'layernorm': ['x', 'residual', 'weight', 'bias', 'eps', 'rows', 'C', 'out', 'stream'],
    'layernorm_bwd': ['x', 'grad_out', 'weight', 'eps', 'rows', 'C', 'grad_x', 'partial', 'stream'],
}
# a call that would LAUNCH (so no row below is this alone): one sample, a bf16 ring of 16 frames (17 with the current one) of 80
# channels on an 8 x 8 x 8 grid, dense strides, a workspace of any size; every pointer non-null and 16-byte aligned
H_BASE = dict(B=1, T=16, T1=17, C=80, Cout=80, CH=80, Z=8, Y=8, X=8, N=512, inner=1, elem_type=1, voxel_major=1, chunks=0,
              history_stride_b=0, next_stride_b=0, out_stride_b=0, curr_stride_b=0, feats_stride_b=0, workspace_bytes=1 << 40,
              freq=0.5, eps=1e-5, rows=256, stream=DA_NULL)
H_FRAME = 512 * 80                                                   # elements of a frame of H_BASE
# grids at the limits of the 32-bit offsets (no pointer is dereferenced in these rows, so the sizes are free)
H_2G_VOXELS = dict(Z=2048, Y=1024, X=1024)                           # 2^31 voxels
H_BELOW_2G = dict(Z=2047, Y=1024, X=1024)
H_C80_AT_4G = dict(Z=2, Y=2, X=6710887)                              # 16-bit frames of 80 channels: 2^32 bytes lie between these two
H_C80_BELOW_4G = dict(Z=2, Y=2, X=6710886)
H_C8_AT_4G = dict(C=8, Z=16, Y=4096, X=4096)                         # 16-bit frames of 8 channels: exactly 2^32 bytes
H_C8_BELOW_4G = dict(C=8, Z=16, Y=4096, X=4095)
H_C8_F32_AT_4G = dict(C=8, elem_type=0, Z=8, Y=4096, X=4096)         # fp32 frames of 8 channels: exactly 2^32 bytes
H_C8_F32_BELOW_4G = dict(C=8, elem_type=0, Z=8, Y=4096, X=4095)


def h_call(lib, entry, case):
    """`entry` with H_BASE's operands, `case` on top of them; 'null': every pointer the entry takes is null unless `case` names it"""
    case = dict(case)
    null = case.pop('null', False)
    args = []
    for name in H_PARAMS[entry]:
        if name in case:
            args.append(case.pop(name))
        elif name in H_BASE:
            args.append(H_BASE[name])
        else:
            args.append(DA_NULL if null else DA_P16)
    assert not case, (entry, 'operands the entry does not take', case)
    return getattr(lib, 'fbbev_' + entry)(*args)


def test_history_entries_keep_their_error_codes():
    """Every entry of the temporal-history family: the code of each argument check, and which code wins where two defects
    coincide (the order of an entry's checks is part of the ABI).  Every row returns BEFORE any runtime call, so this runs
    without a GPU.  Checks behind a launch (the workgroup counts of the x3 convolutions' segments and of the one-kernel steps)
    are not here."""
    lib = _capi.declare(ctypes.CDLL(_capi.LIB_PATH))
    NULL, P16, P8 = DA_NULL, DA_P16, DA_P8
    F = H_FRAME
    dx3 = (ctypes.c_float * 3)(0.4, 0.4, 0.4)                       # flow / stream_prologue read dx3 on the host
    dx3_zero = (ctypes.c_float * 3)(0.4, 0.0, 0.4)
    dx3_nan = (ctypes.c_float * 3)(0.4, 0.4, float('nan'))
    many_wgs = dict(B=1 << 26, N=2048)                               # 2^31 workgroups of 64 voxels
    table = [
        # ---- fbbev_history_flow: B, empty (0), pointers, voxel sizes
        ('history_flow', dict(dx3=dx3, B=-1), -1),
        ('history_flow', dict(B=0, null=True), 0),
        ('history_flow', dict(B=-1, null=True), -1),
        ('history_flow', dict(dx3=dx3, rt_flow=NULL), -1),
        ('history_flow', dict(dx3=dx3, bda=NULL), -1),
        ('history_flow', dict(dx3=dx3, lower3=NULL), -1),
        ('history_flow', dict(dx3=NULL), -1),
        ('history_flow', dict(dx3=dx3_zero), -1),
        ('history_flow', dict(dx3=dx3_nan), -1),
        ('history_flow', dict(dx3=dx3_zero, B=0), 0),
        # ---- fbbev_history_stream_prologue: dimensions, empty (0), pointers (sweep_time only with frames), voxel sizes, T > 8192 (-2)
        ('history_stream_prologue', dict(dx3=dx3, B=-1), -1),
        ('history_stream_prologue', dict(dx3=dx3, T=-1), -1),
        ('history_stream_prologue', dict(dx3=dx3, C=0), -1),
        ('history_stream_prologue', dict(B=0, null=True), 0),
        ('history_stream_prologue', dict(B=0, C=0, null=True), -1),
        ('history_stream_prologue', dict(dx3=dx3, flags=NULL), -1),
        ('history_stream_prologue', dict(dx3=dx3, bias1=NULL), -1),
        ('history_stream_prologue', dict(dx3=dx3, wt=NULL), -1),
        ('history_stream_prologue', dict(dx3=dx3, sweep_time=NULL), -1),
        ('history_stream_prologue', dict(dx3=NULL), -1),
        ('history_stream_prologue', dict(dx3=dx3_zero), -1),
        ('history_stream_prologue', dict(dx3=dx3, T=8193), -2),
        ('history_stream_prologue', dict(dx3=dx3_zero, T=8193), -1),
        ('history_stream_prologue', dict(dx3=dx3, T=8193, sweep_time=NULL), -1),
        ('history_stream_prologue', dict(dx3=dx3_nan, T=0, sweep_time=NULL), -1),
        # ---- fbbev_history_warp_e / _warp: planes (B, CH, Z, Y, X); axes < 2 are BADARG here; no alignment rule
        ('history_warp_e', dict(B=-1), -1),
        ('history_warp_e', dict(CH=-1), -1),
        ('history_warp_e', dict(Z=1), -1),
        ('history_warp_e', dict(Y=1), -1),
        ('history_warp_e', dict(X=1), -1),
        ('history_warp_e', dict(elem_type=3), -1),
        ('history_warp_e', dict(elem_type=-1), -1),
        ('history_warp_e', dict(B=0, null=True), 0),
        ('history_warp_e', dict(CH=0, null=True), 0),
        ('history_warp_e', dict(B=0, elem_type=3), -1),
        ('history_warp_e', dict(CH=0, Z=1), -1),
        ('history_warp_e', dict(history=NULL), -1),
        ('history_warp_e', dict(rt_flow=NULL), -1),
        ('history_warp_e', dict(out=NULL), -1),
        ('history_warp_e', H_2G_VOXELS, -2),
        ('history_warp_e', dict(H_2G_VOXELS, history=NULL), -1),
        ('history_warp_e', dict(H_2G_VOXELS, history_stride_b=1), -2),
        ('history_warp_e', dict(H_BELOW_2G, history_stride_b=1), -1),
        ('history_warp_e', dict(history_stride_b=F - 1), -1),
        ('history_warp_e', dict(out_stride_b=F - 1), -1),
        ('history_warp_e', dict(out_stride_b=F - 1, elem_type=0), -1),
        ('history_warp_e', dict(H_BELOW_2G, B=256), -2),                       # stride 0 is dense; more workgroups than a grid holds
        ('history_warp_e', dict(H_BELOW_2G, B=256, out_stride_b=80 * (2047 << 20) - 1), -1),
        ('history_warp_e', dict(H_BELOW_2G, B=256, history=P8, out_stride_b=80 * (2047 << 20)), -2),
        ('history_warp', dict(Z=1), -1),
        ('history_warp', dict(B=0, null=True), 0),
        ('history_warp', dict(history=NULL), -1),
        ('history_warp', dict(history_stride_b=F - 1), -1),
        ('history_warp', H_2G_VOXELS, -2),
        ('history_warp', dict(H_BELOW_2G, B=256), -2),
        # ---- fbbev_history_warp_vm: the voxel-major ring (B, T, N, C), rows of 4 (fp32) or 8 (16-bit) elements
        ('history_warp_vm', dict(B=-1), -1),
        ('history_warp_vm', dict(T=-1), -1),
        ('history_warp_vm', dict(C=0), -1),
        ('history_warp_vm', dict(Z=1), -1),
        ('history_warp_vm', dict(Y=1), -1),
        ('history_warp_vm', dict(X=1), -1),
        ('history_warp_vm', dict(elem_type=3), -1),
        ('history_warp_vm', dict(elem_type=3, T=0), -1),
        ('history_warp_vm', dict(B=0, null=True), 0),
        ('history_warp_vm', dict(T=0, null=True), 0),
        ('history_warp_vm', dict(history=NULL), -1),
        ('history_warp_vm', dict(rt_flow=NULL), -1),
        ('history_warp_vm', dict(out=NULL), -1),
        ('history_warp_vm', H_2G_VOXELS, -2),
        ('history_warp_vm', dict(H_2G_VOXELS, out=NULL), -1),
        ('history_warp_vm', dict(H_2G_VOXELS, history_stride_b=1), -2),
        ('history_warp_vm', dict(H_BELOW_2G, history_stride_b=1), -1),
        ('history_warp_vm', dict(history_stride_b=16 * F - 1), -1),
        ('history_warp_vm', dict(out_stride_b=16 * F - 1), -1),
        ('history_warp_vm', dict(history_stride_b=16 * F - 1, out=P8), -1),
        ('history_warp_vm', dict(history=P8, out_stride_b=16 * F - 1), -1),
        ('history_warp_vm', dict(C=84), -2),
        ('history_warp_vm', dict(C=84, history_stride_b=1), -1),
        ('history_warp_vm', dict(C=82, elem_type=0), -2),
        ('history_warp_vm', dict(history_stride_b=16 * F + 4), -2),
        ('history_warp_vm', dict(out_stride_b=16 * F + 4, elem_type=2), -2),
        ('history_warp_vm', dict(history_stride_b=16 * F + 2, elem_type=0), -2),
        ('history_warp_vm', dict(history=P8), -2),
        ('history_warp_vm', dict(out=P8), -2),
        ('history_warp_vm', H_C8_AT_4G, -2),
        ('history_warp_vm', H_C8_F32_AT_4G, -2),
        ('history_warp_vm', dict(H_C80_AT_4G, elem_type=2), -2),
        ('history_warp_vm', dict(B=1 << 25), -2),                              # 2^31 workgroups
        ('history_warp_vm', dict(B=1 << 25, history_stride_b=16 * F - 1), -1),
        # ---- fbbev_history_warp_vm_src: warp_vm's checks, then its own operands (the frame past 32-bit offsets is pinned here:
        # just below it the null `curr` is reached)
        ('history_warp_vm_src', dict(Z=1), -1),
        ('history_warp_vm_src', dict(elem_type=3), -1),
        ('history_warp_vm_src', dict(B=0, null=True), 0),
        ('history_warp_vm_src', dict(T=0, curr=NULL, flags=NULL), 0),
        ('history_warp_vm_src', dict(out=NULL), -1),
        ('history_warp_vm_src', dict(curr=NULL), -1),
        ('history_warp_vm_src', dict(flags=NULL), -1),
        ('history_warp_vm_src', dict(curr=NULL, history=P8), -2),
        ('history_warp_vm_src', dict(curr=NULL, C=84), -2),
        ('history_warp_vm_src', dict(curr=NULL, history_stride_b=16 * F - 1), -1),
        ('history_warp_vm_src', dict(H_C8_AT_4G, curr=NULL), -2),
        ('history_warp_vm_src', dict(H_C8_BELOW_4G, curr=NULL), -1),
        ('history_warp_vm_src', dict(H_C8_F32_AT_4G, curr=NULL), -2),
        ('history_warp_vm_src', dict(H_C8_F32_BELOW_4G, curr=NULL), -1),
        ('history_warp_vm_src', dict(H_C80_AT_4G, flags=NULL), -2),
        ('history_warp_vm_src', dict(H_C80_BELOW_4G, flags=NULL), -1),
        ('history_warp_vm_src', dict(H_2G_VOXELS, curr=NULL), -2),
        ('history_warp_vm_src', dict(curr_stride_b=F - 1), -1),
        ('history_warp_vm_src', dict(curr_stride_b=F + 4), -2),
        ('history_warp_vm_src', dict(curr_stride_b=F + 2, elem_type=0), -2),
        ('history_warp_vm_src', dict(curr=P8), -2),
        ('history_warp_vm_src', dict(curr=P8, curr_stride_b=F - 1), -1),
        ('history_warp_vm_src', dict(curr=P8, flags=NULL), -1),
        ('history_warp_vm_src', dict(B=1 << 25), -2),                          # stride 0 is dense; 2^31 workgroups
        ('history_warp_vm_src', dict(B=1 << 25, curr_stride_b=F - 1), -1),
        ('history_warp_vm_src', dict(B=1 << 25, flags=NULL), -1),
        # ---- fbbev_history_frame_vm: one frame into a ring slot
        ('history_frame_vm', dict(B=-1), -1),
        ('history_frame_vm', dict(C=0), -1),
        ('history_frame_vm', dict(N=-1), -1),
        ('history_frame_vm', dict(elem_type=3), -1),
        ('history_frame_vm', dict(inner=0), -1),
        ('history_frame_vm', dict(inner=3), -1),
        ('history_frame_vm', dict(B=0, null=True), 0),
        ('history_frame_vm', dict(N=0, null=True), 0),
        ('history_frame_vm', dict(N=0, inner=0), -1),
        ('history_frame_vm', dict(B=0, elem_type=3), -1),
        ('history_frame_vm', dict(curr=NULL), -1),
        ('history_frame_vm', dict(out=NULL), -1),
        ('history_frame_vm', dict(out_stride_b=F - 1), -1),
        ('history_frame_vm', dict(out_stride_b=F - 1, out=P8), -1),
        ('history_frame_vm', dict(out_stride_b=F - 1, curr=NULL), -1),
        ('history_frame_vm', dict(C=84), -2),
        ('history_frame_vm', dict(C=84, out_stride_b=1), -1),
        ('history_frame_vm', dict(C=82, elem_type=0), -2),
        ('history_frame_vm', dict(C=520), -2),
        ('history_frame_vm', dict(out_stride_b=F + 4), -2),
        ('history_frame_vm', dict(out_stride_b=F + 2, elem_type=0), -2),
        ('history_frame_vm', dict(out=P8), -2),
        ('history_frame_vm', many_wgs, -2),                                    # stride 0 is dense
        ('history_frame_vm', dict(many_wgs, out_stride_b=2048 * 80 - 1), -1),
        # ---- fbbev_history_conv_e / _conv: planes (B, T1 * C, N); channels in 16s up to 128; bias1's alignment LAST; the
        # workspace only where the register-resident kernel runs (C = Cout in {16, 80})
        ('history_conv_e', dict(B=-1), -1),
        ('history_conv_e', dict(T1=0), -1),
        ('history_conv_e', dict(C=0), -1),
        ('history_conv_e', dict(Cout=0), -1),
        ('history_conv_e', dict(N=-1), -1),
        ('history_conv_e', dict(elem_type=3), -1),
        ('history_conv_e', dict(B=0, null=True), 0),
        ('history_conv_e', dict(N=0, null=True), 0),
        ('history_conv_e', dict(B=0, T1=0), -1),
        ('history_conv_e', dict(feats=NULL), -1),
        ('history_conv_e', dict(w1=NULL), -1),
        ('history_conv_e', dict(bias1=NULL), -1),
        ('history_conv_e', dict(w2=NULL), -1),
        ('history_conv_e', dict(bias2=NULL), -1),
        ('history_conv_e', dict(out=NULL), -1),
        ('history_conv_e', dict(C=40), -2),
        ('history_conv_e', dict(Cout=40), -2),
        ('history_conv_e', dict(C=144, Cout=144), -2),
        ('history_conv_e', dict(C=40, w1=NULL), -1),
        ('history_conv_e', dict(C=40, feats_stride_b=1), -2),
        ('history_conv_e', dict(feats_stride_b=17 * F - 1), -1),
        ('history_conv_e', dict(feats_stride_b=17 * F - 1, bias1=P8), -1),
        ('history_conv_e', dict(bias1=P8), -2),
        ('history_conv_e', dict(bias1=P8, workspace_bytes=16), -2),
        ('history_conv_e', dict(workspace_bytes=16), -3),                      # stride 0 is dense
        ('history_conv_e', dict(workspace_bytes=16, feats=P8, feats_stride_b=17 * F + 1), -3),   # planes: no alignment rule
        ('history_conv_e', dict(workspace_bytes=460799), -3),
        ('history_conv_e', dict(workspace_bytes=18431, C=16, Cout=16, elem_type=0), -3),
        ('history_conv_e', many_wgs, -2),
        ('history_conv_e', dict(many_wgs, workspace_bytes=16), -2),
        ('history_conv', dict(N=-1), -1),
        ('history_conv', dict(B=0, null=True), 0),
        ('history_conv', dict(C=40), -2),
        ('history_conv', dict(feats_stride_b=17 * F - 1), -1),
        ('history_conv', dict(bias1=P8), -2),
        ('history_conv', dict(workspace_bytes=16), -3),
        # ---- fbbev_history_conv_vm: the same arithmetic on a voxel-major ring; the workspace is required and asked for BEFORE the stride
        ('history_conv_vm', dict(B=-1), -1),
        ('history_conv_vm', dict(T1=0), -1),
        ('history_conv_vm', dict(elem_type=3), -1),
        ('history_conv_vm', dict(B=0, null=True), 0),
        ('history_conv_vm', dict(N=0, null=True), 0),
        ('history_conv_vm', dict(N=0, elem_type=3), -1),
        ('history_conv_vm', dict(out=NULL), -1),
        ('history_conv_vm', dict(bias2=NULL), -1),
        ('history_conv_vm', dict(C=32, Cout=32), -2),
        ('history_conv_vm', dict(Cout=16), -2),
        ('history_conv_vm', dict(C=32, Cout=32, feats=NULL), -1),
        ('history_conv_vm', dict(workspace=NULL), -3),
        ('history_conv_vm', dict(workspace=NULL, C=32, Cout=32), -2),
        ('history_conv_vm', dict(workspace=NULL, w2=NULL), -1),
        ('history_conv_vm', dict(workspace=NULL, feats_stride_b=17 * F - 1), -3),
        ('history_conv_vm', dict(feats_stride_b=17 * F - 1), -1),
        ('history_conv_vm', dict(feats_stride_b=17 * F - 1, feats=P8), -1),
        ('history_conv_vm', dict(feats=P8), -2),
        ('history_conv_vm', dict(feats_stride_b=17 * F + 4), -2),
        ('history_conv_vm', dict(feats_stride_b=17 * F + 4, elem_type=0), -2),  # rows of 8 elements whatever the type
        ('history_conv_vm', dict(C=16, Cout=16, N=1 << 27), -2),
        ('history_conv_vm', dict(C=16, Cout=16, N=(1 << 27) - 1, workspace_bytes=16), -3),
        ('history_conv_vm', dict(C=16, Cout=16, N=1 << 26, elem_type=0), -2),
        ('history_conv_vm', dict(C=16, Cout=16, N=(1 << 26) - 1, elem_type=0, workspace_bytes=16), -3),
        ('history_conv_vm', dict(bias1=P8), -2),
        ('history_conv_vm', dict(bias1=P8, workspace_bytes=16), -2),
        ('history_conv_vm', dict(bias1=P8, feats_stride_b=1), -1),
        ('history_conv_vm', dict(workspace_bytes=16), -3),                     # stride 0 is dense
        ('history_conv_vm', dict(workspace_bytes=460799), -3),
        ('history_conv_vm', dict(workspace=P8, workspace_bytes=16), -3),
        ('history_conv_vm', many_wgs, -2),
        ('history_conv_vm', dict(many_wgs, workspace_bytes=16), -2),
        # ---- fbbev_history_conv_bf16: either layout (the flag right after the dimensions); row and 32-bit rules only voxel-major
        ('history_conv_bf16', dict(B=-1), -1),
        ('history_conv_bf16', dict(Cout=0), -1),
        ('history_conv_bf16', dict(elem_type=-1), -1),
        ('history_conv_bf16', dict(voxel_major=2), -1),
        ('history_conv_bf16', dict(voxel_major=-1, B=0), -1),
        ('history_conv_bf16', dict(B=0, null=True), 0),
        ('history_conv_bf16', dict(N=0, null=True), 0),
        ('history_conv_bf16', dict(w1=NULL), -1),
        ('history_conv_bf16', dict(out=NULL), -1),
        ('history_conv_bf16', dict(C=32, Cout=32), -2),
        ('history_conv_bf16', dict(C=16), -2),
        ('history_conv_bf16', dict(C=32, Cout=32, bias2=NULL), -1),
        ('history_conv_bf16', dict(C=32, Cout=32, feats_stride_b=1), -2),
        ('history_conv_bf16', dict(feats_stride_b=17 * F - 1), -1),
        ('history_conv_bf16', dict(feats_stride_b=17 * F - 1, voxel_major=0), -1),
        ('history_conv_bf16', dict(feats_stride_b=17 * F - 1, feats=P8), -1),
        ('history_conv_bf16', dict(feats=P8), -2),
        ('history_conv_bf16', dict(feats_stride_b=17 * F + 4), -2),
        ('history_conv_bf16', dict(feats_stride_b=17 * F + 4, elem_type=0), -2),
        ('history_conv_bf16', dict(feats=P8, feats_stride_b=17 * F + 1, voxel_major=0, workspace=NULL), -3),
        ('history_conv_bf16', dict(bias1=P8), -2),
        ('history_conv_bf16', dict(bias1=P8, voxel_major=0), -2),
        ('history_conv_bf16', dict(bias1=P8, workspace=NULL), -2),
        ('history_conv_bf16', dict(bias1=P8, feats_stride_b=1), -1),
        ('history_conv_bf16', dict(C=16, Cout=16, N=1 << 27), -2),
        ('history_conv_bf16', dict(C=16, Cout=16, N=(1 << 27) - 1, workspace=NULL), -3),
        ('history_conv_bf16', dict(C=16, Cout=16, N=1 << 27, voxel_major=0, workspace=NULL), -3),
        ('history_conv_bf16', dict(C=16, Cout=16, N=1 << 26, elem_type=0), -2),
        ('history_conv_bf16', dict(C=16, Cout=16, N=(1 << 26) - 1, elem_type=0, workspace=NULL), -3),
        ('history_conv_bf16', dict(workspace=NULL), -3),                       # stride 0 is dense
        ('history_conv_bf16', dict(workspace=P8), -3),
        ('history_conv_bf16', dict(workspace_bytes=276479), -3),
        ('history_conv_bf16', dict(workspace_bytes=276479, voxel_major=0, elem_type=2), -3),
        ('history_conv_bf16', many_wgs, -2),
        ('history_conv_bf16', dict(many_wgs, workspace=NULL), -2),
        # ---- fbbev_history_conv_bf16x3: 16-bit voxel-major rings only (fp32: -2, with the channel counts); the workspace also
        # holds B * T1 * C scaled biases; the preparation launch covers fewer than 2^31 items
        ('history_conv_bf16x3', dict(B=-1), -1),
        ('history_conv_bf16x3', dict(N=-1), -1),
        ('history_conv_bf16x3', dict(elem_type=3), -1),
        ('history_conv_bf16x3', dict(B=0, null=True), 0),
        ('history_conv_bf16x3', dict(N=0, null=True), 0),
        ('history_conv_bf16x3', dict(B=0, elem_type=3), -1),
        ('history_conv_bf16x3', dict(feats=NULL), -1),
        ('history_conv_bf16x3', dict(bias1=NULL), -1),
        ('history_conv_bf16x3', dict(C=32, Cout=32), -2),
        ('history_conv_bf16x3', dict(elem_type=0), -2),
        ('history_conv_bf16x3', dict(elem_type=0, out=NULL), -1),
        ('history_conv_bf16x3', dict(elem_type=0, feats_stride_b=1), -2),
        ('history_conv_bf16x3', dict(feats_stride_b=17 * F - 1), -1),
        ('history_conv_bf16x3', dict(feats_stride_b=17 * F - 1, bias1=P8), -1),
        ('history_conv_bf16x3', dict(feats=P8), -2),
        ('history_conv_bf16x3', dict(feats_stride_b=17 * F + 4), -2),
        ('history_conv_bf16x3', dict(bias1=P8), -2),
        ('history_conv_bf16x3', dict(bias1=P8, workspace=NULL), -2),
        ('history_conv_bf16x3', dict(C=16, Cout=16, N=1 << 27), -2),
        ('history_conv_bf16x3', dict(C=16, Cout=16, N=(1 << 27) - 1, workspace=NULL), -3),
        ('history_conv_bf16x3', dict(workspace=NULL), -3),                     # stride 0 is dense
        ('history_conv_bf16x3', dict(workspace=P8), -3),
        ('history_conv_bf16x3', dict(workspace_bytes=558399), -3),
        ('history_conv_bf16x3', dict(B=1 << 26), -2),
        ('history_conv_bf16x3', dict(B=1 << 26, workspace_bytes=16), -3),
        # ---- fbbev_history_fused_x3_vm: axes <= 0 are BADARG, < 2 UNSUPPORTED (with the channel counts and the type); both rings;
        # the workspace's 64 spare bytes BEFORE the convolutions' own checks (bias1, workspace, preparation launch)
        ('history_fused_x3_vm', dict(B=-1), -1),
        ('history_fused_x3_vm', dict(T=0), -1),
        ('history_fused_x3_vm', dict(C=0), -1),
        ('history_fused_x3_vm', dict(Cout=0), -1),
        ('history_fused_x3_vm', dict(Z=0), -1),
        ('history_fused_x3_vm', dict(Y=0), -1),
        ('history_fused_x3_vm', dict(X=0), -1),
        ('history_fused_x3_vm', dict(B=0, null=True), 0),
        ('history_fused_x3_vm', dict(B=0, T=0), -1),
        ('history_fused_x3_vm', dict(B=0, elem_type=7, Z=1), 0),
        ('history_fused_x3_vm', dict(history=NULL), -1),
        ('history_fused_x3_vm', dict(next=NULL), -1),
        ('history_fused_x3_vm', dict(rt_flow=NULL), -1),
        ('history_fused_x3_vm', dict(w1=NULL), -1),
        ('history_fused_x3_vm', dict(bias1=NULL), -1),
        ('history_fused_x3_vm', dict(w2=NULL), -1),
        ('history_fused_x3_vm', dict(bias2=NULL), -1),
        ('history_fused_x3_vm', dict(out=NULL), -1),
        ('history_fused_x3_vm', dict(C=16, Cout=16), -2),
        ('history_fused_x3_vm', dict(Cout=16), -2),
        ('history_fused_x3_vm', dict(elem_type=0), -2),
        ('history_fused_x3_vm', dict(elem_type=3), -2),
        ('history_fused_x3_vm', dict(Z=1), -2),
        ('history_fused_x3_vm', dict(Y=1), -2),
        ('history_fused_x3_vm', dict(X=1), -2),
        ('history_fused_x3_vm', dict(Z=1, out=NULL), -1),
        ('history_fused_x3_vm', dict(elem_type=3, history_stride_b=1), -2),
        ('history_fused_x3_vm', dict(history_stride_b=16 * F - 1), -1),
        ('history_fused_x3_vm', dict(next_stride_b=17 * F - 1), -1),
        ('history_fused_x3_vm', dict(history_stride_b=16 * F - 1, next=P8), -1),
        ('history_fused_x3_vm', dict(history=P8, next_stride_b=16 * F), -1),
        ('history_fused_x3_vm', dict(history=P8), -2),
        ('history_fused_x3_vm', dict(next=P8), -2),
        ('history_fused_x3_vm', dict(history_stride_b=16 * F + 4), -2),
        ('history_fused_x3_vm', dict(next_stride_b=17 * F + 4), -2),
        ('history_fused_x3_vm', dict(next=P8, workspace_bytes=32), -2),
        ('history_fused_x3_vm', dict(H_C80_AT_4G, workspace_bytes=32), -2),
        ('history_fused_x3_vm', dict(H_C80_BELOW_4G, workspace_bytes=32), -3),
        ('history_fused_x3_vm', dict(workspace_bytes=63), -3),                 # stride 0 is dense
        ('history_fused_x3_vm', dict(workspace_bytes=63, bias1=P8), -3),
        ('history_fused_x3_vm', dict(workspace_bytes=64, bias1=P8), -2),
        ('history_fused_x3_vm', dict(bias1=P8), -2),
        ('history_fused_x3_vm', dict(bias1=P8, workspace=NULL), -2),
        ('history_fused_x3_vm', dict(workspace=NULL), -3),
        ('history_fused_x3_vm', dict(workspace=P8), -3),
        ('history_fused_x3_vm', dict(workspace_bytes=558400 + 63), -3),
        ('history_fused_x3_vm', dict(B=1 << 26), -2),
        ('history_fused_x3_vm', dict(B=1 << 26, workspace=NULL), -3),
        # ---- fbbev_history_step_x3_vm: `chunks` with the dimensions; `next`'s stride here, the history's left to the warp's plan
        # (where an axis < 2 is BADARG), then the convolutions' checks (where the channel counts are looked at)
        ('history_step_x3_vm', dict(B=-1), -1),
        ('history_step_x3_vm', dict(T=0), -1),
        ('history_step_x3_vm', dict(Cout=0), -1),
        ('history_step_x3_vm', dict(X=0), -1),
        ('history_step_x3_vm', dict(chunks=-1), -1),
        ('history_step_x3_vm', dict(chunks=65), -1),
        ('history_step_x3_vm', dict(chunks=64, workspace=NULL), -3),
        ('history_step_x3_vm', dict(B=0, null=True), 0),
        ('history_step_x3_vm', dict(B=0, chunks=65), -1),
        ('history_step_x3_vm', dict(history=NULL), -1),
        ('history_step_x3_vm', dict(next=NULL), -1),
        ('history_step_x3_vm', dict(rt_flow=NULL), -1),
        ('history_step_x3_vm', dict(bias2=NULL), -1),
        ('history_step_x3_vm', dict(out=NULL), -1),
        ('history_step_x3_vm', dict(elem_type=0), -2),
        ('history_step_x3_vm', dict(elem_type=3), -2),
        ('history_step_x3_vm', dict(elem_type=3, w1=NULL), -1),
        ('history_step_x3_vm', dict(elem_type=3, next_stride_b=1), -2),
        ('history_step_x3_vm', H_2G_VOXELS, -2),
        ('history_step_x3_vm', dict(H_2G_VOXELS, next_stride_b=1), -2),
        ('history_step_x3_vm', dict(H_BELOW_2G, next_stride_b=1), -1),
        ('history_step_x3_vm', dict(next_stride_b=17 * F - 1), -1),
        ('history_step_x3_vm', dict(next_stride_b=17 * F - 1, history=P8), -1),
        ('history_step_x3_vm', dict(Z=1), -1),
        ('history_step_x3_vm', dict(Y=1), -1),
        ('history_step_x3_vm', dict(Z=1, elem_type=3), -2),
        ('history_step_x3_vm', dict(Z=1, history=P8), -1),
        ('history_step_x3_vm', dict(history_stride_b=16 * F - 1), -1),
        ('history_step_x3_vm', dict(history_stride_b=16 * F - 1, next=P8), -1),
        ('history_step_x3_vm', dict(history_stride_b=16 * F - 1, C=84, Cout=84), -1),
        ('history_step_x3_vm', dict(history=P8), -2),
        ('history_step_x3_vm', dict(next=P8), -2),
        ('history_step_x3_vm', dict(history_stride_b=16 * F + 4), -2),
        ('history_step_x3_vm', dict(next_stride_b=17 * F + 4), -2),
        ('history_step_x3_vm', dict(C=84, Cout=84), -2),
        ('history_step_x3_vm', dict(C=32, Cout=32), -2),
        ('history_step_x3_vm', dict(C=32, Cout=32, workspace=NULL), -2),
        ('history_step_x3_vm', dict(Cout=16, workspace=NULL), -2),
        ('history_step_x3_vm', dict(C=16, Cout=16, workspace=NULL), -3),
        ('history_step_x3_vm', dict(H_C80_AT_4G, workspace=NULL), -2),
        ('history_step_x3_vm', dict(H_C80_BELOW_4G, workspace=NULL), -3),
        ('history_step_x3_vm', dict(bias1=P8), -2),
        ('history_step_x3_vm', dict(bias1=P8, workspace=NULL), -2),
        ('history_step_x3_vm', dict(workspace=NULL), -3),                      # stride 0 is dense
        ('history_step_x3_vm', dict(workspace=P8), -3),
        ('history_step_x3_vm', dict(workspace_bytes=558399), -3),
        ('history_step_x3_vm', dict(B=1 << 26), -2),
        ('history_step_x3_vm', dict(B=1 << 26, workspace=NULL), -3),
        # ---- fbbev_history_fused_vm: fused_x3_vm's order with bias1 among the row alignments and the bf16 fragments' workspace
        ('history_fused_vm', dict(B=-1), -1),
        ('history_fused_vm', dict(T=0), -1),
        ('history_fused_vm', dict(C=0), -1),
        ('history_fused_vm', dict(Z=0), -1),
        ('history_fused_vm', dict(B=0, null=True), 0),
        ('history_fused_vm', dict(B=0, Y=0), -1),
        ('history_fused_vm', dict(history=NULL), -1),
        ('history_fused_vm', dict(next=NULL), -1),
        ('history_fused_vm', dict(w2=NULL), -1),
        ('history_fused_vm', dict(out=NULL), -1),
        ('history_fused_vm', dict(C=16, Cout=16), -2),
        ('history_fused_vm', dict(C=96), -2),
        ('history_fused_vm', dict(elem_type=0), -2),
        ('history_fused_vm', dict(elem_type=3), -2),
        ('history_fused_vm', dict(Z=1), -2),
        ('history_fused_vm', dict(X=1), -2),
        ('history_fused_vm', dict(Z=1, rt_flow=NULL), -1),
        ('history_fused_vm', dict(Z=1, history_stride_b=1), -2),
        ('history_fused_vm', dict(history_stride_b=16 * F - 1), -1),
        ('history_fused_vm', dict(next_stride_b=17 * F - 1), -1),
        ('history_fused_vm', dict(next_stride_b=17 * F - 1, history=P8), -1),
        ('history_fused_vm', dict(history_stride_b=16 * F - 1, bias1=P8), -1),
        ('history_fused_vm', dict(history=P8), -2),
        ('history_fused_vm', dict(next=P8), -2),
        ('history_fused_vm', dict(bias1=P8), -2),
        ('history_fused_vm', dict(bias1=P8, workspace=NULL), -2),
        ('history_fused_vm', dict(history_stride_b=16 * F + 4), -2),
        ('history_fused_vm', dict(next_stride_b=17 * F + 4), -2),
        ('history_fused_vm', dict(H_C80_AT_4G, workspace=NULL), -2),
        ('history_fused_vm', dict(H_C80_BELOW_4G, workspace=NULL), -3),
        ('history_fused_vm', dict(H_2G_VOXELS, workspace=NULL), -2),
        ('history_fused_vm', dict(workspace=NULL), -3),                        # stride 0 is dense
        ('history_fused_vm', dict(workspace=P8), -3),
        ('history_fused_vm', dict(workspace_bytes=276479), -3),
        # ---- the LayerNorm entries between the two halves of the family
        ('layernorm', dict(rows=-1), -1),
        ('layernorm', dict(C=0), -1),
        ('layernorm', dict(eps=-1.0), -1),
        ('layernorm', dict(eps=float('nan')), -1),
        ('layernorm', dict(rows=0, null=True), 0),
        ('layernorm', dict(rows=0, C=0), -1),
        ('layernorm', dict(x=NULL), -1),
        ('layernorm', dict(out=NULL), -1),
        ('layernorm', dict(C=82), -2),
        ('layernorm', dict(C=132), -2),
        ('layernorm', dict(C=82, weight=NULL), -1),
        ('layernorm', dict(x=P8), -2),
        ('layernorm', dict(residual=P8), -2),
        ('layernorm', dict(residual=NULL, bias=P8), -2),
        ('layernorm', dict(rows=1 << 34), -2),
        ('layernorm_bwd', dict(rows=-1), -1),
        ('layernorm_bwd', dict(eps=-1.0), -1),
        ('layernorm_bwd', dict(partial=NULL), -1),
        ('layernorm_bwd', dict(rows=0, partial=NULL), -1),
        ('layernorm_bwd', dict(grad_out=NULL), -1),
        ('layernorm_bwd', dict(grad_x=NULL, C=82), -1),
        ('layernorm_bwd', dict(C=82), -2),
        ('layernorm_bwd', dict(C=132), -2),
        ('layernorm_bwd', dict(grad_x=P8), -2),
        ('layernorm_bwd', dict(rows=0, C=82, null=True, partial=P16), -2),
    ]
    shown = lambda case: {k: (v.value if isinstance(v, ctypes.c_void_p) else repr(v[:]) if isinstance(v, ctypes.Array) else v)   # noqa: E731
                          for k, v in case.items()}
    got = [(entry, shown(case), h_call(lib, entry, case)) for entry, case, _ in table]
    want = [(entry, shown(case), code) for entry, case, code in table]
    assert got == want, [(g, w[2]) for g, w in zip(got, want) if g != w]
    assert {entry for entry, _, _ in table} == set(H_PARAMS)
    assert [lib.fbbev_layernorm_bwd_partials(r) for r in (-1, 0, 1, 8, 9, 16384, 16385, 1 << 40)] == [1, 1, 1, 1, 2, 2048, 2048, 2048]


# ---- the pooling family (tile index, dense forward in its planar / channels-last / row / pipelined forms, Z-mean, one-entry
# lift-splat, store-floor diagnostic, fused backward): one table, recorded on the launchers before they shared their operand records
PL_GATHER = ['depth', 'feat', 'ranks_depth', 'ranks_feat', 'interval_rank', 'interval_starts', 'interval_lengths', 'B', 'C', 'Z', 'Y', 'X']
PL_TABLE = ['tile_ws', 'tile_ws_bytes', 'tile_voxels', 'flags']
PL_INDEX = ['interval_rank', 'interval_starts', 'counts', 'n_intervals_max', 'B', 'Z', 'Y', 'X', 'tile_voxels', 'flags', 'tile_ws', 'tile_ws_bytes']
PL_BWD = ['depth', 'feat', 'ranks_depth', 'interval_rank', 'interval_starts', 'counts', 'n_intervals_max', 'B', 'N', 'D', 'H', 'W', 'C',
          'Z', 'Y', 'X', 'depth_grad', 'feat_grad', 'workspace', 'workspace_bytes', 'stream']
PL_PARAMS = {
    'pool_tile_index': PL_INDEX + ['stream'],
    'pool_tile_index_cached': PL_INDEX + ['cache_state', 'table_gate', 'stream'],
    'bev_pool_v2_dense_fwd': PL_GATHER + ['out', 'out_stride_b', 'out_stride_c'] + PL_TABLE + ['stream'],
    'bev_pool_v2_dense_fwd_add': PL_GATHER + ['out', 'out_stride_b', 'out_stride_c'] + PL_TABLE + ['addend', 'stream'],
    'bev_pool_v2_dense_fwd_rows': PL_GATHER + ['out_rows', 'out_stride_b', 'addend_rows', 'addend_row_stride'] + PL_TABLE + ['stream'],
    'diag_pool_store_floor': PL_GATHER + ['out'] + PL_TABLE + ['mode', 'stream'],
    'lift_splat_fused': ['frustum', 'xs', 'ys', 'ds', 'rots', 'trans', 'intrins', 'post_rots', 'post_trans', 'bda', 'depth', 'context',
                         'B', 'N', 'D', 'H', 'W', 'C', 'lower3', 'interval3', 'grid_size3', 'Z', 'Y', 'X', 'out', 'out_stride_b',
                         'out_stride_c', 'tile_voxels', 'flags', 'workspace', 'workspace_bytes', 'cam_key', 'cache_state', 'stream'],
    'pool_zmean': PL_GATHER + ['out_mean'] + PL_TABLE + ['stream'],
    'pool_zmean_split': PL_GATHER + ['out_mean'] + PL_TABLE + ['z_groups', 'partial_ws', 'partial_ws_bytes', 'stream'],
    'pool_zmean_rows': PL_GATHER + ['row_bias', 'out_rows'] + PL_TABLE + ['stream'],
    'bev_pool_v2_dense_bwd': ['out_grad', 'og_stride_b', 'og_stride_c'] + PL_BWD,
    'bev_pool_v2_dense_bwd_z': ['out_grad', 'og_stride_b', 'og_stride_c', 'zgrad', 'zscale'] + PL_BWD,
}
# a call that would LAUNCH (so no row below is this alone): one sample of one 2 x 4 camera with 2 depth bins, 16 channels into a
# 12 x 12 x 3 grid (432 voxels), 128-voxel tiles (6 planar tiles: a table of 56 bytes; 4 flat ones: 40; 27 of 16 voxels: 216),
# `sc1 nt` stores, 8 channels per lane, dense strides, workspaces of any size; every pointer non-null and 16-byte aligned
PL_SC1_NT, PL_CPL8, PL_WG128, PL_CL, PL_BF16, PL_F16, PL_SPLIT, PL_PIPE, PL_G8 = (0x20000, 0x4, 0x100, 0x100000, 0x800000, 0x1000000,
                                                                                 0x2000000, 0x4000000, 0x8000000)
PL_BASE = dict(B=1, N=1, D=2, H=2, W=4, C=16, Z=3, Y=12, X=12, tile_voxels=128, flags=PL_SC1_NT | PL_CPL8, n_intervals_max=10,
               out_stride_b=0, out_stride_c=0, og_stride_b=0, og_stride_c=0, addend_row_stride=0, tile_ws_bytes=1 << 40,
               workspace_bytes=1 << 40, partial_ws_bytes=1 << 40, mode=1, z_groups=1, zscale=0.5, stream=DA_NULL)
PL_2G_VOXELS = dict(Z=2048, Y=1024, X=1024)                          # 2^31 voxels
PL_BELOW_2G = dict(Z=2047, Y=1024, X=1024)
PL_2G_POINTS = dict(N=2048, D=1024, H=1024, W=1)                     # 2^31 frustum points
PL_POINTS_BELOW_2G = dict(N=2048, D=1023, H=1024, W=1)
PL_2G_WGS = dict(B=1 << 14, Z=1 << 14, Y=2, X=2, C=32, tile_voxels=64)   # 2^28 one-tile planes (2^30 voxels): x a channel split of 8
PL_LIFT_WS = 1189120                                                    # fbbev_lift_splat_fused_ws_bytes / _dense_bwd_workspace_bytes of PL_BASE
PL_BWD_WS = 1536


def pl_call(lib, entry, case):
    """`entry` with PL_BASE's operands, `case` on top of them; 'null': every pointer the entry takes is null unless `case` names it"""
    case = dict(case)
    null = case.pop('null', False)
    args = []
    for name in PL_PARAMS[entry]:
        if name in case:
            args.append(case.pop(name))
        elif name in PL_BASE:
            args.append(PL_BASE[name])
        else:
            args.append(DA_NULL if null else DA_P16)
    assert not case, (entry, 'operands the entry does not take', case)
    return getattr(lib, 'fbbev_' + entry)(*args)


def test_pool_entries_keep_their_error_codes():
    """Every entry of the pooling family: the code of each argument check, which code wins where two defects coincide (the order of
    an entry's checks is part of the ABI), and the routes a flags word refuses.  Every row returns BEFORE the entry's first runtime
    call (a launch, a memset, the opt-in to large LDS), so this runs without a GPU; what lies behind a launch -- the tile index
    inside fbbev_pool_tile_index_cached and fbbev_lift_splat_fused, the backward's `C > 128 && C % 8` -- is on the emulator
    (tests/test_emu_pool_launch_record.py).  The four host functions are pinned as values."""
    lib = _capi.declare(ctypes.CDLL(_capi.LIB_PATH))
    NULL, P16, P8 = DA_NULL, DA_P16, DA_P8
    F, CL = PL_SC1_NT | PL_CPL8, PL_CL
    GATHER7 = PL_GATHER[:7]
    table = []
    row = lambda entry, case, code: table.append((entry, case, code))   # noqa: E731
    # ---- fbbev_pool_tile_index: dimensions, pointers, 2^31 voxels (-2), the table's bytes per form (-3)
    for k in ('B', 'Z', 'Y', 'X'):
        row('pool_tile_index', {k: 0}, -1)
    row('pool_tile_index', dict(n_intervals_max=-1), -1)
    for k in ('interval_rank', 'interval_starts', 'counts', 'tile_ws'):
        row('pool_tile_index', {k: NULL}, -1)
    row('pool_tile_index', dict(B=0, null=True), -1)
    row('pool_tile_index', PL_2G_VOXELS, -2)
    row('pool_tile_index', dict(PL_2G_VOXELS, counts=NULL), -1)
    row('pool_tile_index', dict(PL_2G_VOXELS, tile_ws_bytes=0), -2)
    row('pool_tile_index', dict(PL_BELOW_2G, tile_ws_bytes=0), -3)
    row('pool_tile_index', dict(PL_2G_VOXELS, flags=CL, tile_voxels=16, tile_ws_bytes=0), -2)
    row('pool_tile_index', dict(PL_BELOW_2G, flags=CL, tile_voxels=16, tile_ws_bytes=0), -3)
    row('pool_tile_index', dict(tile_ws_bytes=55), -3)
    row('pool_tile_index', dict(tile_ws_bytes=79, tile_voxels=64), -3)              # 9 tiles
    row('pool_tile_index', dict(tile_ws_bytes=79, tile_voxels=100), -3)             # no tile size: 64
    row('pool_tile_index', dict(tile_ws_bytes=31, tile_voxels=256), -3)
    row('pool_tile_index', dict(tile_ws_bytes=79, tile_voxels=16), -3)              # small tiles only with channels-last: 64 here
    row('pool_tile_index', dict(tile_ws_bytes=39, flags=CL), -3)
    row('pool_tile_index', dict(tile_ws_bytes=63, flags=CL, tile_voxels=64), -3)    # 7 flat tiles
    row('pool_tile_index', dict(tile_ws_bytes=215, flags=CL, tile_voxels=16), -3)
    row('pool_tile_index', dict(tile_ws_bytes=431, flags=CL, tile_voxels=8), -3)
    row('pool_tile_index', dict(tile_ws_bytes=111, flags=CL, tile_voxels=32), -3)
    # ---- fbbev_pool_tile_index_cached: its own two checks; the gate kernel is launched before the shared ones run
    row('pool_tile_index_cached', dict(cache_state=NULL), -1)
    row('pool_tile_index_cached', dict(table_gate=NULL), -1)
    row('pool_tile_index_cached', dict(flags=CL, tile_voxels=16), -2)
    row('pool_tile_index_cached', dict(flags=CL, tile_voxels=8, B=0), -2)
    row('pool_tile_index_cached', dict(flags=CL, tile_voxels=32, table_gate=NULL), -1)
    # ---- fbbev_bev_pool_v2_dense_fwd[_add]: dimensions, pointers, shape and alignment (-2), 2^31 voxels (-2), strides (-1), table
    # bytes (-3), THEN the storage flags, the addend, the channels-last rules, LDS and workgroup bounds, the routes
    for fwd in ('bev_pool_v2_dense_fwd', 'bev_pool_v2_dense_fwd_add'):
        for k in ('B', 'C', 'Z', 'Y', 'X'):
            row(fwd, {k: 0}, -1)
        for k in GATHER7 + ['out', 'tile_ws']:
            row(fwd, {k: NULL}, -1)
        row(fwd, dict(C=18), -2)
        row(fwd, dict(C=260), -2)
        row(fwd, dict(Y=1, X=6), -2)
        row(fwd, dict(out=P8), -2)
        row(fwd, dict(feat=P8), -2)
        row(fwd, dict(C=18, out=NULL), -1)
        row(fwd, dict(C=18, out_stride_c=1), -2)
        row(fwd, PL_2G_VOXELS, -2)
        row(fwd, dict(PL_2G_VOXELS, out_stride_c=4), -2)
        row(fwd, dict(PL_BELOW_2G, out_stride_c=4), -1)
        row(fwd, dict(PL_BELOW_2G, tile_ws_bytes=0), -3)
        row(fwd, dict(out_stride_c=428), -1)
        row(fwd, dict(out_stride_c=434), -1)
        row(fwd, dict(out_stride_c=436, out_stride_b=16 * 436 - 4), -1)
        row(fwd, dict(out_stride_b=16 * 432 + 2), -1)
        row(fwd, dict(out_stride_b=16 * 432 - 4), -1)
        row(fwd, dict(out_stride_c=428, tile_ws_bytes=0), -1)
        row(fwd, dict(tile_ws_bytes=55), -3)
        row(fwd, dict(tile_ws_bytes=79, tile_voxels=64), -3)
        row(fwd, dict(tile_ws_bytes=79, tile_voxels=16), -3)                        # no planar tile size: 64
        row(fwd, dict(tile_ws_bytes=31, tile_voxels=256), -3)
        row(fwd, dict(flags=F | PL_BF16 | PL_F16), -1)
        row(fwd, dict(flags=F | PL_BF16 | PL_F16, tile_ws_bytes=55), -3)            # the storage flags come after the table's bytes
        row(fwd, dict(flags=F | PL_BF16 | PL_F16 | CL), -1)
        row(fwd, dict(flags=F | PL_BF16 | CL), -2)
        row(fwd, dict(flags=F | PL_F16 | CL), -2)
        row(fwd, dict(flags=F | PL_BF16 | CL, tile_ws_bytes=55), -3)
        row(fwd, dict(flags=F | PL_BF16, Y=6, X=6), -2)                             # Y * X % 8
        row(fwd, dict(flags=F | PL_F16, out_stride_c=436), -2)
        row(fwd, dict(flags=F | PL_BF16, out_stride_b=16 * 432 + 4), -2)
        # channels-last: dense strides only (-1), the small tiles' table (-3) and thread count (-2), the flat tiles' table (-3)
        if fwd == 'bev_pool_v2_dense_fwd':                                          # (with an addend channels-last is -2 before any of it)
            row(fwd, dict(flags=F | CL, out_stride_c=436), -1)
            row(fwd, dict(flags=F | CL, out_stride_b=16 * 432 + 4), -1)
            row(fwd, dict(flags=F | CL, out_stride_b=16 * 432 + 4, tile_ws_bytes=0), -3)   # the planar table, never smaller than the flat one
            row(fwd, dict(flags=F | CL, tile_voxels=16, out_stride_c=436, tile_ws_bytes=215), -1)
            row(fwd, dict(flags=F | CL, tile_voxels=16, tile_ws_bytes=215), -3)
            row(fwd, dict(flags=F | CL, tile_voxels=8, tile_ws_bytes=431), -3)
            row(fwd, dict(flags=F | CL, tile_voxels=32, C=132), -2)                     # 33 * 32 lanes
            row(fwd, dict(flags=F | CL, tile_voxels=32, C=132, tile_ws_bytes=111), -3)
            row(fwd, dict(flags=F | CL, tile_voxels=32, C=132, tile_ws_bytes=55), -3)   # (the planar table's bytes are looked at first)
        # LDS above 160 KiB and 2^31 workgroups (-2), behind the table's bytes
        row(fwd, dict(tile_voxels=1024, C=256), -2)
        row(fwd, dict(tile_voxels=1024, C=40), -2)
        row(fwd, dict(tile_voxels=1024, C=256, tile_ws_bytes=31), -3)
        row(fwd, dict(tile_voxels=256, C=160, flags=F | PL_PIPE), -2)              # the pipe's second staging buffer tips it over
        row(fwd, dict(PL_2G_WGS, flags=F | (8 << 4)), -2)
        # routes a flags word refuses: split-long / gather-8 are built for 256 threads, fp32, `sc1 nt`, 64- / 128-voxel tiles
        for route in (PL_SPLIT, PL_G8, PL_SPLIT | PL_G8):
            row(fwd, dict(flags=F | route | PL_WG128), -2)
            row(fwd, dict(flags=F | route | PL_BF16), -2)
            row(fwd, dict(flags=F | route | PL_F16), -2)
            row(fwd, dict(flags=PL_CPL8 | route), -2)
            row(fwd, dict(flags=PL_CPL8 | route | 1), -2)
            row(fwd, dict(flags=F | route, tile_voxels=256), -2)
            row(fwd, dict(flags=F | route, tile_voxels=1024), -2)
            row(fwd, dict(flags=F | route | PL_PIPE | PL_WG128), -2)
            row(fwd, dict(flags=F | route | PL_WG128, tile_ws_bytes=55), -3)
    row('bev_pool_v2_dense_fwd_add', dict(addend=NULL), -1)
    row('bev_pool_v2_dense_fwd_add', dict(addend=NULL, C=18), -1)
    row('bev_pool_v2_dense_fwd_add', dict(addend=NULL, flags=F | CL), -1)
    row('bev_pool_v2_dense_fwd_add', dict(addend=P8), -2)
    row('bev_pool_v2_dense_fwd_add', dict(addend=P8, B=0), -1)
    row('bev_pool_v2_dense_fwd_add', dict(addend=P8, tile_ws_bytes=55), -3)
    row('bev_pool_v2_dense_fwd_add', dict(addend=P8, flags=F | PL_BF16 | PL_F16), -1)
    row('bev_pool_v2_dense_fwd_add', dict(flags=F | CL), -2)                        # no addend with channels-last
    row('bev_pool_v2_dense_fwd_add', dict(flags=F | CL, out_stride_c=436), -2)      # ... seen before its stride rule
    row('bev_pool_v2_dense_fwd_add', dict(flags=F | CL, tile_voxels=16, tile_ws_bytes=215), -2)
    row('bev_pool_v2_dense_fwd_add', dict(flags=F | CL, tile_voxels=32, C=132), -2)
    row('bev_pool_v2_dense_fwd_add', dict(flags=F | CL, tile_ws_bytes=0), -3)
    # ---- fbbev_bev_pool_v2_dense_fwd_rows: both storage flags (-1) right after the pointers, flat index (-2), strides (-1), rows (-2)
    rows = 'bev_pool_v2_dense_fwd_rows'
    for k in ('B', 'C', 'Z', 'Y', 'X'):
        row(rows, {k: 0}, -1)
    for k in GATHER7 + ['out_rows', 'tile_ws']:
        row(rows, {k: NULL}, -1)
    row(rows, dict(flags=F | PL_BF16 | PL_F16), -1)
    row(rows, dict(flags=F | PL_BF16 | PL_F16, tile_ws_bytes=0), -1)                # ... before the table's bytes here
    row(rows, dict(PL_2G_VOXELS, flags=F | PL_BF16 | PL_F16), -1)
    row(rows, PL_2G_VOXELS, -2)
    row(rows, dict(B=2, Z=1, Y=1 << 15, X=1 << 15), -2)
    row(rows, dict(B=1, Z=1, Y=1 << 16, X=1 << 15), -2)
    row(rows, dict(PL_2G_VOXELS, out_stride_b=16), -2)
    row(rows, dict(PL_BELOW_2G, out_stride_b=16), -1)
    row(rows, dict(PL_BELOW_2G, tile_ws_bytes=0), -3)
    row(rows, dict(out_stride_b=432 * 16 - 4), -1)
    row(rows, dict(addend_row_stride=12), -1)
    row(rows, dict(addend_row_stride=12, C=18), -1)
    row(rows, dict(addend_rows=NULL, addend_row_stride=12), -1)                     # the stride is looked at without an addend too
    row(rows, dict(C=18), -2)
    row(rows, dict(C=260), -2)
    row(rows, dict(C=20, flags=F | PL_BF16), -2)                                    # 16-bit rows: C % 8
    row(rows, dict(out_stride_b=432 * 16 + 4, B=2, flags=F | PL_F16), -2)
    row(rows, dict(out_stride_b=432 * 16 + 2, B=2), -2)
    row(rows, dict(addend_row_stride=18), -2)
    row(rows, dict(out_rows=P8), -2)
    row(rows, dict(feat=P8), -2)
    row(rows, dict(addend_rows=P8), -2)
    row(rows, dict(C=18, tile_ws_bytes=0), -2)
    row(rows, dict(tile_voxels=16), -2)
    row(rows, dict(tile_voxels=8, tile_ws_bytes=0), -2)
    row(rows, dict(tile_ws_bytes=39), -3)
    row(rows, dict(tile_ws_bytes=63, tile_voxels=64), -3)
    row(rows, dict(tile_ws_bytes=63, tile_voxels=100, addend_rows=NULL), -3)
    # ---- fbbev_diag_pool_store_floor: one instantiation; LDS bound 64 KiB
    diag = 'diag_pool_store_floor'
    for k in ('B', 'C', 'Z', 'Y', 'X'):
        row(diag, {k: 0}, -1)
    row(diag, dict(mode=0), -1)
    row(diag, dict(mode=4), -1)
    for k in GATHER7 + ['out', 'tile_ws']:
        row(diag, {k: NULL}, -1)
    row(diag, dict(tile_voxels=64, out=NULL), -1)
    row(diag, dict(tile_voxels=64), -2)
    row(diag, dict(tile_voxels=100), -2)
    row(diag, dict(Y=1, X=6), -2)
    row(diag, dict(Y=6, X=6, flags=F | PL_BF16), -2)
    row(diag, dict(out=P8), -2)
    row(diag, dict(flags=F | CL), -2)
    row(diag, dict(flags=F | PL_F16), -2)
    row(diag, PL_2G_VOXELS, -2)
    row(diag, dict(PL_2G_VOXELS, tile_ws_bytes=0), -2)
    row(diag, dict(PL_BELOW_2G, tile_ws_bytes=0), -3)
    row(diag, dict(flags=PL_SC1_NT), -2)                                            # 4 channels per lane
    row(diag, dict(flags=PL_SC1_NT, tile_ws_bytes=0), -2)
    row(diag, dict(C=20), -2)
    row(diag, dict(C=24, flags=F | (2 << 4)), -2)                                   # 12 channels per workgroup
    row(diag, dict(flags=PL_CPL8 | 1), -2)
    row(diag, dict(flags=PL_CPL8), -2)
    row(diag, dict(flags=F | PL_WG128), -2)
    row(diag, dict(tile_ws_bytes=55), -3)
    row(diag, dict(C=128), -2)                                                      # 73 216 bytes of LDS
    row(diag, dict(C=128, tile_ws_bytes=55), -3)
    row(diag, dict(C=256, flags=F | PL_BF16), -2)                                   # 75 264 bytes
    row(diag, dict(C=256, flags=F | PL_BF16 | (2 << 4), tile_ws_bytes=55), -3)
    # ---- fbbev_lift_splat_fused: its four pointers, the plan, the cache pair, the workspace; then the rank build (another family)
    lift = 'lift_splat_fused'
    for k in ('depth', 'context', 'out', 'workspace'):
        row(lift, {k: NULL}, -1)
    for k in ('B', 'N', 'D', 'H', 'W', 'C', 'Z', 'Y', 'X'):
        row(lift, {k: 0}, -1)
    row(lift, PL_2G_POINTS, -1)
    row(lift, dict(PL_2G_POINTS, workspace_bytes=0), -1)
    row(lift, dict(PL_POINTS_BELOW_2G, workspace_bytes=0), -3)
    row(lift, dict(cam_key=NULL), -1)
    row(lift, dict(cache_state=NULL), -1)
    row(lift, dict(cache_state=NULL, workspace_bytes=0), -1)
    row(lift, dict(workspace_bytes=PL_LIFT_WS - 1), -3)
    row(lift, dict(workspace_bytes=PL_LIFT_WS - 1, workspace=P8), -3)
    row(lift, dict(workspace=P8), -2)
    row(lift, dict(workspace=P8, cam_key=NULL, cache_state=NULL), -2)
    row(lift, dict(workspace=P8, workspace_bytes=PL_LIFT_WS), -2)
    # ---- fbbev_pool_zmean / _split / _rows
    for zm in ('pool_zmean', 'pool_zmean_split', 'pool_zmean_rows'):
        out = 'out_rows' if zm == 'pool_zmean_rows' else 'out_mean'
        for k in ('B', 'C', 'Z', 'Y', 'X'):
            row(zm, {k: 0}, -1)
        for k in GATHER7 + [out, 'tile_ws']:
            row(zm, {k: NULL}, -1)
        row(zm, dict(C=18), -2)
        row(zm, dict(C=18, depth=NULL), -1)
        row(zm, dict(C=260), -2)
        row(zm, dict(Y=1, X=6), -2)
        row(zm, {out: P8}, -2)
        row(zm, dict(feat=P8), -2)
        row(zm, PL_2G_VOXELS, -2)
        row(zm, dict(PL_2G_VOXELS, tile_ws_bytes=0), -2)
        row(zm, dict(PL_BELOW_2G, tile_ws_bytes=0), -3)
        row(zm, dict(flags=F | CL), -2)
        row(zm, dict(flags=F | CL, tile_ws_bytes=0), -2)
        row(zm, dict(tile_voxels=512), -2)
        row(zm, dict(tile_voxels=1024, tile_ws_bytes=0), -2)
        row(zm, dict(tile_ws_bytes=55), -3)
        row(zm, dict(tile_ws_bytes=79, tile_voxels=64), -3)
        row(zm, dict(tile_ws_bytes=79, tile_voxels=16), -3)
        row(zm, dict(tile_ws_bytes=31, tile_voxels=256), -3)
        row(zm, dict(C=128), -2)                                                    # 73 216 bytes of LDS: the bound is 64 KiB
        row(zm, dict(C=64, tile_voxels=256), -2)
        row(zm, dict(C=128, tile_ws_bytes=55), -3)
    split = 'pool_zmean_split'
    row(split, dict(z_groups=0), -1)
    row(split, dict(z_groups=65), -1)
    row(split, dict(z_groups=65, C=18), -1)
    row(split, dict(z_groups=2, partial_ws=NULL), -1)
    row(split, dict(z_groups=2, partial_ws=P8), -1)
    row(split, dict(z_groups=2, partial_ws=P8, C=18), -1)
    row(split, dict(z_groups=2, partial_ws_bytes=2 * 16 * 144 * 4 - 1), -3)
    row(split, dict(z_groups=64, partial_ws_bytes=3 * 16 * 144 * 4 - 1), -3)        # more groups than planes: Z of them
    row(split, dict(z_groups=2, partial_ws_bytes=0, C=128), -2)                     # LDS before the partial buffer
    row(split, dict(z_groups=2, partial_ws_bytes=0, tile_ws_bytes=55), -3)
    row(split, dict(B=1 << 25, Z=8, Y=2, X=2, C=32, tile_voxels=64, flags=F | (8 << 4), z_groups=8, partial_ws_bytes=1 << 62), -2)   # 2^31 workgroups
    row(split, dict(B=1 << 25, Z=8, Y=2, X=2, C=32, tile_voxels=64, flags=F | (8 << 4), z_groups=8, partial_ws_bytes=0), -3)
    zrows = 'pool_zmean_rows'
    row(zrows, dict(row_bias=P8), -2)
    row(zrows, dict(row_bias=P8, depth=NULL), -2)                                   # the bias comes before the pointers
    row(zrows, dict(row_bias=P8, B=0), -1)
    row(zrows, dict(row_bias=NULL, tile_ws_bytes=55), -3)
    # ---- fbbev_bev_pool_v2_dense_bwd[_z]
    for bwd in ('bev_pool_v2_dense_bwd', 'bev_pool_v2_dense_bwd_z'):
        for k in ('B', 'N', 'D', 'H', 'W', 'C', 'Z', 'Y', 'X'):
            row(bwd, {k: 0}, -1)
        row(bwd, dict(n_intervals_max=-1), -1)
        for k in ('out_grad', 'depth', 'feat', 'ranks_depth', 'interval_rank', 'interval_starts', 'counts', 'depth_grad', 'feat_grad',
                  'workspace'):
            row(bwd, {k: NULL}, -1)
        row(bwd, dict(C=18), -2)
        row(bwd, dict(C=18, counts=NULL), -1)
        row(bwd, dict(C=260), -2)
        row(bwd, dict(Y=1, X=6), -2)
        for k in ('out_grad', 'feat', 'feat_grad', 'workspace'):
            row(bwd, {k: P8}, -2)
        row(bwd, PL_2G_VOXELS, -2)
        row(bwd, PL_2G_POINTS, -2)
        row(bwd, dict(PL_2G_VOXELS, og_stride_c=4), -2)
        row(bwd, dict(PL_BELOW_2G, og_stride_c=4), -1)
        row(bwd, dict(PL_2G_POINTS, og_stride_c=4), -2)
        row(bwd, dict(PL_POINTS_BELOW_2G, og_stride_c=4), -1)
        row(bwd, dict(PL_BELOW_2G, workspace_bytes=0), -3)
        row(bwd, dict(PL_POINTS_BELOW_2G, workspace_bytes=0), -3)
        row(bwd, dict(og_stride_c=428), -1)
        row(bwd, dict(og_stride_c=434), -1)
        row(bwd, dict(og_stride_b=16 * 432 - 4), -1)
        row(bwd, dict(og_stride_b=16 * 432 + 2), -1)
        row(bwd, dict(og_stride_c=436, og_stride_b=16 * 436 - 4), -1)
        row(bwd, dict(og_stride_c=428, workspace_bytes=0), -1)
        row(bwd, dict(workspace_bytes=PL_BWD_WS - 1), -3)
    bwdz = 'bev_pool_v2_dense_bwd_z'
    row(bwdz, dict(zgrad=NULL), -1)
    row(bwdz, dict(zgrad=NULL, C=18), -1)
    row(bwdz, dict(zgrad=P8), -2)
    row(bwdz, dict(zgrad=P8, B=0), -2)                                              # its alignment comes before the dimensions
    row(bwdz, dict(zgrad=P8, depth=NULL), -2)
    shown = lambda case: {k: (v.value if isinstance(v, ctypes.c_void_p) else v) for k, v in case.items()}   # noqa: E731
    got = [(entry, shown(case), pl_call(lib, entry, case)) for entry, case, _ in table]
    want = [(entry, shown(case), code) for entry, case, code in table]
    assert got == want, [(g, w[2]) for g, w in zip(got, want) if g != w]
    assert {entry for entry, _, _ in table} == set(PL_PARAMS)
    # ---- the host functions, as values: the shipped grid (100 x 100 x 8) and BASELINE configs[2] (6 cameras of 16 x 44 pixels and
    # 59 depth bins, 80 channels, 200 x 200 x 16), the 12 x 12 x 3 grid, non-positive sizes, 2^31 points
    tile, bwd_ws, lift_ws = lib.fbbev_pool_dense_workspace_bytes, lib.fbbev_pool_dense_bwd_workspace_bytes, lib.fbbev_lift_splat_fused_ws_bytes
    assert [tile(*a) for a in ((1, 8, 100, 100), (4, 16, 200, 200), (1, 3, 12, 12), (2, 3, 12, 12), (0, 3, 12, 12), (1, -1, 12, 12),
                               (1, 3, 0, 12), (1, 3, 12, 0))] == PL_TILE_BYTES
    shapes = ((1, 6, 59, 16, 44, 80, 8, 100, 100), (4, 6, 59, 16, 44, 80, 16, 200, 200), (1, 1, 2, 2, 4, 16, 3, 12, 12),
              (2, 1, 2, 2, 4, 16, 3, 12, 12), (1, 2048, 1024, 1024, 1, 16, 3, 12, 12), (1, 2048, 1023, 1024, 1, 16, 3, 12, 12))
    zeros = [tuple(0 if i == k else v for i, v in enumerate(shapes[2])) for k in range(9)]
    assert [bwd_ws(*a) for a in shapes + tuple(zeros)] == PL_BWD_BYTES
    assert [lift_ws(*a) for a in shapes + tuple(zeros)] == PL_LIFT_BYTES
    off = (ctypes.c_size_t * 8)()
    got = []
    for a in shapes + (zeros[0], zeros[5]):
        got.append([lib.fbbev_lift_splat_fused_ws_offsets(*a, ctypes.cast(off, ctypes.c_void_p))] + list(off))
        for i in range(8):
            off[i] = 0
    assert got == PL_LIFT_OFFSETS
    assert lib.fbbev_lift_splat_fused_ws_offsets(*shapes[2], NULL) == -1
    assert (bwd_ws(*shapes[2]), lift_ws(*shapes[2])) == (PL_BWD_WS, PL_LIFT_WS)


PL_TILE_BYTES = [80128, 2560768, 512, 1024, 256, 256, 256, 256]
PL_BWD_BYTES = [26601984, 323144448, 1536, 2560, 8589962496, 8581573888, 256, 256, 256, 256, 256, 256, 256, 256, 256]
PL_LIFT_BYTES = [13680128, 47504128, 1189120, 1321216, 0, 78447119616, 0, 0, 0, 0, 0, 0, 0, 0, 0]
PL_LIFT_OFFSETS = [[0, 0, 996864, 1993728, 2990592, 3987456, 4984320, 5981184, 5981440],
                   [0, 0, 3987456, 7974912, 11962368, 15949824, 19937280, 23924736, 23924992],
                   [0, 0, 256, 512, 768, 1024, 1280, 1536, 1792], [0, 0, 256, 512, 768, 1024, 1280, 1536, 1792], [-1, 0, 0, 0, 0, 0, 0, 0, 0],
                   [0, 0, 8581545984, 17163091968, 25744637952, 34326183936, 42907729920, 51489275904, 51489276160],
                   [-1, 0, 0, 0, 0, 0, 0, 0, 0], [-1, 0, 0, 0, 0, 0, 0, 0, 0]]


# ---- the row-wise linear layers (split-bf16 x3, exact f32, head planes, FFN, tail + FFN) and the convolutions (fp32, 2-D, bf16,
# tiled bf16, dgrad, wgrad): one table, recorded on the launchers before they shared their operand records
RC_IO = ['x', 'x_row_stride', 'weights', 'bias', 'rows', 'in_features', 'out_features']
RC_ADD = ['x', 'x_row_stride', 'addend', 'addend_row_stride', 'addend_period', 'weights', 'bias', 'rows', 'in_features', 'out_features', 'relu']
RC_LN = RC_IO + ['residual', 'residual_row_stride', 'ln_weight', 'ln_bias', 'ln_eps', 'out', 'out_row_stride', 'stream']
RC_TAIL = ['x', 'x_row_stride', 'w0_fragments', 'b0', 'residual0', 'residual0_row_stride', 'ln0_weight', 'ln0_bias', 'ln0_eps',
           'w1_fragments', 'b1', 'w2_fragments', 'b2', 'rows', 'embed', 'hidden', 'ln1_weight', 'ln1_bias', 'ln1_eps']
RC_VOL = ['B', 'Di', 'Hi', 'Wi', 'Cin', 'Do', 'Ho', 'Wo', 'Cout', 'ksize', 'stride', 'pad']
RC_PARAMS = {
    'rows_linear_x3': RC_IO + ['relu', 'out', 'out_row_stride', 'stream'],
    'rows_linear_x3_add': RC_ADD + ['out', 'out_row_stride', 'stream'],
    'rows_linear_x3_train': RC_ADD + ['residual', 'residual_row_stride', 'mask', 'mask_row_stride', 'out', 'out_row_stride', 'stream'],
    'rows_linear_x3_ln': RC_LN,
    'rows_linear_x3_planes': RC_IO + ['tokens_per_image', 'head_dim', 'out', 'stream'],
    'rows_linear_x3_planes_e': RC_IO + ['tokens_per_image', 'head_dim', 'elem_type', 'out', 'stream'],
    'rows_linear_f32': RC_IO + ['relu', 'out', 'out_row_stride', 'stream'],
    'rows_linear_f32_add': RC_ADD + ['out', 'out_row_stride', 'stream'],
    'rows_linear_f32_ln': RC_LN,
    'rows_ffn_x3': ['x', 'x_row_stride', 'w1_fragments', 'b1', 'w2_fragments', 'b2', 'rows', 'in_features', 'hidden', 'out_features',
                    'residual', 'residual_row_stride', 'ln_weight', 'ln_bias', 'ln_eps', 'out', 'out_row_stride', 'stream'],
    'rows_tail_ffn_x3': RC_TAIL + ['out', 'out_row_stride', 'stream'],
    'rows_tail_ffn_x3_planes': RC_TAIL + ['tokens_per_image', 'out', 'stream'],
    'rows_linear_x3_fragments': ['weight', 'in_features', 'out_features', 'fragments', 'fragment_bytes', 'stream'],
    'conv3d_ndhwc': ['x', 'weights', 'bias', 'residual'] + RC_VOL + ['relu', 'transposed', 'out', 'stream'],
    'conv2d_nhwc': ['x', 'weights', 'bias', 'residual', 'B', 'Hi', 'Wi', 'Cin', 'Ho', 'Wo', 'Cout', 'ksize', 'stride', 'pad', 'relu', 'out', 'stream'],
    'conv3d_ndhwc_bf16': ['x', 'weights', 'bias', 'residual'] + RC_VOL + ['relu', 'transposed', 'planar', 'out', 'stream'],
    'conv3d_k3s1_tiled_bf16': ['x', 'weights', 'bias', 'residual', 'B', 'D', 'H', 'W', 'Cin', 'Cout', 'relu', 'out', 'stream'],
    'conv3d_dgrad_ndhwc': ['dy', 'weights', 'bias', 'B', 'Do', 'Ho', 'Wo', 'Cout', 'Di', 'Hi', 'Wi', 'Cin', 'ksize', 'stride', 'pad', 'dx', 'stream'],
    'conv3d_wgrad_ndhwc': ['x', 'dy'] + RC_VOL + ['dw', 'stream'],
    'conv3d_wgrad_ndhwc_ex': ['x', 'dy'] + RC_VOL + ['dw', 'flags', 'ws', 'ws_bytes', 'stream'],
}
# a call that would LAUNCH (so no row below is this alone): 256 rows, 80 -> 80 features (embed 80), hidden 320, every optional operand
# given, an addend for every row, 128 tokens per image in heads of 10 bf16 channels; 3 x 3 x 3, stride 1, padding 1 on one 8 x 8 x 8
# volume (image, tile volume) of 32 -> 32 channels, the deterministic weight gradient; every pointer non-null and 16-byte aligned
RC_BASE = dict(x_row_stride=0, out_row_stride=0, addend_row_stride=0, addend_period=1, residual_row_stride=0, residual0_row_stride=0,
               mask_row_stride=0, rows=256, in_features=80, out_features=80, embed=80, hidden=320, relu=1, ln_eps=1e-5, ln0_eps=1e-5,
               ln1_eps=1e-5, tokens_per_image=128, head_dim=10, elem_type=1, fragment_bytes=1 << 40, B=1, D=8, H=8, W=8, Di=8, Hi=8, Wi=8,
               Cin=32, Do=8, Ho=8, Wo=8, Cout=32, ksize=3, stride=1, pad=1, transposed=0, planar=0, flags=1, ws_bytes=1 << 40,
               stream=DA_NULL)
RC_2G_ROW_TILES = 128 << 31                                          # rows of 2^31 128-row workgroups
RC_2G_BLOCKS_X8 = dict(B=1 << 16, Di=1 << 10, Hi=1 << 10, Wi=1, Do=1 << 10, Ho=1 << 10, Wo=1)   # 2^28 blocks of 256 voxels: x 8 parities
# 2^33 voxels in 2^21 chunks, 64 x 64 blocks of 64 x 64 channels, one tap: 2^33 tasks, four to a workgroup
RC_2G_WGRAD = dict(ksize=1, pad=0, B=1 << 13, Di=1 << 10, Hi=1 << 10, Wi=1, Do=1 << 10, Ho=1 << 10, Wo=1, Cin=4096, Cout=4096)


def rc_call(lib, entry, case):
    """`entry` with RC_BASE's operands, `case` on top of them; 'null': every pointer the entry takes is null unless `case` names it"""
    case = dict(case)
    null = case.pop('null', False)
    args = []
    for name in RC_PARAMS[entry]:
        if name in case:
            args.append(case.pop(name))
        elif name in RC_BASE:
            args.append(RC_BASE[name])
        else:
            args.append(DA_NULL if null else DA_P16)
    assert not case, (entry, 'operands the entry does not take', case)
    return getattr(lib, 'fbbev_' + entry)(*args)


def test_rows_and_conv_entries_keep_their_error_codes():
    """Every entry of the row-wise linear layers and of the convolutions: the code of each argument check and which code wins where
    two defects coincide (the order of an entry's checks is part of the ABI; the rows of
    test_invalid_arguments_return_error_codes_without_touching_the_gpu hold the row-operand rule).  Every row returns BEFORE the
    entry's first runtime call, so this runs without a GPU; below a 2^31-workgroup limit the next thing is a launch, so the limits
    are pinned from the refusing side.  The two host functions are pinned as values."""
    lib = _capi.declare(ctypes.CDLL(_capi.LIB_PATH))
    NULL, P16, P8, P4 = DA_NULL, DA_P16, DA_P8, DA_P4
    table = []
    row = lambda entry, case, code: table.append((entry, case, code))   # noqa: E731
    # ---- fbbev_rows_linear_x3 / _f32 and what their _add and _ln forms check in front
    for fam in ('x3', 'f32'):
        lin, add, ln = f'rows_linear_{fam}', f'rows_linear_{fam}_add', f'rows_linear_{fam}_ln'
        for e in (lin, add, ln):
            row(e, dict(rows=-1), -1)
            row(e, dict(in_features=0), -1)
            row(e, dict(out_features=0), -1)
            row(e, dict(rows=0), 0)
            row(e, dict(rows=0, x=NULL, weights=NULL, out=NULL, bias=NULL), 0)       # the empty call comes before the pointers
            row(e, dict(rows=0, in_features=0, x=NULL), -1)                          # ... and behind the dimensions
            for k in ('x', 'weights', 'out'):
                row(e, {k: NULL}, -1)
            row(e, dict(out=NULL, x=P8), -1)                                         # pointers before the row operands
            row(e, dict(out=NULL, in_features=84), -1)
            row(e, dict(in_features=84), -2)                                         # % 8
            row(e, dict(weights=P8), -2)
            row(e, dict(bias=P8), -2)
            row(e, dict(in_features=84, x_row_stride=80), -1)                        # the row operands before the feature counts
            row(e, dict(rows=RC_2G_ROW_TILES), -2)
            row(e, dict(rows=RC_2G_ROW_TILES, x_row_stride=40), -1)                  # the row operands before the grid
            row(e, dict(rows=RC_2G_ROW_TILES, weights=NULL), -1)
        row(lin, dict(out_features=84, out_row_stride=80), -1)
        row(lin, dict(out_features=82), -2)
        row(lin, dict(rows=RC_2G_ROW_TILES >> 1, out_features=256), -2)              # two output chunks: 2^30 tiles x 2
        row(add, dict(rows=RC_2G_ROW_TILES >> 1, out_features=256), -2)
        row(add, dict(addend=NULL), -1)
        row(add, dict(addend_period=0), -1)
        row(add, dict(addend_period=-1), -1)
        row(add, dict(addend=NULL, rows=-1), -1)
        row(add, dict(addend_period=0, addend=P8), -1)
        row(add, dict(addend=P8, in_features=0), -2)                                 # the addend before in_features <= 0
        row(add, dict(addend_row_stride=82, rows=0), -2)                             # ... and before the empty call
        row(add, dict(addend_row_stride=40, x=NULL), -1)
        row(add, dict(addend=P8, x=NULL), -2)
        row(ln, dict(ln_weight=NULL), -1)
        row(ln, dict(ln_bias=NULL), -1)
        row(ln, dict(ln_bias=NULL, out_features=132), -1)
        row(ln, dict(out_features=132), -2)                                          # a workgroup holds whole rows: <= 128
        row(ln, dict(out_features=256), -2)
        row(ln, dict(out_features=132, residual_row_stride=40), -2)                  # ... before the residual
        row(ln, dict(ln_weight=P8), -2)
        row(ln, dict(ln_bias=P8), -2)
        row(ln, dict(ln_weight=P8, rows=-1), -2)                                     # the LayerNorm operands before rows < 0
        row(ln, dict(ln_weight=P8, rows=0), -2)
        row(ln, dict(ln_weight=NULL, rows=0), -1)
        row(ln, dict(residual=P8, ln_weight=NULL), -1)
        row(ln, dict(residual=NULL, residual_row_stride=40, x=NULL), -1)
    # ---- fbbev_rows_linear_x3_train: the feature counts first, an addend only when there is one (its period then 1), residual, mask
    train = 'rows_linear_x3_train'
    row(train, dict(out_features=0), -1)
    row(train, dict(in_features=0), -1)
    row(train, dict(in_features=0, addend=P8), -1)                                   # the feature counts before the addend
    row(train, dict(out_features=0, residual=P8), -1)
    row(train, dict(addend_period=0), -1)
    row(train, dict(addend_period=0, x=P8), -1)
    row(train, dict(addend=NULL, addend_period=0, x=P8), -2)                         # no addend: its period is not looked at
    row(train, dict(addend=NULL, addend_period=-5, addend_row_stride=3, rows=-1), -1)
    row(train, dict(addend=P8), -2)
    row(train, dict(addend=P8, residual_row_stride=40), -2)
    row(train, dict(residual=P8, mask_row_stride=40), -2)
    row(train, dict(mask=P8, rows=-1), -2)                                           # mask before rows < 0
    row(train, dict(mask=NULL, mask_row_stride=40, residual=NULL, residual_row_stride=40, rows=-1), -1)
    row(train, dict(rows=-1), -1)
    row(train, dict(rows=0), 0)
    row(train, dict(rows=0, mask=P8), -2)
    for k in ('x', 'weights', 'out'):
        row(train, {k: NULL}, -1)
    row(train, dict(in_features=84), -2)
    row(train, dict(rows=RC_2G_ROW_TILES), -2)
    # ---- the head planes: their own dimensions (-1) and divisibility / 16-bit limits (-2), out's alignment, then the shared checks
    for e in ('rows_linear_x3_planes', 'rows_linear_x3_planes_e'):
        row(e, dict(tokens_per_image=0), -1)
        row(e, dict(head_dim=0), -1)
        row(e, dict(out_features=0), -1)
        row(e, dict(tokens_per_image=0, head_dim=11), -1)
        row(e, dict(head_dim=11), -2)                                                # odd
        row(e, dict(head_dim=32), -2)                                                # 80 % 32
        row(e, dict(rows=250), -2)                                                   # rows % tokens_per_image
        row(e, dict(rows=-1), -2)                                                    # ... which a negative count fails first
        row(e, dict(rows=-128), -1)
        row(e, dict(out_features=0x10000, head_dim=16), -2)                          # the 16-bit limits of the packed head width
        row(e, dict(out_features=0x20000, head_dim=0x20000), -2)
        row(e, dict(out_features=0x10000, head_dim=16, x=NULL), -2)
        row(e, dict(head_dim=11, out=P4), -2)
        row(e, dict(out=P4), -2)
        row(e, dict(out=P4, rows=-128), -2)                                          # out's alignment before the shared checks
        row(e, dict(out=P4, x=NULL), -2)
        row(e, dict(rows=0), 0)
        row(e, dict(rows=0, out=NULL, x=NULL), 0)
        for k in ('x', 'weights', 'out'):
            row(e, {k: NULL}, -1)
        row(e, dict(in_features=84), -2)
        row(e, dict(rows=RC_2G_ROW_TILES), -2)
    row('rows_linear_x3_planes', dict(out=P8, x_row_stride=40), -1)                  # 8 bytes do for the entry's own test: x's rows win
    row('rows_linear_x3_planes', dict(out=P8), -2)                                   # ... and the shared checks want 16
    row('rows_linear_x3_planes_e', dict(out=P8, x_row_stride=40), -2)                # the 16-bit planes test 16 bytes themselves
    row('rows_linear_x3_planes_e', dict(out=P8, x_row_stride=40, elem_type=0), -2)
    row('rows_linear_x3_planes_e', dict(out=P4, elem_type=0), -2)
    row('rows_linear_x3_planes_e', dict(elem_type=3), -1)
    row('rows_linear_x3_planes_e', dict(elem_type=-1), -1)
    row('rows_linear_x3_planes_e', dict(elem_type=3, head_dim=11), -1)
    # ---- fbbev_rows_ffn_x3
    ffn = 'rows_ffn_x3'
    for k in ('in_features', 'hidden', 'out_features'):
        row(ffn, {k: 0}, -1)
    row(ffn, dict(rows=-1), -1)
    row(ffn, dict(rows=0), 0)
    row(ffn, dict(rows=0, null=True), 0)
    row(ffn, dict(rows=0, hidden=0), -1)
    for k in ('x', 'w1_fragments', 'b1', 'w2_fragments', 'b2', 'out'):
        row(ffn, {k: NULL}, -1)
    row(ffn, dict(ln_bias=NULL), -1)                                                 # a LayerNorm weight wants its bias
    row(ffn, dict(ln_bias=NULL, x_row_stride=82), -1)
    row(ffn, dict(ln_weight=NULL, ln_bias=NULL, residual=NULL, x=P8), -2)            # no LayerNorm, no residual: fine as far as they go
    row(ffn, dict(residual=NULL, x=P8), -2)                                          # a LayerNorm without a residual is accepted
    row(ffn, dict(b1=NULL, x_row_stride=40), -1)
    row(ffn, dict(in_features=104), -2)                                              # > 96
    row(ffn, dict(in_features=104, x_row_stride=100), -1)                            # the row operands before the shape limits
    row(ffn, dict(in_features=84), -2)
    row(ffn, dict(hidden=96), -2)
    row(ffn, dict(hidden=352), -2)                                                   # % 32 is not enough
    row(ffn, dict(out_features=84), -2)
    row(ffn, dict(out_features=82), -2)
    for k in ('w1_fragments', 'w2_fragments', 'b1', 'b2', 'ln_weight', 'ln_bias'):
        row(ffn, {k: P8}, -2)
    row(ffn, dict(rows=RC_2G_ROW_TILES), -2)
    row(ffn, dict(rows=RC_2G_ROW_TILES, out_row_stride=40), -1)
    row(ffn, dict(rows=RC_2G_ROW_TILES, out=NULL), -1)
    # ---- fbbev_rows_tail_ffn_x3[_planes]
    tail, tail_planes = 'rows_tail_ffn_x3', 'rows_tail_ffn_x3_planes'
    TAIL_PTRS = ('x', 'w0_fragments', 'b0', 'ln0_weight', 'ln0_bias', 'w1_fragments', 'b1', 'w2_fragments', 'b2', 'ln1_weight', 'ln1_bias', 'out')
    for e in (tail, tail_planes):
        row(e, dict(rows=-1), -1)
        row(e, dict(embed=0), -1)
        row(e, dict(hidden=0), -1)
        row(e, dict(rows=0), 0)
        row(e, dict(rows=0, null=True), 0)
        row(e, dict(rows=0, embed=0), -1)
        for k in TAIL_PTRS:
            row(e, {k: NULL}, -1)
        row(e, dict(b0=NULL, x=P8), -1)
        row(e, dict(embed=96), -2)
        row(e, dict(embed=40), -2)                                                   # % 16
        row(e, dict(hidden=96), -2)
        row(e, dict(embed=96, x_row_stride=80), -1)
        for k in TAIL_PTRS[1:-1]:
            row(e, {k: P8}, -2)
        row(e, dict(rows=RC_2G_ROW_TILES), -2)
    row(tail, dict(rows=RC_2G_ROW_TILES, out_row_stride=40), -1)
    row(tail, dict(rows=RC_2G_ROW_TILES, x=NULL), -1)
    row(tail_planes, dict(tokens_per_image=0), -1)
    row(tail_planes, dict(tokens_per_image=-1), -1)
    row(tail_planes, dict(tokens_per_image=0, rows=0), -1)                           # the entry's own test before the empty call
    row(tail_planes, dict(rows=250), -1)                                             # rows % tokens_per_image is BADARG here
    row(tail_planes, dict(rows=250, embed=96), -1)
    row(tail_planes, dict(rows=1 << 31), -2)                                         # 32-bit row arithmetic in the planes' store
    row(tail_planes, dict(rows=1 << 31, x=NULL), -2)                                 # ... both tested before the pointers
    row(tail_planes, dict(rows=250, x=NULL), -1)
    row(tail_planes, dict(rows=(1 << 31) + 1), -1)
    row(tail_planes, dict(rows=1 << 31, tokens_per_image=1 << 31), -2)
    row(tail_planes, dict(rows=1 << 32, tokens_per_image=1 << 31, x=NULL), -2)
    row(tail_planes, dict(rows=RC_2G_ROW_TILES, x_row_stride=40), -2)
    # ---- fbbev_rows_linear_x3_fragments
    frag = 'rows_linear_x3_fragments'
    row(frag, dict(in_features=0), -1)
    row(frag, dict(out_features=0), -1)
    row(frag, dict(weight=NULL), -1)
    row(frag, dict(fragments=NULL), -1)
    row(frag, dict(fragments=NULL, fragment_bytes=0), -1)
    row(frag, dict(fragments=P8), -3)
    row(frag, dict(fragment_bytes=65535), -3)
    row(frag, dict(fragment_bytes=393215, in_features=129, out_features=257), -3)
    row(frag, dict(fragments=P8, in_features=0), -1)
    # ---- the forward convolutions: dimensions (-1), the window (-2: kernel size 2 only in fp32 3-D), geometry (-1), the empty batch,
    # pointers (-1), channels and alignment (-2), 2^31 workgroups (-2)
    c3, c2, cb, ct = 'conv3d_ndhwc', 'conv2d_nhwc', 'conv3d_ndhwc_bf16', 'conv3d_k3s1_tiled_bf16'
    for e in (c3, cb):
        row(e, dict(B=-1), -1)
        for k in RC_VOL[1:9]:
            row(e, {k: 0}, -1)
        row(e, dict(Di=0, ksize=4), -1)
        for bad in (dict(ksize=0), dict(ksize=4), dict(stride=0), dict(stride=3), dict(pad=-1), dict(pad=2)):
            row(e, bad, -2)
            row(e, dict(bad, Do=7), -2)                                              # the window before the geometry
            row(e, dict(bad, transposed=1, x=NULL), -1)                              # the transposed route sets its own window
        for k in ('Do', 'Ho', 'Wo'):
            row(e, {k: 7}, -1)
            row(e, {k: 7, 'B': 0}, -1)                                               # the geometry before the empty batch
            row(e, {k: 16, 'transposed': 1}, -1)
        row(e, dict(B=0, ksize=4), -2)
        row(e, dict(B=0), 0)
        row(e, dict(B=0, null=True), 0)
        row(e, dict(B=0, transposed=1, null=True), 0)
        for k in ('x', 'weights', 'bias', 'out'):
            row(e, {k: NULL}, -1)
            row(e, {k: P8}, -2)
        row(e, dict(residual=P8), -2)
        row(e, dict(Cin=24), -2)
        row(e, dict(Cin=24, out=NULL), -1)
        row(e, dict(RC_2G_BLOCKS_X8, transposed=1), -2)
        row(e, dict(RC_2G_BLOCKS_X8, transposed=1, Cout=48), -2)
        row(e, dict(RC_2G_BLOCKS_X8, transposed=1, bias=NULL), -1)
    row(c3, dict(ksize=2), -1)                                                       # fp32 has the 2 x 2 x 2 kernel: 8 -> 9 voxels is its geometry's refusal
    row(c3, dict(ksize=2, stride=2, pad=0, Do=4, Ho=4, Wo=4, x=NULL), -1)
    row(cb, dict(ksize=2), -2)
    row(cb, dict(ksize=2, stride=2, pad=0, Do=4, Ho=4, Wo=4, x=NULL), -2)
    row(cb, dict(Cin=16), -2)
    row(cb, dict(planar=1), -1)                                                      # planar: one plane in, one plane out instead of the depth geometry
    row(cb, dict(planar=1, Di=1, Do=1, x=NULL), -1)
    row(cb, dict(planar=1, Di=1, Do=1, Cin=16), -2)                                  # ... accepted as far as the channels
    row(cb, dict(planar=1, Di=1, Do=2), -1)
    row(cb, dict(planar=1, Di=3, Do=1, pad=0, Ho=6, Wo=6, Cin=16), -1)               # (where the depth geometry itself would hold)
    row(cb, dict(planar=1, Di=1, Do=1, Ho=7, Cin=16), -1)
    row(cb, dict(planar=1, transposed=1), -1)
    row(cb, dict(planar=1, transposed=1, Di=1, Do=1, ksize=9), -1)
    row(cb, dict(planar=1, Di=1, Do=1, ksize=2), -2)
    row(c2, dict(B=-1), -1)
    for k in ('Hi', 'Wi', 'Cin', 'Ho', 'Wo', 'Cout'):
        row(c2, {k: 0}, -1)
    for bad in (dict(ksize=0), dict(ksize=2), dict(ksize=4), dict(stride=0), dict(stride=3), dict(pad=-1), dict(pad=2)):
        row(c2, bad, -2)
        row(c2, dict(bad, Ho=7), -2)
        row(c2, dict(bad, Hi=0), -1)
    for k in ('Ho', 'Wo'):
        row(c2, {k: 7}, -1)
        row(c2, {k: 7, 'B': 0}, -1)
    row(c2, dict(B=0), 0)
    row(c2, dict(B=0, null=True), 0)
    for k in ('x', 'weights', 'bias', 'out'):
        row(c2, {k: NULL}, -1)
        row(c2, {k: P8}, -2)
    row(c2, dict(residual=P8), -2)
    row(c2, dict(Cin=24), -2)
    row(c2, dict(Cin=24, x=NULL), -1)
    row(ct, dict(B=-1), -1)
    for k in ('D', 'H', 'W', 'Cin', 'Cout'):
        row(ct, {k: 0}, -1)
    row(ct, dict(B=0), 0)
    row(ct, dict(B=0, null=True), 0)
    row(ct, dict(B=0, D=0), -1)
    for k in ('x', 'weights', 'bias', 'out'):
        row(ct, {k: NULL}, -1)
        row(ct, {k: P8}, -2)
    row(ct, dict(residual=P8), -2)
    row(ct, dict(Cin=16), -2)
    row(ct, dict(Cin=16, bias=NULL), -1)
    row(ct, dict(B=1 << 20, D=1 << 12, H=16, W=8), -2)                               # 2^31 tiles of 4 x 8 x 8
    row(ct, dict(B=1 << 20, D=1 << 12, H=16, W=8, out=NULL), -1)
    # ---- dgrad (the forward's checks; its kernel reads dy, so the 16-channel rule is Cout's) and wgrad
    dg, wg, wgx = 'conv3d_dgrad_ndhwc', 'conv3d_wgrad_ndhwc', 'conv3d_wgrad_ndhwc_ex'
    for e in (dg, wg, wgx):
        ex = dict(flags=0) if e == wgx else {}
        row(e, dict(ex, B=-1), -1)
        for k in RC_VOL[1:9]:
            row(e, dict(ex, **{k: 0}), -1)
        for bad in (dict(ksize=0), dict(ksize=4), dict(stride=0), dict(stride=3), dict(pad=-1), dict(pad=2)):
            row(e, dict(ex, **bad), -2)
            row(e, dict(ex, Do=7, **bad), -2)
            row(e, dict(ex, Di=0, **bad), -1)
        row(e, dict(ex, ksize=2), -1)                                                # the 2 x 2 x 2 kernel is known: its geometry refuses
        for k in ('Do', 'Ho', 'Wo'):
            row(e, dict(ex, **{k: 7}), -1)
            row(e, dict(ex, B=0, **{k: 7}), -1)
        row(e, dict(ex, B=0), 0)
        row(e, dict(ex, B=0, null=True), 0)
    for k in ('dy', 'weights', 'bias', 'dx'):
        row(dg, {k: NULL}, -1)
        row(dg, {k: P8}, -2)
    row(dg, dict(Cout=24), -2)
    row(dg, dict(Cout=24, dx=NULL), -1)
    for e in (wg, wgx):
        for k in ('x', 'dy', 'dw'):
            row(e, {k: NULL}, -1)
        for k in ('x', 'dy'):
            row(e, {k: P8}, -2)
        row(e, dict(Cin=30), -2)
        row(e, dict(Cout=30), -2)
        row(e, dict(Cin=30, dw=NULL), -1)
        row(e, dict(RC_2G_WGRAD, flags=0) if e == wgx else RC_2G_WGRAD, -2)
    row(wgx, dict(RC_2G_WGRAD, ws_bytes=1 << 62), -2)
    row(wgx, RC_2G_WGRAD, -3)                                                        # (2^57 bytes of partial sums: the workspace comes first)
    row(wgx, dict(B=0, Di=0), 0)                                                     # deterministic: the empty batch before everything
    row(wgx, dict(B=0, ws=NULL, ksize=4), 0)
    row(wgx, dict(ws=NULL), -1)
    row(wgx, dict(ws=NULL, ws_bytes=0), -1)
    row(wgx, dict(ws_bytes=221183), -3)
    row(wgx, dict(ws_bytes=221183, Di=0), -3)                                        # the workspace before the shape
    row(wgx, dict(ws=NULL, Di=0), -1)
    row(wgx, dict(Di=0), -1)
    row(wgx, dict(ksize=4), -2)
    row(wgx, dict(flags=0, ws=NULL, ws_bytes=0, x=P8), -2)                           # the atomic route takes no workspace
    shown = lambda case: {k: (v.value if isinstance(v, ctypes.c_void_p) else v) for k, v in case.items()}   # noqa: E731
    got = [(entry, shown(case), rc_call(lib, entry, case)) for entry, case, _ in table]
    want = [(entry, shown(case), code) for entry, case, code in table]
    assert got == want, [(g, w[2]) for g, w in zip(got, want) if g != w]
    assert {entry for entry, _, _ in table} == set(RC_PARAMS)
    frag_bytes, ws_bytes = lib.fbbev_rows_linear_x3_fragment_bytes, lib.fbbev_conv3d_wgrad_ws_bytes
    assert [frag_bytes(i, o) for i, o in ((80, 80), (128, 128), (129, 128), (80, 129), (129, 257), (0, 80), (80, 0), (-1, -1))] == \
        [65536, 65536, 131072, 131072, 393216, 0, 0, 0]
    assert [ws_bytes(*a) for a in ((1, 8, 8, 8, 32, 32, 3, 1), (2, 9, 9, 9, 16, 32, 3, 1), (1, 8, 8, 8, 32, 32, 3, 0), (0, 8, 8, 8, 32, 32, 3, 1),
                                  (1, 8, 8, 8, 32, 32, 0, 1), (1, 8, 8, 0, 32, 32, 3, 1), (1, 128, 128, 128, 80, 80, 1, 1))] == \
        [221184, 331776, 0, 0, 0, 0, 13107200]
