"""fb_bev_amd -- MI355X (gfx950) native forward-backward view transformation of FB-OCC.

Only the hot path lives here: HIP kernels behind the C ABI of
include/fbbev.h (csrc/), and the host-side mirrors of the reference's operator interface:
  bev_pool_v2_ext   <-> mmdet3d.ops.bev_pool_v2.bev_pool_v2_ext        (compiled ext in the reference)
  bev_pool          <-> mmdet3d/ops/bev_pool_v2/bev_pool.py
  view_transformer  <-> fbbev/view_transformation/forward_projection/view_transformer.py
  ms_deform_attn    <-> mmcv._ext.ms_deform_attn_* + multi_scale_deformable_attn_function.py
There is no CPU fallback: ops raise if libfbbev_hip.so is missing or tensors are not on the GPU.
"""
__version__ = '0.1.0'

_deterministic_override = None


def set_deterministic(mode):
    """Deterministic mode of the library's backward kernels: True forces it on, False off, None follows torch
    (deterministic_enabled).  Process-wide, like torch.use_deterministic_algorithms."""
    global _deterministic_override
    if mode is not None and not isinstance(mode, bool):
        raise TypeError('set_deterministic takes True, False or None')
    _deterministic_override = mode


def deterministic_enabled():
    """True when the library's gradients must be bit-reproducible: set_deterministic(True), or -- with no override --
    torch.are_deterministic_algorithms_enabled() or torch.backends.cudnn.deterministic (what the reference's
    tools/train.py --deterministic sets).  Read on every call, so the mode can change inside one process."""
    if _deterministic_override is not None:
        return _deterministic_override
    import torch
    return bool(torch.are_deterministic_algorithms_enabled() or torch.backends.cudnn.deterministic)


def set_rows_linear_mode(name):
    """Route of the backward projection's row-wise linear layers: 'x3' (split-operand bf16 MFMA, the default), 'f32' (vendor fp32
    GEMM) or 'f32_mfma' (exact fp32 on the FP32 MFMA, in inference and under autograd: the arithmetic contracts of fbbev_rows_linear_f32
    and fbbev_rows_wgrad_f32 in include/fbbev.h).
    Returns the previous mode; `rows_linear.set_mode` is the same switch.  FBBEV_ROWS_LINEAR only sets the initial mode."""
    from . import rows_linear
    return rows_linear.set_mode(name)
