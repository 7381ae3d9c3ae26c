"""Host reference of fbbev_rows_wgrad_f32 (contract in include/fbbev.h): the two-stage chain, built on the exact fp32 fmaf of
tests/rows_linear_f32_ref.py.  Vectorised over the slices -- the S partial results are one (S, O, I) tensor stepped L times -- so a
full-size case (160 000 rows) costs seconds on the device the tensors live on.  Shares no code with the kernel under test."""
import torch

from rows_linear_f32_ref import fmaf32


def two_stage_chain(gy, x, L, bias=True):
    """gy (R, O), x (R, I) float32, L = fbbev_rows_wgrad_f32_slice_rows(R, I, O) -> (grad_weight (O, I), grad_bias (O) or None).
    Stage 1: per slice one fmaf chain over its rows in ascending order (rows beyond R are zeros: fmaf(0, 0, p) == p up to the sign of
    a zero, which the contract leaves open); stage 2: plain fp32 adds of the partial results in ascending slice order."""
    R, O = gy.shape
    I = x.shape[1]
    assert L > 0 and L % 4 == 0 and x.shape[0] == R
    S = max(1, (R + L - 1) // L)
    g3 = torch.zeros((S * L, O), dtype=torch.float32, device=gy.device)
    x3 = torch.zeros((S * L, I), dtype=torch.float32, device=gy.device)
    g3[:R] = gy
    x3[:R] = x
    g3, x3 = g3.view(S, L, O), x3.view(S, L, I)
    p = torch.zeros((S, O, I), dtype=torch.float32, device=gy.device)
    q = torch.zeros((S, O), dtype=torch.float32, device=gy.device)
    for t in range(L):
        a = g3[:, t, :, None].expand(S, O, I).contiguous()
        b = x3[:, t, None, :].expand(S, O, I).contiguous()
        p = fmaf32(a, b, p)
        if bias:
            q = q + g3[:, t]                                           # one fp32 add == fmaf(gy, 1, q)
    gw, gb = p[0].clone(), q[0].clone()
    for s in range(1, S):
        gw = gw + p[s]
        gb = gb + q[s]
    return gw, (gb if bias else None)
