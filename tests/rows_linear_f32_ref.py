"""Host reference of the exact-fp32 row-wise linear layers (fbbev_rows_linear_f32*, contract in include/fbbev.h), written with torch
element-wise float64 operations only: it runs on the CPU or, over row chunks, on the GPU, and shares no code with the kernel under
test.  `fmaf32` is an exact fp32 fmaf (the float64 product of two floats is exact; the sum is rounded to odd through its TwoSum
error, then rounded once to float32); tests/test_emu_rows_linear_f32.py pins it against libm."""
import torch


def fmaf32(a, b, c):
    """float32 tensors -> float32, == libm fmaf element-wise"""
    a, b, c = a.double(), b.double(), c.double()
    p = a * b                              # exact: 24 + 24 bits
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)          # TwoSum: the exact error of s
    fix = (e != 0) & ((s.contiguous().view(torch.int64) & 1) == 0) & torch.isfinite(s)
    inf = torch.full_like(s, float('inf'))
    s = torch.where(fix, torch.nextafter(s, torch.where(e > 0, inf, -inf)), s)   # round to odd
    return s.float()                       # one final rounding to nearest


def host_chain(x, w, order, bias=None, relu=False, residual=None, addend=None, chunk=16384):
    """steps 1-3 of the contract: x (R, I), w (O, I) float32, `order` from fbbev_rows_linear_f32_k_order -> (R, O) float32.
    addend (P, I): rows are x[r] + addend[r % P] (one fp32 add)."""
    R, O = x.shape[0], w.shape[0]
    out = torch.empty((R, O), dtype=torch.float32, device=x.device)
    wt = w.t().contiguous()                                            # (I, O)
    for r0 in range(0, R, chunk):
        xr = x[r0:r0 + chunk]
        if addend is not None:
            idx = torch.arange(r0, r0 + xr.shape[0], device=x.device) % addend.shape[0]
            xr = xr + addend[idx]
        xr = xr.contiguous()
        acc = torch.zeros((xr.shape[0], O), dtype=torch.float32, device=x.device)
        for k in order:
            acc = fmaf32(wt[k][None, :].expand_as(acc).contiguous(), xr[:, k, None].expand_as(acc).contiguous(), acc)
        if bias is not None:
            acc = acc + bias
        if residual is not None:
            acc = acc + residual[r0:r0 + chunk]
        out[r0:r0 + chunk] = acc.relu() if relu else acc
    return out
