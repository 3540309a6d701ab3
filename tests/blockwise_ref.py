"""Oracle of the block-scaled fp8 GEMM (conch_amd.ops.quantization.block_fp8.scaled_gemm_blockwise).

Every 128-wide K block's dot product is taken in float64 (exact for e4m3fn operands: a product has at most 8 significant bits,
a block sum of 128 of them stays far inside float64's 53), multiplied by its scales in float64 and summed over the blocks.  The
result is rounded to fp32, then to the output dtype (RNE), and the bias is added in the output dtype, as scaled_gemm's oracle
does it (oracle/reference.py, scaled_gemm_ref).
"""

from __future__ import annotations

import torch

BLOCK = 128


def blockwise_terms(a: torch.Tensor, b: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                    acc_dtype: torch.dtype = torch.float64, magnitude: bool = False):
    """(sum_kb s * dot_kb, sum_kb |s| * (|a_kb| @ |b_kb|) or None) in `acc_dtype`, on the operands' device.  a: [M, K], b: [K, N]
    (any float dtype), scale_a: [M, K/128], scale_b: [ceil(N/128), K/128]."""
    m, k = a.shape
    n = b.shape[1]
    kb = k // BLOCK
    af, bf = a.to(acc_dtype), b.to(acc_dtype)
    sa = scale_a.to(acc_dtype)
    sb = scale_b.to(acc_dtype).repeat_interleave(BLOCK, dim=0)[:n]  # [N, K/128]
    acc = torch.zeros((m, n), dtype=acc_dtype, device=a.device)
    mag = torch.zeros_like(acc) if magnitude else None
    for j in range(kb):
        blk = slice(j * BLOCK, (j + 1) * BLOCK)
        s = sa[:, j : j + 1] * sb[:, j].unsqueeze(0)
        acc += s * (af[:, blk] @ bf[blk, :])
        if magnitude:
            mag += s.abs() * (af[:, blk].abs() @ bf[blk, :].abs())
    return acc, mag


def blockwise_gemm_ref(a: torch.Tensor, b: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor, out_dtype: torch.dtype,
                       bias: torch.Tensor | None = None, acc_dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """C = out_dtype(fp32(sum_kb (scale_a[m, kb] * scale_b[n // 128, kb]) * dot(a[m, kb block], b[kb block, n]))) (+ bias)."""
    acc, _ = blockwise_terms(a, b, scale_a, scale_b, acc_dtype)
    res = acc.to(torch.float32).to(out_dtype)
    if bias is not None:
        res = res + bias.to(res.device)
    return res
