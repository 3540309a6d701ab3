"""Block-scaled fp8 (DeepSeek-V3 format), public API: the GEMM, the activation feeder and the offline weight quantiser.

    x_q, x_s = per_token_group_fp8_quant(x)                 # [M, K] e4m3fn, [M, K/128] fp32 ("1x128")
    w_q, w_s = blockwise_fp8_quant_weights(w)               # [N, K] e4m3fn, [ceil(N/128), K/128] fp32 ("128x128")
    y = scaled_gemm_blockwise(x_q, w_q.T, x_s, w_s, torch.bfloat16)

A checkpoint's `weight` / `weight_scale_inv` pair is (w_q, w_s) as it is stored.
"""

from __future__ import annotations

import torch

from conch_amd.kernels.quantization.fp8 import dynamic_scaled_fp8_quant_launcher
from conch_amd.kernels.quantization.gemm_blockwise import BLOCK, check_blockwise_args, launch_checked

_FP8 = torch.float8_e4m3fn
_FP8_MAX = 448.0


def scaled_gemm_blockwise(a: torch.Tensor, b: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                          output_dtype: torch.dtype, bias: torch.Tensor | None = None) -> torch.Tensor:
    """cast(sum_kb (scale_a[m, kb] * scale_b[n // 128, kb]) * dot(a[m, kb block], b[kb block, n])) (+ bias, in the output dtype).

    a: [M, K] float8_e4m3fn, K-contiguous.  b: [K, N] float8_e4m3fn with b.stride(0) == 1 (w.T of a [N, K] weight).
    scale_a: [M, K/128] fp32, scale_b: [ceil(N/128), K/128] fp32, any strides.  K % 128 == 0; M, N arbitrary.
    """
    dims = check_blockwise_args(a, b, scale_a, scale_b, output_dtype, bias)
    out = torch.empty(dims[:2], dtype=output_dtype, device=a.device)
    launch_checked(out, a, b, scale_a, scale_b, bias, dims)
    return out


def per_token_group_fp8_quant(x: torch.Tensor, group_size: int = BLOCK) -> tuple[torch.Tensor, torch.Tensor]:
    """Dynamic fp8 quantisation of every `group_size` elements of the last dimension: scale = absmax / 448 (1.0 for an all-zero
    group), q = RNE(clamp(x * (1 / scale))) -- the per-token dynamic quantisation of `scaled_fp8_quant`, applied to the groups.
    Returns (x_q shaped like x, scale of shape x.shape[:-1] + (K / group_size,))."""
    if group_size != BLOCK:
        raise ValueError(f"per_token_group_fp8_quant: group_size must be {BLOCK} (got {group_size})")
    if x.dim() < 1 or x.shape[-1] == 0 or x.shape[-1] % group_size:
        raise ValueError(f"per_token_group_fp8_quant: the last dimension ({tuple(x.shape)}) must be a positive multiple of {group_size}")
    groups = x.shape[-1] // group_size
    x = x.contiguous()
    rows = x.numel() // group_size
    q = torch.empty(x.shape, dtype=_FP8, device=x.device)
    scale = torch.empty((*x.shape[:-1], groups), dtype=torch.float32, device=x.device)
    if rows:
        dynamic_scaled_fp8_quant_launcher(q.view(rows, group_size), scale.view(rows), x.view(rows, group_size))
    return q, scale


def blockwise_fp8_quant_weights(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Offline weight quantiser (torch ops, on w's device): one scale per 128 x 128 block, scale = absmax / 448 (1.0 for an
    all-zero block), q = RNE(clamp(w * (1 / scale))).  w: [N, K], K % 128 == 0.  Returns (w_q [N, K] float8_e4m3fn,
    scale [ceil(N/128), K/128] fp32); the ragged last row block takes its absmax over the rows it has."""
    if w.dim() != 2 or w.shape[1] == 0 or w.shape[1] % BLOCK:
        raise ValueError(f"blockwise_fp8_quant_weights: w must be [N, K] with K a positive multiple of {BLOCK} (got {tuple(w.shape)})")
    n, k = w.shape
    nb, kb = (n + BLOCK - 1) // BLOCK, k // BLOCK
    wf = w.to(torch.float32)
    padded = wf.new_zeros((nb * BLOCK, k))
    padded[:n] = wf.abs()
    absmax = padded.view(nb, BLOCK, kb, BLOCK).amax(dim=(1, 3))
    scale = torch.where(absmax > 0, absmax / _FP8_MAX, torch.ones_like(absmax))
    inv = scale.reciprocal().repeat_interleave(BLOCK, dim=0)[:n].repeat_interleave(BLOCK, dim=1)
    q = (wf * inv).clamp(min=-_FP8_MAX, max=_FP8_MAX).to(_FP8)
    return q, scale
