"""Launcher of the block-scaled fp8 GEMM (C-ABI seam: conch_scaled_gemm_blockwise, csrc/gemm_blockscale.hip).

Format of DeepSeek-V3 and most current fp8 checkpoints: `a` [M, K] e4m3fn with one fp32 scale per row per 128 elements of K
(`scale_a` [M, K/128]), `b` [K, N] e4m3fn -- the transpose of a K-contiguous [N, K] weight -- with one fp32 scale per 128 x 128
block (`scale_b` [ceil(N/128), K/128]).  Every argument is checked here, before anything is launched.
"""

from __future__ import annotations

import ctypes

import torch

from conch_amd import _C

BLOCK = 128
_OUT_DTYPES = (torch.bfloat16, torch.float16)


def check_blockwise_args(a: torch.Tensor, b: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                         output_dtype: torch.dtype, bias: torch.Tensor | None) -> tuple[int, int, int, int, int]:
    """Refuse what the kernels do not take (ValueError; NotImplementedError for e4m3fnuz); return (M, N, K, lda, ldb)."""
    for name, t in (("a", a), ("b", b)):
        if t.dtype == torch.float8_e4m3fnuz:
            raise NotImplementedError(f"scaled_gemm_blockwise: {name} is float8_e4m3fnuz; gfx950 runs OCP float8_e4m3fn only")
        if t.dtype != torch.float8_e4m3fn:
            raise ValueError(f"scaled_gemm_blockwise: {name} must be float8_e4m3fn (got {t.dtype})")
        if t.dim() != 2:
            raise ValueError(f"scaled_gemm_blockwise: {name} must be 2-D (got shape {tuple(t.shape)})")
    if output_dtype not in _OUT_DTYPES:
        raise ValueError(f"scaled_gemm_blockwise: output_dtype must be bfloat16 or float16 (got {output_dtype})")
    m, k = a.shape
    k2, n = b.shape
    if k != k2:
        raise ValueError(f"scaled_gemm_blockwise: a {tuple(a.shape)} and b {tuple(b.shape)} disagree on K")
    if k == 0 or k % BLOCK:
        raise ValueError(f"scaled_gemm_blockwise: K={k} must be a positive multiple of {BLOCK}")
    # K-contiguous rows of a and of b's [N, K] weight (b = w.T).  K >= 128, so the K strides always matter; the row strides mean
    # nothing for a single row (M == 1 / N == 1), which is then read as K contiguous bytes
    if a.stride(1) != 1:
        raise ValueError("scaled_gemm_blockwise: a must be K-contiguous (a.stride(1) == 1)")
    if b.stride(0) != 1:
        raise ValueError("scaled_gemm_blockwise: b must be the transpose of a K-contiguous [N, K] weight (b.stride(0) == 1)")
    lda = a.stride(0) if m > 1 else k
    ldb = b.stride(1) if n > 1 else k
    if lda % 16 or ldb % 16:
        raise ValueError(f"scaled_gemm_blockwise: operand row strides must be multiples of 16 bytes (a: {lda}, b: {ldb})")
    if a.data_ptr() % 16 or b.data_ptr() % 16:
        raise ValueError("scaled_gemm_blockwise: a and b must start on 16-byte boundaries (the kernels load 16-byte chunks)")
    kb = k // BLOCK
    want_sa, want_sb = (m, kb), ((n + BLOCK - 1) // BLOCK, kb)
    for name, s, want in (("scale_a", scale_a, want_sa), ("scale_b", scale_b, want_sb)):
        if s.dtype != torch.float32:
            raise ValueError(f"scaled_gemm_blockwise: {name} must be float32 (got {s.dtype})")
        if tuple(s.shape) != want:
            raise ValueError(f"scaled_gemm_blockwise: {name} has shape {tuple(s.shape)}, want {want}")
    if bias is not None:
        if bias.dtype != output_dtype:
            raise ValueError(f"scaled_gemm_blockwise: bias must be {output_dtype} (got {bias.dtype})")
        if tuple(bias.shape) != (n,):
            raise ValueError(f"scaled_gemm_blockwise: bias has shape {tuple(bias.shape)}, want ({n},)")
    devices = {t.device for t in (a, b, scale_a, scale_b, bias) if t is not None}
    if len(devices) != 1:
        raise ValueError(f"scaled_gemm_blockwise: tensors on different devices ({sorted(map(str, devices))})")
    return m, n, k, lda, ldb


def scaled_gemm_blockwise_launcher(output: torch.Tensor, a: torch.Tensor, b: torch.Tensor, scale_a: torch.Tensor,
                                   scale_b: torch.Tensor, bias: torch.Tensor | None = None) -> None:
    """output[m, n] = cast(sum_kb scale_a[m, kb] * scale_b[n // 128, kb] * dot(a[m, kb block], b[kb block, n])) (+ bias)."""
    launch_checked(output, a, b, scale_a, scale_b, bias, check_blockwise_args(a, b, scale_a, scale_b, output.dtype, bias))


def launch_checked(output: torch.Tensor, a: torch.Tensor, b: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                   bias: torch.Tensor | None, dims: tuple[int, int, int, int, int]) -> None:
    """The launch behind check_blockwise_args (whose result `dims` is)."""
    m, n, k, lda, ldb = dims
    _C.require_device(output, a, b, scale_a, scale_b, bias)
    if tuple(output.shape) != (m, n) or (output.stride(1) != 1 and n > 1):
        raise ValueError(f"scaled_gemm_blockwise: output must be a row-major ({m}, {n}) tensor")
    if bias is not None and bias.stride(0) != 1:
        bias = bias.contiguous()
    ldc = output.stride(0) if m > 1 else n
    with _C.on_device_of(output, a, b, scale_a, scale_b, bias):
        status = _C.load().conch_scaled_gemm_blockwise(
            _C.ptr(output), _C.ptr(a), _C.ptr(b), _C.ptr(scale_a), _C.ptr(scale_b), _C.ptr(bias),
            m, n, k, lda, ldb, ldc,
            scale_a.stride(0), scale_a.stride(1), scale_b.stride(0), scale_b.stride(1),
            _C.dtype_id(output.dtype), _C.current_stream_handle(a.device),
        )
    _C.check(status, "scaled_gemm_blockwise")


def workspace_bytes(m: int, n: int, k: int) -> int:
    """Scratch bound of one call of this shape (pass it to `_C.reserve_scratch` before a graph capture)."""
    return int(_C.load().conch_scaled_gemm_blockwise_workspace_bytes(m, n, k))


def plan(m: int, n: int, k: int) -> tuple[int, int]:
    """(kernel, K slices) the dispatcher picks for contiguous operands of this shape under the current tuning keys: kernel
    1 = 128x128 tiles, 2 = tiles with split-K, 3 = the decode kernel.  Host-only: needs no GPU."""
    kernel, splits = ctypes.c_int(0), ctypes.c_int(0)
    _C.check(_C.load().conch_debug_blockwise_plan(m, n, k, ctypes.byref(kernel), ctypes.byref(splits)), "conch_debug_blockwise_plan")
    return kernel.value, splits.value
