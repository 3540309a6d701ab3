"""Block-scaled fp8 GEMM without a GPU: the oracle against scaled_gemm's, the weight quantiser, the activation feeder's definition,
argument validation and the dispatcher's picks (conch_debug_blockwise_plan is host-only)."""

from __future__ import annotations

import pytest
import torch

from conch_amd import _C
from conch_amd.kernels.quantization import gemm_blockwise
from conch_amd.ops.quantization.block_fp8 import blockwise_fp8_quant_weights, per_token_group_fp8_quant, scaled_gemm_blockwise
from oracle.reference import dynamic_scaled_fp8_quant_ref, scaled_gemm_ref
from tests.blockwise_ref import blockwise_gemm_ref

FP8 = torch.float8_e4m3fn


def _small_ints(shape, gen):
    return torch.randint(-4, 5, shape, generator=gen).to(torch.float32).to(FP8)


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize(("m", "n", "k"), [(1, 128, 128), (7, 200, 384), (33, 576, 1024)])
def test_oracle_equals_scaled_gemm_ref_under_uniform_scales(m, n, k, out_dtype):
    gen = torch.Generator().manual_seed(m * 1000 + n + k)
    a = _small_ints((m, k), gen)
    w = _small_ints((n, k), gen)
    ca, cb = 0.5, 2.0 ** -3
    sa = torch.full((m, k // 128), ca)
    sb = torch.full(((n + 127) // 128, k // 128), cb)
    bias = torch.randint(-8, 9, (n,), generator=gen).to(out_dtype)
    got = blockwise_gemm_ref(a, w.T, sa, sb, out_dtype, bias)
    want = scaled_gemm_ref(a, w.T, torch.full((m, 1), ca), torch.full((n, 1), cb), out_dtype, bias)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_oracle_scales_every_block_before_the_sum():
    """Different scales per block: the oracle is not scale-after-sum (what an epilogue-only kernel would compute)."""
    a = torch.ones((1, 256)).to(FP8)
    w = torch.ones((1, 256)).to(FP8)
    sa = torch.tensor([[1.0, 2.0]])
    sb = torch.tensor([[1.0, 4.0]])
    got = blockwise_gemm_ref(a, w.T, sa, sb, torch.float32)
    assert got.item() == 128 * 1.0 + 128 * 8.0


@pytest.mark.parametrize(("n", "k"), [(128, 128), (200, 256), (576, 384)])
def test_weight_quantiser_against_a_direct_loop(n, k):
    gen = torch.Generator().manual_seed(n + k)
    w = torch.randn((n, k), generator=gen).to(torch.bfloat16)
    w[:128, :128] = 0  # an all-zero block: scale 1
    q, s = blockwise_fp8_quant_weights(w)
    assert q.dtype == FP8 and q.shape == (n, k)
    assert s.dtype == torch.float32 and s.shape == ((n + 127) // 128, k // 128)
    for bi in range(s.shape[0]):
        for bj in range(s.shape[1]):
            blk = w[bi * 128 : (bi + 1) * 128, bj * 128 : (bj + 1) * 128].to(torch.float32)
            amax = blk.abs().max()
            scale = amax / 448.0 if amax > 0 else torch.tensor(1.0)
            assert s[bi, bj].item() == scale.item()
            want = (blk * scale.reciprocal()).clamp(-448.0, 448.0).to(FP8)
            assert torch.equal(q[bi * 128 : (bi + 1) * 128, bj * 128 : (bj + 1) * 128].view(torch.uint8), want.view(torch.uint8))
    assert s[0, 0].item() == 1.0


def _host_row_quant(out, scale_out, x):
    """Stand-in for the per-token quant launcher on host tensors: the oracle's arithmetic, written into the caller's buffers."""
    assert out.shape == x.shape and x.shape[1] == 128 and x.is_contiguous() and scale_out.shape == (x.shape[0],)
    q, s = dynamic_scaled_fp8_quant_ref(x)
    out.copy_(q)
    scale_out.copy_(s.reshape(-1))


@pytest.mark.parametrize("layout", ["contiguous", "transposed", "3d"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_group_quant_is_the_per_group_definition(dtype, layout, monkeypatch):
    """per_token_group_fp8_quant's own view / shape logic, with the device launcher replaced by the oracle's row quantisation
    (the launcher itself is checked bit for bit on the GPU, tests/test_gpu_block_fp8.py): its [M, K] / [M, K/128] results are
    the per-group definition (scale = absmax / 448, 1 for a zero group; q = RNE(clamp(x * (1 / scale))))."""
    from conch_amd.ops.quantization import block_fp8

    monkeypatch.setattr(block_fp8, "dynamic_scaled_fp8_quant_launcher", _host_row_quant)
    gen = torch.Generator().manual_seed(5)
    m, k = 6, 512
    x = (4 * torch.randn((m, k), generator=gen)).to(dtype)
    x[2, 128:256] = 0
    if layout == "transposed":
        arg = x.T.contiguous().T  # column-major: made contiguous by the op
    elif layout == "3d":
        arg = x.reshape(2, 3, k)
    else:
        arg = x
    q, s = per_token_group_fp8_quant(arg)
    assert q.dtype == FP8 and q.shape == arg.shape and s.dtype == torch.float32 and s.shape == (*arg.shape[:-1], k // 128)
    q, s = q.reshape(m, k), s.reshape(m, k // 128)
    for i in range(m):
        for j in range(k // 128):
            g = x[i, j * 128 : (j + 1) * 128].to(torch.float32)
            amax = g.abs().max()
            scale = amax / 448.0 if amax > 0 else torch.tensor(1.0)
            assert s[i, j].item() == scale.item()
            want = (g * scale.reciprocal()).clamp(-448.0, 448.0).to(FP8)
            assert torch.equal(q[i, j * 128 : (j + 1) * 128].view(torch.uint8), want.view(torch.uint8))
    assert s[2, 1].item() == 1.0


def _operands(m=4, n=256, k=256, dtype=FP8):
    a = torch.zeros((m, k)).to(dtype)
    w = torch.zeros((n, k)).to(dtype)
    sa = torch.ones((m, k // 128))
    sb = torch.ones(((n + 127) // 128, k // 128))
    return a, w.T, sa, sb


def test_refusals_on_cpu_tensors():
    a, b, sa, sb = _operands()
    out = torch.bfloat16
    with pytest.raises(NotImplementedError, match="e4m3fnuz"):
        scaled_gemm_blockwise(*_operands(dtype=torch.float8_e4m3fnuz), out)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        scaled_gemm_blockwise(a.to(torch.float32), b, sa, sb, out)
    with pytest.raises(ValueError, match="output_dtype"):
        scaled_gemm_blockwise(a, b, sa, sb, torch.float32)
    with pytest.raises(ValueError, match="multiple of 128"):
        scaled_gemm_blockwise(*_operands(k=192), out)
    with pytest.raises(ValueError, match="disagree on K"):
        scaled_gemm_blockwise(a, torch.zeros((256, 384)).to(FP8).T, sa, sb, out)
    with pytest.raises(ValueError, match="K-contiguous"):
        scaled_gemm_blockwise(torch.zeros((256, 4)).to(FP8).T, b, sa, sb, out)
    with pytest.raises(ValueError, match="b.stride"):
        scaled_gemm_blockwise(a, torch.zeros((256, 256)).to(FP8), sa, sb, out)
    # row stride 272 bytes (a multiple of 16) but the first row starts 8 bytes into the buffer
    with pytest.raises(ValueError, match="16-byte boundaries"):
        scaled_gemm_blockwise(torch.zeros((4, 272)).to(FP8)[:, 8:264], b, sa, sb, out)
    with pytest.raises(ValueError, match="16-byte boundaries"):
        scaled_gemm_blockwise(a, torch.zeros((256, 272)).to(FP8)[:, 8:264].T, sa, sb, out)
    # a single row / column that is not K-contiguous: the K stride matters whatever M and N are
    a1 = torch.zeros((256, 4)).to(FP8)[:, :1].T  # [1, 256], strides (1, 4)
    assert a1.shape == (1, 256) and a1.stride(1) == 4
    with pytest.raises(ValueError, match="K-contiguous"):
        scaled_gemm_blockwise(a1, b, torch.ones((1, 2)), sb, out)
    b1 = torch.zeros((256, 64)).to(FP8)[:, :1]  # [256, 1] of a row-major [K, N] weight, strides (64, 1)
    assert b1.shape == (256, 1) and b1.stride(0) == 64
    with pytest.raises(ValueError, match="b.stride"):
        scaled_gemm_blockwise(a, b1, sa, torch.ones((1, 2)), out)
    # row strides: 264 bytes is not a multiple of 16
    with pytest.raises(ValueError, match="16 bytes"):
        scaled_gemm_blockwise(torch.zeros((4, 264)).to(FP8)[:, :256], b, sa, sb, out)
    with pytest.raises(ValueError, match="16 bytes"):
        scaled_gemm_blockwise(a, torch.zeros((256, 264)).to(FP8)[:, :256].T, sa, sb, out)
    with pytest.raises(ValueError, match="scale_a has shape"):
        scaled_gemm_blockwise(a, b, torch.ones((4, 1)), sb, out)
    with pytest.raises(ValueError, match="scale_b has shape"):
        scaled_gemm_blockwise(a, b, sa, torch.ones((1, 2)), out)
    with pytest.raises(ValueError, match="scale_b has shape"):
        scaled_gemm_blockwise(*_operands(n=129)[:3], torch.ones((1, 2)), out)  # ragged N: ceil(129 / 128) = 2 row blocks
    with pytest.raises(ValueError, match="scale_a must be float32"):
        scaled_gemm_blockwise(a, b, sa.to(torch.bfloat16), sb, out)
    with pytest.raises(ValueError, match="bias must be"):
        scaled_gemm_blockwise(a, b, sa, sb, out, bias=torch.zeros(256, dtype=torch.float16))
    with pytest.raises(ValueError, match="bias has shape"):
        scaled_gemm_blockwise(a, b, sa, sb, out, bias=torch.zeros(255, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="group_size"):
        per_token_group_fp8_quant(torch.zeros((2, 256)), group_size=64)
    with pytest.raises(ValueError, match="multiple of 128"):
        per_token_group_fp8_quant(torch.zeros((2, 192)))
    with pytest.raises(ValueError, match="multiple of 128"):
        blockwise_fp8_quant_weights(torch.zeros((2, 192)))


def test_valid_cpu_operands_are_refused_as_cpu_tensors_not_computed():
    """No CPU fallback: operands that pass validation on the host fail at the device check."""
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scaled_gemm_blockwise(*_operands(), torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        per_token_group_fp8_quant(torch.zeros((2, 256)))


def test_mixed_host_and_device_tensors_are_refused():
    a, b, sa, sb = _operands()
    meta = torch.ones(sb.shape, device="meta")
    with pytest.raises(ValueError, match="different devices"):
        scaled_gemm_blockwise(a, b, sa, meta, torch.bfloat16)


# (M, N, K) -> (kernel, K slices) under the automatic dispatcher on a 256-CU chip: 3 = decode kernel (M <= 64), 1 = 128 x 128
# tiles, 2 = tiles with split-K (few tiles, long K).  DeepSeek-V3's projections first.
PLAN_CASES = [
    ((1, 1536, 7168), (3, 10)),
    ((16, 576, 7168), (3, 14)),
    ((16, 1536, 7168), (3, 10)),
    ((64, 24576, 1536), (3, 1)),
    ((64, 7168, 16384), (3, 3)),
    ((1, 4096, 7168), (3, 4)),
    ((256, 1536, 7168), (2, 7)),
    ((256, 576, 7168), (2, 7)),
    ((256, 4096, 7168), (2, 4)),
    ((256, 24576, 1536), (1, 1)),
    ((2048, 7168, 16384), (1, 1)),
    ((4096, 4096, 7168), (1, 1)),
    ((65, 128, 128), (1, 1)),
    ((200, 1000, 1536), (1, 1)),
]


@pytest.mark.parametrize(("shape", "want"), PLAN_CASES)
def test_dispatcher_picks(shape, want):
    assert gemm_blockwise.plan(*shape) == want


@pytest.mark.parametrize(("forced", "kernel"), [(1, 1), (2, 2), (3, 3)])
@pytest.mark.parametrize("shape", [s for s, _ in PLAN_CASES] + [(7, 128, 128), (2048, 128, 128)])
def test_forced_kernels_and_workspace_bound(shape, forced, kernel):
    """Each tuning value forces its kernel on every shape, and the slabs it asks for fit the workspace bound."""
    m, n, k = shape
    try:
        _C.set_tuning(_C.TUNE_BLOCKWISE_KERNEL, forced)
        got_kernel, splits = gemm_blockwise.plan(m, n, k)
        bound = gemm_blockwise.workspace_bytes(m, n, k)
    finally:
        _C.set_tuning(_C.TUNE_BLOCKWISE_KERNEL, 0)
    assert got_kernel == kernel
    assert 1 <= splits <= k // 128
    if forced == 1:
        assert splits == 1
    assert splits * m * n * 4 <= bound
