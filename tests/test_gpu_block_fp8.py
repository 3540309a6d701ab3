"""Block-scaled fp8 GEMM on the GPU (conch_amd.ops.quantization.block_fp8): bit-exact results in the exact regime under every
kernel, parity with scaled_gemm, a per-element bound on quantised random data at DeepSeek-V3's shapes, the activation feeder,
strided operands and scales, and graph capture."""

from __future__ import annotations

import pytest
import torch

from conch_amd import _C
from conch_amd.kernels.quantization import gemm_blockwise
from conch_amd.ops.quantization.block_fp8 import blockwise_fp8_quant_weights, per_token_group_fp8_quant, scaled_gemm_blockwise
from conch_amd.ops.quantization.gemm import scaled_gemm
from oracle.reference import dynamic_scaled_fp8_quant_ref
from tests.blockwise_ref import blockwise_gemm_ref, blockwise_terms

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
OUT = (torch.bfloat16, torch.float16)
KERNELS = (_C.BLOCKWISE_TILES, _C.BLOCKWISE_SPLITK, _C.BLOCKWISE_DECODE)


class forced_kernel:  # noqa: N801
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        _C.set_tuning(_C.TUNE_BLOCKWISE_KERNEL, self.value)

    def __exit__(self, *exc):
        _C.set_tuning(_C.TUNE_BLOCKWISE_KERNEL, 0)


def _exact_operands(m, n, k, gen, dev):
    """Integers in [-4, 4] (exact in e4m3fn), scales 2^-2 .. 2^1: every partial sum is exact in fp32 in any order."""
    a = torch.randint(-4, 5, (m, k), generator=gen).to(torch.float32).to(FP8).to(dev)
    w = torch.randint(-4, 5, (n, k), generator=gen).to(torch.float32).to(FP8).to(dev)
    sa = torch.pow(2.0, torch.randint(-2, 2, (m, k // 128), generator=gen).to(torch.float32)).to(dev)
    sb = torch.pow(2.0, torch.randint(-2, 2, ((n + 127) // 128, k // 128), generator=gen).to(torch.float32)).to(dev)
    return a, w, sa, sb


def _bits(t):
    return t.view(torch.int16)


EXACT_NK = [(128, 128), (576, 4096), (1000, 1536), (1536, 4096), (4096, 512), (7168, 2048)]
EXACT_M = [1, 7, 16, 64, 65, 128, 200, 1000, 2048]


@pytest.mark.parametrize(("n", "k"), EXACT_NK)
@pytest.mark.parametrize("m", EXACT_M)
def test_exact_regime_every_kernel_bit_identical(m, n, k):
    gen = torch.Generator().manual_seed(m * 7919 + n * 31 + k)
    dev = torch.device("cuda")
    a, w, sa, sb = _exact_operands(m, n, k, gen, dev)
    acc, _ = blockwise_terms(a, w.T, sa, sb, torch.float32)  # per-block fp32 matmuls: exact here
    bias = {dt: (torch.randint(-64, 65, (n,), generator=gen).to(torch.float32) / 8).to(dt).to(dev) for dt in OUT}
    for kernel in KERNELS:
        with forced_kernel(kernel):
            for dt in OUT:
                want = acc.to(dt)
                got = scaled_gemm_blockwise(a, w.T, sa, sb, dt)
                assert torch.equal(_bits(got), _bits(want)), f"kernel {kernel}, {dt}, no bias"
                got = scaled_gemm_blockwise(a, w.T, sa, sb, dt, bias=bias[dt])
                assert torch.equal(_bits(got), _bits(want + bias[dt])), f"kernel {kernel}, {dt}, bias"


@pytest.mark.parametrize(("m", "n", "k"), [(1, 576, 7168), (16, 1536, 4096), (200, 1000, 1536), (1024, 4096, 2048)])
def test_uniform_scales_equal_per_tensor_scaled_gemm(m, n, k):
    gen = torch.Generator().manual_seed(m + n + k)
    dev = torch.device("cuda")
    a, w, _, _ = _exact_operands(m, n, k, gen, dev)
    ca, cb = 0.5, 0.125
    sa = torch.full((m, k // 128), ca, device=dev)
    sb = torch.full(((n + 127) // 128, k // 128), cb, device=dev)
    bias = (torch.randint(-64, 65, (n,), generator=gen).to(torch.float32) / 4).to(torch.bfloat16).to(dev)
    want = scaled_gemm(a, w.T, torch.tensor([ca], device=dev), torch.tensor([cb], device=dev), torch.bfloat16, bias)
    got = scaled_gemm_blockwise(a, w.T, sa, sb, torch.bfloat16, bias)
    assert torch.equal(_bits(got), _bits(want))


DEEPSEEK_NK = [(1536, 7168), (576, 7168), (24576, 1536), (7168, 16384), (4096, 7168)]


def _sample_rows(m):
    """All rows up to 128; beyond, 128 rows that put every in-tile row offset 0..127 on some 128-row tile of the output."""
    if m <= 128:
        return torch.arange(m)
    tiles = m // 128
    return torch.tensor(sorted({(i % tiles) * 128 + i for i in range(128)}))


@pytest.mark.parametrize(("n", "k"), DEEPSEEK_NK)
@pytest.mark.parametrize("m", [1, 16, 64, 256, 2048])
def test_quantised_random_data_within_the_bound(m, n, k):
    torch.manual_seed(m * 131 + n + k)
    dev = torch.device("cuda")
    x = torch.randn((m, k), device=dev).to(torch.bfloat16)
    wt = (0.05 * torch.randn((n, k), device=dev)).to(torch.bfloat16)
    bias = (0.1 * torch.randn(n, device=dev)).to(torch.bfloat16)
    a, sa = per_token_group_fp8_quant(x)
    w, sb = blockwise_fp8_quant_weights(wt)
    got = scaled_gemm_blockwise(a, w.T, sa, sb, torch.bfloat16, bias).cpu()
    rows = _sample_rows(m)
    ref, mag = blockwise_terms(a[rows].cpu(), w.T.cpu(), sa[rows].cpu(), sb.cpu(), torch.float64, magnitude=True)
    out_ref = ref.to(torch.float32).to(torch.bfloat16) + bias.cpu()
    fi = torch.finfo(torch.bfloat16)
    b64 = bias.cpu().to(torch.float64).abs()
    bound = 2 * fi.eps * (ref.abs() + b64) + 2.0**-24 * (k // 128 + 130) * mag + 2 * fi.tiny
    err = (got[rows].to(torch.float64) - out_ref.to(torch.float64)).abs()
    assert torch.isfinite(got).all()
    bad = err > bound
    assert not bad.any(), f"{int(bad.sum())} elements outside the bound; worst excess {float((err - bound).max()):.3g}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize(("m", "k"), [(1, 128), (7, 7168), (64, 1536), (513, 2048)])
def test_group_quant_bit_identical_to_the_per_token_oracle(m, k, dtype):
    torch.manual_seed(m + k)
    x = (8 * torch.randn((m, k), device="cuda")).to(dtype)
    x[0, :128] = 0  # all-zero groups: scale 1
    if k >= 256:
        x[m // 2, 128:256] = 0
    q, s = per_token_group_fp8_quant(x)
    q_ref, s_ref = dynamic_scaled_fp8_quant_ref(x.cpu().reshape(-1, 128))
    assert q.shape == (m, k) and s.shape == (m, k // 128)
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.reshape(m, k).view(torch.uint8))
    assert torch.equal(s.cpu(), s_ref.reshape(m, k // 128))
    assert s[0, 0].item() == 1.0


@pytest.mark.parametrize(("m", "n", "k"), [(16, 576, 4096), (300, 1000, 1536)])
def test_strided_operands_and_column_major_scales(m, n, k):
    gen = torch.Generator().manual_seed(m + n)
    dev = torch.device("cuda")
    a, w, sa, sb = _exact_operands(m, n, k, gen, dev)
    # the padding holds nonzero values: a kernel that read past K into it would change the result
    a_pad = torch.full((m, k + 64), 3.0, device=dev).to(FP8)
    a_pad[:, :k] = a
    w_pad = torch.full((n, k + 32), -2.0, device=dev).to(FP8)
    w_pad[:, :k] = w
    sa_cm = sa.T.contiguous().T  # column-major [M, K/128]
    sb_cm = sb.T.contiguous().T
    assert sa_cm.stride() == (1, m) and a_pad[:, :k].stride(0) == k + 64
    want = blockwise_gemm_ref(a, w.T, sa, sb, torch.bfloat16, acc_dtype=torch.float32)
    for kernel in KERNELS:
        with forced_kernel(kernel):
            got = scaled_gemm_blockwise(a_pad[:, :k], w_pad[:, :k].T, sa_cm, sb_cm, torch.bfloat16)
        assert torch.equal(_bits(got), _bits(want)), f"kernel {kernel}"


def test_single_row_and_column_from_odd_stride_matrices():
    """M == 1 / N == 1: a row of a matrix whose row stride is not a multiple of 16 is still K-contiguous and is read as K bytes
    (the row stride of a single row means nothing); the neighbouring rows hold nonzero values."""
    gen = torch.Generator().manual_seed(3)
    dev = torch.device("cuda")
    k, n = 1024, 576
    a, w, sa, sb = _exact_operands(1, n, k, gen, dev)
    a_big = torch.full((4, k + 8), 3.0, device=dev).to(FP8)
    a_big[0, :k] = a[0]
    w1, _, _, sb1 = _exact_operands(1, 1, k, gen, dev)
    w_big = torch.full((4, k + 8), -2.0, device=dev).to(FP8)
    w_big[0, :k] = w1[0]
    for kernel in KERNELS:
        with forced_kernel(kernel):
            got = scaled_gemm_blockwise(a_big[:1, :k], w.T, sa, sb, torch.bfloat16)
            assert torch.equal(_bits(got), _bits(blockwise_gemm_ref(a, w.T, sa, sb, torch.bfloat16, acc_dtype=torch.float32)))
            got = scaled_gemm_blockwise(a_big[:1, :k], w_big[:1, :k].T, sa, sb1, torch.bfloat16)
            assert torch.equal(_bits(got), _bits(blockwise_gemm_ref(a, w1.T, sa, sb1, torch.bfloat16, acc_dtype=torch.float32)))


@pytest.mark.parametrize(("m", "n", "k"), [(16, 1536, 7168), (256, 576, 7168)])
def test_quant_and_gemm_replay_from_a_graph_bit_identical(m, n, k):
    torch.manual_seed(m + n)
    dev = torch.device("cuda")
    x = torch.randn((m, k), device=dev).to(torch.bfloat16)
    w, sb = blockwise_fp8_quant_weights((0.05 * torch.randn((n, k), device=dev)).to(torch.bfloat16))

    def step():
        a, sa = per_token_group_fp8_quant(x)
        return scaled_gemm_blockwise(a, w.T, sa, sb, torch.bfloat16)

    assert gemm_blockwise.plan(m, n, k)[1] > 1  # a split-K form: the library scratch is in the graph
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _C.reserve_scratch(gemm_blockwise.workspace_bytes(m, n, k))
        step()
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = step()
    x.copy_(torch.randn((m, k), device=dev).to(torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone()
    want = step()
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want))
