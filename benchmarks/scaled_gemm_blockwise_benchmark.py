"""Block-scaled fp8 GEMM microbenchmark (DeepSeek-V3 format: 1x128 activation scales, 128x128 weight scales).

In one process it times, on the same operands: scaled_gemm_blockwise, per-tensor fp8 scaled_gemm (same fp8 bytes, scales in
the epilogue), and bf16 torch.matmul on the dequantised weights (what a user without a block-scaled kernel runs).  Default:
one shape with the CLI of scaled_gemm_benchmark.py; --sweep: DeepSeek-V3's projections at M in {1, 16, 64, 256, 2048, 4096},
one table line per shape (device time per call, median, L2 flushed between calls).
"""

import click
import torch

from _common import DTYPES, report_match, run_pair
from conch_amd.ops.quantization.block_fp8 import blockwise_fp8_quant_weights, per_token_group_fp8_quant, scaled_gemm_blockwise
from conch_amd.ops.quantization.gemm import scaled_gemm
from conch_amd.third_party.vllm.utils import seed_everything
from conch_amd.utils.benchmark import device_times_ms

DEEPSEEK_NK = [(1536, 7168), (576, 7168), (24576, 1536), (7168, 16384), (4096, 7168)]
SWEEP_M = [1, 16, 64, 256, 2048, 4096]


def _problem(m, n, k, out_dtype, use_bias):
    x = torch.randn((m, k)).to(torch.bfloat16)
    w = (0.05 * torch.randn((n, k))).to(torch.bfloat16)
    a, sa = per_token_group_fp8_quant(x)
    wq, sb = blockwise_fp8_quant_weights(w)
    bias = torch.rand((n,), dtype=out_dtype) if use_bias else None
    # bf16 weights dequantised from the blocks: the path without a block-scaled kernel
    w_deq = (wq.to(torch.float32) * sb.repeat_interleave(128, 0)[:n].repeat_interleave(128, 1)).to(torch.bfloat16)
    x_deq = (a.to(torch.float32) * sa.repeat_interleave(128, 1)).to(torch.bfloat16)
    pt_sa, pt_sb = torch.ones((1, 1)), torch.ones((1, 1))
    return {
        "blockwise": lambda: scaled_gemm_blockwise(a, wq.T, sa, sb, out_dtype, bias),
        "per_tensor": lambda: scaled_gemm(a, wq.T, pt_sa, pt_sb, out_dtype, bias),
        "bf16_dequant": lambda: torch.matmul(x_deq, w_deq.T) if bias is None else torch.matmul(x_deq, w_deq.T) + bias,
    }


def _median_us(fn, iteration_time_ms, warmup_time_ms):
    t = sorted(device_times_ms(fn, iteration_time_ms, warmup_time_ms))
    return 1000.0 * t[len(t) // 2]


@click.command()
@click.option("--m-dim", default=4096, type=int)
@click.option("--k-dim", default=8192, type=int)
@click.option("--n-dim", default=4096, type=int)
@click.option("--output-dtype", default="bfloat16", type=click.Choice(["float16", "bfloat16"]))
@click.option("--use-bias", is_flag=True)
@click.option("--iteration-time-ms", default=2000, type=int)
@click.option("--warmup-time-ms", default=500, type=int)
@click.option("--sweep", is_flag=True, help="DeepSeek-V3 shapes x M in {1, 16, 64, 256, 2048, 4096}: one line each")
@click.option("--gpu", default="cuda:0")
@click.option("--csv", is_flag=True)
def main(m_dim, k_dim, n_dim, output_dtype, use_bias, iteration_time_ms, warmup_time_ms, sweep, gpu, csv):
    seed_everything(0)
    torch.set_default_device(torch.device(gpu))
    out_dtype = DTYPES[output_dtype]
    if sweep:
        print("M,N,K,blockwise_us,per_tensor_us,bf16_dequant_us,blockwise/per_tensor,bf16/blockwise")
        for n, k in DEEPSEEK_NK:
            for m in SWEEP_M:
                fns = _problem(m, n, k, out_dtype, use_bias)
                us = {tag: _median_us(fn, iteration_time_ms, warmup_time_ms) for tag, fn in fns.items()}
                print(f"{m},{n},{k},{us['blockwise']:.1f},{us['per_tensor']:.1f},{us['bf16_dequant']:.1f},"
                      f"{us['blockwise'] / us['per_tensor']:.2f},{us['bf16_dequant'] / us['blockwise']:.2f}", flush=True)
                del fns
                torch.cuda.empty_cache()
        return
    fns = _problem(m_dim, n_dim, k_dim, out_dtype, use_bias)
    ours, deq = fns["blockwise"](), fns["bf16_dequant"]()
    ok = torch.allclose(ours.float(), deq.float(), rtol=5e-2, atol=5e-2)
    report_match(ok, f"(max |diff| {(ours.float() - deq.float()).abs().max().item():.4g})")
    params = {"m_dim": m_dim, "k_dim": k_dim, "n_dim": n_dim, "output_dtype": output_dtype, "bias": use_bias}
    run_pair("scaled_gemm_blockwise", fns["blockwise"], fns["bf16_dequant"], params, iteration_time_ms, warmup_time_ms, csv,
             flops=2.0 * m_dim * n_dim * k_dim)
    if not csv:
        per_tensor = _median_us(fns["per_tensor"], iteration_time_ms, warmup_time_ms)
        print(f"per-tensor fp8 scaled_gemm on the same operands: {per_tensor:.1f} us (median)")


if __name__ == "__main__":
    main()
