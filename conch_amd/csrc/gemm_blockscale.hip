// Block-scaled fp8 GEMM (DeepSeek-V3 format): activations with one fp32 scale per row per 128 K elements ("1x128"), weights with
// one fp32 scale per 128 x 128 block ("128x128"):
//     C[m][n] = out( sum_kb (sa[m][kb] * sb[n / 128][kb]) * dot(A[m, kb block], B^T[n, kb block]) )  (+ bias, in out dtype)
// The scales change inside the K loop, so they cannot ride in the epilogue as scaled_gemm's do: every 128-byte K step -- exactly one
// scale block, exactly one v_mfma_f32_16x16x128_f8f6f4 per 16 x 16 tile -- is multiplied into a ZEROED temporary (C operand 0, unit
// MFMA scales) and added to the accumulator by four scalar v_fma_f32 with the combined scale s = sa * sb.  The operands are swapped
// in the MFMA (D rows = n, D columns = m), so a lane's four accumulator values are four columns of ONE row, all inside one 128-column
// block: one s per lane per m tile per step.
//
// Three kernels, one dispatcher (conch_scaled_gemm_blockwise below):
//   tiles  -- gemm_mid.hip's design: 128 x 128 tiles, 4 waves, LDS-DMA staging with the (row>>1)&7 source swizzle, conflict-free
//             ds_read_b128 fragments, V-row permutation; the tile is one scale block wide, so sb is workgroup-uniform.
//   split  -- the same kernel on a K slice per blockIdx.y: the already-scaled fp32 partial tile goes to slabs [slice][M][N].
//   decode -- M <= 64 (any M when forced: 64-row blocks on blockIdx.z): operands straight from memory into MFMA registers, no LDS;
//             a workgroup owns 32 columns and its K slice, the 4 waves split the slice, fixed-order fp32 reduction in LDS, then
//             slabs across workgroups.
// The slab reduce kernel adds the slices in slice order, casts (RNE) and adds the bias in the output dtype: no float atomics,
// results are deterministic.
#include "common.hpp"
#include "gemm.hpp"
#include "mfma_tile.hpp"
#include "epilogue_rows.hpp"

#include <algorithm>

namespace conch {
namespace {

using namespace tile;

struct BlockGemmArgs {
  // c, a, b, bias, m, n, k, a_stride_m (lda, bytes), b_stride_n (ldb, bytes), c_stride_m (ldc, elements), out_dtype, raster: the
  // fields the shared tile helpers (map_tile, epilogue_rows_body) read
  ScaledGemmArgs base;
  const float* sa;
  const float* sb;
  int sa_sm, sa_skb, sb_snb, sb_skb;  // scale strides in elements (the entry point keeps every scale offset below 2^31)
  int split_steps;                    // K steps per slice (split and decode forms)
  float* slabs;                       // [slice][M][N] scaled fp32 partial sums (slices > 1)
};

__device__ __forceinline__ f32x4 mfma_fresh(const Frag& fb, const Frag& fa) {
  const i32x8 b = {fb.lo[0], fb.lo[1], fb.lo[2], fb.lo[3], fb.hi[0], fb.hi[1], fb.hi[2], fb.hi[3]};
  const i32x8 a = {fa.lo[0], fa.lo[1], fa.lo[2], fa.lo[3], fa.hi[0], fa.hi[1], fa.hi[2], fa.hi[3]};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(b, a, f32x4{0, 0, 0, 0}, 0, 0, 0, 0, 0, 0);
}

// acc += s * t, four scalar fused multiply-adds.  Not v_pk_fma_f32, which hipcc's SLP vectoriser makes of this form unless the
// file is built with -fno-slp-vectorize (_build.py): beside MFMAs the packed form costs issue slots (MI355X_MICROARCH.md).
__device__ __forceinline__ void scale_add(f32x4& acc, float s, const f32x4& t) {
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(s, t[e], acc[e]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 128 x 128 tiles
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kBsThreads = 256;
constexpr int kBsTile = 128;
constexpr int kBsBuf = 2 * kUnitBytes;  // U (128 rows of A) + V (128 rows of B^T)

template <int OUT_DT, int STAGES, bool SPLIT>
__global__ __launch_bounds__(kBsThreads, STAGES == 2 ? 2 : 1) void blockscale_tiles_kernel(BlockGemmArgs q) {
  const ScaledGemmArgs& p = q.base;
  constexpr int kEpi = STAGES * kBsBuf;
  constexpr int kLds = kEpi + 3 * 128 * 4;
  __shared__ __attribute__((aligned(1024))) char lds[kLds];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const int tiles_m = ((int)p.m + kBsTile - 1) / kBsTile;
  const int tiles_n = ((int)p.n + kBsTile - 1) / kBsTile;
  const TileCoord tc = map_tile(blockIdx.x, tiles_m, tiles_n, p.raster_magic, p.raster_shift);
  const int bm0 = tc.tm * kBsTile, bn0 = tc.tn * kBsTile;

  Srcs src;
  src.a = make_uniform_rsrc(p.a, (uint32_t)((p.m - 1) * p.a_stride_m + p.k));
  src.b = make_uniform_rsrc(p.b, (uint32_t)((p.n - 1) * p.b_stride_n + p.k));
  // staging (gemm_mid.hip): wave w feeds unit rows [32w, 32w + 32); rows past M / N re-read the last row and are never stored
  int so_u[4], so_v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int rho = 32 * wave + 8 * j + (lane >> 3);
    const int chunk = (lane & 7) ^ ((rho >> 1) & 7);
    const int r5 = rho & 31, r = r5 & 15, t = r5 >> 4;
    const int nrow = (rho >> 5) * 32 + 8 * (r >> 2) + (r & 3) + 4 * t;  // MFMA D rows 4g+e of tile t <-> n = 8g+e+4t
    so_u[j] = min(bm0 + rho, (int)p.m - 1) * (int)p.a_stride_m + chunk * 16;
    so_v[j] = min(bn0 + nrow, (int)p.n - 1) * (int)p.b_stride_n + chunk * 16;
  }
  const int total_steps = (int)(p.k / kStepBytes);
  const int step0 = SPLIT ? (int)blockIdx.y * q.split_steps : 0;
  const int steps = SPLIT ? min(q.split_steps, total_steps - step0) : total_steps;
  auto stage = [&](int step) {
    char* dst = lds + (step % STAGES) * kBsBuf + wave * 4096;
    const int koff = (step0 + step) * kStepBytes;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(src.a, (lds_void_t*)(dst + j * 1024), 16, so_u[j], koff, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(src.b, (lds_void_t*)(dst + kUnitBytes + j * 1024), 16, so_v[j], koff, 0, 0);
    }
  };

  // block scales: sa of this lane's row in each of its four m tiles (per lane, one step ahead), sb of the tile's column block
  // (one value for the whole workgroup).  (Measured and not kept: threads 0-127 fetching one row's scale each into a 2-step LDS
  // ring, the waves reading theirs from LDS -- within +-3 % on seven shapes; the scale fetches are not what the loop waits for.)
  const int r = lane & 15, g = lane >> 4;
  int sa_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) sa_off[i] = min(bm0 + wr * 64 + i * 16 + r, (int)p.m - 1) * q.sa_sm;
  float sa_next[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) sa_next[i] = q.sa[sa_off[i] + step0 * q.sa_skb];
  const float* sb_row = q.sb + tc.tn * q.sb_snb;
  float sb_next = sb_row[step0 * q.sb_skb];

  // epilogue constant: the bias of column tt (threads 128-255), requested ahead of the operands (gemm_mid.hip)
  [[maybe_unused]] uint32_t bias_bits = 0;
  if constexpr (!SPLIT) {
    const int tt = threadIdx.x & 127;
    const uint16_t* bias_src = p.bias ? (const uint16_t*)p.bias + min(bn0 + tt, (int)p.n - 1) : (const uint16_t*)q.sb;
    bias_bits = *bias_src;
  }
#pragma unroll
  for (int s0 = 0; s0 < STAGES - 1; ++s0)
    if (s0 < steps) stage(s0);

  const int lane_off = (r >> 3) * 1024 + (r & 7) * 128 + ((g ^ ((r >> 1) & 7)) * 16);
  const int m_base = (wr * 8) * 1024 + lane_off;
  const int n_base = kUnitBytes + (wc * 8) * 1024 + lane_off;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = f32x4{0, 0, 0, 0};

  for (int t = 0; t < steps; ++t) {
    // the counted wait of gemm_mid.hip: the scale loads issued in between only make it wait longer, never shorter
    if (STAGES > 2 && steps - 1 - t >= STAGES - 2) {
      wait_vmcnt_n<8 * (STAGES - 2)>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (t + STAGES - 1 < steps) stage(t + STAGES - 1);
    float s[4];
    const float sbv = sb_next;
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = sa_next[i] * sbv;
    {
      const int kn = step0 + min(t + 1, steps - 1);
#pragma unroll
      for (int i = 0; i < 4; ++i) sa_next[i] = q.sa[sa_off[i] + kn * q.sa_skb];
      sb_next = sb_row[kn * q.sb_skb];
    }
    const int buf = (t % STAGES) * kBsBuf;
    Frag fn[4], fm[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) fn[qq] = read_frag(lds, buf + n_base + qq * 2048);
#pragma unroll
    for (int i = 0; i < 4; ++i) fm[i] = read_frag(lds, buf + m_base + i * 2048);
    // boustrophedon over (m tile, n tile) as in gemm_mid.hip.  Each product lands in a fresh temporary and is folded in by the FMAs
    // issued two MFMAs later, in this order (sched_barrier): left to hipcc, the FMAs followed their own MFMA at once and waited for
    // it (s_nop padding); with the order pinned, 2048 x 1536 x 7168 takes 87 us instead of 102, 256 x 7168 x 16384 121 instead
    // of 133 (three temporaries in flight: no better).
    constexpr int kLag = 2;
    f32x4 tmp[kLag + 1];
#pragma unroll
    for (int j = 0; j < 16 + kLag; ++j) {
      if (j < 16) {
        const int i = j >> 2, qq = j & 3, qn = (i & 1) ? 3 - qq : qq;
        tmp[j % (kLag + 1)] = mfma_fresh(fn[qn], fm[i]);
      }
      if (j >= kLag) {
        const int jj = j - kLag, i = jj >> 2, qq = jj & 3, qn = (i & 1) ? 3 - qq : qq;
        scale_add(acc[i][qn], s[i], tmp[jj % (kLag + 1)]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  if constexpr (SPLIT) {
    // the scaled partial tile, row-major fp32: lane (r, g) holds four consecutive columns of row r per (m tile, n tile)
    float* slab = q.slabs + (int64_t)blockIdx.y * p.m * p.n;
    const bool vec = (p.n & 3) == 0;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
      const int n0 = bn0 + wc * 64 + nh * 32 + 8 * g;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int m = bm0 + wr * 64 + mt * 16 + r;
        if (m >= p.m) continue;
        float* dst = slab + (int64_t)m * p.n + n0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 v = acc[mt][nh * 2 + h];
          if (vec && n0 + 4 * h + 4 <= p.n) {
            *(f32x4*)(dst + 4 * h) = v;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (n0 + 4 * h + e < p.n) dst[4 * h + e] = v[e];
          }
        }
      }
    }
    return;
  }
  // epilogue: the scales are already in the accumulators, so the shared row-major epilogue runs with unit scales (1 * x is exact)
  {
    float* f = (float*)(lds + kEpi);
    f[threadIdx.x] = 1.0f;
    if (threadIdx.x >= 128) f[threadIdx.x + 128] = bits16_to_float<OUT_DT>((uint16_t)bias_bits);
  }
  __syncthreads();  // constants in LDS; every wave past its last operand read; nothing in flight
  if (tile_stores_whole_lines(p, bm0, bn0, kBsTile, kBsTile)) {
    if (p.bias) epilogue_rows_body<kMmaFp8, OUT_DT, true, 4, kBsTile>(acc, p, lds, 0, bm0, bn0, wr, wc, lane, wave, kEpi);
    else epilogue_rows_body<kMmaFp8, OUT_DT, false, 4, kBsTile>(acc, p, lds, 0, bm0, bn0, wr, wc, lane, wave, kEpi);
    return;
  }
  // ragged tiles: direct stores from the accumulator layout
  const bool vec_store = (p.c_stride_m % 8 == 0) && (((uintptr_t)p.c & 15) == 0);
  const float* lbias = (const float*)(lds + kEpi) + 256;
#pragma unroll
  for (int nh = 0; nh < 2; ++nh) {
    const int nl = wc * 64 + nh * 32 + 8 * g;
    const int n0 = bn0 + nl;
    const f32x4 bs_lo = *(const f32x4*)(lbias + nl), bs_hi = *(const f32x4*)(lbias + nl + 4);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m = bm0 + wr * 64 + mt * 16 + r;
      i32x4 pk;
#pragma unroll
      for (int e2 = 0; e2 < 4; ++e2) {
        const int e = 2 * e2;
        const f32x2 a2 = {acc[mt][nh * 2 + (e >> 2)][e & 3], acc[mt][nh * 2 + (e >> 2)][(e & 3) + 1]};
        uint32_t h = pack2_bits16<OUT_DT>(a2);
        if (p.bias) {
          const f32x2 b2 = e < 4 ? f32x2{bs_lo[e & 3], bs_lo[(e & 3) + 1]} : f32x2{bs_hi[e & 3], bs_hi[(e & 3) + 1]};
          h = pack2_bits16<OUT_DT>(pin_f32x2(unpack2_bits16<OUT_DT>(h) + b2));
        }
        pk[e2] = (int)h;
      }
      if (m < p.m) {
        uint16_t* dst = (uint16_t*)p.c + (int64_t)m * p.c_stride_m + n0;
        if (vec_store && n0 + 8 <= p.n) {
          *(i32x4*)dst = pk;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (n0 + e < p.n) dst[e] = (uint16_t)((uint32_t)pk[e >> 1] >> (16 * (e & 1)));
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// decode kernel
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kDcThreads = 256;
constexpr int kDcCols = 32;  // columns per workgroup: two 16-column MFMA tiles, the same for every wave
constexpr int kDcRows = 64;  // rows per workgroup (blockIdx.z: the next 64)

// 32 contiguous bytes of row `row` at K byte `koff`: lane (r, g) takes bytes [32 g, 32 g + 32) of the 128-byte step for BOTH
// operands -- the MFMA pairs element j of lane group g of A with the same element of B, so any K order shared by both sides is a
// legal split of the dot product.  The whole offset is in the VGPR: the buffer range check applies to it (not to soffset), so an
// offset past the buffer reads zeros
__device__ __forceinline__ Frag load_frag(__amdgpu_buffer_rsrc_t rsrc, int off) {
  Frag f;
  f.lo = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
  f.hi = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + 16, 0, 0));
  return f;
}

// MT = 16-row MFMA tiles in use (rows of the 64-row block), U = K steps a wave requests before it multiplies
template <int MT, int U, int OUT_DT, bool SPLIT>
__global__ __launch_bounds__(kDcThreads) void blockscale_decode_kernel(BlockGemmArgs q) {
  const ScaledGemmArgs& p = q.base;
  __shared__ __attribute__((aligned(16))) f32x4 red[3][MT * 2][64];  // waves 1-3's sums; wave 0 adds them in wave order
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kDcCols, m0 = blockIdx.z * kDcRows;
  const int total_steps = (int)(p.k / kStepBytes);
  const int step0 = (int)blockIdx.y * q.split_steps;
  const int step_end = min(step0 + q.split_steps, total_steps);

  const __amdgpu_buffer_rsrc_t ra = make_uniform_rsrc(p.a, (uint32_t)((p.m - 1) * p.a_stride_m + p.k));
  const __amdgpu_buffer_rsrc_t rb = make_uniform_rsrc(p.b, (uint32_t)((p.n - 1) * p.b_stride_n + p.k));
  int off_b[2], off_a[MT], sa_off[MT];
#pragma unroll
  for (int j = 0; j < 2; ++j) off_b[j] = min(n0 + 16 * j + r, (int)p.n - 1) * (int)p.b_stride_n + 32 * g;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = min(m0 + 16 * i + r, (int)p.m - 1);
    off_a[i] = m * (int)p.a_stride_m + 32 * g;
    sa_off[i] = m * q.sa_sm;
  }
  const float* sb_row = q.sb + (n0 / 128) * q.sb_snb;  // 32 | 128: both tiles in one column block

  f32x4 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i][0] = acc[i][1] = f32x4{0, 0, 0, 0};

  // wave w takes the groups of U consecutive steps w, w + 4, w + 8, ... of the slice; a step past the slice reads at byte offset
  // 2^31 - 64 (past both buffers, which the entry point keeps below 2^31 bytes: zeros) under a zero scale
  for (int base = step0 + wave * U; base < step_end; base += 4 * U) {
    Frag fb[U][2], fa[U][MT];
    float sa[U][MT], sb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = base + u < step_end;
      const int kb = live ? base + u : step0;
      const int koff = kb * kStepBytes;
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[u][j] = load_frag(rb, live ? off_b[j] + koff : 0x7fffffc0);
#pragma unroll
      for (int i = 0; i < MT; ++i) fa[u][i] = load_frag(ra, live ? off_a[i] + koff : 0x7fffffc0);
#pragma unroll
      for (int i = 0; i < MT; ++i) sa[u][i] = q.sa[sa_off[i] + kb * q.sa_skb];
      sb[u] = live ? sb_row[kb * q.sb_skb] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const float s = sa[u][i] * sb[u];
#pragma unroll
        for (int j = 0; j < 2; ++j) scale_add(acc[i][j], s, mfma_fresh(fb[u][j], fa[u][i]));
      }
  }

  if (wave != 0) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) red[wave - 1][i * 2 + j][lane] = acc[i][j];
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 0; w < 3; ++w)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] += red[w][i * 2 + j][lane];

  // lane (r, g) holds columns n0 + 16 j + 4 g + e of row m0 + 16 i + r
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + 16 * i + r;
    if (m >= p.m || m >= m0 + kDcRows) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nq = n0 + 16 * j + 4 * g;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (nq + e >= p.n) break;
        if constexpr (SPLIT) {
          q.slabs[((int64_t)blockIdx.y * p.m + m) * p.n + nq + e] = acc[i][j][e];
        } else {
          uint16_t h = float_to_bits16<OUT_DT>(acc[i][j][e]);
          if (p.bias) h = float_to_bits16<OUT_DT>(pin_f32(bits16_to_float<OUT_DT>(h) + bits16_to_float<OUT_DT>(((const uint16_t*)p.bias)[nq + e])));
          ((uint16_t*)p.c)[(int64_t)m * p.c_stride_m + nq + e] = h;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// slab reduce: C = out(sum over slices, in slice order) (+ bias in the output dtype)
// ---------------------------------------------------------------------------------------------------------------------------------
template <int OUT_DT>
__global__ __launch_bounds__(256) void blockscale_reduce_kernel(BlockGemmArgs q, int slices) {
  const ScaledGemmArgs& p = q.base;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= p.n) return;
  const int64_t plane = p.m * p.n;
  const float bias = p.bias ? bits16_to_float<OUT_DT>(((const uint16_t*)p.bias)[n]) : 0.0f;
  for (int64_t m = blockIdx.y; m < p.m; m += gridDim.y) {
    const float* src = q.slabs + m * p.n + n;
    float s = src[0];
    for (int sl = 1; sl < slices; ++sl) s += src[sl * plane];
    uint16_t h = float_to_bits16<OUT_DT>(s);
    if (p.bias) h = float_to_bits16<OUT_DT>(pin_f32(bits16_to_float<OUT_DT>(h) + bias));
    ((uint16_t*)p.c)[m * p.c_stride_m + n] = h;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dispatcher
// ---------------------------------------------------------------------------------------------------------------------------------
enum { kBsPickTiles = 1, kBsPickSplit = 2, kBsPickDecode = 3 };
constexpr int kBsMaxTileSlices = 8;
constexpr int kBsMaxDecodeSlices = 32;

struct BlockPlan {
  int kernel;
  int slices;
};

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// no empty slice: `want` slices of ceil(steps / want) steps each, then as many as that step count needs
int even_slices(int64_t steps, int64_t want) {
  want = std::max<int64_t>(1, std::min(want, steps));
  const int64_t per = cdiv(steps, want);
  return (int)cdiv(steps, per);
}

// decode kernel: about two workgroups per CU, each wave at least one step; slabs (written and read back) at most a quarter of the
// weight bytes (K / (16 M) slices)
int decode_slices(int64_t m, int64_t n, int64_t k, int cus) {
  const int64_t steps = k / kStepBytes;
  const int64_t wgs = cdiv(n, kDcCols) * cdiv(m, kDcRows);
  int64_t want = cdiv(2 * (int64_t)cus, wgs);
  want = std::min<int64_t>(want, kBsMaxDecodeSlices);
  want = std::min<int64_t>(want, std::max<int64_t>(1, steps / 4));
  want = std::min<int64_t>(want, std::max<int64_t>(1, k / (16 * m)));
  return even_slices(steps, want);
}

// tiles: split K only where the tiles leave most of the chip idle and K is long (gemm_mid.hip's rule: one workgroup per CU up to
// half a chip of tiles, two up to ~0.7 of a chip; a slice at least eight steps)
int tile_slices(int64_t m, int64_t n, int64_t k, int cus, bool forced) {
  const int64_t steps = k / kStepBytes;
  const int64_t tiles = cdiv(m, kBsTile) * cdiv(n, kBsTile);
  int64_t want;
  if (forced) {
    want = std::max<int64_t>(2, cus / tiles);
  } else {
    if (tiles * 10 > (int64_t)cus * 7 || steps < 16) return 1;
    want = tiles * 2 <= cus ? cus / tiles : (2 * (int64_t)cus) / tiles;
    want = std::min<int64_t>(want, steps / 8);
  }
  return even_slices(steps, std::min<int64_t>(want, kBsMaxTileSlices));
}

BlockPlan blockscale_plan(int64_t m, int64_t n, int64_t k) {
  const int forced = tuning(CONCH_TUNE_BLOCKWISE_KERNEL);
  const int cus = device_cu_count();
  BlockPlan plan;
  plan.kernel = (forced >= kBsPickTiles && forced <= kBsPickDecode) ? forced : (m <= kDcRows ? kBsPickDecode : kBsPickTiles);
  if (plan.kernel == kBsPickDecode) {
    plan.slices = decode_slices(m, n, k, cus);
  } else if (forced == kBsPickTiles) {
    plan.slices = 1;
  } else {
    plan.slices = tile_slices(m, n, k, cus, plan.kernel == kBsPickSplit);
    if (plan.slices > 1) plan.kernel = kBsPickSplit;
  }
  return plan;
}

template <int OUT_DT>
int launch_reduce(const BlockGemmArgs& q, int slices, hipStream_t stream) {
  const dim3 grid((unsigned)cdiv(q.base.n, 256), (unsigned)std::min<int64_t>(q.base.m, 65535));
  hipLaunchKernelGGL((blockscale_reduce_kernel<OUT_DT>), grid, dim3(256), 0, stream, q, slices);
  return check_launch("blockscale_reduce");
}

template <int MT, int OUT_DT>
void launch_decode_mt(const BlockGemmArgs& q, dim3 grid, bool split, hipStream_t stream) {
  constexpr int kU = MT == 4 ? 2 : 4;
  if (split) hipLaunchKernelGGL((blockscale_decode_kernel<MT, kU, OUT_DT, true>), grid, dim3(kDcThreads), 0, stream, q);
  else hipLaunchKernelGGL((blockscale_decode_kernel<MT, kU, OUT_DT, false>), grid, dim3(kDcThreads), 0, stream, q);
}

template <int OUT_DT>
int launch_blockscale(BlockGemmArgs q, hipStream_t stream) {
  const ScaledGemmArgs& p = q.base;
  const BlockPlan plan = blockscale_plan(p.m, p.n, p.k);
  const int64_t steps = p.k / kStepBytes;
  const bool split = plan.slices > 1 || plan.kernel == kBsPickSplit;
  q.split_steps = (int)cdiv(steps, plan.slices);
  if (split) {
    void* ws = nullptr;
    if (int rc = get_scratch(stream, kScratchSplitK, (size_t)plan.slices * (size_t)p.m * (size_t)p.n * 4, &ws)) return rc;
    q.slabs = (float*)ws;
  }
  if (plan.kernel == kBsPickDecode) {
    const dim3 grid((unsigned)cdiv(p.n, kDcCols), (unsigned)plan.slices, (unsigned)cdiv(p.m, kDcRows));
    const int64_t rows = std::min<int64_t>(p.m, kDcRows);
    if (rows <= 16) launch_decode_mt<1, OUT_DT>(q, grid, split, stream);
    else if (rows <= 32) launch_decode_mt<2, OUT_DT>(q, grid, split, stream);
    else launch_decode_mt<4, OUT_DT>(q, grid, split, stream);
    if (int rc = check_launch("blockscale_decode")) return rc;
  } else {
    set_raster_divisor((uint32_t)(kGroupM * cdiv(p.n, kBsTile)), &q.base.raster_magic, &q.base.raster_shift);
    const int64_t tiles = cdiv(p.m, kBsTile) * cdiv(p.n, kBsTile);
    const dim3 grid((unsigned)tiles, (unsigned)plan.slices);
    // at most one workgroup per CU: the 4-stage ring (gemm_mid.hip)
    const bool deep = tiles * plan.slices <= device_cu_count();
    if (split) {
      if (deep) hipLaunchKernelGGL((blockscale_tiles_kernel<OUT_DT, 4, true>), grid, dim3(kBsThreads), 0, stream, q);
      else hipLaunchKernelGGL((blockscale_tiles_kernel<OUT_DT, 2, true>), grid, dim3(kBsThreads), 0, stream, q);
    } else {
      if (deep) hipLaunchKernelGGL((blockscale_tiles_kernel<OUT_DT, 4, false>), grid, dim3(kBsThreads), 0, stream, q);
      else hipLaunchKernelGGL((blockscale_tiles_kernel<OUT_DT, 2, false>), grid, dim3(kBsThreads), 0, stream, q);
    }
    if (int rc = check_launch("blockscale_tiles")) return rc;
  }
  return split ? launch_reduce<OUT_DT>(q, plan.slices, stream) : CONCH_OK;
}

}  // namespace
}  // namespace conch

using namespace conch;

extern "C" int64_t conch_scaled_gemm_blockwise_workspace_bytes(int64_t m, int64_t n, int64_t k) {
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  // the most slices any kernel may take under any tuning: 8 for the tiles, the decode rule's cap for the decode kernel
  const int64_t decode_cap = std::min<int64_t>(kBsMaxDecodeSlices, std::max<int64_t>(1, k / (16 * m)));
  return std::max<int64_t>(kBsMaxTileSlices, decode_cap) * m * n * 4 + ((int64_t)1 << 20);
}

extern "C" int conch_debug_blockwise_plan(int64_t m, int64_t n, int64_t k, int* kernel, int* splits) {
  CONCH_CHECK_ARG(kernel && splits && m > 0 && n > 0 && k > 0 && k % 128 == 0, "conch_debug_blockwise_plan: bad arguments");
  const BlockPlan plan = blockscale_plan(m, n, k);
  *kernel = plan.kernel;
  *splits = plan.slices;
  return CONCH_OK;
}

extern "C" int conch_scaled_gemm_blockwise(void* c, const void* a, const void* b, const float* scale_a, const float* scale_b,
                                           const void* bias, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, int64_t ldc,
                                           int64_t sa_stride_m, int64_t sa_stride_kb, int64_t sb_stride_nb, int64_t sb_stride_kb,
                                           int out_dtype, void* stream) {
  CONCH_CHECK_ARG(m >= 0 && n >= 0 && k >= 0, "scaled_gemm_blockwise: negative size (m=%lld n=%lld k=%lld)", (long long)m,
                  (long long)n, (long long)k);
  if (out_dtype != CONCH_DT_FP16 && out_dtype != CONCH_DT_BF16) {
    set_error("scaled_gemm_blockwise: output dtype %d (want FP16 or BF16)", out_dtype);
    return CONCH_ERR_UNSUPPORTED;
  }
  CONCH_CHECK_ARG(k % 128 == 0 && k > 0, "scaled_gemm_blockwise: K=%lld is not a positive multiple of 128", (long long)k);
  if (m == 0 || n == 0) return CONCH_OK;
  CONCH_CHECK_ARG(c && a && b && scale_a && scale_b, "scaled_gemm_blockwise: NULL operand or scale");
  CONCH_CHECK_ARG(lda >= k && ldb >= k && lda % 16 == 0 && ldb % 16 == 0, "scaled_gemm_blockwise: row strides lda=%lld ldb=%lld must be "
                  ">= K and multiples of 16 bytes", (long long)lda, (long long)ldb);
  CONCH_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "scaled_gemm_blockwise: a and b must be 16-byte aligned");
  CONCH_CHECK_ARG(((uintptr_t)c & 1) == 0 && (!bias || ((uintptr_t)bias & 1) == 0), "scaled_gemm_blockwise: misaligned c or bias");
  CONCH_CHECK_ARG(ldc >= n, "scaled_gemm_blockwise: ldc=%lld < N", (long long)ldc);
  CONCH_CHECK_ARG(sa_stride_m >= 0 && sa_stride_kb >= 0 && sb_stride_nb >= 0 && sb_stride_kb >= 0,
                  "scaled_gemm_blockwise: negative scale stride");
  const int64_t kblocks = k / 128, nblocks = (n + 127) / 128;
  const int64_t lim = (int64_t)1 << 31;
  if ((m - 1) * lda + k >= lim || (n - 1) * ldb + k >= lim || (m - 1) * sa_stride_m + (kblocks - 1) * sa_stride_kb >= lim ||
      (nblocks - 1) * sb_stride_nb + (kblocks - 1) * sb_stride_kb >= lim || (m - 1) * ldc + n >= lim) {
    set_error("scaled_gemm_blockwise: an operand spans 2^31 bytes or elements or more (32-bit offsets)");
    return CONCH_ERR_UNSUPPORTED;
  }
  BlockGemmArgs q{};
  q.base.c = c;
  q.base.a = a;
  q.base.b = b;
  q.base.bias = bias;
  q.base.m = m, q.base.n = n, q.base.k = k;
  q.base.a_stride_m = lda, q.base.a_stride_k = 1;
  q.base.b_stride_n = ldb, q.base.b_stride_k = 1;
  q.base.c_stride_m = ldc, q.base.c_stride_n = 1;
  q.base.in_dtype = CONCH_DT_FP8_E4M3FN, q.base.out_dtype = out_dtype;
  q.sa = scale_a;
  q.sb = scale_b;
  q.sa_sm = (int)sa_stride_m, q.sa_skb = (int)sa_stride_kb, q.sb_snb = (int)sb_stride_nb, q.sb_skb = (int)sb_stride_kb;
  if (out_dtype == CONCH_DT_BF16) return launch_blockscale<CONCH_DT_BF16>(q, (hipStream_t)stream);
  return launch_blockscale<CONCH_DT_FP16>(q, (hipStream_t)stream);
}
