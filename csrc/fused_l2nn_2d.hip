// Fused L2-NN, 2D-grid variant: one block per (row-tile, col-tile-GROUP) with
// an XCD-contiguous block swizzle + a per-row partials-combine kernel.
//
// WHY (measured, profiles/pmc_fused_l2nn_tcc_l2.txt): the v1 kernel loops all
// col-tiles inside one block, so every block re-stages its 131 KB X tile once
// per col-tile; the per-XCD working set (64 resident blocks x 131 KB) blows
// the 4 MiB per-XCD L2 -> 48.6% hit rate, HBM reads == full 8x X re-read.
// Here the col-tiles of a row tile are TEMPORALLY ADJACENT ON ONE XCD
// (guide T1: default dispatch round-robins blockIdx across the 8 XCDs, so we
// remap bijectively so XCD x executes a contiguous range of row-major tile
// indices): the X tile is read into that XCD's L2 once and the other
// col-tile groups hit (measured 93.2% hit rate, HBM 49 GB -> 6.7 GB,
// profiles/pmc_fused_l2nn_2d_tcc.txt). Each block emits per-row
// (best, second, argmin) PARTIALS for its group; a bandwidth-bound combine
// kernel merges the n/128/GT partials per row (disjoint column ranges -> a
// plain top-2 merge) and applies ||x||^2.
//
// GT (col-tiles per block) trades L2 working set against epilogue
// amortization: GT=1 minimizes the per-XCD X footprint (64 resident blocks
// share 8 row tiles) but pays the reduce epilogue per tile; GT=4 pays it
// once per 4 tiles but doubles the X footprint. The epilogue itself is an
// LDS-transpose serial merge (each of 128 threads merges its row's 32 lane
// candidates) instead of the 12-shuffle butterfly — cheaper, and it
// subsumes the column-half-wave combine.
//
// Reference parity: same fused-L2-NN contract as fused_l2nn.hip (RAFT's
// fusedL2NN / k-means assignment step).

#include <hip/hip_runtime.h>

#include "l2nn_engine.h"
#include "l2nn_top2.h"

namespace raft_amd {

template <int NSLICE, int GT, bool PHASED = false, bool ADIRECT = false>
__launch_bounds__(256, 2)
__global__ void fused_l2nn_2d_kernel(const __bf16* __restrict__ x0,
                                     const __bf16* __restrict__ x1,
                                     const __bf16* __restrict__ x2,
                                     const __bf16* __restrict__ c0,
                                     const __bf16* __restrict__ c1,
                                     const __bf16* __restrict__ c2,
                                     const float* __restrict__ cn,
                                     float* __restrict__ pd,
                                     float* __restrict__ pd2,
                                     int* __restrict__ pi,
                                     long long m, int n, int d, int n_groups) {
  extern __shared__ __bf16 smem[];
  __bf16* xs[NSLICE];
  __bf16* cs[NSLICE];
  const __bf16* const xg[3] = {x0, x1, x2};
  const __bf16* const cg[3] = {c0, c1, c2};
#pragma unroll
  for (int s = 0; s < NSLICE; s++) {
    if constexpr (ADIRECT) {
      cs[s] = smem + s * 8192;   // C-only LDS; X reads are direct
      xs[s] = smem;
    } else {
      xs[s] = smem + s * 8192;
      cs[s] = smem + (NSLICE + s) * 8192;
    }
  }

  const int t = xcd_contiguous_tile(blockIdx.x, gridDim.x);
  const long long row0 = (long long)(t / n_groups) * 128;
  const int grp = t % n_groups;

  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const int w = threadIdx.x / RAFT_AMD_WAVE;
  const int wr = w >> 1, wc = w & 1;  // 2x2 wave grid

  float best[4][4], best2[4][4];
  int bidx[4][4];
  top2_init(best, best2, bidx);

  // NOT unrolled: the k-loop body is large; unrolling it GT times (8 at the
  // 1-slice default) bloats I-cache for zero register benefit
#pragma unroll 1
  for (int g = 0; g < GT; g++) {
    const long long col0 = ((long long)grp * GT + g) * 128;
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    if constexpr (ADIRECT) {
      mfma_tile_kloop_ad<NSLICE>(xg, cg, cs, acc, row0, col0, d, m - 1, n - 1,
                                 wr, wc, lane);
    } else if constexpr (PHASED && NSLICE == 2) {
      mfma_tile_kloop_p2(xg, cg, xs, cs, acc, row0, col0, d, m - 1, n - 1, wr,
                         wc, lane);
    } else {
      mfma_tile_kloop<NSLICE>(xg, cg, xs, cs, acc, row0, col0, d, m - 1, n - 1,
                              wr, wc, lane);
    }

    // lane-local running top-2 across the group's tiles (disjoint columns)
    top2_fold_tile(acc, cn, (int)col0 + wc * 64 + (lane & 15), best, best2, bidx);
  }

  // LDS-transpose epilogue: EVERY lane parks its 16 (fr,reg) triples; then
  // one thread per row serially merges the row's 32 lane-candidates (both
  // column-half waves at once — subsumes the wc-combine). [128][33]: measured
  // faster than the shuffle reduce here (BASELINE.md, 26.7 -> 21.8 ms).
  top2_park_tile<4, 128 * 33, 33, 1>(smem, true, wr * 64, lane,
                                     wc * 16 + (lane & 15), best, best2, bidx);
  const int rl = threadIdx.x;
  if (rl < 128 && row0 + rl < m)
    top2_write_partial<32, 128 * 33, 33, 1, false>(smem, rl, pd, pd2, pi,
                                                   (long long)grp * m + row0 + rl);
}

// BK=32 / 4-blocks-per-CU variant: 8 KiB LDS tiles (32 KiB total for
// 2 slices) double the resident blocks per CU, so 4 independent load-drains
// interleave per SIMD instead of 2. Epilogue is the v1-style shuffle reduce
// (once per GT tiles) + tiny LDS half-combine — the [128][33] transpose
// epilogue would need 50 KiB and cap occupancy back at 2.
template <int NSLICE, int GT>
__launch_bounds__(256, 4)
__global__ void fused_l2nn_2d_bk32_kernel(const __bf16* __restrict__ x0,
                                          const __bf16* __restrict__ x1,
                                          const __bf16* __restrict__ x2,
                                          const __bf16* __restrict__ c0,
                                          const __bf16* __restrict__ c1,
                                          const __bf16* __restrict__ c2,
                                          const float* __restrict__ cn,
                                          float* __restrict__ pd,
                                          float* __restrict__ pd2,
                                          int* __restrict__ pi,
                                          long long m, int n, int d,
                                          int n_groups) {
  extern __shared__ __bf16 smem[];
  __bf16* xs[NSLICE];
  __bf16* cs[NSLICE];
  const __bf16* const xg[3] = {x0, x1, x2};
  const __bf16* const cg[3] = {c0, c1, c2};
#pragma unroll
  for (int s = 0; s < NSLICE; s++) {
    xs[s] = smem + s * 4096;
    cs[s] = smem + (NSLICE + s) * 4096;
  }
  const int t = xcd_contiguous_tile(blockIdx.x, gridDim.x);
  const long long row0 = (long long)(t / n_groups) * 128;
  const int grp = t % n_groups;

  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const int w = threadIdx.x / RAFT_AMD_WAVE;
  const int wr = w >> 1, wc = w & 1;

  float best[4][4], best2[4][4];
  int bidx[4][4];
  top2_init(best, best2, bidx);

  // NOT unrolled: the k-loop body is large; unrolling it GT times bloats
  // I-cache for zero register benefit
#pragma unroll 1
  for (int g = 0; g < GT; g++) {
    const long long col0 = ((long long)grp * GT + g) * 128;
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    mfma_tile_kloop_s32<NSLICE>(xg, cg, xs, cs, acc, row0, col0, d, m - 1,
                                n - 1, wr, wc, lane);
    top2_fold_tile(acc, cn, (int)col0 + wc * 64 + (lane & 15), best, best2, bidx);
  }

  // ONE cross-lane reduce, then the [2][128] LDS half-combine
  top2_reduce16(best, best2, bidx);
  top2_park_tile<4, 256, 1, 128>(smem, (lane & 15) == 0, wr * 64, lane, wc, best,
                                 best2, bidx);
  const int rl = threadIdx.x;
  if (rl < 128 && row0 + rl < m)
    top2_write_partial<2, 256, 1, 128, false>(smem, rl, pd, pd2, pi,
                                              (long long)grp * m + row0 + rl);
}

// 2D launch for a resolved variant and gt (l2nn_resolve_engine keeps gt
// within what is instantiated: <= 4 for 2 slices and for bk32)
void launch_l2nn_2d(const SlicePtrs& p, const float* xn, const float* cn, float* pd,
                    float* pd2, int* pi, float* dmin, int* amin, float* dmin2,
                    long long m, int n, int d, int nslice, L2nnEngine variant, int gt,
                    hipStream_t stream) {
  const bool bk32 = variant == L2nnEngine::TwoDBk32;
  const bool adirect = variant == L2nnEngine::TwoDAd;
  const bool ph = variant == L2nnEngine::TwoDPhased;  // resolver: nslice == 2
  const int n_groups = n / 128 / gt;
  const int grid = (int)((m + 127) / 128) * n_groups;
  // kloop needs NSLICE*2 tiles of 16 KiB (8 KiB at BK=32; C-only when
  // A-direct); the [128][33] epilogue reuses it
  const size_t lds_kloop =
      (size_t)nslice * (adirect ? 1 : 2) * (bk32 ? 4096 : 8192) * sizeof(__bf16);
  const size_t lds_epi = bk32 ? 0 : 3 * 128 * 33 * 4;
  const size_t lds = lds_kloop > lds_epi ? lds_kloop : lds_epi;
#define L2NN2D_LAUNCH(...)                                                     \
  hipLaunchKernelGGL((__VA_ARGS__), dim3(grid), dim3(256), lds, stream, p.x[0], \
                     p.x[1], p.x[2], p.c[0], p.c[1], p.c[2], cn, pd, pd2, pi,  \
                     m, n, d, n_groups)
  // G8 exists for one slice only and the resolver never asks bk32 for it
#define L2NN2D_VARIANT(NS, G)                                                   \
  do {                                                                          \
    constexpr int G32 = G == 8 ? 4 : G;                                         \
    if (bk32) L2NN2D_LAUNCH(fused_l2nn_2d_bk32_kernel<NS, G32>);                \
    else if (adirect) L2NN2D_LAUNCH(fused_l2nn_2d_kernel<NS, G, false, true>);  \
    else if (ph) L2NN2D_LAUNCH(fused_l2nn_2d_kernel<2, G == 8 ? 4 : G, true>);  \
    else L2NN2D_LAUNCH(fused_l2nn_2d_kernel<NS, G>);                            \
  } while (0)
  if (nslice == 1) {
    if (gt == 1) L2NN2D_VARIANT(1, 1);
    else if (gt == 2) L2NN2D_VARIANT(1, 2);
    else if (gt == 4) L2NN2D_VARIANT(1, 4);
    else L2NN2D_VARIANT(1, 8);
  } else {
    if (gt == 1) L2NN2D_VARIANT(2, 1);
    else if (gt == 2) L2NN2D_VARIANT(2, 2);
    else L2NN2D_VARIANT(2, 4);
  }
#undef L2NN2D_VARIANT
#undef L2NN2D_LAUNCH
  launch_l2nn_combine<false>(pd, pd2, pi, xn, dmin, amin, dmin2, m, n_groups, stream);
}

}  // namespace raft_amd
