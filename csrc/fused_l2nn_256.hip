// Fused L2-NN, 256x256-tile engine over the BK=32 product-phase
// counted-vmcnt K-loop (mfma_common.h mfma256_bk32_kloop; design history and
// measured A/B in profiles/pmc_l2nn_256_ab.txt — on THIS op the round-1
// 128^2 2-blocks/CU engine stays faster, so this engine ships disabled; it
// is the production K-loop for the pairwise tile kernel, whose old schedule
// was 1 block/CU WITH full drains).
//
// Epilogue: fused top-2 argmin (never materializes the distance tile):
// per-lane top-2 over the tile columns, 16-lane shuffle merge, [256][17]
// LDS wave-combine, per-(row, col-tile) partials merged by
// l2nn_combine_kernel (l2nn_top2.h).
//
// Reference parity: RAFT's fusedL2NN (k-means assignment), the contraction
// engine role of linalg/detail/contractions.cuh:140-307.

#include <hip/hip_runtime.h>

#include "l2nn_engine.h"
#include "l2nn_top2.h"

namespace raft_amd {

template <int NSLICE>
__launch_bounds__(512, 1)
__global__ void fused_l2nn_256_kernel(const __bf16* __restrict__ x0,
                                      const __bf16* __restrict__ x1,
                                      const __bf16* __restrict__ c0,
                                      const __bf16* __restrict__ c1,
                                      const float* __restrict__ cn,
                                      float* __restrict__ pd,
                                      float* __restrict__ pd2,
                                      int* __restrict__ pi,
                                      long long m, int n, int d, int n_groups) {
  extern __shared__ __bf16 smem[];

  const int t = xcd_contiguous_tile(blockIdx.x, gridDim.x);
  const long long row0 = (long long)(t / n_groups) * 256;
  const int grp = t % n_groups;
  const long long col0 = (long long)grp * 256;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wm = w >> 2, wn = w & 3;   // 2 x 4 wave grid

  Mfma256BK32 st;
  mfma256_bk32_setup(st, row0, col0, d, m - 1, n - 1, wm, wn, lane);

  f32x4 acc[8][4];
#pragma unroll
  for (int a = 0; a < 8; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  mfma256_bk32_kloop<NSLICE>(x0, x1, c0, c1, smem, st, acc, d / 32);

  // fused top-2 argmin epilogue: per-lane top-2 over this thread's 4 columns
  // per (fr, reg) row slot, 16-lane merge, then the 4 column-slice waves
  // combine through LDS ([256][17])
  float best[8][4], best2[8][4];
  int bidx[8][4];
  top2_init(best, best2, bidx);
  top2_fold_tile(acc, cn, (int)col0 + wn * 64 + (lane & 15), best, best2, bidx);
  top2_reduce16(best, best2, bidx);
  top2_park_tile<8, 256 * 17, 17, 1>(smem, (lane & 15) == 0, wm * 128, lane, wn,
                                     best, best2, bidx);
  if (tid < 256 && row0 + tid < m)
    top2_write_partial<4, 256 * 17, 17, 1, false>(smem, tid, pd, pd2, pi,
                                                  (long long)grp * m + row0 + tid);
}

void launch_l2nn_256(const SlicePtrs& p, const float* xn, const float* cn, float* pd,
                     float* pd2, int* pi, float* dmin, int* amin, float* dmin2,
                     long long m, int n, int d, int nslice, hipStream_t stream) {
  const int n_groups = n / 256;
  const int grid = (int)((m + 255) / 256) * n_groups;
  const size_t lds = 8 * 16384;  // K-loop 128 KiB; the 52 KiB epilogue reuses it
  static bool attr_set = false;
  if (!attr_set) {
    HIP_CHECK(hipFuncSetAttribute((const void*)&fused_l2nn_256_kernel<1>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    HIP_CHECK(hipFuncSetAttribute((const void*)&fused_l2nn_256_kernel<2>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    attr_set = true;
  }
#define L2NN256_LAUNCH(NS)                                                      \
  hipLaunchKernelGGL((fused_l2nn_256_kernel<NS>), dim3(grid), dim3(512), lds,   \
                     stream, p.x[0], p.x[1], p.c[0], p.c[1], cn, pd, pd2, pi, m, \
                     n, d, n_groups)
  if (nslice == 1) L2NN256_LAUNCH(1);
  else L2NN256_LAUNCH(2);
#undef L2NN256_LAUNCH
  launch_l2nn_combine<false>(pd, pd2, pi, xn, dmin, amin, dmin2, m, n_groups, stream);
}

}  // namespace raft_amd
