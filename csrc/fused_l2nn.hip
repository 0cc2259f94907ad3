// Fused L2 nearest-neighbor: split-bf16 MFMA distance + in-register argmin.
//
// Reference parity (WHAT): RAFT's historical fused-L2-NN (contraction engine
// + key-value argmin epilogue) — the k-means assignment step and BASELINE
// config 5. The m x n distance matrix NEVER touches HBM.
//
// MI355X design (why this shape — see cdna_hip_programming.md §5):
//  * CDNA4 has no fp32 MFMA. fp32 x is pre-split into NSLICE bf16 slices
//    (x = x0 + x1 [+ x2]); the dot term is the sum of slice-product MFMAs
//    accumulated into ONE fp32 AGPR tile:
//      NSLICE=1: bf16 input (3 per-element bits) — the bf16 data path
//      NSLICE=2: 3 products, ~2^-16 accuracy (TF32-class)
//      NSLICE=3: 6 products, fp32-class (~2^-24)
//    at bf16 MFMA rate (2.5 PF dense) instead of the 157 TF fp32 vector ALU.
//  * Tile: 128 rows x 128 centroids per 256-thread block (4 waves, 2x2),
//    K-step 64. LDS = NSLICE * 32 KiB (dynamic).
//  * Staging via __builtin_amdgcn_global_load_lds width=16 (direct HBM->LDS).
//    LDS rows are 128 B — a 32-way bank conflict for ds_read_b128 column
//    slices — so tiles are XOR-swizzled (byte ^= (row&7)<<4): gload_lds
//    writes linearly, therefore the SOURCE address is inverse-swizzled
//    per-lane and reads apply the same XOR (both-sides-or-neither rule).
//  * argmin epilogue: MFMA C/D layout (col=lane&15, row=(lane>>4)*4+reg) puts
//    each output row across the 16 lanes of a row-group: 4 xor-shuffles
//    reduce (score, index) pairs; the running best stays in registers across
//    centroid tiles. score = ||c||^2 - 2 x.c (||x||^2 added only at the
//    final write — it does not affect the argmin).

#include <hip/hip_runtime.h>

#include "l2nn_engine.h"
#include "l2nn_top2.h"

namespace raft_amd {

template <int NSLICE, bool DB = false, bool PHASED = false>
__launch_bounds__(256, 2)
__global__ void fused_l2nn_kernel(const __bf16* __restrict__ x0,
                                  const __bf16* __restrict__ x1,
                                  const __bf16* __restrict__ x2,
                                  const __bf16* __restrict__ c0,
                                  const __bf16* __restrict__ c1,
                                  const __bf16* __restrict__ c2,
                                  const float* __restrict__ xn,
                                  const float* __restrict__ cn,
                                  float* __restrict__ dmin, int* __restrict__ amin,
                                  float* __restrict__ dmin2,
                                  long long m, int n, int d) {
  extern __shared__ __bf16 smem[];
  __bf16* xs[NSLICE];
  __bf16* cs[NSLICE];
  __bf16* xs2[2][NSLICE];
  __bf16* cs2[2][NSLICE];
  const __bf16* const xg[3] = {x0, x1, x2};
  const __bf16* const cg[3] = {c0, c1, c2};
#pragma unroll
  for (int s = 0; s < NSLICE; s++) {
    xs[s] = smem + s * 8192;
    cs[s] = smem + (NSLICE + s) * 8192;
#pragma unroll
    for (int b = 0; b < 2; b++) {
      xs2[b][s] = smem + (b * 2 * NSLICE + s) * 4096;
      cs2[b][s] = smem + (b * 2 * NSLICE + NSLICE + s) * 4096;
    }
  }

  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const int w = threadIdx.x / RAFT_AMD_WAVE;
  const int wr = w >> 1, wc = w & 1;  // 2x2 wave grid
  const long long row0 = (long long)blockIdx.x * 128;

  float best[4][4], best2[4][4];
  int bidx[4][4];
  top2_init(best, best2, bidx);

  const int n_tiles = n / 128;

  for (int nt = 0; nt < n_tiles; nt++) {
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    if constexpr (PHASED && NSLICE == 2) {
      mfma_tile_kloop_p2(xg, cg, xs, cs, acc, row0, (long long)nt * 128, d,
                         m - 1, n - 1, wr, wc, lane);
    } else if constexpr (DB) {
      mfma_tile_kloop_db32<NSLICE>(xg, cg, xs2, cs2, acc, row0,
                                   (long long)nt * 128, d, m - 1, n - 1, wr, wc,
                                   lane);
    } else {
      mfma_tile_kloop<NSLICE>(xg, cg, xs, cs, acc, row0, (long long)nt * 128, d,
                              m - 1, n - 1, wr, wc, lane);
    }

    // lanes own disjoint column sets, so the per-tile fold is lane-local
    top2_fold_tile(acc, cn, nt * 128 + wc * 64 + (lane & 15), best, best2, bidx);
  }

  top2_reduce16(best, best2, bidx);

  // combine the two column-half waves (wc = 0,1) of each row through LDS
  // ([2][128]), then one wave per row-half writes
  __syncthreads();
  if ((lane & 15) == 0) {
#pragma unroll
    for (int fr = 0; fr < 4; fr++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int rl = wr * 64 + fr * 16 + (lane >> 4) * 4 + reg;
        top2_park<256>(smem, wc * 128 + rl, best[fr][reg], best2[fr][reg],
                     bidx[fr][reg]);
      }
  }
  __syncthreads();
  if (wc == 0 && (lane & 15) == 0) {
#pragma unroll
    for (int fr = 0; fr < 4; fr++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int rl = wr * 64 + fr * 16 + (lane >> 4) * 4 + reg;
        float v, v2;
        int vi;
        top2_merge_parked<2, 256, 1, 128, false>(smem, rl, v, v2, vi);
        const long long row = row0 + rl;
        if (row < m) {
          dmin[row] = fmaxf(v + xn[row], 0.f);
          amin[row] = vi;
          if (dmin2) dmin2[row] = v2 + xn[row];  // second-best, unclamped
        }
      }
  }
}

template <int NSLICE, bool DB, bool PHASED>
static void launch_v1(const SlicePtrs& p, const float* xn, const float* cn,
                      float* dmin, int* amin, float* dmin2, long long m, int n,
                      int d, hipStream_t stream) {
  if constexpr (NSLICE == 3) {  // 96 KiB passes the default dynamic-LDS limit
    static bool attr_set = false;
    if (!attr_set) {
      HIP_CHECK(hipFuncSetAttribute(
          (const void*)&fused_l2nn_kernel<NSLICE, DB, PHASED>,
          hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
      attr_set = true;
    }
  }
  const size_t lds = (size_t)NSLICE * 2 * 8192 * sizeof(__bf16);
  hipLaunchKernelGGL((fused_l2nn_kernel<NSLICE, DB, PHASED>),
                     dim3((int)((m + 127) / 128)), dim3(256), lds, stream, p.x[0],
                     p.x[1], p.x[2], p.c[0], p.c[1], p.c[2], xn, cn, dmin, amin,
                     dmin2, m, n, d);
}

void launch_l2nn_v1(const SlicePtrs& p, const float* xn, const float* cn,
                    float* dmin, int* amin, float* dmin2, long long m, int n, int d,
                    int nslice, L2nnEngine variant, hipStream_t stream) {
#define L2NN_V1(NS, DB, PH) \
  launch_v1<NS, DB, PH>(p, xn, cn, dmin, amin, dmin2, m, n, d, stream)
  const bool db = variant == L2nnEngine::V1Db;
  if (variant == L2nnEngine::V1Phased) L2NN_V1(2, false, true);  // resolver: nslice == 2
  else if (nslice == 1) { if (db) L2NN_V1(1, true, false); else L2NN_V1(1, false, false); }
  else if (nslice == 2) { if (db) L2NN_V1(2, true, false); else L2NN_V1(2, false, false); }
  else { if (db) L2NN_V1(3, true, false); else L2NN_V1(3, false, false); }
#undef L2NN_V1
}

}  // namespace raft_amd
