// The fused L2-NN epilogue, written once: the running per-row
// (best, second-best, index) triple of every fused_l2nn*.hip engine and of
// masked_l2nn.hip. The verified modes (docs/verified_engines.md) prove the
// argmin from second-best minus best, so every engine must keep the same
// two rules:
//  * equal scores go to the SMALLER column index;
//  * second-best is the second smallest score over DISTINCT columns: two
//    candidates that name the same column (or the same "no column yet"
//    sentinel) never donate the loser's best as a second-best.
// Fragment layout is the MFMA C/D layout of mfma_common.h: acc[fr][fc][reg]
// is row fr*16 + (lane>>4)*4 + reg, column fc*16 + (lane&15) of the wave's
// tile, so the 16 lanes of a row group hold one row's columns.
#pragma once

#include <hip/hip_runtime.h>

#include "mfma_common.h"

namespace raft_amd {

// index of "no allowed column seen" (masked engine): loses every
// smaller-index tie-break
constexpr int MASKED_NN_NONE = 0x7fffffff;

template <int RF>
__device__ __forceinline__ void top2_init(float (&best)[RF][4],
                                          float (&best2)[RF][4],
                                          int (&bidx)[RF][4], int none = 0) {
#pragma unroll
  for (int a = 0; a < RF; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) {
      best[a][b] = INFINITY;
      best2[a][b] = INFINITY;
      bidx[a][b] = none;
    }
}

// fold one score into a lane's running triple. New second-best = middle of
// {s, best, best2} (invariant best <= best2): one v_med3_f32. Columns arrive
// in ascending order, so strict < keeps the smallest index among equals.
__device__ __forceinline__ void top2_push(float& best, float& best2, int& idx,
                                          float s, int col) {
  best2 = __builtin_amdgcn_fmed3f(s, best, best2);
  if (s < best) {
    best = s;
    idx = col;
  }
}

// fold a wave's RF x CF fragment tile: score = ||c||^2 - 2 x.c (||x||^2 is
// added at the final write — it does not move the argmin). col0 is this
// lane's column at fragment 0; fragment fc is col0 + fc*16, and its norm
// depends only on fc (CF loads per tile, not RF*4*CF).
// The norms arrive in registers: cn_r[fc] is ||c||^2 of column col0 + fc*16.
template <int RF, int CF>
__device__ __forceinline__ void top2_fold_tile_cn(const f32x4 (&acc)[RF][CF],
                                                  const float (&cn_r)[CF], int col0,
                                                  float (&best)[RF][4],
                                                  float (&best2)[RF][4],
                                                  int (&bidx)[RF][4]) {
#pragma unroll
  for (int fr = 0; fr < RF; fr++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++)
#pragma unroll
      for (int fc = 0; fc < CF; fc++)
        top2_push(best[fr][reg], best2[fr][reg], bidx[fr][reg],
                  cn_r[fc] - 2.f * acc[fr][fc][reg], col0 + fc * 16);
}

// ... and the same with the norms read from global memory
template <int RF, int CF>
__device__ __forceinline__ void top2_fold_tile(const f32x4 (&acc)[RF][CF],
                                               const float* __restrict__ cn,
                                               int col0, float (&best)[RF][4],
                                               float (&best2)[RF][4],
                                               int (&bidx)[RF][4]) {
  float cn_r[CF];
#pragma unroll
  for (int fc = 0; fc < CF; fc++) cn_r[fc] = cn[col0 + fc * 16];
  top2_fold_tile_cn(acc, cn_r, col0, best, best2, bidx);
}

// merge candidate (b, b2, bi) into (v, v2, vi). Plain: the two sides cover
// disjoint columns. INDEX_GUARD: the sides may both hold MASKED_NN_NONE.
template <bool INDEX_GUARD>
__device__ __forceinline__ void top2_merge(float& v, float& v2, int& vi, float b,
                                           float b2, int bi) {
  if constexpr (INDEX_GUARD) {
    v2 = fminf(v2, b2);
    if (bi != vi) v2 = fminf(v2, fmaxf(v, b));
  } else {
    v2 = fminf(fminf(v2, b2), fmaxf(v, b));
  }
  const bool take = b < v || (b == v && bi < vi);
  v = take ? b : v;
  vi = take ? bi : vi;
}

// ONE cross-lane reduce per (fr, reg) over the 16 lanes of a row group, after
// the column-tile loop (a per-tile reduce was ~1/3 of v1's non-MFMA time).
// Always index-aware: lanes that never saw a column share one index.
template <int RF>
__device__ __forceinline__ void top2_reduce16(float (&best)[RF][4],
                                              float (&best2)[RF][4],
                                              int (&bidx)[RF][4]) {
#pragma unroll
  for (int fr = 0; fr < RF; fr++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      float v = best[fr][reg], v2 = best2[fr][reg];
      int vi = bidx[fr][reg];
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, RAFT_AMD_WAVE);
        const float ov2 = __shfl_xor(v2, off, RAFT_AMD_WAVE);
        const int oi = __shfl_xor(vi, off, RAFT_AMD_WAVE);
        top2_merge<true>(v, v2, vi, ov, ov2, oi);
      }
      best[fr][reg] = v;
      best2[fr][reg] = v2;
      bidx[fr][reg] = vi;
    }
}

// Candidate staging in the (dead) K-loop LDS: three planes (best, second,
// index) of PLANE words; candidate c of block row rl sits at rl*RS + c*CS.
// Two barriers frame the stores: the first ends the K-loop's use of the LDS,
// the second publishes. Shapes in use:
//   wave representative parks ((lane&15)==0 after top2_reduce16, candidate =
//   the wave's column slice): [NCAND][ROWS] (RS=1, CS=ROWS) or [ROWS][17];
//   every lane parks (no shuffle reduce, candidate = slice*16 + lane&15):
//   [ROWS][33], the odd stride keeping a row's candidates off one bank.
// top2_park stores one triple; top2_park_tile is the whole sequence. The v1
// and w8 kernels write the sequence out around top2_park instead: at their
// 256-VGPR cap, handing the register arrays to a helper costs scratch.
template <int PLANE>
__device__ __forceinline__ void top2_park(__bf16* smem, int o, float b, float b2,
                                          int bi) {
  float* pv = reinterpret_cast<float*>(smem);
  float* pv2 = pv + PLANE;
  int* pi = reinterpret_cast<int*>(pv2 + PLANE);
  pv[o] = b;
  pv2[o] = b2;
  pi[o] = bi;
}

// rows wave_row0 + fr*16 + (lane>>4)*4 + reg as candidate `cand`, when `parks`
template <int RF, int PLANE, int RS, int CS>
__device__ __forceinline__ void top2_park_tile(__bf16* smem, bool parks,
                                               int wave_row0, int lane, int cand,
                                               const float (&best)[RF][4],
                                               const float (&best2)[RF][4],
                                               const int (&bidx)[RF][4]) {
  __syncthreads();
  if (parks) {
#pragma unroll
    for (int fr = 0; fr < RF; fr++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int rl = wave_row0 + fr * 16 + (lane >> 4) * 4 + reg;
        top2_park<PLANE>(smem, cand * CS + rl * RS, best[fr][reg], best2[fr][reg],
                         bidx[fr][reg]);
      }
  }
  __syncthreads();
}

// the owning thread's serial merge of block row rl's NCAND parked candidates
template <int NCAND, int PLANE, int RS, int CS, bool INDEX_GUARD>
__device__ __forceinline__ void top2_merge_parked(const __bf16* smem, int rl,
                                                  float& v, float& v2, int& vi) {
  const float* pv = reinterpret_cast<const float*>(smem);
  const float* pv2 = pv + PLANE;
  const int* pi = reinterpret_cast<const int*>(pv2 + PLANE);
  v = INFINITY;
  v2 = INFINITY;
  vi = INDEX_GUARD ? MASKED_NN_NONE : 0;
#pragma unroll 8
  for (int c = 0; c < NCAND; c++) {
    const int o = rl * RS + c * CS;
    top2_merge<INDEX_GUARD>(v, v2, vi, pv[o], pv2[o], pi[o]);
  }
}

// ... written as the block's partial triple o of the [n_groups][m] arrays
template <int NCAND, int PLANE, int RS, int CS, bool INDEX_GUARD>
__device__ __forceinline__ void top2_write_partial(const __bf16* smem, int rl,
                                                   float* __restrict__ pd,
                                                   float* __restrict__ pd2,
                                                   int* __restrict__ pi,
                                                   long long o) {
  float v, v2;
  int vi;
  top2_merge_parked<NCAND, PLANE, RS, CS, INDEX_GUARD>(smem, rl, v, v2, vi);
  pd[o] = v;
  pd2[o] = v2;
  pi[o] = vi;
}

// Merge the n_groups partial triples of every row (pd/pd2/pi are
// [n_groups][m]); groups cover disjoint column ranges. Adds ||x||^2 once and
// clamps the best; the second-best stays unclamped. MASKED: a group may hold
// no candidate (MASKED_NN_NONE), and a row with none gets (+inf, -1, +inf).
template <bool MASKED>
__global__ void l2nn_combine_kernel(const float* __restrict__ pd,
                                    const float* __restrict__ pd2,
                                    const int* __restrict__ pi,
                                    const float* __restrict__ xn,
                                    float* __restrict__ dmin,
                                    int* __restrict__ amin,
                                    float* __restrict__ dmin2, long long m,
                                    int n_groups) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= m) return;
  float v = INFINITY, v2 = INFINITY;
  int vi = MASKED ? MASKED_NN_NONE : 0;
  for (int g = 0; g < n_groups; g++) {
    const long long o = (long long)g * m + row;
    top2_merge<MASKED>(v, v2, vi, pd[o], pd2[o], pi[o]);
  }
  if (MASKED && vi == MASKED_NN_NONE) {
    dmin[row] = INFINITY;
    amin[row] = -1;
    dmin2[row] = INFINITY;
    return;
  }
  const float x = xn[row];
  dmin[row] = fmaxf(v + x, 0.f);
  amin[row] = vi;
  if (dmin2) dmin2[row] = v2 + x;
}

template <bool MASKED>
inline void launch_l2nn_combine(const float* pd, const float* pd2, const int* pi,
                                const float* xn, float* dmin, int* amin,
                                float* dmin2, long long m, int n_groups,
                                hipStream_t stream) {
  hipLaunchKernelGGL(l2nn_combine_kernel<MASKED>, dim3((unsigned)((m + 255) / 256)),
                     dim3(256), 0, stream, pd, pd2, pi, xn, dmin, amin, dmin2, m,
                     n_groups);
}

}  // namespace raft_amd
