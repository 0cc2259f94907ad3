// Masked fused L2 nearest-neighbor: for every row of x, the nearest row of y
// among the GROUPS of y that a per-row mask allows, plus the exact verify /
// repair pass that makes the fp32 result provably the unexpanded-fp32 argmin.
//
// Reference parity (WHAT): the historical raft::distance::masked_l2_nn (and,
// through x_group, the nearest cross-component pair under
// raft::sparse::neighbors::cross_component_nn / connect_components). HOW is
// CDNA4-native: the 128x128 split-bf16 MFMA tile of fused_l2nn.hip /
// eps_neighbors.hip (same geometry, same K-loop); the mask is applied to the
// accumulator in registers and a tile the mask excludes entirely never runs
// its K-loop.
//
// Mask model: y rows are grouped, rows of one group contiguous (y_group is
// non-decreasing). A column of group g is allowed for row i iff
//   (adj == null  or  bit g of adj row i is set)  and  g != x_group[i]
// (x_group == null excludes nothing). adj is the core/bitset.py layout:
// 32-bit little-endian words, every row on a word boundary.
//
// Grid: 1D, block = (row tile, column split). A block walks the column tiles
// of its split with the running (best, second-best, index) triple in
// registers, as fused_l2nn_kernel does, and writes one partial triple per row;
// l2nn_combine_kernel<true> (l2nn_top2.h) merges the splits, adds ||x||^2 and
// turns "no candidate" into (+inf, -1).
//
// Tile skip: before the K-loop the block decides whether any (row, column)
// pair of the tile is allowed. With adj, each row builds the tile's 128-bit
// column mask in LDS (one adj lookup per group change, the group ids of the
// tile staged in LDS); the same mask then serves the epilogue. Without adj the
// tile is dead only when all its columns are one group and no live row's
// x_group differs from it.
//
// Exactness (docs/verified_engines.md, "Masked L2-NN exactness"): second-best
// is taken over ALLOWED candidates only, so margin > 2E proves the emulated
// argmin equals the exact one over the allowed set; every other row rescans.

#include <hip/hip_runtime.h>

#include "l2nn_engine.h"
#include "l2nn_top2.h"

namespace raft_amd {

template <int NSLICE, bool HAS_ADJ>
__launch_bounds__(256, 2)
__global__ void masked_l2nn_kernel(const __bf16* __restrict__ x0,
                                   const __bf16* __restrict__ x1,
                                   const __bf16* __restrict__ c0,
                                   const __bf16* __restrict__ c1,
                                   const float* __restrict__ yn,
                                   const int* __restrict__ y_group,
                                   const unsigned int* __restrict__ adj,
                                   const int* __restrict__ x_group,
                                   float* __restrict__ pd,
                                   float* __restrict__ pd2,
                                   int* __restrict__ pi,
                                   unsigned long long* __restrict__ counters,
                                   long long m, int n, int d,
                                   long long adj_words, int n_split,
                                   int tiles_per_split) {
  extern __shared__ __bf16 smem[];
  __bf16* xs[NSLICE];
  __bf16* cs[NSLICE];
  const __bf16* const xg[3] = {x0, x1, x0};
  const __bf16* const cg[3] = {c0, c1, c0};
#pragma unroll
  for (int s = 0; s < NSLICE; s++) {
    xs[s] = smem + s * 8192;
    cs[s] = smem + (NSLICE + s) * 8192;
  }
  // mask state lives past the staging tiles: it must survive the K-loop
  int* xgs = reinterpret_cast<int*>(smem + NSLICE * 2 * 8192);        // [128]
  int* ygs = xgs + 128;                                               // [128]
  unsigned int* masks = reinterpret_cast<unsigned int*>(ygs + 128);   // [128][4]

  const int t = threadIdx.x;
  const int lane = t % RAFT_AMD_WAVE;
  const int w = t / RAFT_AMD_WAVE;
  const int wr = w >> 1, wc = w & 1;  // 2x2 wave grid
  const int sp = blockIdx.x % n_split;
  const long long row0 = (long long)(blockIdx.x / n_split) * 128;
  const int col_tiles = (n + 127) / 128;
  const int ct0 = sp * tiles_per_split;
  const int ct1 = min(ct0 + tiles_per_split, col_tiles);

  if (t < 128) {
    const long long row = min(row0 + t, m - 1);
    xgs[t] = x_group ? x_group[row] : -1;  // group ids are >= 0
  }
  __syncthreads();

  float best[4][4], best2[4][4];
  int bidx[4][4];
  top2_init(best, best2, bidx, MASKED_NN_NONE);
  unsigned int n_visited = 0, n_skipped = 0;

  for (int ct = ct0; ct < ct1; ct++) {
    const int col0 = ct * 128;
    int live = 0;
    if constexpr (HAS_ADJ) {
      if (t < 128) ygs[t] = y_group[min(col0 + t, n - 1)];
      __syncthreads();
      // thread -> (row, 64-column half); the half is wave-uniform, so the
      // group-change branch below is taken by all lanes of a wave together
      const int rl = t & 127, half = t >> 7;
      const long long row = row0 + rl;
      unsigned long long mk = 0ull;
      if (row < m) {
        const unsigned int* ar = adj + row * adj_words;
        const int xgv = xgs[rl];
        const int ncol = min(64, n - (col0 + half * 64));  // may be <= 0
        int prev = -1;
        bool ok = false;
        for (int j = 0; j < ncol; j++) {
          const int g = ygs[half * 64 + j];
          if (g != prev) {
            prev = g;
            ok = g != xgv && ((ar[g >> 5] >> (g & 31)) & 1u);
          }
          if (ok) mk |= 1ull << j;
        }
      }
      masks[rl * 4 + half * 2] = (unsigned int)mk;
      masks[rl * 4 + half * 2 + 1] = (unsigned int)(mk >> 32);
      live = mk != 0ull;
    } else {
      // the tile's columns cover the group range [g_lo, g_hi]
      const int g_lo = y_group[col0];
      const int g_hi = y_group[min(col0 + 127, n - 1)];
      if (t < 128 && row0 + t < m) live = !(g_lo == g_hi && g_lo == xgs[t]);
    }
    // block-uniform decision (and the barrier that publishes the masks)
    if (!__syncthreads_or(live)) {
      n_skipped++;
      continue;  // every score of the tile is +inf: nothing to fold
    }
    n_visited++;

    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    mfma_tile_kloop<NSLICE>(xg, cg, xs, cs, acc, row0, (long long)col0, d, m - 1,
                            (long long)n - 1, wr, wc, lane);

    // epilogue: fold the tile into each lane's LOCAL running top-2 (lanes own
    // disjoint columns, visited in ascending order: strict < keeps the
    // smallest index among equal scores). ||x||^2 is added by the combine.
    const int colb = col0 + wc * 64 + (lane & 15);
    float yn_r[4];
    int yg_r[4];
#pragma unroll
    for (int fc = 0; fc < 4; fc++) {
      const int col = colb + fc * 16;
      yn_r[fc] = col < n ? yn[col] : INFINITY;
      yg_r[fc] = HAS_ADJ ? 0 : y_group[min(col, n - 1)];
    }
#pragma unroll
    for (int fr = 0; fr < 4; fr++) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int rl = wr * 64 + fr * 16 + (lane >> 4) * 4 + reg;
        unsigned long long mk = 0ull;
        int xgv = 0;
        if constexpr (HAS_ADJ) {
          mk = (unsigned long long)masks[rl * 4 + wc * 2] |
               ((unsigned long long)masks[rl * 4 + wc * 2 + 1] << 32);
          mk >>= (lane & 15);
        } else {
          xgv = xgs[rl];
        }
#pragma unroll
        for (int fc = 0; fc < 4; fc++) {
          const bool ok = HAS_ADJ ? ((mk >> (fc * 16)) & 1ull) != 0ull
                                  : yg_r[fc] != xgv;
          const float s = ok ? yn_r[fc] - 2.f * acc[fr][fc][reg] : INFINITY;
          top2_push(best[fr][reg], best2[fr][reg], bidx[fr][reg], s, colb + fc * 16);
        }
      }
    }
  }

  // ONE cross-lane reduce, then the two column-half waves of each row combine
  // through the (dead) staging LDS ([2][128]) and one thread per row writes
  // the split's partial. Index-guarded: both halves may hold MASKED_NN_NONE.
  top2_reduce16(best, best2, bidx);
  top2_park_tile<4, 256, 1, 128>(smem, (lane & 15) == 0, wr * 64, lane, wc, best,
                                 best2, bidx);
  if (t < 128 && row0 + t < m)
    top2_write_partial<2, 256, 1, 128, true>(smem, t, pd, pd2, pi,
                                             (long long)sp * m + row0 + t);
  // one vector atomic per counter per block
  if (t == 0) {
    if (n_visited) atomicAdd(&counters[0], (unsigned long long)n_visited);
    if (n_skipped) atomicAdd(&counters[1], (unsigned long long)n_skipped);
  }
}

void launch_masked_l2nn(const void** xsl, const void** csl, const float* xn,
                        const float* yn, const int* y_group,
                        const unsigned int* adj, long long adj_words,
                        const int* x_group, float* pd, float* pd2, int* pi,
                        float* dmin, int* amin, float* dmin2,
                        unsigned long long* counters, long long m, int n, int d,
                        int n_split, int nslice, hipStream_t stream) {
  if (m <= 0) return;
  if (n <= 0 || d <= 0 || d % 64 != 0)
    throw std::runtime_error("masked_l2nn: n > 0 and d a positive multiple of 64");
  if (adj == nullptr && x_group == nullptr)
    throw std::runtime_error("masked_l2nn: adj or x_group is required");
  const int col_tiles = (n + 127) / 128;
  if (n_split < 1 || n_split > col_tiles)
    throw std::runtime_error("masked_l2nn: n_split must be in [1, ceil(n/128)]");
  const int tps = (col_tiles + n_split - 1) / n_split;
  const long long blocks = ((m + 127) / 128) * n_split;
  if (blocks > 2147483647ll)
    throw std::runtime_error("masked_l2nn: grid too large, chunk the rows");
  const bool has_adj = adj != nullptr;
  const SlicePtrs p(xsl, csl, nslice);
  const size_t lds = (size_t)nslice * 2 * 8192 * sizeof(__bf16) +
                     (128 + 128 + 512) * sizeof(int);
  const dim3 grid((unsigned)blocks);
  if (nslice == 2) {
    // two slices + the mask state pass the 64 KiB default dynamic-LDS limit
    static bool attr_set = false;
    if (!attr_set) {
      HIP_CHECK(hipFuncSetAttribute((const void*)&masked_l2nn_kernel<2, true>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    72 * 1024));
      HIP_CHECK(hipFuncSetAttribute((const void*)&masked_l2nn_kernel<2, false>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    72 * 1024));
      attr_set = true;
    }
  }
#define RAFT_MASKED_NN_LAUNCH(NS, ADJ)                                          \
  hipLaunchKernelGGL((masked_l2nn_kernel<NS, ADJ>), grid, dim3(256), lds,       \
                     stream, p.x[0], p.x[1], p.c[0], p.c[1], yn, y_group, adj,  \
                     x_group, pd, pd2, pi, counters, m, n, d, adj_words, n_split, \
                     tps)
  if (nslice == 1 && has_adj) RAFT_MASKED_NN_LAUNCH(1, true);
  else if (nslice == 1) RAFT_MASKED_NN_LAUNCH(1, false);
  else if (nslice == 2 && has_adj) RAFT_MASKED_NN_LAUNCH(2, true);
  else if (nslice == 2) RAFT_MASKED_NN_LAUNCH(2, false);
  else throw std::runtime_error("masked_l2nn: nslice must be 1 or 2");
#undef RAFT_MASKED_NN_LAUNCH
  launch_l2nn_combine<true>(pd, pd2, pi, xn, dmin, amin, dmin2, m, n_split, stream);
}

// ---------------------------------------------------------------------------
// Masked verify / repair. Three launches, no host sync:
//  1. verify: one wave per row, the (lead, tail) bound of
//     l2nn_verify_repair_kernel (csrc/kmeans.hip) with yn_max over ALL y rows
//     (a superset of the allowed ones: conservative). A row inside the bound
//     is appended to the rescan list; every other row recomputes its chosen
//     distance exactly.
//  2. rescan: the listed rows x 2048-column chunks are spread over the whole
//     grid (a wave-per-row serial walk of all n columns is latency-bound:
//     0.046 s -> 0.020 s per call at 65536 x 128 with 2.8 % of the rows
//     listed, docs/performance.md "Masked L2-NN").
//     Each wave walks its columns in ascending order, skips disallowed
//     groups, takes the exact fp32 distance and keeps the strict minimum;
//     waves merge through one 64-bit atomicMin per row on
//     (distance bits << 32 | tie key). Distances are sums of squares (>= +0),
//     so their bit patterns order like the values, and the key — the column
//     index, or the caller's rank — makes exact ties resolve to the smallest.
//  3. finish: unpack the listed rows' keys into (dmin, amin).
// The result is the minimum over the allowed columns of one fixed exact
// function, so it does not depend on how columns are spread over waves.
// ---------------------------------------------------------------------------

constexpr int MASKED_NN_RESCAN_CHUNK = 2048;  // columns per block work item

// lane-strided partial of the unexpanded fp32 distance; every caller finishes
// it with wave_reduce_sum, so all exact distances are sums in one order
__device__ __forceinline__ float masked_nn_partial_d2(const float* __restrict__ xp,
                                                      const float* __restrict__ yp,
                                                      int df, int lane) {
  float a = 0.f;
  for (int k = lane; k < df; k += RAFT_AMD_WAVE) {
    const float diff = xp[k] - yp[k];
    a = fmaf(diff, diff, a);
  }
  return a;
}

__global__ void masked_l2nn_verify_kernel(
    const float* __restrict__ x, const float* __restrict__ y,
    const float* __restrict__ xn, float* __restrict__ dmin,
    const int* __restrict__ amin, const float* __restrict__ dmin2,
    const float* __restrict__ yn_max_p, int* __restrict__ rescan_rows,
    unsigned int* __restrict__ rescan_count, unsigned long long* __restrict__ keys,
    long long m, int n, int df, float lead, float tail) {
  const float yn_max = *yn_max_p;
  const long long waves_per_block = blockDim.x / RAFT_AMD_WAVE;
  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  long long row = (long long)blockIdx.x * waves_per_block + threadIdx.x / RAFT_AMD_WAVE;
  const long long stride = (long long)gridDim.x * waves_per_block;
  for (; row < m; row += stride) {
    const int a = amin[row];
    if (a < 0 || a >= n) continue;  // no allowed column: stays (+inf, -1)
    const float xnr = xn[row];
    const float margin = dmin2[row] - dmin[row];
    const float bound = 2.f * (lead * sqrtf(fmaxf(xnr * yn_max, 0.f)) +
                               tail * (xnr + yn_max));
    // <=: with zero norms the bound is 0 and an exact tie has margin 0
    if (margin <= bound) {
      if (lane == 0) {
        // every row appends at most once: slot < m
        const unsigned int slot = atomicAdd(rescan_count, 1u);
        rescan_rows[slot] = (int)row;
        keys[row] = ~0ull;
      }
    } else {
      const float v = wave_reduce_sum(masked_nn_partial_d2(
          x + row * (long long)df, y + (long long)a * df, df, lane));
      if (lane == 0) dmin[row] = v;
    }
  }
}

__launch_bounds__(256)
__global__ void masked_l2nn_rescan_kernel(
    const float* __restrict__ x, const float* __restrict__ y,
    const int* __restrict__ y_group, const unsigned int* __restrict__ adj,
    const int* __restrict__ x_group, const int* __restrict__ y_rank,
    const int* __restrict__ rescan_rows, const unsigned int* __restrict__ rescan_count,
    unsigned long long* __restrict__ keys, int n, int df, long long adj_words,
    int n_chunks) {
  const long long count = *rescan_count;
  const long long items = count * n_chunks;
  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const int w = threadIdx.x / RAFT_AMD_WAVE;
  // chunk-major item order: blocks running together share a y chunk in L2
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long row = rescan_rows[it % count];
    const int c0 = (int)(it / count) * MASKED_NN_RESCAN_CHUNK;
    const int c1 = min(c0 + MASKED_NN_RESCAN_CHUNK, n);
    const float* xp = x + row * (long long)df;
    const unsigned int* ar = adj ? adj + row * adj_words : nullptr;
    const int xgv = x_group ? x_group[row] : -1;
    float bestv = INFINITY;
    unsigned int bestk = 0xffffffffu;
    bool found = false;
    int prev = -1;
    bool ok = false;
    // wave w takes 4 adjacent columns of every 16, ascending; the 4 partial
    // sums and reductions are independent (latency hiding)
    for (int j0 = c0 + w * 4; j0 < c1; j0 += 16) {
      float a[4];
      bool al[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int j = j0 + u;
        al[u] = false;
        a[u] = 0.f;
        if (j < c1) {
          const int g = y_group[j];
          if (g != prev) {  // wave-uniform
            prev = g;
            ok = g != xgv && (!ar || ((ar[g >> 5] >> (g & 31)) & 1u));
          }
          al[u] = ok;
        }
        if (al[u]) a[u] = masked_nn_partial_d2(xp, y + (long long)j * df, df, lane);
      }
#pragma unroll
      for (int u = 0; u < 4; u++) a[u] = wave_reduce_sum(a[u]);
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (!al[u]) continue;
        const unsigned int key = y_rank ? (unsigned int)y_rank[j0 + u]
                                        : (unsigned int)(j0 + u);
        if (!found || a[u] < bestv || (a[u] == bestv && key < bestk)) {
          bestv = a[u];
          bestk = key;
          found = true;
        }
      }
    }
    if (lane == 0 && found)
      atomicMin(&keys[row], ((unsigned long long)__float_as_uint(bestv) << 32) | bestk);
  }
}

__global__ void masked_l2nn_rescan_finish_kernel(
    const int* __restrict__ rescan_rows, const unsigned int* __restrict__ rescan_count,
    const unsigned long long* __restrict__ keys, const int* __restrict__ inv_rank,
    float* __restrict__ dmin, int* __restrict__ amin,
    unsigned long long* __restrict__ rescanned) {
  const unsigned int count = *rescan_count;
  const unsigned int tid = blockIdx.x * blockDim.x + threadIdx.x;
  for (unsigned int i = tid; i < count; i += gridDim.x * blockDim.x) {
    const int row = rescan_rows[i];
    const unsigned long long key = keys[row];
    if (key == ~0ull) continue;  // cannot happen: a listed row has a candidate
    const unsigned int k = (unsigned int)key;
    dmin[row] = __uint_as_float((unsigned int)(key >> 32));
    amin[row] = inv_rank ? inv_rank[k] : (int)k;
  }
  if (tid == 0 && count) atomicAdd(rescanned, (unsigned long long)count);
}

void launch_masked_l2nn_verify_repair(const float* x, const float* y, const float* xn,
                                      const int* y_group, const unsigned int* adj,
                                      long long adj_words, const int* x_group,
                                      const int* y_rank, const int* inv_rank,
                                      float* dmin, int* amin, const float* dmin2,
                                      const float* yn_max_dev, int* rescan_rows,
                                      unsigned int* rescan_count,
                                      unsigned long long* keys,
                                      unsigned long long* rescanned, long long m,
                                      int n, int df, float lead, float tail,
                                      hipStream_t stream) {
  if (m <= 0 || n <= 0) return;
  if ((y_rank == nullptr) != (inv_rank == nullptr))
    throw std::runtime_error("masked_l2nn_verify_repair: y_rank needs its inverse");
  HIP_CHECK(hipMemsetAsync(rescan_count, 0, sizeof(unsigned int), stream));
  // one wave per row; the kernel grid-strides past the grid cap
  const long long blocks = (m * RAFT_AMD_WAVE + 255) / 256;
  const int grid = (int)(blocks > 2147483647ll ? 2147483647ll : blocks);
  hipLaunchKernelGGL(masked_l2nn_verify_kernel, dim3(grid), dim3(256), 0, stream, x,
                     y, xn, dmin, amin, dmin2, yn_max_dev, rescan_rows, rescan_count,
                     keys, m, n, df, lead, tail);
  // the listed-row count stays on the device: a fixed grid strides the items
  const int n_chunks = (n + MASKED_NN_RESCAN_CHUNK - 1) / MASKED_NN_RESCAN_CHUNK;
  const long long most = m * n_chunks;
  hipLaunchKernelGGL(masked_l2nn_rescan_kernel, dim3((unsigned)(most < 8192 ? most : 8192)),
                     dim3(256), 0, stream, x, y, y_group, adj, x_group, y_rank,
                     rescan_rows, rescan_count, keys, n, df, adj_words, n_chunks);
  const long long fb = (m + 255) / 256;
  hipLaunchKernelGGL(masked_l2nn_rescan_finish_kernel, dim3((unsigned)(fb < 1024 ? fb : 1024)),
                     dim3(256), 0, stream, rescan_rows, rescan_count, keys, inv_rank,
                     dmin, amin, rescanned);
}

}  // namespace raft_amd
