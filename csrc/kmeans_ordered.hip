// k-means update + verify fed by a native row ordering.
//
// launch_kmeans_order_rows sorts the rows by label (a stable counting sort)
// and decides per row, in natural order, whether the row must rescan;
// launch_kmeans_update_verify_ordered then walks the rows exactly as
// kmeans_update_verify_kernel does (kmeans_walk.h) with the X row as its only
// gather. Together they replace sort + cast + three per-row gathers and, for
// a caller that reads neither dmin nor amin afterwards, the per-row stores.

#include <hip/hip_runtime.h>

#include "common.h"
#include "kmeans_walk.h"

namespace raft_amd {

template <int MAX_DREG, bool VEC4, int R, bool WRITE_BACK>
KMUV_BOUNDS(MAX_DREG, R)
__global__ void kmeans_update_verify_ordered_kernel(
    const float* __restrict__ x, const unsigned* __restrict__ order,
    const int* __restrict__ offsets, const float* __restrict__ c,
    float* __restrict__ dmin, int* __restrict__ amin, float* __restrict__ sums,
    float* __restrict__ counts, float* __restrict__ inertia_acc,
    long long n_rows, long long d, int n_centroids, long long chunk) {
  kmuv_walk<MAX_DREG, VEC4, R, true, WRITE_BACK>(
      x, reinterpret_cast<const int*>(order), offsets, c, nullptr, dmin, amin,
      nullptr, nullptr, sums, counts, inertia_acc, n_rows, d, n_centroids, chunk,
      0.f, 0.f);
}
#undef KMUV_BOUNDS

void launch_kmeans_update_verify_ordered(const float* x, const unsigned* order,
                                         const int* offsets, const float* c,
                                         float* dmin, int* amin, float* sums,
                                         float* counts, float* inertia_acc,
                                         long long n_rows, long long d,
                                         int n_centroids, bool write_back,
                                         hipStream_t stream) {
  const KmuvShape s = kmuv_shape(n_rows, d);
#define KMUV_LAUNCH(MD, V4, WB)                                                \
  hipLaunchKernelGGL((kmeans_update_verify_ordered_kernel<MD, V4, MD == 4 ? KMUV_ROWS_D4 : KMUV_ROWS_D16, WB>), \
                     dim3(s.grid), dim3(256), 0, stream, x, order, offsets, c, \
                     dmin, amin, sums, counts, inertia_acc, n_rows, d,         \
                     n_centroids, s.chunk)
#define KMUV_LAUNCH_WB(MD, V4) \
  do { if (write_back) KMUV_LAUNCH(MD, V4, true); else KMUV_LAUNCH(MD, V4, false); } while (0)
  if (d <= 256) {
    if (s.v4) KMUV_LAUNCH_WB(4, true); else KMUV_LAUNCH_WB(4, false);
  } else {
    if (s.v4) KMUV_LAUNCH_WB(16, true); else KMUV_LAUNCH_WB(16, false);
  }
#undef KMUV_LAUNCH_WB
#undef KMUV_LAUNCH
}

// Row ordering for the ordered update/verify: a stable counting sort of the
// rows by label, in place of a general sort of (label, int64 index) pairs and
// a cast. A block owns KM_ORDER_ROWS consecutive rows and a wave a quarter of
// them, so "rows ascending inside a key" is block order, then wave order,
// then lane order.
//   hist         table[b][key] = rows of key in block b (LDS histogram)
//   group_sums   gsum[g][key]  = the same summed over group g of the blocks
//   offsets      gsum -> its exclusive scan over g; offsets = scan over keys
//   block_bases  table[b][key] -> first position of block b's rows of key
//   scatter      per wave: its own histogram again, bases per wave, then 16
//                steps of 64 rows; the lanes of a step that share a key find
//                each other by ballots over the key's bits, the lowest of them
//                takes the wave's counter for that key, and each row goes to
//                counter + its rank among them. No atomics decide an order.
// Each order word also carries, in bit 31, whether the row must rescan.
// Labels outside [0, k) are clamped into it: the walk takes a row's key from
// offsets, so no label can index past the sums.
constexpr int KM_ORDER_ITEMS = 16;
constexpr int KM_ORDER_ROWS = 256 * KM_ORDER_ITEMS;
constexpr int KM_ORDER_GROUPS = 32;
constexpr int KM_ORDER_MAX_K = 4096;   // 4 waves x k counters in 64 KiB of LDS

__device__ __forceinline__ int km_clamp_key(int key, int k) {
  return min(max(key, 0), k - 1);
}

__global__ void __launch_bounds__(256)
kmeans_order_hist_kernel(const int* __restrict__ amin, int* __restrict__ table,
                         long long n_rows, int k) {
  extern __shared__ int km_lds[];
  for (int j = threadIdx.x; j < k; j += 256) km_lds[j] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * KM_ORDER_ROWS;
#pragma unroll
  for (int it = 0; it < KM_ORDER_ITEMS; it++) {
    const long long row = base + it * 256 + threadIdx.x;
    if (row < n_rows) atomicAdd(&km_lds[km_clamp_key(amin[row], k)], 1);
  }
  __syncthreads();
  int* out = table + (long long)blockIdx.x * k;
  for (int j = threadIdx.x; j < k; j += 256) out[j] = km_lds[j];
}

__global__ void __launch_bounds__(256)
kmeans_order_group_sums_kernel(const int* __restrict__ table, int* __restrict__ gsum,
                               long long n_blocks, int k, long long per_group) {
  const int key = blockIdx.x * 256 + threadIdx.x;
  if (key >= k) return;
  const long long b0 = blockIdx.y * per_group;
  const long long b1 = min(b0 + per_group, n_blocks);
  int s = 0;
  for (long long b = b0; b < b1; b++) s += table[b * k + key];
  gsum[(long long)blockIdx.y * k + key] = s;
}

__global__ void __launch_bounds__(256)
kmeans_order_offsets_kernel(int* __restrict__ gsum, int* __restrict__ offsets, int k,
                            long long n_rows) {
  __shared__ int tot[KM_ORDER_MAX_K];
  __shared__ int part[256];
  for (int key = threadIdx.x; key < k; key += 256) {
    int t[KM_ORDER_GROUPS];
#pragma unroll
    for (int g = 0; g < KM_ORDER_GROUPS; g++) t[g] = gsum[g * k + key];
    int run = 0;
#pragma unroll
    for (int g = 0; g < KM_ORDER_GROUPS; g++) {
      gsum[g * k + key] = run;
      run += t[g];
    }
    tot[key] = run;
  }
  __syncthreads();
  const int seg = (k + 255) / 256;
  const int lo = min((int)threadIdx.x * seg, k), hi = min(lo + seg, k);
  int s = 0;
  for (int j = lo; j < hi; j++) s += tot[j];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < 256; t++) {
      const int v = part[t];
      part[t] = run;
      run += v;
    }
    offsets[k] = (int)n_rows;
  }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int j = lo; j < hi; j++) {
    offsets[j] = run;
    run += tot[j];
  }
}

__global__ void __launch_bounds__(256)
kmeans_order_block_bases_kernel(int* __restrict__ table, const int* __restrict__ gsum,
                                const int* __restrict__ offsets, long long n_blocks,
                                int k, long long per_group) {
  const int key = blockIdx.x * 256 + threadIdx.x;
  if (key >= k) return;
  const long long b0 = blockIdx.y * per_group;
  const long long b1 = min(b0 + per_group, n_blocks);
  int run = offsets[key] + gsum[(long long)blockIdx.y * k + key];
  for (long long b = b0; b < b1; b++) {
    const int t = table[b * k + key];
    table[b * k + key] = run;
    run += t;
  }
}

__global__ void __launch_bounds__(256)
kmeans_order_scatter_kernel(const int* __restrict__ amin,
                            const float* __restrict__ dmin,
                            const float* __restrict__ dmin2,
                            const float* __restrict__ xn,
                            const float* __restrict__ cn_max_p,
                            const int* __restrict__ table,
                            unsigned* __restrict__ order, long long n_rows, int k,
                            int key_bits, float lead, float tail) {
  extern __shared__ int km_lds[];
  constexpr int NW = 256 / RAFT_AMD_WAVE;
  const int lane = threadIdx.x % RAFT_AMD_WAVE, wave = threadIdx.x / RAFT_AMD_WAVE;
  int* mine = km_lds + wave * k;
  for (int j = threadIdx.x; j < NW * k; j += 256) km_lds[j] = 0;
  __syncthreads();
  const float cn_max = *cn_max_p;
  const long long wave_base = (long long)blockIdx.x * KM_ORDER_ROWS +
                              (long long)wave * (KM_ORDER_ROWS / NW);
  // key in the low bits, the rescan decision in bit 31, -1 past the last row
  int kf[KM_ORDER_ITEMS];
#pragma unroll
  for (int it = 0; it < KM_ORDER_ITEMS; it++) {
    const long long row = wave_base + it * RAFT_AMD_WAVE + lane;
    kf[it] = -1;
    if (row < n_rows) {
      const int key = km_clamp_key(amin[row], k);
      const bool near = kmuv_near(dmin2[row] - dmin[row], xn[row], cn_max, lead, tail);
      kf[it] = key | (near ? (int)KM_ORDER_NEAR : 0);
      atomicAdd(&mine[key], 1);
    }
  }
  __syncthreads();
  // counts per wave -> first position per wave: the block's base, then the
  // waves before this one
  const int* bases = table + (long long)blockIdx.x * k;
  for (int j = threadIdx.x; j < k; j += 256) {
    int run = bases[j];
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const int t = km_lds[w * k + j];
      km_lds[w * k + j] = run;
      run += t;
    }
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int it = 0; it < KM_ORDER_ITEMS; it++) {
    const long long row = wave_base + it * RAFT_AMD_WAVE + lane;
    const bool valid = kf[it] != -1;
    const int key = kf[it] & (int)~KM_ORDER_NEAR;
    // the lanes of this step that hold the same key
    unsigned long long same = __ballot(valid);
    for (int b = 0; b < key_bits; b++) {
      const bool bit = (key >> b) & 1;
      const unsigned long long set = __ballot(valid && bit);
      same &= bit ? set : ~set;
    }
    if (!valid) same = 0;
    const int rank = __popcll(same & below);
    int pos = 0;
    if (valid && rank == 0) {
      pos = mine[key];
      mine[key] = pos + __popcll(same);
    }
    pos = __shfl(pos, same ? __ffsll((long long)same) - 1 : lane, RAFT_AMD_WAVE) + rank;
    if (valid)
      order[pos] = (unsigned)row | ((unsigned)kf[it] & KM_ORDER_NEAR);
    // the next step's lanes read the counters this step's lanes wrote
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

long long kmeans_order_rows_workspace(long long n_rows, int k) {
  const long long n_blocks = (n_rows + KM_ORDER_ROWS - 1) / KM_ORDER_ROWS;
  return (n_blocks + KM_ORDER_GROUPS) * k;
}

int kmeans_order_rows_max_k() { return KM_ORDER_MAX_K; }

void launch_kmeans_order_rows(const int* amin, const float* dmin, const float* dmin2,
                              const float* xn, const float* cn_max_dev, float lead,
                              float tail, long long n_rows, int k, int* offsets,
                              unsigned* order, int* workspace, hipStream_t stream) {
  const long long n_blocks = (n_rows + KM_ORDER_ROWS - 1) / KM_ORDER_ROWS;
  const long long per_group = (n_blocks + KM_ORDER_GROUPS - 1) / KM_ORDER_GROUPS;
  int* table = workspace;
  int* gsum = workspace + n_blocks * k;
  int key_bits = 0;
  while ((1 << key_bits) < k) key_bits++;
  const dim3 by_key((k + 255) / 256, KM_ORDER_GROUPS);
  hipLaunchKernelGGL(kmeans_order_hist_kernel, dim3((unsigned)n_blocks), dim3(256),
                     k * sizeof(int), stream, amin, table, n_rows, k);
  hipLaunchKernelGGL(kmeans_order_group_sums_kernel, by_key, dim3(256), 0, stream,
                     table, gsum, n_blocks, k, per_group);
  hipLaunchKernelGGL(kmeans_order_offsets_kernel, dim3(1), dim3(256), 0, stream, gsum,
                     offsets, k, n_rows);
  hipLaunchKernelGGL(kmeans_order_block_bases_kernel, by_key, dim3(256), 0, stream,
                     table, gsum, offsets, n_blocks, k, per_group);
  hipLaunchKernelGGL(kmeans_order_scatter_kernel, dim3((unsigned)n_blocks), dim3(256),
                     4 * k * sizeof(int), stream, amin, dmin, dmin2, xn, cn_max_dev,
                     table, order, n_rows, k, key_bits, lead, tail);
}


}  // namespace raft_amd
