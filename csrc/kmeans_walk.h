// The k-means update + verify walk: one body for the sorted-label kernel
// (kmeans.hip) and the ordered kernel (kmeans_ordered.hip), with the launch
// shape both use.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

namespace raft_amd {

// Fused centroid-update + exact-fp32 verify/refine in ONE X pass.
// Rows arrive key-sorted, so the chosen centroid row is run-constant and
// lives in registers; each row's x fragment is loaded once and used for BOTH
// the exact distance refinement and the centroid-sum accumulation. Rows
// inside the split-error margin rescan all centroids exactly (rare); a
// rescan that CHANGES the assignment routes that row's contribution to the
// new cluster via direct atomics (and fixes amin/dmin).
// VEC4: lane-contiguous column map col(j) = (j/4)*256 + lane*4 + j%4 so each
// lane's 4-column chunk loads as ONE dwordx4 (wave covers 1024 B/chunk);
// requires d % 4 == 0. Otherwise the classic col(j) = j*64 + lane scalar map.
// R: rows in flight per wave. A wave walks its chunk in batches of R rows:
// first the R perm / key loads, then the R per-row scalars, then all R row
// loads, and only then the per-row work, row by row in the original order.
// One row at a time (a dependent perm load, a 1 KiB row load, a 6-step wave
// reduction, strictly serial) left 8 MiB in flight across the chip and the
// kernel at 3.5 TB/s. Per wave every floating-point add and every write
// keeps its order, so results move only with the atomic order between waves.
//
// Two kernels share this one walk. ORDERED = false: the rows' order comes as
// perm / keys_sorted from a sort of the labels, and the wave gathers xn, dmin
// and dmin2 per row to decide whether the row rescans. ORDERED = true: the
// order comes from launch_kmeans_order_rows as one packed word per row (row
// index, and in bit 31 that same decision, made while the per-row values
// streamed past in natural order) plus the k + 1 run boundaries, so the X row
// is the wave's only gather. WRITE_BACK = false leaves dmin / amin alone (a
// caller that reads neither afterwards): sums, counts and the inertia are
// the same either way.

// the rescan decision: one expression for both places that take it
__device__ __forceinline__ bool kmuv_near(float margin, float xnr, float cn_max,
                                          float lead, float tail) {
  const float bound = 2.f * (lead * sqrtf(fmaxf(xnr * cn_max, 0.f)) +
                             tail * (xnr + cn_max));
  return margin < bound;
}

constexpr unsigned KM_ORDER_NEAR = 0x80000000u;  // bit 31 of an order word

template <int MAX_DREG, bool VEC4, int R, bool ORDERED, bool WRITE_BACK>
__device__ __forceinline__ void kmuv_walk(
    const float* __restrict__ x, const int* __restrict__ perm,
    const int* __restrict__ keys_sorted, const float* __restrict__ c,
    const float* __restrict__ xn, float* __restrict__ dmin,
    int* __restrict__ amin, const float* __restrict__ dmin2,
    const float* __restrict__ cn_max_p, float* __restrict__ sums,
    float* __restrict__ counts, float* __restrict__ inertia_acc,
    long long n_rows, long long d, int n_centroids, long long chunk,
    float lead, float tail) {
  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const long long wave_id =
      ((long long)blockIdx.x * blockDim.x + threadIdx.x) / RAFT_AMD_WAVE;
  const long long start = wave_id * chunk;
  if (start >= n_rows) return;
  const long long stop = min(start + chunk, n_rows);
  float cn_max = 0.f;
  if constexpr (!ORDERED) cn_max = *cn_max_p;
  // ORDERED: perm holds the order words and keys_sorted the k + 1 offsets.
  // pos_key is the key whose run holds the position the walk stands at
  // (offsets[pos_key] <= i < pos_end = offsets[pos_key + 1]): found once by
  // bisection, then advanced past run ends, empty runs included. Every
  // position is below n_rows = offsets[k], so pos_key stays below k.
  const int* __restrict__ offsets = keys_sorted;
  int pos_key = 0;
  long long pos_end = 0;
  if constexpr (ORDERED) {
    int lo = 0, hi = n_centroids;      // first j in (0, k] with offsets[j] > start
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((long long)offsets[mid] > start) hi = mid; else lo = mid;
    }
    pos_key = hi - 1;
    pos_end = offsets[hi];
  }

  float acc[MAX_DREG], creg[MAX_DREG];
#pragma unroll
  for (int j = 0; j < MAX_DREG; j++) acc[j] = 0.f;
  int cur_key = -1;
  int run_len = 0;
  double local_inertia = 0.0;

  auto colmap = [&](int j) -> long long {
    if constexpr (VEC4)
      return (long long)(j >> 2) * (RAFT_AMD_WAVE * 4) + lane * 4 + (j & 3);
    else
      return (long long)j * RAFT_AMD_WAVE + lane;
  };
  auto load_row = [&](const float* __restrict__ rp, float* dst) {
    if constexpr (VEC4) {
      #pragma unroll
      for (int q = 0; q < (MAX_DREG + 3) / 4; q++) {
        const long long base = (long long)q * (RAFT_AMD_WAVE * 4) + lane * 4;
        if (base + 3 < d) {
          const float4 t = *reinterpret_cast<const float4*>(rp + base);
          dst[q * 4 + 0] = t.x; dst[q * 4 + 1] = t.y;
          dst[q * 4 + 2] = t.z; dst[q * 4 + 3] = t.w;
        } else {
          for (int jj = 0; jj < 4 && q * 4 + jj < MAX_DREG; jj++) {
            const long long col = base + jj;
            dst[q * 4 + jj] = col < d ? rp[col] : 0.f;
          }
        }
      }
    } else {
      #pragma unroll
      for (int j = 0; j < MAX_DREG; j++) {
        const long long col = colmap(j);
        dst[j] = col < d ? rp[col] : 0.f;
      }
    }
  };

  auto flush = [&]() {
    if (cur_key < 0) return;
    float* sp = sums + (long long)cur_key * d;
    #pragma unroll
    for (int j = 0; j < MAX_DREG; j++) {
      const long long col = colmap(j);
      if (col < d) atomicAdd(&sp[col], acc[j]);
      acc[j] = 0.f;
    }
    if (lane == 0 && run_len) atomicAdd(&counts[cur_key], (float)run_len);
    run_len = 0;
  };

  // the three steps of one row, its operands already in registers
  auto enter_key = [&](int key) {
    if (key != cur_key) {
      flush();
      cur_key = key;
      load_row(c + (long long)key * d, creg);
    }
  };
  // exact fp32 refinement of the chosen distance (creg is run-resident)
  auto refine = [&](long long row, const float (&xv)[MAX_DREG]) {
    float a = 0.f;
    #pragma unroll
    for (int j = 0; j < MAX_DREG; j++) {
      const float diff = xv[j] - creg[j];
      a += diff * diff;
    }
    a = wave_reduce_sum(a);
    if constexpr (WRITE_BACK)
      if (lane == 0) dmin[row] = a;
    local_inertia += (double)a;
    #pragma unroll
    for (int j = 0; j < MAX_DREG; j++) acc[j] += xv[j];
    run_len++;
  };
  // exact rescan over all centroids (rare: near-ties only)
  auto rescan = [&](long long row, const float (&xv)[MAX_DREG]) {
    float bestv = INFINITY;
    int besti = 0;
    for (int jc = 0; jc < n_centroids; jc++) {
      const float* cp = c + (long long)jc * d;
      float a = 0.f;
      #pragma unroll
      for (int j = 0; j < MAX_DREG; j++) {
        const long long col = colmap(j);
        if (col < d) {
          const float diff = xv[j] - cp[col];
          a += diff * diff;
        }
      }
      a = wave_reduce_sum(a);
      if (a < bestv) { bestv = a; besti = jc; }
    }
    if constexpr (WRITE_BACK)
      if (lane == 0) {
        dmin[row] = bestv;
        amin[row] = besti;
      }
    local_inertia += (double)bestv;
    if (besti == cur_key) {
      #pragma unroll
      for (int j = 0; j < MAX_DREG; j++) acc[j] += xv[j];
      run_len++;
    } else {
      // reassigned: direct atomics into the new cluster
      float* sp = sums + (long long)besti * d;
      #pragma unroll
      for (int j = 0; j < MAX_DREG; j++) {
        const long long col = colmap(j);
        if (col < d) atomicAdd(&sp[col], xv[j]);
      }
      if (lane == 0) atomicAdd(&counts[besti], 1.f);
    }
  };

  for (long long i0 = start; i0 < stop; i0 += R) {
    // a short last batch re-reads the chunk's last row into the spare slots
    // (rows of a permutation are distinct: nothing below writes what a later
    // slot of the batch has read) and processes only the real ones
    long long row[R];
    int key[R];
    float xv[R][MAX_DREG];
    bool near[R], any_near = false;
    if constexpr (ORDERED) {
      unsigned word[R];
#pragma unroll
      for (int r = 0; r < R; r++) word[r] = (unsigned)perm[min(i0 + r, stop - 1)];
#pragma unroll
      for (int r = 0; r < R; r++) {
        row[r] = word[r] & ~KM_ORDER_NEAR;
        near[r] = (word[r] & KM_ORDER_NEAR) != 0;
        load_row(x + row[r] * d, xv[r]);
      }
#pragma unroll
      for (int r = 0; r < R; r++) {
        while (min(i0 + r, stop - 1) >= pos_end) pos_end = offsets[++pos_key + 1];
        key[r] = pos_key;
        any_near |= near[r];
      }
    } else {
      float xnr[R], margin[R];
#pragma unroll
      for (int r = 0; r < R; r++) {
        const long long i = min(i0 + r, stop - 1);
        row[r] = perm[i];
        key[r] = keys_sorted[i];
      }
#pragma unroll
      for (int r = 0; r < R; r++) {
        xnr[r] = xn[row[r]];
        margin[r] = dmin2[row[r]] - dmin[row[r]];
      }
#pragma unroll
      for (int r = 0; r < R; r++) load_row(x + row[r] * d, xv[r]);
#pragma unroll
      for (int r = 0; r < R; r++) {
        near[r] = kmuv_near(margin[r], xnr[r], cn_max, lead, tail);
        any_near |= near[r];
      }
    }
    if constexpr (R == 1) {
      enter_key(key[0]);
      if (near[0]) rescan(row[0], xv[0]);
      else refine(row[0], xv[0]);
    } else if (!any_near) {
#pragma unroll
      for (int r = 0; r < R; r++)
        if (i0 + r < stop) {
          enter_key(key[r]);
          refine(row[r], xv[r]);
        }
    } else {
      // a batch with a near-tie: ONE rolled copy of the row steps (the rescan
      // unrolled R times costs the registers that keep 8 waves per SIMD),
      // slot r picked by wave-uniform selects; same order, same arithmetic
#pragma unroll 1
      for (int r = 0; r < R && i0 + r < stop; r++) {
        long long row_r = row[0];
        int key_r = key[0];
        bool near_r = near[0];
        float xv_r[MAX_DREG];
#pragma unroll
        for (int j = 0; j < MAX_DREG; j++) xv_r[j] = xv[0][j];
#pragma unroll
        for (int q = 1; q < R; q++)
          if (r == q) {
            row_r = row[q];
            key_r = key[q];
            near_r = near[q];
#pragma unroll
            for (int j = 0; j < MAX_DREG; j++) xv_r[j] = xv[q][j];
          }
        enter_key(key_r);
        if (near_r) rescan(row_r, xv_r);
        else refine(row_r, xv_r);
      }
    }
  }
  flush();
  if (inertia_acc && lane == 0) atomicAdd(inertia_acc, (float)local_inertia);
}

// launch bounds: the waves per SIMD each variant compiles to without scratch
#define KMUV_BOUNDS(MD, R) \
  __launch_bounds__(256, MD == 4 ? (R <= 2 ? 8 : 5) : (R == 1 ? 6 : 4))

// rows in flight per wave, per registers-per-row variant. Measured (round 3,
// BASELINE.md): at 4 registers 2 rows keep 64 VGPRs and 8 waves per SIMD and
// win; 4 rows (83 VGPRs, 5 waves) and a software-pipelined next-row load both
// lose to the parent. At 16 registers 2 rows (4 waves) beat 1 row (6 waves).
constexpr int KMUV_ROWS_D4 = 2;
constexpr int KMUV_ROWS_D16 = 2;

// one chunking and one variant choice for both kernels: the same rows in the
// same order reach the same wave
struct KmuvShape {
  long long chunk;
  int grid;
  bool v4;
};
inline KmuvShape kmuv_shape(long long n_rows, long long d) {
  const long long n_waves_target = 2048 * 4;
  long long chunk = (n_rows + n_waves_target - 1) / n_waves_target;
  if (chunk < 8) chunk = 8;
  const long long n_waves = (n_rows + chunk - 1) / chunk;
  // VEC4 keeps only d/4 lanes loading (4 cols per lane): require d >= 256
  // so all 64 lanes stay active
  return {chunk, (int)((n_waves * RAFT_AMD_WAVE + 255) / 256),
          (d % 4 == 0) && d >= 256};
}

}  // namespace raft_amd
