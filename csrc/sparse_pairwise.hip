// Sparse (CSR x CSR) pairwise distances — wave64, gfx950.
//
// Reference parity (WHAT): raft/sparse/distance (pairwise distances between
// the rows of two CSR matrices) and the distance step of raft/sparse/neighbors
// brute-force kNN. HOW differs: the reference runs a semiring SpMV with a
// second "B-only" pass; here every metric is written as
//
//   sum_c f(a_c, b_c) = sum_c f(a_c, 0) + sum_c f(0, b_c)
//                     + sum_{c in nz(a) & nz(b)} g(a_c, b_c),
//   g(a, b) = f(a, b) - f(a, 0) - f(0, b),          f(0, 0) = 0
//
// so only S = sum g is pairwise and it touches only columns stored in both
// rows. g(a, b) vanishes whenever a == 0 or b == 0, so a stored explicit zero
// needs no special case, as long as the row statistics are sums of f(v, 0)
// over the stored VALUES (never counts of stored entries).
//
// Kernel: a 256-thread block owns R = 4 consecutive A rows and one contiguous
// split of B's rows. It stages the A rows in LDS once — a dense [R][W] slab
// over a window of W columns, or one open-addressing table per A row — and
// streams B's CSR past them in tiles of JT rows: one wave per B row, lanes
// stride over the row's stored entries, each lane keeps R partial sums, one
// shared butterfly reduces all R of them per B row. The [R][JT] results go
// through LDS and leave as coalesced row segments with the metric's epilogue
// applied.
// Rows too long for one table (or d wider than one window) take several
// passes; S is additive, so earlier passes park the partial S in `out`, later
// passes read the block's own partials back, the last applies the epilogue.
// No block reads another block's output; no atomics on global memory.
//
// Input contract: column ids within a row may be unsorted but must be unique
// (duplicates give an unspecified finite result). Column ids outside [0, d)
// and indptr values outside [0, nnz] are ignored / clamped, never dereferenced.

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace raft_amd {

namespace {

// metric codes: keep in sync with SparseDistanceCode (include/raft_amd/sparse.hpp)
// and _SPARSE_CODES (raft_amd/sparse/distance.py)
enum : int {
  SP_IP = 0, SP_L2 = 1, SP_L2SQRT = 2, SP_COS = 3, SP_CORR = 4, SP_L1 = 5,
  SP_LP = 6, SP_CANBERRA = 7, SP_HAMMING = 8, SP_JS = 9, SP_HELLINGER = 10,
  SP_JACCARD = 11, SP_DICE = 12, SP_RUSSELRAO = 13, SP_NCODES = 14,
};

// the per-pair function family g is built from
enum : int { K_DOT = 0, K_L1, K_LP, K_CANBERRA, K_HAMMING, K_JS, K_HELLINGER };

inline int kind_of(int metric) {
  switch (metric) {
    case SP_L1: return K_L1;
    case SP_LP: return K_LP;
    case SP_CANBERRA: return K_CANBERRA;
    case SP_HAMMING: return K_HAMMING;
    case SP_JS: return K_JS;
    case SP_HELLINGER: return K_HELLINGER;
    default: return K_DOT;
  }
}

constexpr int BLOCK = 256;
constexpr int NWAVE = BLOCK / RAFT_AMD_WAVE;
constexpr int R = 4;    // A rows per block
constexpr int JT = 64;  // B rows per output tile (R * JT == BLOCK: one output per thread)
static_assert(R * JT == BLOCK, "output tile is written one element per thread");
constexpr int RPW = JT / NWAVE;  // B rows of a tile per wave
static_assert(R == 4 && RPW < RAFT_AMD_WAVE, "wave_reduce_sum4 / row-offset lanes");

constexpr int DENSE_WINDOW_MAX = 8192;
// "auto" takes the dense slab up to this many columns: a 64 KiB slab still
// lets two blocks share a CU. Measured (8192^2 rows, 64 per row, L1): dense
// 4.0 / 7.5 / 16.3 ms against hash 8.0 / 9.0 / 9.0 ms at d = 2048 / 4096 / 8192.
constexpr int DENSE_AUTO_MAX = 4096;
constexpr int HASH_CAP_MIN = 64;
constexpr int HASH_CAP_MAX = 4096;
constexpr float HALF_LN2 = 0.34657359027997264f;

// f(v, 0) — the ONE definition shared by the row statistics and by g below,
// so the statistics and the intersection correction cannot drift apart.
// (JS / Hellinger clamp negative entries to 0 first, as the dense kernels do.)
template <int KIND>
__device__ __forceinline__ float sp_f0(float v, float p) {
  if constexpr (KIND == K_L1) return fabsf(v);
  if constexpr (KIND == K_LP) return powf(fabsf(v), p);
  if constexpr (KIND == K_CANBERRA || KIND == K_HAMMING) return v != 0.f ? 1.f : 0.f;
  if constexpr (KIND == K_JS) return HALF_LN2 * fmaxf(v, 0.f);
  return 0.f;  // K_DOT, K_HELLINGER: f(a, b) is a product
}

// g(a, b) = f(a, b) - f(a, 0) - f(0, b); exactly 0 when either side is 0
template <int KIND>
__device__ __forceinline__ float sp_g(float a, float b, float p) {
  if constexpr (KIND == K_JS || KIND == K_HELLINGER) {
    a = fmaxf(a, 0.f);
    b = fmaxf(b, 0.f);
  }
  if (a == 0.f || b == 0.f) return 0.f;
  float f;
  if constexpr (KIND == K_DOT) f = a * b;
  if constexpr (KIND == K_L1) f = fabsf(a - b);
  if constexpr (KIND == K_LP) f = powf(fabsf(a - b), p);
  if constexpr (KIND == K_CANBERRA) f = fabsf(a - b) / (fabsf(a) + fabsf(b));
  if constexpr (KIND == K_HAMMING) f = a != b ? 1.f : 0.f;
  if constexpr (KIND == K_JS) {
    const float mid = 0.5f * (a + b);
    f = 0.5f * (a * logf(a / mid) + b * logf(b / mid));
  }
  if constexpr (KIND == K_HELLINGER) f = sqrtf(a) * sqrtf(b);
  return (f - sp_f0<KIND>(a, p)) - sp_f0<KIND>(b, p);
}

// final value from S = sum g and the two rows' statistics (s0, s1); matches
// raft_amd/distance/pairwise.py including its clamps and zero-denominator rules
__device__ __forceinline__ float sp_epilogue(int metric, float S, float a0, float a1,
                                             float b0, float b1, float d, float p) {
  switch (metric) {
    case SP_IP: return S;
    case SP_L2: return fmaxf(a0 + b0 - 2.f * S, 0.f);
    case SP_L2SQRT: return sqrtf(fmaxf(a0 + b0 - 2.f * S, 0.f));
    case SP_COS: {
      const float na = fmaxf(sqrtf(a0), 1e-12f), nb = fmaxf(sqrtf(b0), 1e-12f);
      return fmaxf(1.f - S / (na * nb), 0.f);
    }
    case SP_CORR: {
      const float ma = a1 / d, mb = b1 / d;
      const float na = fmaxf(sqrtf(fmaxf(a0 - d * ma * ma, 0.f)), 1e-12f);
      const float nb = fmaxf(sqrtf(fmaxf(b0 - d * mb * mb, 0.f)), 1e-12f);
      return fmaxf(1.f - (S - d * ma * mb) / (na * nb), 0.f);
    }
    case SP_L1:
    case SP_CANBERRA: return a0 + b0 + S;
    case SP_LP: return powf(fmaxf(a0 + b0 + S, 0.f), 1.f / p);
    case SP_HAMMING: return (a0 + b0 + S) / d;
    case SP_JS: return sqrtf(fmaxf(a0 + b0 + S, 0.f));
    case SP_HELLINGER: return sqrtf(fmaxf(1.f - S, 0.f));
    case SP_JACCARD: {
      const float den = a0 + b0 - S;
      return den != 0.f ? 1.f - S / den : 0.f;
    }
    case SP_DICE: {
      const float den = a0 + b0;
      return den != 0.f ? 1.f - 2.f * S / den : 0.f;
    }
    case SP_RUSSELRAO: return (d - S) / d;
    default: return S;
  }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// Four wave-wide sums for 7 cross-lane exchanges instead of 24: the first two
// butterfly steps also hand each quarter of the wave one of the four values.
// Lanes 16 r .. 16 r + 15 return sum(acc[r]). The pairing tree (xor 32, 16, 8,
// 4, 2, 1) is that of wave_reduce_sum, and float addition commutes, so each
// sum is bitwise what wave_reduce_sum(acc[r]) returns.
__device__ __forceinline__ float wave_reduce_sum4(const float (&acc)[4], int lane) {
  const bool up32 = lane & 32, up16 = lane & 16;
  float k0 = up32 ? acc[2] : acc[0], k1 = up32 ? acc[3] : acc[1];
  const float s0 = up32 ? acc[0] : acc[2], s1 = up32 ? acc[1] : acc[3];
  k0 += __shfl_xor(s0, 32, RAFT_AMD_WAVE);
  k1 += __shfl_xor(s1, 32, RAFT_AMD_WAVE);
  float k = up16 ? k1 : k0;
  const float s = up16 ? k0 : k1;
  k += __shfl_xor(s, 16, RAFT_AMD_WAVE);
  for (int off = 8; off > 0; off >>= 1) k += __shfl_xor(k, off, RAFT_AMD_WAVE);
  return k;
}

// ---------------------------------------------------------------------------
// row statistics: one wave per row. The lane stride and the butterfly are the
// same as the pair kernel's walk over a B row, so on a self-join the L1
// statistic and the intersection sum of a row with itself cancel exactly.
// ---------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(BLOCK)
csr_row_stats_kernel(const int* __restrict__ indptr, const float* __restrict__ values,
                     float* __restrict__ stats, long long n_rows, int nnz, float p) {
  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  long long row = (long long)blockIdx.x * NWAVE + threadIdx.x / RAFT_AMD_WAVE;
  const long long stride = (long long)gridDim.x * NWAVE;
  for (; row < n_rows; row += stride) {
    const int lo = clampi(indptr[row], 0, nnz), hi = clampi(indptr[row + 1], 0, nnz);
    float s0 = 0.f, s1 = 0.f;
    for (int e = lo + lane; e < hi; e += RAFT_AMD_WAVE) {
      const float v = values[e];
      if constexpr (KIND == K_DOT) {
        s0 += v * v;
        s1 += v;
      } else {
        s0 += sp_f0<KIND>(v, p);
      }
    }
    s0 = wave_reduce_sum(s0);
    s1 = wave_reduce_sum(s1);
    if (lane == 0) {
      stats[2 * row] = s0;
      stats[2 * row + 1] = s1;
    }
  }
}

// ---------------------------------------------------------------------------
// pair kernel
// ---------------------------------------------------------------------------
// LDS layout (dynamic): float stage[R][JT], then
//   dense: float slab[R][W]
//   hash:  int keys[R][CAP], float vals[R][CAP]
template <int KIND, bool HASH>
__global__ void __launch_bounds__(BLOCK)
csr_pairwise_kernel(const int* __restrict__ a_indptr, const int* __restrict__ a_indices,
                    const float* __restrict__ a_values, long long m, int a_nnz,
                    const int* __restrict__ b_indptr, const int* __restrict__ b_indices,
                    const float* __restrict__ b_values, long long n, int b_nnz,
                    const float* __restrict__ a_stats, const float* __restrict__ b_stats,
                    float* __restrict__ out, int d, int metric, float p,
                    int width /* W or CAP */, long long tiles_per_split) {
  extern __shared__ float lds[];
  float* stage = lds;                     // [R][JT]
  float* slab = lds + R * JT;             // dense: [R][W]
  int* keys = (int*)(lds + R * JT);       // hash:  [R][CAP]
  float* vals = slab + (size_t)R * width; // hash:  [R][CAP]
  __shared__ int a_lo[R], a_hi[R];

  const int tid = threadIdx.x;
  const int lane = tid % RAFT_AMD_WAVE;
  const int wave = tid / RAFT_AMD_WAVE;
  const long long i0 = (long long)blockIdx.x * R;
  const long long ntiles = (n + JT - 1) / JT;
  const long long t_begin = (long long)blockIdx.y * tiles_per_split;
  const long long t_end = t_begin + tiles_per_split < ntiles ? t_begin + tiles_per_split : ntiles;
  if (t_begin >= t_end) return;  // block-uniform

  if (tid < R) {
    const long long i = i0 + tid;
    a_lo[tid] = i < m ? clampi(a_indptr[i], 0, a_nnz) : 0;
    a_hi[tid] = i < m ? clampi(a_indptr[i + 1], 0, a_nnz) : 0;
  }
  __syncthreads();

  // number of passes (block-uniform): hash = chunks of CAP/2 stored entries of
  // the longest of the R rows; dense = windows of W columns
  int npass;
  const int chunk = width >> 1;
  if constexpr (HASH) {
    int longest = 0;
    for (int r = 0; r < R; ++r) longest = max(longest, a_hi[r] - a_lo[r]);
    npass = max(1, (longest + chunk - 1) / chunk);
  } else {
    npass = max(1, (d + width - 1) / width);
    for (int k = tid; k < R * width; k += BLOCK) slab[k] = 0.f;
  }

  for (int pass = 0; pass < npass; ++pass) {
    const int w0 = HASH ? 0 : pass * width;  // dense window origin
    // ---- stage this pass's part of the A rows --------------------------------
    if constexpr (HASH) {
      for (int k = tid; k < R * width; k += BLOCK) keys[k] = -1;
      __syncthreads();
      for (int r = 0; r < R; ++r) {
        const int lo = min(a_lo[r] + pass * chunk, a_hi[r]);
        const int hi = min(lo + chunk, a_hi[r]);  // <= CAP/2 entries: never more than half full
        for (int e = lo + tid; e < hi; e += BLOCK) {
          const int col = a_indices[e];
          if ((unsigned)col >= (unsigned)d) continue;  // malformed id: ignored (-1 is the empty key)
          const float v = a_values[e];
          int h = col & (width - 1);
          for (int t = 0; t < width; ++t) {  // trip count bounded by the capacity
            const int prev = atomicCAS(&keys[r * width + h], -1, col);
            if (prev == -1 || prev == col) {
              vals[r * width + h] = v;
              break;
            }
            h = (h + 1) & (width - 1);
          }
        }
      }
    } else {
      __syncthreads();  // slab zero / un-scatter of the previous window is complete
      for (int r = 0; r < R; ++r)
        for (int e = a_lo[r] + tid; e < a_hi[r]; e += BLOCK) {
          const int col = a_indices[e];
          if ((unsigned)col >= (unsigned)d) continue;  // malformed id: ignored
          const int c = col - w0;
          if ((unsigned)c < (unsigned)width) slab[r * width + c] = a_values[e];
        }
    }
    __syncthreads();

    // ---- stream the split's B rows past the staged A rows --------------------
    for (long long t = t_begin; t < t_end; ++t) {
      const long long j0 = t * JT;
      // a wave owns RPW consecutive B rows of the tile: one coalesced read of
      // their RPW + 1 row offsets, handed out below by readlane
      const long long jw = j0 + wave * RPW;
      int ptr_lane = 0;
      if (lane <= RPW && jw + lane <= n) ptr_lane = clampi(b_indptr[jw + lane], 0, b_nnz);
      for (int k = 0; k < RPW; ++k) {
        const int jj = wave * RPW + k;
        if (jw + k >= n) break;  // wave-uniform
        const int lo = __builtin_amdgcn_readlane(ptr_lane, k);
        const int hi = __builtin_amdgcn_readlane(ptr_lane, k + 1);
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        for (int e = lo + lane; e < hi; e += RAFT_AMD_WAVE) {
          const int col = b_indices[e];
          const float bv = b_values[e];
          if ((unsigned)col >= (unsigned)d) continue;  // malformed id: ignored
          if constexpr (HASH) {
            const int h0 = col & (width - 1);
#pragma unroll
            for (int r = 0; r < R; ++r) {
              int h = h0;
              for (int k = 0; k < width; ++k) {  // bounded by the capacity
                const int key = keys[r * width + h];
                if (key == col) {
                  acc[r] += sp_g<KIND>(vals[r * width + h], bv, p);
                  break;
                }
                if (key == -1) break;
                h = (h + 1) & (width - 1);
              }
            }
          } else {
            const int c = col - w0;
            if ((unsigned)c >= (unsigned)width) continue;
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] += sp_g<KIND>(slab[r * width + c], bv, p);
          }
        }
        const float s = wave_reduce_sum4(acc, lane);
        if ((lane & 15) == 0) stage[(lane >> 4) * JT + jj] = s;
      }
      __syncthreads();
      // ---- coalesced write of the [R][JT] tile: partial S or final value -----
      {
        const int r = tid / JT, jj = tid % JT;
        const long long i = i0 + r, j = j0 + jj;
        if (i < m && j < n) {
          float* o = out + i * n + j;  // 64-bit indexing
          float S = stage[r * JT + jj];
          if (pass > 0) S += *o;  // this block's own partial from the earlier passes
          if (pass == npass - 1)
            S = sp_epilogue(metric, S, a_stats[2 * i], a_stats[2 * i + 1], b_stats[2 * j],
                            b_stats[2 * j + 1], (float)d, p);
          *o = S;
        }
      }
      __syncthreads();  // stage is reused by the next tile
    }

    // ---- dense: clear this window's entries instead of re-zeroing the slab ---
    if constexpr (!HASH) {
      if (pass + 1 < npass)
        for (int r = 0; r < R; ++r)
          for (int e = a_lo[r] + tid; e < a_hi[r]; e += BLOCK) {
            const int col = a_indices[e];
            if ((unsigned)col >= (unsigned)d) continue;
            const int c = col - w0;
            if ((unsigned)c < (unsigned)width) slab[r * width + c] = 0.f;
          }
    }
  }
}

inline bool is_pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

template <int KIND, bool HASH>
void launch_pair(const int* a_indptr, const int* a_indices, const float* a_values, long long m,
                 long long a_nnz, const int* b_indptr, const int* b_indices,
                 const float* b_values, long long n, long long b_nnz, const float* a_stats,
                 const float* b_stats, float* out, long long d, int metric, float p, int width,
                 hipStream_t stream) {
  const long long groups = (m + R - 1) / R;
  const long long ntiles = (n + JT - 1) / JT;
  // 2-D grid (A-row group, B split): enough blocks for 256 CUs when m is small
  long long nsplit = (1024 + groups - 1) / groups;
  if (nsplit > ntiles) nsplit = ntiles;
  if (nsplit > 1024) nsplit = 1024;
  if (nsplit < 1) nsplit = 1;
  const long long tiles_per_split = (ntiles + nsplit - 1) / nsplit;
  nsplit = (ntiles + tiles_per_split - 1) / tiles_per_split;
  const size_t lds = (size_t)R * JT * 4 + (size_t)R * width * (HASH ? 8 : 4);
  static bool attr_set = false;
  if (!attr_set) {
    // the largest request: the staging tile plus a 128 KiB slab / table set
    // (the kernel's few static LDS bytes must fit under 160 KiB next to it)
    constexpr int max_lds = R * JT * 4 + R * DENSE_WINDOW_MAX * 4;
    static_assert(R * HASH_CAP_MAX * 8 == R * DENSE_WINDOW_MAX * 4, "one LDS budget");
    HIP_CHECK(hipFuncSetAttribute((const void*)&csr_pairwise_kernel<KIND, HASH>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
    attr_set = true;
  }
  hipLaunchKernelGGL((csr_pairwise_kernel<KIND, HASH>), dim3((unsigned)groups, (unsigned)nsplit),
                     dim3(BLOCK), lds, stream, a_indptr, a_indices, a_values, m, (int)a_nnz,
                     b_indptr, b_indices, b_values, n, (int)b_nnz, a_stats, b_stats, out, (int)d,
                     metric, p, width, tiles_per_split);
  HIP_CHECK(hipGetLastError());
}

template <typename F>
void dispatch_kind(int metric, F&& f) {
  switch (kind_of(metric)) {
    case K_L1: f(std::integral_constant<int, K_L1>{}); break;
    case K_LP: f(std::integral_constant<int, K_LP>{}); break;
    case K_CANBERRA: f(std::integral_constant<int, K_CANBERRA>{}); break;
    case K_HAMMING: f(std::integral_constant<int, K_HAMMING>{}); break;
    case K_JS: f(std::integral_constant<int, K_JS>{}); break;
    case K_HELLINGER: f(std::integral_constant<int, K_HELLINGER>{}); break;
    default: f(std::integral_constant<int, K_DOT>{}); break;
  }
}

void check_metric(int metric) {
  if (metric < 0 || metric >= SP_NCODES)
    throw std::invalid_argument("sparse pairwise: unknown metric code " + std::to_string(metric));
}

}  // namespace

void launch_csr_row_stats(const int* indptr, const float* values, float* stats,
                          long long n_rows, long long nnz, int metric, float p,
                          hipStream_t stream) {
  check_metric(metric);
  if (n_rows <= 0 || nnz <= 0) return;
  if (nnz > 2147483647ll) throw std::invalid_argument("sparse pairwise: nnz >= 2^31");
  long long blocks = (n_rows + NWAVE - 1) / NWAVE;
  if (blocks > 1048576) blocks = 1048576;
  dispatch_kind(metric, [&](auto kc) {
    constexpr int KIND = decltype(kc)::value;
    hipLaunchKernelGGL((csr_row_stats_kernel<KIND>), dim3((unsigned)blocks), dim3(BLOCK), 0,
                       stream, indptr, values, stats, n_rows, (int)nnz, p);
  });
  HIP_CHECK(hipGetLastError());
}

void launch_csr_pairwise(const int* a_indptr, const int* a_indices, const float* a_values,
                         long long m, long long a_nnz, const int* b_indptr,
                         const int* b_indices, const float* b_values, long long n,
                         long long b_nnz, const float* a_stats, const float* b_stats,
                         float* out, long long d, int metric, float p, int strategy,
                         int param, hipStream_t stream) {
  check_metric(metric);
  if (strategy < 0 || strategy > 2)
    throw std::invalid_argument("sparse pairwise: unknown strategy " + std::to_string(strategy));
  if (m <= 0 || n <= 0) return;
  if (d <= 0 || d > 2147483647ll || a_nnz > 2147483647ll || b_nnz > 2147483647ll || a_nnz < 0 ||
      b_nnz < 0)
    throw std::invalid_argument("sparse pairwise: d and nnz must be in [0, 2^31)");
  if ((m + R - 1) / R > 2147483647ll)
    throw std::invalid_argument("sparse pairwise: too many rows for one launch");
  if (strategy == 0) strategy = d <= DENSE_AUTO_MAX ? 1 : 2;
  int width = param;
  if (strategy == 1) {
    if (width == 0) {
      // one window over all of d when it fits, rounded up to a power of two
      width = 64;
      while (width < d && width < DENSE_WINDOW_MAX) width <<= 1;
    }
    if (!is_pow2(width) || width > DENSE_WINDOW_MAX)
      throw std::invalid_argument("sparse pairwise: dense_window must be a power of two <= " +
                                  std::to_string(DENSE_WINDOW_MAX));
  } else {
    if (width == 0) {
      // 8 slots per stored entry at the mean row length (known on the host
      // without a device sync): most probes of a B column end at the first,
      // empty, slot. Measured at 8192^2 rows, d = 65536, 64 per row: 2x
      // slots took 2.4 times as long as 8x, 4x 1.3 times, 16x 0.9 times
      // (docs/performance.md).
      // A chunk never fills more than half the table; longer rows take
      // several chunks.
      const long long mean = (a_nnz + m - 1) / m;
      width = HASH_CAP_MIN;
      while (width < 8 * mean && width < HASH_CAP_MAX) width <<= 1;
    }
    if (!is_pow2(width) || width < HASH_CAP_MIN || width > HASH_CAP_MAX)
      throw std::invalid_argument("sparse pairwise: hash_capacity must be a power of two in [" +
                                  std::to_string(HASH_CAP_MIN) + ", " +
                                  std::to_string(HASH_CAP_MAX) + "]");
  }
  dispatch_kind(metric, [&](auto kc) {
    constexpr int KIND = decltype(kc)::value;
    if (strategy == 1)
      launch_pair<KIND, false>(a_indptr, a_indices, a_values, m, a_nnz, b_indptr, b_indices,
                               b_values, n, b_nnz, a_stats, b_stats, out, d, metric, p, width,
                               stream);
    else
      launch_pair<KIND, true>(a_indptr, a_indices, a_values, m, a_nnz, b_indptr, b_indices,
                              b_values, n, b_nnz, a_stats, b_stats, out, d, metric, p, width,
                              stream);
  });
}

}  // namespace raft_amd
