// Sparse kernels (csrc/spmv.hip): CSR SpMV with sub-wave-per-row mapping
// (2..64 lanes chosen by mean nnz/row), uncapped grid.
#pragma once

#include "core.hpp"

namespace raft_amd {

template <typename T>
void launch_csr_spmv(const int* indptr, const int* indices, const T* values, const T* x,
                     T* y, long long n_rows, long long nnz, hipStream_t s);

// sampled dense-dense matmul: vals[e] = dot(a[rows[e]], b[cols[e]]),
// a [m, d] / b [n, d] row-major fp32 (csrc/spmv.hip)
void launch_sddmm(const float* a, const float* b, const int* rows,
                  const int* cols, float* vals, long long nnz, long long d,
                  hipStream_t stream);

// ---------------------------------------------------------------------------
// Sparse (CSR x CSR) pairwise distances (csrc/sparse_pairwise.hip).
//
// Every supported metric is sum_c f(a_c, b_c) with f(0, 0) = 0, so
//   sum_c f(a_c,b_c) = sum f(a_c,0) + sum f(0,b_c) + sum_{c in both} g(a_c,b_c)
// with g(a,b) = f(a,b) - f(a,0) - f(0,b): two per-row statistics plus ONE
// pairwise contraction S over the columns stored in both rows.
//
// Column ids within a row need not be sorted but must be unique; duplicates
// give an unspecified finite result. Column ids outside [0, d) are ignored.
// ---------------------------------------------------------------------------
enum SparseDistanceCode {
  kSparseInnerProduct = 0,
  kSparseL2 = 1,
  kSparseL2Sqrt = 2,
  kSparseCosine = 3,
  kSparseCorrelation = 4,
  kSparseL1 = 5,
  kSparseLp = 6,
  kSparseCanberra = 7,
  kSparseHamming = 8,
  kSparseJensenShannon = 9,
  kSparseHellinger = 10,
  kSparseJaccard = 11,
  kSparseDice = 12,
  kSparseRusselRao = 13,
};

enum SparsePairwiseStrategy {
  kSparseAuto = 0,   // dense when d <= kSparseDenseAutoMax, hash otherwise
  kSparseDense = 1,  // [R][W] fp32 slab over a window of W columns in LDS
  kSparseHash = 2,   // one open-addressing table per A row in LDS
};

// limits of the two staging strategies (powers of two; the Python layer
// validates overrides against the same numbers)
constexpr int kSparseDenseWindowMax = 8192;  // 4 rows x 8192 cols x 4 B = 128 KiB
constexpr int kSparseDenseAutoMax = 4096;    // 64 KiB slab: two blocks per CU
constexpr int kSparseHashCapacityMin = 64;
constexpr int kSparseHashCapacityMax = 4096;  // 4 rows x 4096 x 8 B = 128 KiB

// stats [n_rows, 2] fp32 for the metric: (sum v^2, sum v) for the dot-product
// metrics, (sum f(v, 0), 0) for the others. nnz == 0 or n_rows == 0 zero-fills
// nothing and launches nothing: the caller passes a zeroed buffer.
void launch_csr_row_stats(const int* indptr, const float* values, float* stats,
                          long long n_rows, long long nnz, int metric, float p,
                          hipStream_t stream);

// out [m, n] fp32 row-major = metric(A row i, B row j); a_stats / b_stats from
// launch_csr_row_stats with the same metric and p. strategy is a
// SparsePairwiseStrategy; param is the dense window (dense) or the table
// capacity (hash), 0 = choose. Throws std::invalid_argument on a bad
// metric / strategy / param. m == 0 or n == 0 returns without launching.
void launch_csr_pairwise(const int* a_indptr, const int* a_indices, const float* a_values,
                         long long m, long long a_nnz, const int* b_indptr,
                         const int* b_indices, const float* b_values, long long n,
                         long long b_nnz, const float* a_stats, const float* b_stats,
                         float* out, long long d, int metric, float p, int strategy,
                         int param, hipStream_t stream);

}  // namespace raft_amd
