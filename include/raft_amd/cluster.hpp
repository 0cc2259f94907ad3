// k-means device primitives (csrc/kmeans.hip): keyed row reductions, the
// fused one-X-pass update+verify kernel, and centroid helpers.
#pragma once

#include "core.hpp"

namespace raft_amd {

// naive atomic keyed reduction (small n) — workspace holds `replicas` copies
void launch_reduce_rows_by_key(const float* x, const int* keys, float* workspace,
                               float* out, long long n_rows, long long d,
                               long long n_keys, int replicas, hipStream_t s);
// sort-based: perm/keys_sorted from an argsort of keys; atomics only at run
// boundaries; fused per-key counts
// dmin/inertia_acc (optional, nullable): accumulate sum(dmin[perm[i]]) into
// inertia_acc[0] in the same pass (the k-means inertia fold)
void launch_reduce_rows_by_key_sorted(const float* x, const int* perm,
                                      const int* keys_sorted, float* sums,
                                      float* counts, const float* dmin,
                                      float* inertia_acc, long long n_rows,
                                      long long d, hipStream_t s);
// fused one-X-pass centroid-sum accumulation + exact-fp32 verify/refine of
// rows whose split-error margin is inconclusive (the bf16x2v engine's
// update step)
// lead/tail: margin-bound constants of the split mode that produced
// dmin/dmin2 (defaults = the bf16x2v engine; bf16x1v uses 2^-7 / 2^-12 —
// see csrc/kmeans.hip l2nn_verify_repair_kernel for the derivation)
void launch_kmeans_update_verify(const float* x, const int* perm,
                                 const int* keys_sorted, const float* c,
                                 const float* xn, float* dmin, int* amin,
                                 const float* dmin2, const float* cn_max_dev,
                                 float* sums, float* counts, float* inertia_acc,
                                 long long n_rows, long long d, int n_centroids,
                                 hipStream_t s, float lead = 0x1p-13f,
                                 float tail = 0x1p-18f);
// the same update with the row order made natively (csrc/kmeans_ordered.hip).
// launch_kmeans_order_rows: stable counting sort of the rows by label.
// offsets[k + 1]: position i holds a row of key j iff offsets[j] <= i <
// offsets[j + 1]; order[n_rows]: row index in bits 0..30, in bit 31 whether
// the row must rescan (the decision launch_kmeans_update_verify takes from
// dmin2 - dmin, xn, cn_max, lead, tail). Labels are clamped into [0, k).
// Needs 1 <= n_rows < 2^31, 1 <= k <= kmeans_order_rows_max_k() and a
// workspace of kmeans_order_rows_workspace(n_rows, k) ints; no host sync, no
// allocation.
long long kmeans_order_rows_workspace(long long n_rows, int k);
int kmeans_order_rows_max_k();
void launch_kmeans_order_rows(const int* amin, const float* dmin, const float* dmin2,
                              const float* xn, const float* cn_max_dev, float lead,
                              float tail, long long n_rows, int k, int* offsets,
                              unsigned* order, int* workspace, hipStream_t s);
// launch_kmeans_update_verify_ordered: per wave the same rows, arithmetic and
// order as launch_kmeans_update_verify on the stable sort of the labels, the
// X row its only gather. write_back = false stores neither dmin nor amin
// (both may then be null); sums, counts and inertia_acc are as with true.
void launch_kmeans_update_verify_ordered(const float* x, const unsigned* order,
                                         const int* offsets, const float* c,
                                         float* dmin, int* amin, float* sums,
                                         float* counts, float* inertia_acc,
                                         long long n_rows, long long d,
                                         int n_centroids, bool write_back,
                                         hipStream_t s);
// split fp32 -> nslice bf16 slices + squared row norms in one pass
// cn_max (optional): fused max(cn) into one device float (zeroed first)
void launch_split_bf16_norms(const float* c, void* s0, void* s1, void* s2, float* cn,
                             int nslice, long long n_rows, long long d, hipStream_t s,
                             float* cn_max = nullptr);
void launch_kmeans_update_centroids(const float* sums, const float* counts, float* c,
                                    long long k, long long d, hipStream_t s);

}  // namespace raft_amd
