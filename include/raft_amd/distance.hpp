// Pairwise distances (csrc/pairwise.hip, csrc/pairwise_metrics.hip,
// csrc/pairwise_mfma.hip).
// The fp32 L2 path runs as split-bf16 slice products on MFMA (no fp32 MFMA
// on CDNA4): xsl/csl are nslice in {1,2,3} bf16 slice pointers.
#pragma once

#include "core.hpp"

namespace raft_amd {

void launch_l2_epilogue(float* g, const float* xn, const float* yn, long long m,
                        long long n, hipStream_t s);
void launch_l2nn_epilogue(const float* g, const float* xn, const float* yn,
                          float* dmin, int* amin, long long m, long long n, hipStream_t s);
// code = DistanceCode
void launch_pairwise_unexpanded(const float* x, const float* y, float* out, long long m,
                                long long n, long long d, int code, float p, hipStream_t s);
// in-place expanded-form epilogue over a GEMM result g[m,n] = <x_i, y_j>
// (csrc/pairwise_metrics.hip); code = ExpandedDistanceCode, d = feature
// count (Russel-Rao). xa[m]/ya[n] = squared row norms, read by Jaccard and
// Dice only (may be null for Hellinger / Russel-Rao)
void launch_pairwise_expanded_epilogue(float* g, const float* xa, const float* ya,
                                       long long m, long long n, int code, float d,
                                       hipStream_t s);
// 128x128-tile MFMA kernel; out[ldo] row stride; epilogue fused into the
// single non-temporal C write. launch_pairwise_l2_mfma and
// launch_pairwise_l2_filter apply the tuning environment
// (docs/developer_guide.md); launch_pairwise_l2_mfma256 is the 256x256-tile
// writer, nslice 1 or 2
void launch_pairwise_l2_mfma(const void** xsl, const void** csl, const float* xn,
                             const float* yn, float* out, long long m, long long n,
                             int d, long long ldo, int nslice, bool sqrt_out, hipStream_t s);
void launch_pairwise_l2_mfma256(const void** xsl, const void** csl, const float* xn,
                                const float* yn, float* out, long long m, long long n,
                                int d, long long ldo, int nslice, bool sqrt_out,
                                hipStream_t s);
// filtered variant (kNN candidate emission below per-row thresholds)
void launch_pairwise_l2_filter(const void** xsl, const void** csl, const float* xn,
                               const float* yn, const float* thresh, float* out_d,
                               int* out_i, int* counts, int cap, long long col_offset,
                               long long m, long long n, int d, int nslice,
                               hipStream_t s);

}  // namespace raft_amd
