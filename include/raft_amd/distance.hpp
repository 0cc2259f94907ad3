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

// int8 (is_signed) / uint8 rows on the 8-bit integer MFMA
// (csrc/pairwise_i8.hip). Operands are row-major bytes [rows][d_pad],
// d_pad % 128 == 0 and <= 4096, 16-byte aligned, pad bytes 0 (int8) or 128
// (uint8). launch_row_stats_i8 writes every row's sum of squares and sum in
// the domain the kernels work in (uint8 shifted by -128). metric: 0 squared
// L2, 1 its root, 2 inner product (xsum / ysum and d_real, the unpadded d,
// are read for uint8 inner product only). out[m][n] gets the exact integer
// converted to fp32 once; metric 1 the fp64 root rounded to fp32.
void launch_row_stats_i8(const void* x, bool is_signed, int* norm, int* sum, long long rows,
                         int d_pad, hipStream_t s);
void launch_pairwise_i8(const void* x, const void* y, bool is_signed, const int* xnorm,
                        const int* xsum, const int* ynorm, const int* ysum, float* out,
                        long long m, long long n, int d_pad, int d_real, int metric,
                        hipStream_t s);
// squared L2 <= thresh[row] (exact int32) into the per-row candidate buffers,
// as launch_pairwise_l2_filter; col_offset + n must fit int32
void launch_pairwise_i8_filter(const void* x, const void* y, bool is_signed, const int* xnorm,
                               const int* ynorm, const int* thresh, float* out_d, int* out_i,
                               int* counts, int cap, long long col_offset, long long m,
                               long long n, int d_pad, hipStream_t s);

// Bitwise Hamming over bit-packed rows on the vector ALU (xor + popcount,
// csrc/pairwise_bits.hip). Operands are row-major bytes [rows][nbytes_pad],
// nbytes_pad % 16 == 0 and <= 2^21, 16-byte aligned, pad bytes 0, rows below
// 2^31. out[m][n] gets the count of differing bits as fp32 (exact).
void launch_pairwise_bits(const void* x, const void* y, float* out, long long m, long long n,
                          int nbytes_pad, hipStream_t s);
// count <= thresh[row] into the per-row candidate buffers, as
// launch_pairwise_i8_filter; col_offset + n must fit int32
void launch_pairwise_bits_filter(const void* x, const void* y, const int* thresh, float* out_d,
                                 int* out_i, int* counts, int cap, long long col_offset,
                                 long long m, long long n, int nbytes_pad, hipStream_t s);
// out[rows][ceil(d / 8)]: bit j % 8 of byte j / 8 is x[row * ld + j] > threshold,
// compared in fp32; dtype 0 fp32, 1 bf16, 2 fp16
void launch_pack_bits(const void* x, int dtype, unsigned char* out, long long rows,
                      long long d, long long ld, float threshold, hipStream_t s);

}  // namespace raft_amd
