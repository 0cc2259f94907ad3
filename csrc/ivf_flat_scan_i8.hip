// IVF-Flat list scan over int8 / uint8 rows: the integer sibling of
// ivf_flat_scan.hip. Same index layout (V = 16 one-byte elements per 16-byte
// chunk, rows interleaved in groups of 64), same work decomposition (work item
// = (list, up to QG sorted (query, probe) pairs), grid x bounded on the host,
// blocks past *n_items_p exit, gridDim.y splits the 64-row groups, 256
// threads, lane = row, no cross-lane reduction in the scan) and the same
// validation of item, offset and output ranges before any address is formed.
//
// What differs is the arithmetic: gfx950's 8-bit dot product (v_dot4) does
// four multiply-adds into an int32 accumulator per instruction, so the scan
// issues as many instructions per loaded byte as the fp32 kernel and its
// result is EXACT.
//
// Staging: the item's queries go to LDS as packed bytes [QG][d_pad] (bytes
// past d are zero), followed by int qnorm[QG], the sum of q^2 of every staged
// query. Query rows are [n_queries][d] bytes with any d, so they are not
// 4-byte aligned in general: a thread gathers the 4 bytes of one LDS dword
// with byte loads, adds the dword's dot4 with itself to its partial norm, and
// the wave's partials are folded with shuffles into one LDS atomic add
// (integer, hence order-independent).
//
// Loop: per 16-byte chunk the lane loads its row's 16 bytes once; per staged
// query it reads the query's 16 bytes as one LDS broadcast (every lane the
// same address) and issues four dot4 into acc[qi], a statically indexed, fully
// unrolled array. For L2 the lane also accumulates nx += dot4(x, x) once per
// chunk, shared by all queries: 4 extra dot4 against 4 * QG. Row norms are
// not stored in the index.
//
// Epilogue: L2 = nx + qnorm[qi] - 2 * acc[qi] in int32, IP = acc[qi];
// converted with one (float); euclidean is (float)sqrt((double)v). Pad rows
// and rows the filter rejects get +inf (-inf for inner product).
//
// Range: the launcher serves d_pad <= 4096. |x|, |q| <= 255, so every partial
// sum of nx, qnorm and acc is bounded in magnitude by 255^2 * 4096 =
// 266,342,400, and the largest intermediate of the epilogue is
// nx + qnorm <= 2 * 255^2 * 4096 = 532,684,800 < 2^31 (2 * acc has the same
// bound; for int8, |acc| <= 128^2 * 4096 = 2^26). No int32 overflows, so the
// dot4 clamp is off and the int32 values are the exact integers.

#include <hip/hip_runtime.h>

#include <stdexcept>

#include "common.h"

namespace raft_amd {

int ivf_flat_scan_max_qg(int d_pad, int elem_size);

template <bool SIGNED>
static __device__ __forceinline__ int ivf_dot4(unsigned int a, unsigned int b, int c) {
  if constexpr (SIGNED)
    return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
  else
    return (int)__builtin_amdgcn_udot4(a, b, (unsigned int)c, false);
}

template <bool SIGNED>
static __device__ __forceinline__ int ivf_dot16(const uint4& a, const uint4& b, int c) {
  c = ivf_dot4<SIGNED>(a.x, b.x, c);
  c = ivf_dot4<SIGNED>(a.y, b.y, c);
  c = ivf_dot4<SIGNED>(a.z, b.z, c);
  return ivf_dot4<SIGNED>(a.w, b.w, c);
}

// one 64-row group against the staged queries; gp is the lane's first chunk.
// FULL: all QG slots are live (no guard in the loop); otherwise slot qi is
// live iff qi < nq (wave-uniform). Returns the row's sum of squares (0 for IP)
template <bool SIGNED, int QG, bool IP, bool FULL>
static __device__ __forceinline__ int ivf_scan_group_i8(const uint4* __restrict__ gp,
                                                        const uint4* __restrict__ qs,
                                                        int chunks, int nq,
                                                        int (&acc)[QG]) {
#pragma unroll
  for (int qi = 0; qi < QG; qi++) acc[qi] = 0;
  int nx = 0;
#pragma unroll 2
  for (int j = 0; j < chunks; j++) {
    const uint4 x = gp[(long long)j * RAFT_AMD_WAVE];
    if constexpr (!IP) nx = ivf_dot16<SIGNED>(x, x, nx);
#pragma unroll
    for (int qi = 0; qi < QG; qi++) {
      if (FULL || qi < nq) acc[qi] = ivf_dot16<SIGNED>(x, qs[qi * chunks + j], acc[qi]);
    }
  }
  return nx;
}

template <bool SIGNED, int QG, bool IP>
__launch_bounds__(256)
__global__ void ivf_flat_scan_i8_kernel(
    const unsigned char* __restrict__ data, const long long* __restrict__ list_offsets,
    const long long* __restrict__ indices, const unsigned char* __restrict__ queries,
    const long long* __restrict__ item_list,
    const long long* __restrict__ item_pair_begin,
    const long long* __restrict__ item_pair_count,
    const long long* __restrict__ n_items_p,
    const long long* __restrict__ pair_query,
    const long long* __restrict__ pair_out_off,
    const unsigned int* __restrict__ filter_words, long long filter_bits,
    float* __restrict__ out, long long out_numel, long long n_lists,
    long long total_rows, long long n_queries, long long n_pairs, int d, int d_pad,
    bool sqrt_out) {
  // [QG][d_pad] bytes, then int qnorm[QG]
  extern __shared__ __attribute__((aligned(16))) unsigned int ivf_qb[];

  // every exit below is block-uniform and precedes the barriers
  if ((long long)blockIdx.x >= *n_items_p) return;
  const long long l = item_list[blockIdx.x];
  const long long pb = item_pair_begin[blockIdx.x];
  const long long npair = item_pair_count[blockIdx.x];
  if (l < 0 || l >= n_lists || npair < 1 || npair > QG || pb < 0 || pb + npair > n_pairs)
    return;
  const long long r0 = list_offsets[l], r1 = list_offsets[l + 1];
  if (r0 < 0 || r1 < r0 || r1 > total_rows || (r0 | r1) % RAFT_AMD_WAVE) return;
  const int nq = (int)npair;

  const int t = threadIdx.x;
  const int lane = t % RAFT_AMD_WAVE;
  const int w = t / RAFT_AMD_WAVE;
  const int words = d_pad / 4;
  int* qnorm = reinterpret_cast<int*>(ivf_qb + QG * words);
  if (t < QG) qnorm[t] = 0;
  __syncthreads();
  for (int qi = 0; qi < nq; qi++) {
    const long long qrow = pair_query[pb + qi];
    const bool qok = qrow >= 0 && qrow < n_queries;  // else zeros, never stored
    const unsigned char* qp = queries + (qok ? qrow : 0) * (long long)d;
    int s = 0;
    for (int k = t; k < words; k += 256) {
      unsigned int u = 0;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int e = 4 * k + b;
        if (qok && e < d) u |= (unsigned int)qp[e] << (8 * b);
      }
      ivf_qb[qi * words + k] = u;
      s = ivf_dot4<SIGNED>(u, u, s);
    }
#pragma unroll
    for (int m = RAFT_AMD_WAVE / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0 && s != 0) atomicAdd(&qnorm[qi], s);
  }
  __syncthreads();

  const int chunks = d_pad / 16;
  const uint4* qs = reinterpret_cast<const uint4*>(ivf_qb);
  const long long g0 = r0 / RAFT_AMD_WAVE, g1 = r1 / RAFT_AMD_WAVE;
  const long long gstride = (long long)gridDim.y * 4;
  const float bad = IP ? -INFINITY : INFINITY;
  for (long long g = g0 + (long long)blockIdx.y * 4 + w; g < g1; g += gstride) {
    const long long row = g * RAFT_AMD_WAVE + lane;
    const long long id = indices[row];
    bool ok = id >= 0;
    if (ok && filter_words)
      ok = id < filter_bits && ((filter_words[id >> 5] >> (id & 31)) & 1u);
    const uint4* gp = reinterpret_cast<const uint4*>(data) +
                      (g * chunks * RAFT_AMD_WAVE + lane);
    int acc[QG];
    int nx;
    if (nq == QG)
      nx = ivf_scan_group_i8<SIGNED, QG, IP, true>(gp, qs, chunks, nq, acc);
    else
      nx = ivf_scan_group_i8<SIGNED, QG, IP, false>(gp, qs, chunks, nq, acc);
    const long long in_list = row - r0;
#pragma unroll
    for (int qi = 0; qi < QG; qi++) {
      if (qi < nq) {
        const int iv = IP ? acc[qi] : nx + qnorm[qi] - 2 * acc[qi];
        const float v = sqrt_out ? (float)sqrt((double)iv) : (float)iv;
        const long long qrow = pair_query[pb + qi];
        const long long o = pair_out_off[pb + qi] + in_list;
        if (qrow >= 0 && qrow < n_queries && o >= 0 && o < out_numel)
          out[o] = ok ? v : bad;
      }
    }
  }
}

void launch_ivf_flat_scan_i8(const void* data, bool data_signed,
                             const long long* list_offsets, const long long* indices,
                             const void* queries, const long long* item_list,
                             const long long* item_pair_begin,
                             const long long* item_pair_count, const long long* n_items,
                             const long long* pair_query, const long long* pair_out_off,
                             const unsigned int* filter_words, long long filter_bits,
                             float* out, long long out_numel, long long n_lists,
                             long long total_rows, long long n_queries, long long n_pairs,
                             long long max_items, int d, int metric, int qg, int y_split,
                             hipStream_t stream) {
  if (max_items <= 0 || n_pairs <= 0 || total_rows <= 0) return;
  if (d < 1) throw std::runtime_error("ivf_flat_scan_i8: d must be positive");
  if (d > 4096)
    throw std::runtime_error("ivf_flat_scan_i8: d_pad must be <= 4096 (int32 range)");
  const int d_pad = (d + 15) / 16 * 16;
  if (qg != 4 && qg != 8 && qg != 16 && qg != 32)
    throw std::runtime_error("ivf_flat_scan_i8: qg must be 4, 8, 16 or 32");
  if (qg > ivf_flat_scan_max_qg(d_pad, 1))
    throw std::runtime_error("ivf_flat_scan_i8: qg * (d_pad + 4) must fit 64 KiB of LDS");
  if (metric < 0 || metric > 2)
    throw std::runtime_error("ivf_flat_scan_i8: metric must be 0 (L2), 1 (L2 sqrt) or 2 (IP)");
  if (y_split < 1 || y_split > 65535 || max_items > 2147483647ll)
    throw std::runtime_error("ivf_flat_scan_i8: grid out of range");
  const dim3 grid((unsigned)max_items, (unsigned)y_split);
  const size_t lds = (size_t)qg * d_pad + (size_t)qg * sizeof(int);
  const bool sqrt_out = metric == 1;
#define RAFT_IVF_I8_LAUNCH(S, QG, IP)                                              \
  hipLaunchKernelGGL((ivf_flat_scan_i8_kernel<S, QG, IP>), grid, dim3(256), lds,   \
                     stream, static_cast<const unsigned char*>(data), list_offsets, \
                     indices, static_cast<const unsigned char*>(queries), item_list, \
                     item_pair_begin, item_pair_count, n_items, pair_query,        \
                     pair_out_off, filter_words, filter_bits, out, out_numel,      \
                     n_lists, total_rows, n_queries, n_pairs, d, d_pad, sqrt_out)
#define RAFT_IVF_I8_QG(S, IP)                                                      \
  switch (qg) {                                                                    \
    case 4: RAFT_IVF_I8_LAUNCH(S, 4, IP); break;                                   \
    case 8: RAFT_IVF_I8_LAUNCH(S, 8, IP); break;                                   \
    case 16: RAFT_IVF_I8_LAUNCH(S, 16, IP); break;                                 \
    default: RAFT_IVF_I8_LAUNCH(S, 32, IP); break;                                 \
  }
  if (data_signed) {
    if (metric == 2) { RAFT_IVF_I8_QG(true, true) } else { RAFT_IVF_I8_QG(true, false) }
  } else {
    if (metric == 2) { RAFT_IVF_I8_QG(false, true) } else { RAFT_IVF_I8_QG(false, false) }
  }
#undef RAFT_IVF_I8_QG
#undef RAFT_IVF_I8_LAUNCH
  HIP_CHECK(hipGetLastError());
}

}  // namespace raft_amd
