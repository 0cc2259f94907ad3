// IVF-Flat list scan: distances from many queries to the rows of the lists
// they probe, list-major, so a list is read once per GROUP of queries instead
// of once per query.
//
// Reference parity (WHAT): the interleaved-scan step of the historical
// raft::neighbors::ivf_flat::search. HOW is CDNA4-native: the index stores
// rows interleaved in groups of 64 (the wave width) and 16-byte chunks, so a
// wave's load of chunk j of a group is 1 KiB contiguous with lane = row, and
// no cross-lane reduction exists anywhere.
//
// Index layout (raft_amd/neighbors/ivf_flat.py): V = 16 bytes of elements
// (4 fp32, 8 bf16), d_pad = d rounded up to V with zeros, every list padded
// to a multiple of 64 rows. Element (group g, chunk j, row r, v) lives at
//   ((g * (d_pad / V) + j) * 64 + r) * V + v.
// indices[row] is the dataset id, -1 in pad slots.
//
// Work item = (list, up to QG (query, probe) pairs that probe it). The host
// sorts the pairs by list with device-side torch ops and passes, per item,
// its list, the first sorted pair and the pair count, plus a DEVICE scalar
// n_items: the grid's x size is only an upper bound and blocks past n_items
// exit. gridDim.y splits a list's 64-row groups so a small batch still fills
// the chip. Per sorted pair: its query row and the int64 offset of its list
// segment in the candidate buffer.
//
// Block = 256 threads. The item's query vectors are staged in LDS as fp32
// [QG][d_pad] (QG * d_pad * 4 <= 64 KiB). Waves stride over the 64-row
// groups; per 16-byte chunk the lane loads its row's chunk once and, for each
// staged query, reads the query's chunk from LDS (every lane the same
// address: a broadcast) into per-lane accumulators that are a statically
// indexed, fully unrolled array. L2 accumulates the UNEXPANDED sum
// fma(x - q, x - q, acc): every term is non-negative, so the result is
// within (d + 3) * 2^-24 relative of the exact value in any summation order.
// Each query keeps an (even, odd) element pair of accumulators so the
// subtract and the fma are packed two-wide; they are added at the end.
//
// Epilogue: per query the 64 lanes store 64 consecutive floats at
// pair_out_off + row. Pad rows and rows the filter rejects get +inf (-inf
// for inner product).

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace raft_amd {

typedef float ivf_f32x2 __attribute__((ext_vector_type(2)));

constexpr int IVF_SCAN_LDS_BYTES = 64 * 1024;

template <typename T>
struct IvfChunk;
template <>
struct IvfChunk<float> {
  static constexpr int V = 4;
  static __device__ __forceinline__ void load(const float* p, ivf_f32x2 (&x)[2]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    x[0] = ivf_f32x2{v.x, v.y};
    x[1] = ivf_f32x2{v.z, v.w};
  }
};
template <>
struct IvfChunk<__bf16> {
  static constexpr int V = 8;
  // bf16 -> fp32 is a 16-bit shift; element 2i is the low half of dword i
  static __device__ __forceinline__ ivf_f32x2 widen(unsigned int u) {
    return ivf_f32x2{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
  }
  static __device__ __forceinline__ void load(const __bf16* p, ivf_f32x2 (&x)[4]) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    x[0] = widen(v.x);
    x[1] = widen(v.y);
    x[2] = widen(v.z);
    x[3] = widen(v.w);
  }
};

// one 64-row group against the staged queries. FULL: all QG slots are live
// (no guard in the loop); otherwise slot qi is live iff qi < nq (wave-uniform)
template <typename T, int QG, bool IP, bool FULL>
__device__ __forceinline__ void ivf_scan_group(const T* __restrict__ gp,
                                               const float* __restrict__ qs,
                                               int chunks, int d_pad, int nq,
                                               ivf_f32x2 (&acc)[QG]) {
  constexpr int V = IvfChunk<T>::V;
#pragma unroll
  for (int qi = 0; qi < QG; qi++) acc[qi] = ivf_f32x2{0.f, 0.f};
#pragma unroll 2
  for (int j = 0; j < chunks; j++) {
    ivf_f32x2 x[V / 2];
    IvfChunk<T>::load(gp + (long long)j * (RAFT_AMD_WAVE * V), x);
#pragma unroll
    for (int qi = 0; qi < QG; qi++) {
      if (FULL || qi < nq) {
        const float* qp = qs + qi * d_pad + j * V;
#pragma unroll
        for (int h = 0; h < V / 4; h++) {
          const float4 qv = *reinterpret_cast<const float4*>(qp + 4 * h);
          const ivf_f32x2 q0 = {qv.x, qv.y}, q1 = {qv.z, qv.w};
          if constexpr (IP) {
            acc[qi] = __builtin_elementwise_fma(x[2 * h], q0, acc[qi]);
            acc[qi] = __builtin_elementwise_fma(x[2 * h + 1], q1, acc[qi]);
          } else {
            const ivf_f32x2 d0 = x[2 * h] - q0, d1 = x[2 * h + 1] - q1;
            acc[qi] = __builtin_elementwise_fma(d0, d0, acc[qi]);
            acc[qi] = __builtin_elementwise_fma(d1, d1, acc[qi]);
          }
        }
      }
    }
  }
}

template <typename T, int QG, bool IP>
__launch_bounds__(256)
__global__ void ivf_flat_scan_kernel(
    const T* __restrict__ data, const long long* __restrict__ list_offsets,
    const long long* __restrict__ indices, const float* __restrict__ queries,
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
  constexpr int V = IvfChunk<T>::V;
  extern __shared__ __attribute__((aligned(16))) float ivf_qs[];  // [QG][d_pad]

  // every exit below is block-uniform and precedes the barrier
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
  for (int qi = 0; qi < nq; qi++) {
    const long long qrow = pair_query[pb + qi];
    const bool qok = qrow >= 0 && qrow < n_queries;  // else zeros, never stored
    const float* qp = queries + (qok ? qrow : 0) * (long long)d;
    for (int k = t; k < d_pad; k += 256)
      ivf_qs[qi * d_pad + k] = (qok && k < d) ? qp[k] : 0.f;
  }
  __syncthreads();

  const int chunks = d_pad / V;
  const long long g0 = r0 / RAFT_AMD_WAVE, g1 = r1 / RAFT_AMD_WAVE;
  const long long gstride = (long long)gridDim.y * 4;
  const float bad = IP ? -INFINITY : INFINITY;
  for (long long g = g0 + (long long)blockIdx.y * 4 + w; g < g1; g += gstride) {
    const long long row = g * RAFT_AMD_WAVE + lane;
    const long long id = indices[row];
    bool ok = id >= 0;
    if (ok && filter_words)
      ok = id < filter_bits && ((filter_words[id >> 5] >> (id & 31)) & 1u);
    const T* gp = data + (g * chunks * RAFT_AMD_WAVE + lane) * V;
    ivf_f32x2 acc[QG];
    if (nq == QG)
      ivf_scan_group<T, QG, IP, true>(gp, ivf_qs, chunks, d_pad, nq, acc);
    else
      ivf_scan_group<T, QG, IP, false>(gp, ivf_qs, chunks, d_pad, nq, acc);
    const long long in_list = row - r0;
#pragma unroll
    for (int qi = 0; qi < QG; qi++) {
      if (qi < nq) {
        float v = acc[qi].x + acc[qi].y;
        if (sqrt_out) v = sqrtf(v);
        const long long qrow = pair_query[pb + qi];
        const long long o = pair_out_off[pb + qi] + in_list;
        if (qrow >= 0 && qrow < n_queries && o >= 0 && o < out_numel)
          out[o] = ok ? v : bad;
      }
    }
  }
}

template <typename T, int QG, bool IP>
static void ivf_flat_scan_launch(
    const void* data, const long long* list_offsets, const long long* indices,
    const float* queries, const long long* item_list, const long long* item_pair_begin,
    const long long* item_pair_count, const long long* n_items,
    const long long* pair_query, const long long* pair_out_off,
    const unsigned int* filter_words, long long filter_bits, float* out,
    long long out_numel, long long n_lists, long long total_rows, long long n_queries,
    long long n_pairs, int d, int d_pad, bool sqrt_out, dim3 grid, hipStream_t stream) {
  const size_t lds = (size_t)QG * d_pad * sizeof(float);
  hipLaunchKernelGGL((ivf_flat_scan_kernel<T, QG, IP>), grid, dim3(256), lds, stream,
                     static_cast<const T*>(data), list_offsets, indices, queries,
                     item_list, item_pair_begin, item_pair_count, n_items, pair_query,
                     pair_out_off, filter_words, filter_bits, out, out_numel, n_lists,
                     total_rows, n_queries, n_pairs, d, d_pad, sqrt_out);
  HIP_CHECK(hipGetLastError());
}

int ivf_flat_scan_max_qg(int d_pad) {
  int qg = 32;
  while (qg > 1 && (long long)qg * d_pad * (long long)sizeof(float) > IVF_SCAN_LDS_BYTES)
    qg >>= 1;
  return qg;
}

void launch_ivf_flat_scan(const void* data, bool data_bf16,
                          const long long* list_offsets, const long long* indices,
                          const float* queries, const long long* item_list,
                          const long long* item_pair_begin,
                          const long long* item_pair_count, const long long* n_items,
                          const long long* pair_query, const long long* pair_out_off,
                          const unsigned int* filter_words, long long filter_bits,
                          float* out, long long out_numel, long long n_lists,
                          long long total_rows, long long n_queries, long long n_pairs,
                          long long max_items, int d, int metric, int qg, int y_split,
                          hipStream_t stream) {
  if (max_items <= 0 || n_pairs <= 0 || total_rows <= 0) return;
  const int v = data_bf16 ? 8 : 4;
  if (d < 1) throw std::runtime_error("ivf_flat_scan: d must be positive");
  const int d_pad = (d + v - 1) / v * v;
  if (qg != 4 && qg != 8 && qg != 16 && qg != 32)
    throw std::runtime_error("ivf_flat_scan: qg must be 4, 8, 16 or 32");
  if (qg > ivf_flat_scan_max_qg(d_pad))
    throw std::runtime_error("ivf_flat_scan: qg * d_pad * 4 must fit 64 KiB of LDS");
  if (metric < 0 || metric > 2)
    throw std::runtime_error("ivf_flat_scan: metric must be 0 (L2), 1 (L2 sqrt) or 2 (IP)");
  if (y_split < 1 || y_split > 65535 || max_items > 2147483647ll)
    throw std::runtime_error("ivf_flat_scan: grid out of range");
  const dim3 grid((unsigned)max_items, (unsigned)y_split);
  const bool ip = metric == 2;
  const bool sqrt_out = metric == 1;
#define RAFT_IVF_SCAN_LAUNCH(T, QG, IP)                                          \
  ivf_flat_scan_launch<T, QG, IP>(data, list_offsets, indices, queries, item_list, \
                                  item_pair_begin, item_pair_count, n_items,     \
                                  pair_query, pair_out_off, filter_words,        \
                                  filter_bits, out, out_numel, n_lists,          \
                                  total_rows, n_queries, n_pairs, d, d_pad,      \
                                  sqrt_out, grid, stream)
#define RAFT_IVF_SCAN_QG(T, IP)                                                  \
  switch (qg) {                                                                  \
    case 4: RAFT_IVF_SCAN_LAUNCH(T, 4, IP); break;                               \
    case 8: RAFT_IVF_SCAN_LAUNCH(T, 8, IP); break;                               \
    case 16: RAFT_IVF_SCAN_LAUNCH(T, 16, IP); break;                             \
    default: RAFT_IVF_SCAN_LAUNCH(T, 32, IP); break;                             \
  }
  if (data_bf16) {
    if (ip) { RAFT_IVF_SCAN_QG(__bf16, true) } else { RAFT_IVF_SCAN_QG(__bf16, false) }
  } else {
    if (ip) { RAFT_IVF_SCAN_QG(float, true) } else { RAFT_IVF_SCAN_QG(float, false) }
  }
#undef RAFT_IVF_SCAN_QG
#undef RAFT_IVF_SCAN_LAUNCH
}

}  // namespace raft_amd
