// IVF-PQ: product-quantisation encode and the look-up-table (LUT) list scan.
//
// Reference parity (WHAT): the encode step of the historical
// raft::neighbors::ivf_pq::{build, extend} and the LUT scan of ivf_pq::search,
// with 8-bit codes and per-subspace codebooks. HOW is CDNA4-native: a
// workgroup may hold 160 KiB of LDS, so a scan block keeps the FULL fp32 table
// of one (query, list) pair, up to pq_dim = 128 subspaces x 256 entries =
// 128 KiB, which the 48/64 KiB kernels this was modelled on had to split or
// store narrower.
//
// Codebooks are fp32 [pq_dim][pq_len][256], entry-minor: 256 threads that
// each own one entry read 1 KiB contiguous per (subspace, feature).
// d_rot = pq_dim * pq_len >= d; features past d are zero.
//
// ---- ivf_pq_encode --------------------------------------------------------
// Grid (row blocks, pq_dim), block = 256 threads, lane = row. The block stages
// subspace s of the codebook in LDS as [PL][256] (PL = pq_len rounded up to a
// power of two, the template tier; the rows past pq_len are zero, and so are
// the residual's, so they add exactly 0 and the loop needs no guard). A thread
// forms its row's residual sub-vector x - centroid[label] in a statically
// indexed register array (it never reaches HBM), walks the 256 entries as LDS
// broadcasts, accumulates the unexpanded fp32 sum fma(r - cb, r - cb, acc) and
// keeps (best, index) with strict <, so exact ties go to the smallest entry.
// A row whose label is out of range writes code 0. Output is row-major
// [n, pq_dim_pad] bytes; the block of the last subspace also writes the pad
// bytes (0). Interleaving is the packer's job, not this kernel's.
//
// ---- ivf_pq_scan ----------------------------------------------------------
// PAIR-major, unlike the list-major flat scan: codes are pq_dim bytes a row,
// so reading a list again for every query costs little, and a table belongs
// to one (query, list) pair. Grid x = the exact number of (query, probe)
// pairs (the host knows it: no sort, no item list, no device-side count);
// grid y splits the list's 64-row groups. Block = 256 threads.
//
// Phase 1. r = q - centroid[l] goes to LDS as fp32 [d_rot] (tail zero); for
// inner product r = q and the block also reduces base = q . centroid[l].
// Then thread j builds column j of lut[s][j] (s < pq_dim_pad, j < 256):
// per subspace it reads codebooks[s][t][j] (coalesced across j) and r (an LDS
// broadcast) and accumulates fma(r - cb, r - cb, acc), or fma(r, cb, acc) for
// inner product. Rows of padded subspaces are 0, so phase 2 has no guard.
// LDS = pq_dim_pad * 1024 + d_rot * 4 bytes dynamic (+ 16 bytes static);
// above 64 KiB the launcher opts in with hipFuncSetAttribute. EVERY y-split
// block rebuilds the table: 256 * d_rot FMAs and d_rot KiB of codebook reads
// (L2-resident) per block. A y block that owns no group exits before it.
//
// Phase 2. Waves stride over 64-row groups. Per 16-byte chunk a lane loads
// its row's 16 codes (one global_load_dwordx4, 1 KiB contiguous per wave) and
// does 16 reads lut[(16 j + b) * 256 + byte] into FOUR independent
// accumulators, so the gather latency of one read overlaps the next three;
// they are summed at the end, plus base for inner product. A code byte is
// < 256 and s < pq_dim_pad by construction, so no read leaves the table.
//
// Bank conflicts: the whole wave reads the same subspace at once, that is 64
// addresses inside one 1 KiB table row (256 dwords, four dwords per bank with
// 64 banks). Lanes with EQUAL bytes read one address (a broadcast, free);
// lanes whose bytes differ by a multiple of the bank count collide. For
// uniformly distributed codes that is the balls-in-bins maximum of 64 lanes
// over the banks, about 3-4 serialised passes per read, so the loop is
// LDS-gather bound, not HBM bound; clustered data (many equal bytes in a
// list) does better. This is reasoned from the layout, NOT measured: no PMC
// run of its own has been taken.
//
// Epilogue (the flat scan's): 64 consecutive floats per group at
// pair_out_off + row in list. Pad rows (id < 0) and rows the filter rejects
// get +inf (-inf for inner product); sqrtf for euclidean.
//
// Every index read from memory (probe list, offsets, output offset, filter
// word) is checked before use; every early exit is block-uniform and ahead of
// the first barrier.

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace raft_amd {

constexpr int IVF_PQ_BLOCK = 256;
constexpr int IVF_PQ_BOOK = 256;                     // 8-bit codes
constexpr int IVF_PQ_MAX_LDS = 160 * 1024;           // CDNA4, per workgroup
constexpr int IVF_PQ_SCAN_STATIC_LDS = 4 * (int)sizeof(float);

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------

template <int PL>
__launch_bounds__(IVF_PQ_BLOCK)
__global__ void ivf_pq_encode_kernel(const float* __restrict__ x,
                                     const long long* __restrict__ labels,
                                     const float* __restrict__ centroids,
                                     const float* __restrict__ codebooks,
                                     unsigned char* __restrict__ codes, long long n,
                                     long long n_lists, int d, int pq_dim, int pq_len,
                                     int pq_dim_pad) {
  __shared__ float cb[PL * IVF_PQ_BOOK];
  const int t = threadIdx.x;
  const int s = blockIdx.y;
  const float* book = codebooks + (long long)s * pq_len * IVF_PQ_BOOK;
#pragma unroll
  for (int k = 0; k < PL; k++)
    cb[k * IVF_PQ_BOOK + t] = k < pq_len ? book[k * IVF_PQ_BOOK + t] : 0.f;

  const long long row = (long long)blockIdx.x * IVF_PQ_BLOCK + t;
  const long long label = row < n ? labels[row] : -1;
  const bool live = label >= 0 && label < n_lists;
  float r[PL];
  const int f0 = s * pq_len;
#pragma unroll
  for (int k = 0; k < PL; k++) {
    const int f = f0 + k;
    r[k] = (live && k < pq_len && f < d) ? x[row * d + f] - centroids[label * d + f] : 0.f;
  }
  __syncthreads();

  float best = INFINITY;
  int code = 0;
#pragma unroll 4
  for (int j = 0; j < IVF_PQ_BOOK; j++) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < PL; k++) {
      const float diff = r[k] - cb[k * IVF_PQ_BOOK + j];
      acc = fmaf(diff, diff, acc);
    }
    if (acc < best) {
      best = acc;
      code = j;
    }
  }
  if (row < n) {
    unsigned char* out = codes + row * pq_dim_pad;
    out[s] = live ? (unsigned char)code : (unsigned char)0;
    if (s == pq_dim - 1)
      for (int p = pq_dim; p < pq_dim_pad; p++) out[p] = 0;
  }
}

void launch_ivf_pq_encode(const float* x, const long long* labels, const float* centroids,
                          const float* codebooks, unsigned char* codes, long long n,
                          long long n_lists, int d, int pq_dim, int pq_len,
                          hipStream_t stream) {
  if (n <= 0) return;
  if (d < 1 || pq_dim < 1 || pq_len < 1 || pq_len > 32 || pq_dim > 65535 ||
      (long long)pq_dim * pq_len < d)
    throw std::runtime_error(
        "ivf_pq_encode: needs pq_dim * pq_len >= d, pq_len <= 32 and pq_dim <= 65535");
  if (n_lists < 1) throw std::runtime_error("ivf_pq_encode: n_lists must be positive");
  const long long row_blocks = (n + IVF_PQ_BLOCK - 1) / IVF_PQ_BLOCK;
  if (row_blocks > 2147483647ll) throw std::runtime_error("ivf_pq_encode: grid out of range");
  const int pq_dim_pad = (pq_dim + 15) / 16 * 16;
  const dim3 grid((unsigned)row_blocks, (unsigned)pq_dim);
#define RAFT_IVF_PQ_ENCODE(PL)                                                       \
  hipLaunchKernelGGL((ivf_pq_encode_kernel<PL>), grid, dim3(IVF_PQ_BLOCK), 0, stream, x, \
                     labels, centroids, codebooks, codes, n, n_lists, d, pq_dim,    \
                     pq_len, pq_dim_pad)
  if (pq_len <= 1) RAFT_IVF_PQ_ENCODE(1);
  else if (pq_len <= 2) RAFT_IVF_PQ_ENCODE(2);
  else if (pq_len <= 4) RAFT_IVF_PQ_ENCODE(4);
  else if (pq_len <= 8) RAFT_IVF_PQ_ENCODE(8);
  else if (pq_len <= 16) RAFT_IVF_PQ_ENCODE(16);
  else RAFT_IVF_PQ_ENCODE(32);
#undef RAFT_IVF_PQ_ENCODE
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------

// the four code bytes of one dword against table rows s0 .. s0 + 3
__device__ __forceinline__ void ivf_pq_gather4(const float* __restrict__ lut, unsigned int w,
                                               int s0, float (&acc)[4]) {
  acc[0] += lut[(s0 + 0) * IVF_PQ_BOOK + (w & 0xffu)];
  acc[1] += lut[(s0 + 1) * IVF_PQ_BOOK + ((w >> 8) & 0xffu)];
  acc[2] += lut[(s0 + 2) * IVF_PQ_BOOK + ((w >> 16) & 0xffu)];
  acc[3] += lut[(s0 + 3) * IVF_PQ_BOOK + (w >> 24)];
}

template <bool IP>
__launch_bounds__(IVF_PQ_BLOCK)
__global__ void ivf_pq_scan_kernel(
    const unsigned char* __restrict__ codes, const long long* __restrict__ list_offsets,
    const long long* __restrict__ indices, const float* __restrict__ queries,
    const float* __restrict__ centroids, const float* __restrict__ codebooks,
    const long long* __restrict__ probes, const long long* __restrict__ pair_out_off,
    const unsigned int* __restrict__ filter_words, long long filter_bits,
    float* __restrict__ out, long long out_numel, long long n_lists, long long total_rows,
    int n_probes, int d, int pq_dim, int pq_len, int pq_dim_pad, bool sqrt_out) {
  extern __shared__ __attribute__((aligned(16))) float ivf_pq_lds[];
  __shared__ float red[IVF_PQ_BLOCK / RAFT_AMD_WAVE];
  float* lut = ivf_pq_lds;                                   // [pq_dim_pad][256]
  float* rs = ivf_pq_lds + (long long)pq_dim_pad * IVF_PQ_BOOK;  // [d_rot]

  // every exit below is block-uniform and precedes the first barrier
  const long long pair = blockIdx.x;
  const long long l = probes[pair];
  if (l < 0 || l >= n_lists) return;
  const long long r0 = list_offsets[l], r1 = list_offsets[l + 1];
  if (r0 < 0 || r1 < r0 || r1 > total_rows || (r0 | r1) % RAFT_AMD_WAVE) return;
  const long long po = pair_out_off[pair];
  if (po < 0 || po > out_numel || r1 - r0 > out_numel - po) return;
  constexpr int NW = IVF_PQ_BLOCK / RAFT_AMD_WAVE;
  const long long g0 = r0 / RAFT_AMD_WAVE, g1 = r1 / RAFT_AMD_WAVE;
  if (g0 + (long long)blockIdx.y * NW >= g1) return;          // no group for this block

  const int t = threadIdx.x;
  const int lane = t % RAFT_AMD_WAVE;
  const int w = t / RAFT_AMD_WAVE;
  const int d_rot = pq_dim * pq_len;
  const float* qp = queries + (pair / n_probes) * (long long)d;
  const float* cp = centroids + l * (long long)d;

  // phase 1a: the residual (or the query) and, for inner product, q . c
  float dot = 0.f;
  for (int k = t; k < d_rot; k += IVF_PQ_BLOCK) {
    float v = 0.f;
    if (k < d) {
      if constexpr (IP) {
        v = qp[k];
        dot = fmaf(v, cp[k], dot);
      } else {
        v = qp[k] - cp[k];
      }
    }
    rs[k] = v;
  }
  float base = 0.f;
  if constexpr (IP) {
    dot = wave_reduce_sum(dot);
    if (lane == 0) red[w] = dot;
  }
  __syncthreads();
  if constexpr (IP) base = (red[0] + red[1]) + (red[2] + red[3]);

  // phase 1b: thread t owns entry t of every subspace
  for (int s = 0; s < pq_dim_pad; s++) {
    float acc = 0.f;
    if (s < pq_dim) {
      const float* book = codebooks + ((long long)s * pq_len) * IVF_PQ_BOOK + t;
      const float* rp = rs + s * pq_len;
#pragma unroll 4
      for (int k = 0; k < pq_len; k++) {
        const float c = book[k * IVF_PQ_BOOK];
        if constexpr (IP) {
          acc = fmaf(rp[k], c, acc);
        } else {
          const float diff = rp[k] - c;
          acc = fmaf(diff, diff, acc);
        }
      }
    }
    lut[s * IVF_PQ_BOOK + t] = acc;
  }
  __syncthreads();

  // phase 2: lane = row, 16 codes per chunk
  const int chunks = pq_dim_pad / 16;
  const long long gstride = (long long)gridDim.y * NW;
  const float bad = IP ? -INFINITY : INFINITY;
  for (long long g = g0 + (long long)blockIdx.y * NW + w; g < g1; g += gstride) {
    const long long row = g * RAFT_AMD_WAVE + lane;
    const long long id = indices[row];
    bool ok = id >= 0;
    if (ok && filter_words)
      ok = id < filter_bits && ((filter_words[id >> 5] >> (id & 31)) & 1u);
    const uint4* gp = reinterpret_cast<const uint4*>(codes) + g * chunks * RAFT_AMD_WAVE + lane;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int j = 0; j < chunks; j++) {
      const uint4 c = gp[(long long)j * RAFT_AMD_WAVE];
      ivf_pq_gather4(lut, c.x, 16 * j, acc);
      ivf_pq_gather4(lut, c.y, 16 * j + 4, acc);
      ivf_pq_gather4(lut, c.z, 16 * j + 8, acc);
      ivf_pq_gather4(lut, c.w, 16 * j + 12, acc);
    }
    float v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + base;
    if (sqrt_out) v = sqrtf(v);
    out[po + (row - r0)] = ok ? v : bad;
  }
}

size_t ivf_pq_scan_lds_bytes(int pq_dim, int pq_len) {
  const size_t pq_dim_pad = ((size_t)pq_dim + 15) / 16 * 16;
  return pq_dim_pad * IVF_PQ_BOOK * sizeof(float) + (size_t)pq_dim * pq_len * sizeof(float);
}

template <bool IP>
static void ivf_pq_scan_launch(
    const unsigned char* codes, const long long* list_offsets, const long long* indices,
    const float* queries, const float* centroids, const float* codebooks,
    const long long* probes, const long long* pair_out_off, const unsigned int* filter_words,
    long long filter_bits, float* out, long long out_numel, long long n_lists,
    long long total_rows, int n_probes, int d, int pq_dim, int pq_len, int pq_dim_pad,
    bool sqrt_out, dim3 grid, size_t lds, hipStream_t stream) {
  static bool attr_set = false;
  if (lds > 64 * 1024 && !attr_set) {
    // the largest request the launcher admits next to the static bytes
    HIP_CHECK(hipFuncSetAttribute((const void*)&ivf_pq_scan_kernel<IP>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  IVF_PQ_MAX_LDS - IVF_PQ_SCAN_STATIC_LDS));
    attr_set = true;
  }
  hipLaunchKernelGGL((ivf_pq_scan_kernel<IP>), grid, dim3(IVF_PQ_BLOCK), lds, stream, codes,
                     list_offsets, indices, queries, centroids, codebooks, probes,
                     pair_out_off, filter_words, filter_bits, out, out_numel, n_lists,
                     total_rows, n_probes, d, pq_dim, pq_len, pq_dim_pad, sqrt_out);
  HIP_CHECK(hipGetLastError());
}

void launch_ivf_pq_scan(const unsigned char* codes, const long long* list_offsets,
                        const long long* indices, const float* queries,
                        const float* centroids, const float* codebooks,
                        const long long* probes, const long long* pair_out_off,
                        const unsigned int* filter_words, long long filter_bits, float* out,
                        long long out_numel, long long n_lists, long long total_rows,
                        long long n_queries, int n_probes, int d, int pq_dim, int pq_len,
                        int metric, int y_split, hipStream_t stream) {
  if (n_queries <= 0 || n_probes <= 0 || total_rows <= 0) return;
  if (d < 1 || pq_dim < 1 || pq_len < 1 || (long long)pq_dim * pq_len < d)
    throw std::runtime_error("ivf_pq_scan: needs pq_dim * pq_len >= d");
  if (n_lists < 1) throw std::runtime_error("ivf_pq_scan: n_lists must be positive");
  if (metric < 0 || metric > 2)
    throw std::runtime_error("ivf_pq_scan: metric must be 0 (L2), 1 (L2 sqrt) or 2 (IP)");
  const size_t lds = ivf_pq_scan_lds_bytes(pq_dim, pq_len);
  if (lds > (size_t)(IVF_PQ_MAX_LDS - IVF_PQ_SCAN_STATIC_LDS))
    throw std::runtime_error("ivf_pq_scan: the look-up table of pq_dim = " +
                             std::to_string(pq_dim) + ", pq_len = " + std::to_string(pq_len) +
                             " does not fit 160 KiB of LDS");
  const long long n_pairs = n_queries * n_probes;
  if (y_split < 1 || y_split > 65535 || n_pairs > 2147483647ll)
    throw std::runtime_error("ivf_pq_scan: grid out of range");
  const int pq_dim_pad = (pq_dim + 15) / 16 * 16;
  const dim3 grid((unsigned)n_pairs, (unsigned)y_split);
  if (metric == 2)
    ivf_pq_scan_launch<true>(codes, list_offsets, indices, queries, centroids, codebooks,
                             probes, pair_out_off, filter_words, filter_bits, out, out_numel,
                             n_lists, total_rows, n_probes, d, pq_dim, pq_len, pq_dim_pad,
                             false, grid, lds, stream);
  else
    ivf_pq_scan_launch<false>(codes, list_offsets, indices, queries, centroids, codebooks,
                              probes, pair_out_off, filter_words, filter_bits, out, out_numel,
                              n_lists, total_rows, n_probes, d, pq_dim, pq_len, pq_dim_pad,
                              metric == 1, grid, lds, stream);
}

}  // namespace raft_amd
