// IVF-PQ with 4-bit codes: the encode kernel and the LIST-major look-up-table
// (LUT) scan over nibble-packed rows.
//
// Reference parity (WHAT): the pq_bits = 4 mode of the historical
// raft::neighbors::ivf_pq::{build, extend, search}: 16-entry codebooks per
// subspace, two codes per byte. HOW is CDNA4-native and NOT the 8-bit kernels
// of ivf_pq.hip with a smaller book: a 16-entry table row is 64 bytes, so a
// block holds the tables of SEVERAL queries and streams a list once for all
// of them (the decomposition of ivf_flat_scan.hip), and the gather is free of
// bank conflicts by construction.
//
// Codebooks are fp32 [pq_dim][pq_len][16], entry-minor. d_rot = pq_dim *
// pq_len >= d; features past d are zero.
//
// Row layout (raft_amd/neighbors/ivf_pq.py): byte t of a row holds subspace
// 2t in bits 0..3 and subspace 2t + 1 in bits 4..7; row_bytes =
// ceil(pq_dim / 2) rounded up to 16, pad nibbles and pad bytes 0. One 16-byte
// chunk is 32 subspaces; n_chunks = row_bytes / 16 <= 8. Rows are interleaved
// as in IVF-Flat: byte (group g, chunk j, row r, b) at
//   ((g * n_chunks + j) * 64 + r) * 16 + b.
//
// ---- ivf_pq4_encode -------------------------------------------------------
// Grid (row blocks, n_chunks), block = 256 threads, lane = row. The block
// stages the codebooks of its chunk's 32 subspaces in LDS as [32][PL][16]
// (PL = pq_len rounded up to a power of two, the template tier; 2 KiB * PL,
// 64 KiB at PL = 32, static); entries of pad subspaces and pad features are
// zero. Per subspace a thread forms the residual sub-vector
// x - centroid[label] in a statically indexed register array, walks the 16
// entries as LDS broadcasts with the unexpanded sum fma(r - cb, r - cb, acc)
// and strict <, so exact ties go to the smallest entry, and packs the nibble
// into one of four dwords; a pad subspace (block-uniform test) contributes
// nibble 0. Each thread writes ONE 16-byte store per (row, chunk) into the
// row-major [n, row_bytes] output. A row whose label is out of range writes
// zeros. Interleaving is the packer's job.
//
// ---- ivf_pq4_scan ---------------------------------------------------------
// LIST-major. Work item = (list, up to QG (query, probe) pairs that probe
// it), built on the device exactly as for ivf_flat_scan: per item its list,
// first sorted pair and pair count, plus a DEVICE scalar n_items; grid x is
// only an upper bound and blocks past n_items exit. Grid y splits the list's
// 64-row groups. Block = 256 threads.
//
// LDS map (dynamic, floats):
//   lut  [n_chunks][QG][32][16]   QG * n_chunks * 2048 bytes
//   rs   [QG][d_rot]              QG * d_rot * 4 bytes
// plus 16 + 4 * QG bytes static (the inner-product bases). The table is
// chunk-major, THEN query, then subspace: inside one chunk the address of
// (query g, subspace s, entry e) is g * 2048 + s * 64 + e * 4 bytes past the
// chunk's base, and QG is a template parameter, so the query and subspace
// parts are compile-time immediates of the LDS read (at most 7 * 2048 + 31 *
// 64 + 60 < 2^16). Budget: QG * (2048 * n_chunks + 4 * d_rot) + static <=
// 64 KiB, which needs no opt-in attribute; QG is the largest of {8, 4, 2, 1}
// that fits (ivf_pq4_scan_max_qg; 0 if none does). Every pq_dim <= 256 with
// pq_len <= 32 fits QG = 1 (16 + 32 KiB). Two or more blocks per CU at
// 160 KiB of LDS per CU follow from the budget; that figure is a claim from
// the layout, not a counter reading.
//
// Phase 1. r = q - centroid[l] (r = q for inner product) of every staged
// query goes to rs, tail zero; for inner product the block also reduces
// base[g] = q . centroid[l] (wave butterflies, then the four wave sums in a
// fixed order). Then a thread owns (subspace s, entry e) pairs, 512 *
// n_chunks of them, 16 consecutive threads on one subspace: it loads its
// pq_len codebook values ONCE into a statically indexed register array
// (template tier PL) and for every staged query accumulates
// fma(r - cb, r - cb, acc), or fma(r, cb, acc), in feature order, as the
// 8-bit kernel does. Rows of pad subspaces are 0, so phase 2 has no guard.
//
// Phase 2. Waves stride over the block's 64-row groups, lane = row. Per
// chunk a lane loads its row's 16 bytes with one global_load_dwordx4 (1 KiB
// contiguous per wave); the NEXT chunk's load is issued before this chunk's
// gathers. The 32 nibbles become 32 LDS addresses (chunk base + nibble * 4)
// ONCE per chunk and are reused by every staged query, whose 32 reads differ
// only in the immediate. A query adds its reads alternately into TWO
// independent accumulators, summed at the end (plus base for inner product,
// then sqrtf for euclidean). A query's arithmetic never depends on
// which other queries share its group, nor on the group size: results are
// bitwise identical for any query chunking.
//
// Bank conflicts: a wave-wide read has one (query, subspace), so its 64
// addresses lie inside 16 consecutive dwords: distinct addresses fall in
// distinct banks and equal addresses broadcast. The gather is conflict-free
// by construction. This is reasoned from the layout, NOT measured: no counter
// run has been taken.
//
// Epilogue (the flat scan's): 64 consecutive floats per (query, group) at
// pair_out_off + row in list. Pad rows (id < 0) and rows the filter rejects
// get +inf (-inf for inner product); sqrtf for euclidean.
//
// Every index read from memory (item count, list, pair range, offsets, pair
// query, output offset, filter word) is range-checked before it forms an
// address. Every early exit (past n_items, a bad item, bad offsets, a y block
// without a group) is block-uniform and ahead of the first barrier.
//
// Register budget (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no
// kernel uses scratch). ivf_pq4_scan_kernel<QG, PL, L2 / IP>, VGPRs over the
// tiers PL = 2 / 8 / 32: QG 8: 94 / 96 / 115 (IP 122 / 122 / 123), QG 4:
// 86 / 86 / 86 (IP 100 / 100 / 114), QG 2: 80 / 80 / 83 (IP 84 / 84 / 85),
// QG 1: 47 / 47 / 48 (IP 48 / 48 / 49); that is 4 or 5 waves per SIMD at
// QG 8 and 4, 5 or 6 at QG 2, 7 or 8 at QG 1, before LDS, which at up to
// 64 KiB a block is the tighter limit (2 blocks = 2 waves per SIMD).
// ivf_pq4_encode_kernel<PL>: 21 / 26 / 36 / 56 / 95 / 176 VGPRs at PL = 1 / 2 /
// 4 / 8 / 16 / 32.
//
// What the compiler emits for a nibble is a shift, a mask and an add of the
// chunk's base (three VALU operations shared by the QG queries), and every
// gather is a ds_read_b32 whose query and subspace offset is the immediate.

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace raft_amd {

constexpr int IVF_PQ4_BLOCK = 256;
constexpr int IVF_PQ4_BOOK = 16;                 // 4-bit codes
constexpr int IVF_PQ4_CHUNK_SUB = 32;            // subspaces in one 16-byte chunk
constexpr int IVF_PQ4_MAX_PQ_DIM = 256;
constexpr int IVF_PQ4_MAX_PQ_LEN = 32;
constexpr int IVF_PQ4_LDS_BYTES = 64 * 1024;
constexpr int IVF_PQ4_QSTRIDE = IVF_PQ4_CHUNK_SUB * IVF_PQ4_BOOK;   // floats per (chunk, query)

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------

template <int PL>
__launch_bounds__(IVF_PQ4_BLOCK)
__global__ void ivf_pq4_encode_kernel(const float* __restrict__ x,
                                      const long long* __restrict__ labels,
                                      const float* __restrict__ centroids,
                                      const float* __restrict__ codebooks,
                                      unsigned char* __restrict__ codes, long long n,
                                      long long n_lists, int d, int pq_dim, int pq_len,
                                      int row_bytes) {
  __shared__ float cb[IVF_PQ4_CHUNK_SUB * PL * IVF_PQ4_BOOK];
  const int t = threadIdx.x;
  const int s_base = blockIdx.y * IVF_PQ4_CHUNK_SUB;
  for (int i = t; i < IVF_PQ4_CHUNK_SUB * PL * IVF_PQ4_BOOK; i += IVF_PQ4_BLOCK) {
    const int e = i % IVF_PQ4_BOOK;
    const int k = (i / IVF_PQ4_BOOK) % PL;
    const int s = s_base + i / (IVF_PQ4_BOOK * PL);
    cb[i] = (s < pq_dim && k < pq_len)
                ? codebooks[((long long)s * pq_len + k) * IVF_PQ4_BOOK + e] : 0.f;
  }
  const long long row = (long long)blockIdx.x * IVF_PQ4_BLOCK + t;
  const long long label = row < n ? labels[row] : -1;
  const bool live = label >= 0 && label < n_lists;
  const float* xp = x + (live ? row : 0) * (long long)d;
  const float* cp = centroids + (live ? label : 0) * (long long)d;
  __syncthreads();

  unsigned int word[4];
#pragma unroll
  for (int w = 0; w < 4; w++) {
    unsigned int packed = 0;
#pragma unroll 1
    for (int b = 0; b < 8; b++) {
      const int sl = w * 8 + b;
      const int s = s_base + sl;
      if (s >= pq_dim) break;                          // block-uniform; pad nibbles stay 0
      float r[PL];
      const int f0 = s * pq_len;
#pragma unroll
      for (int k = 0; k < PL; k++) {
        const int f = f0 + k;
        r[k] = (live && k < pq_len && f < d) ? xp[f] - cp[f] : 0.f;
      }
      const float* book = cb + sl * (PL * IVF_PQ4_BOOK);
      float best = INFINITY;
      unsigned int code = 0;
#pragma unroll 4
      for (int e = 0; e < IVF_PQ4_BOOK; e++) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < PL; k++) {
          const float diff = r[k] - book[k * IVF_PQ4_BOOK + e];
          acc = fmaf(diff, diff, acc);
        }
        if (acc < best) {
          best = acc;
          code = (unsigned int)e;
        }
      }
      packed |= code << (4 * b);
    }
    word[w] = live ? packed : 0u;
  }
  if (row < n)
    *reinterpret_cast<uint4*>(codes + row * row_bytes + (long long)blockIdx.y * 16) =
        make_uint4(word[0], word[1], word[2], word[3]);
}

static int ivf_pq4_row_bytes(int pq_dim) { return ((pq_dim + 1) / 2 + 15) / 16 * 16; }

void launch_ivf_pq4_encode(const float* x, const long long* labels, const float* centroids,
                           const float* codebooks, unsigned char* codes, long long n,
                           long long n_lists, int d, int pq_dim, int pq_len,
                           hipStream_t stream) {
  if (n <= 0) return;
  if (d < 1 || pq_dim < 1 || pq_len < 1 || pq_len > IVF_PQ4_MAX_PQ_LEN || pq_dim > 65535 * 32 ||
      (long long)pq_dim * pq_len < d)
    throw std::runtime_error("ivf_pq4_encode: needs pq_dim * pq_len >= d and pq_len <= 32");
  if (n_lists < 1) throw std::runtime_error("ivf_pq4_encode: n_lists must be positive");
  const long long row_blocks = (n + IVF_PQ4_BLOCK - 1) / IVF_PQ4_BLOCK;
  if (row_blocks > 2147483647ll) throw std::runtime_error("ivf_pq4_encode: grid out of range");
  const int row_bytes = ivf_pq4_row_bytes(pq_dim);
  const dim3 grid((unsigned)row_blocks, (unsigned)(row_bytes / 16));
#define RAFT_IVF_PQ4_ENCODE(PL)                                                         \
  hipLaunchKernelGGL((ivf_pq4_encode_kernel<PL>), grid, dim3(IVF_PQ4_BLOCK), 0, stream, x, \
                     labels, centroids, codebooks, codes, n, n_lists, d, pq_dim, pq_len, \
                     row_bytes)
  if (pq_len <= 1) RAFT_IVF_PQ4_ENCODE(1);
  else if (pq_len <= 2) RAFT_IVF_PQ4_ENCODE(2);
  else if (pq_len <= 4) RAFT_IVF_PQ4_ENCODE(4);
  else if (pq_len <= 8) RAFT_IVF_PQ4_ENCODE(8);
  else if (pq_len <= 16) RAFT_IVF_PQ4_ENCODE(16);
  else RAFT_IVF_PQ4_ENCODE(32);
#undef RAFT_IVF_PQ4_ENCODE
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------

// the eight nibbles of one dword -> eight table addresses in the chunk's slab
__device__ __forceinline__ void ivf_pq4_nibbles(unsigned int w, const float* __restrict__ slab,
                                                const float* (&at)[8]) {
#pragma unroll
  for (int b = 0; b < 8; b++) at[b] = slab + ((w >> (4 * b)) & 0xfu);
}

// one 64-row group against the staged tables. FULL: all QG slots are live;
// otherwise slot g is live iff g < nq (wave-uniform)
template <int QG, bool FULL>
__device__ __forceinline__ void ivf_pq4_scan_group(const uint4* __restrict__ gp,
                                                   const float* __restrict__ lut, int chunks,
                                                   int nq, float (&acc)[QG][2]) {
#pragma unroll
  for (int g = 0; g < QG; g++) acc[g][0] = acc[g][1] = 0.f;
  uint4 c = gp[0];
  for (int j = 0; j < chunks; j++) {
    // the next chunk's load ahead of this chunk's gathers (the last one reloads itself)
    const uint4 next = gp[(long long)(j + 1 < chunks ? j + 1 : j) * RAFT_AMD_WAVE];
    const float* slab = lut + j * (QG * IVF_PQ4_QSTRIDE);
    const float* at[4][8];
    ivf_pq4_nibbles(c.x, slab, at[0]);
    ivf_pq4_nibbles(c.y, slab, at[1]);
    ivf_pq4_nibbles(c.z, slab, at[2]);
    ivf_pq4_nibbles(c.w, slab, at[3]);
#pragma unroll
    for (int g = 0; g < QG; g++) {
      if (FULL || g < nq) {
#pragma unroll
        for (int s = 0; s < IVF_PQ4_CHUNK_SUB; s++)
          acc[g][s & 1] += at[s / 8][s % 8][g * IVF_PQ4_QSTRIDE + s * IVF_PQ4_BOOK];
      }
    }
    c = next;
  }
}

template <int QG, int PL, bool IP>
__launch_bounds__(IVF_PQ4_BLOCK)
__global__ void ivf_pq4_scan_kernel(
    const unsigned char* __restrict__ codes, const long long* __restrict__ list_offsets,
    const long long* __restrict__ indices, const float* __restrict__ queries,
    const float* __restrict__ centroids, const float* __restrict__ codebooks,
    const long long* __restrict__ item_list, const long long* __restrict__ item_pair_begin,
    const long long* __restrict__ item_pair_count, const long long* __restrict__ n_items_p,
    const long long* __restrict__ pair_query, const long long* __restrict__ pair_out_off,
    const unsigned int* __restrict__ filter_words, long long filter_bits,
    float* __restrict__ out, long long out_numel, long long n_lists, long long total_rows,
    long long n_queries, long long n_pairs, int d, int pq_dim, int pq_len, int chunks,
    bool sqrt_out) {
  extern __shared__ __attribute__((aligned(16))) float ivf_pq4_lds[];
  constexpr int NW = IVF_PQ4_BLOCK / RAFT_AMD_WAVE;
  __shared__ float red[NW];
  __shared__ float base_s[QG];
  const int d_rot = pq_dim * pq_len;
  float* lut = ivf_pq4_lds;                                      // [chunks][QG][32][16]
  float* rs = ivf_pq4_lds + chunks * (QG * IVF_PQ4_QSTRIDE);     // [QG][d_rot]

  // every exit below is block-uniform and precedes the first barrier
  if ((long long)blockIdx.x >= *n_items_p) return;
  const long long l = item_list[blockIdx.x];
  const long long pb = item_pair_begin[blockIdx.x];
  const long long npair = item_pair_count[blockIdx.x];
  if (l < 0 || l >= n_lists || npair < 1 || npair > QG || pb < 0 || pb + npair > n_pairs)
    return;
  const long long r0 = list_offsets[l], r1 = list_offsets[l + 1];
  if (r0 < 0 || r1 < r0 || r1 > total_rows || (r0 | r1) % RAFT_AMD_WAVE) return;
  const long long g0 = r0 / RAFT_AMD_WAVE, g1 = r1 / RAFT_AMD_WAVE;
  if (g0 + (long long)blockIdx.y * NW >= g1) return;             // no group for this block
  const int nq = (int)npair;

  const int t = threadIdx.x;
  const int lane = t % RAFT_AMD_WAVE;
  const int w = t / RAFT_AMD_WAVE;
  const float* cp = centroids + l * (long long)d;

  // phase 1a: the residuals (or the queries) and, for inner product, q . c
  for (int g = 0; g < nq; g++) {
    const long long qrow = pair_query[pb + g];
    const bool qok = qrow >= 0 && qrow < n_queries;              // else zeros, never stored
    const float* qp = queries + (qok ? qrow : 0) * (long long)d;
    float dot = 0.f;
    for (int k = t; k < d_rot; k += IVF_PQ4_BLOCK) {
      float v = 0.f;
      if (qok && k < d) {
        if constexpr (IP) {
          v = qp[k];
          dot = fmaf(v, cp[k], dot);
        } else {
          v = qp[k] - cp[k];
        }
      }
      rs[g * d_rot + k] = v;
    }
    if constexpr (IP) {
      dot = wave_reduce_sum(dot);
      __syncthreads();                                           // red of the query before
      if (lane == 0) red[w] = dot;
      __syncthreads();
      if (t == 0) base_s[g] = (red[0] + red[1]) + (red[2] + red[3]);
    }
  }
  __syncthreads();

  // phase 1b: a thread owns (subspace, entry) pairs, its codebook column in registers
  const int n_sub = chunks * IVF_PQ4_CHUNK_SUB;
  for (int p = t; p < n_sub * IVF_PQ4_BOOK; p += IVF_PQ4_BLOCK) {
    const int e = p % IVF_PQ4_BOOK;
    const int s = p / IVF_PQ4_BOOK;
    const bool sub = s < pq_dim;
    float cb[PL];
#pragma unroll
    for (int k = 0; k < PL; k++)
      cb[k] = (sub && k < pq_len)
                  ? codebooks[((long long)s * pq_len + k) * IVF_PQ4_BOOK + e] : 0.f;
    float* dst = lut + (s / IVF_PQ4_CHUNK_SUB) * (QG * IVF_PQ4_QSTRIDE) +
                 (s % IVF_PQ4_CHUNK_SUB) * IVF_PQ4_BOOK + e;
    for (int g = 0; g < nq; g++) {
      float acc = 0.f;
      if (sub) {
        const float* rp = rs + g * d_rot + s * pq_len;
#pragma unroll
        for (int k = 0; k < PL; k++) {
          if (k < pq_len) {
            if constexpr (IP) {
              acc = fmaf(rp[k], cb[k], acc);
            } else {
              const float diff = rp[k] - cb[k];
              acc = fmaf(diff, diff, acc);
            }
          }
        }
      }
      dst[g * IVF_PQ4_QSTRIDE] = acc;
    }
  }
  __syncthreads();

  // phase 2: lane = row, 32 codes per chunk, the list read once for nq queries
  const long long gstride = (long long)gridDim.y * NW;
  const float bad = IP ? -INFINITY : INFINITY;
  for (long long g = g0 + (long long)blockIdx.y * NW + w; g < g1; g += gstride) {
    const long long row = g * RAFT_AMD_WAVE + lane;
    const long long id = indices[row];
    bool ok = id >= 0;
    if (ok && filter_words)
      ok = id < filter_bits && ((filter_words[id >> 5] >> (id & 31)) & 1u);
    const uint4* gp = reinterpret_cast<const uint4*>(codes) + g * chunks * RAFT_AMD_WAVE + lane;
    float acc[QG][2];
    if (nq == QG)
      ivf_pq4_scan_group<QG, true>(gp, lut, chunks, nq, acc);
    else
      ivf_pq4_scan_group<QG, false>(gp, lut, chunks, nq, acc);
    const long long in_list = row - r0;
#pragma unroll
    for (int qi = 0; qi < QG; qi++) {
      if (qi < nq) {
        float v = acc[qi][0] + acc[qi][1];
        if constexpr (IP) v += base_s[qi];
        if (sqrt_out) v = sqrtf(v);
        const long long qrow = pair_query[pb + qi];
        const long long o = pair_out_off[pb + qi] + in_list;
        if (qrow >= 0 && qrow < n_queries && o >= 0 && o < out_numel) out[o] = ok ? v : bad;
      }
    }
  }
}

// dynamic + static LDS bytes of a scan block that stages qg queries
static long long ivf_pq4_scan_lds(int pq_dim, int pq_len, int qg) {
  const long long chunks = ivf_pq4_row_bytes(pq_dim) / 16;
  const long long per_query = chunks * IVF_PQ4_QSTRIDE * (long long)sizeof(float) +
                              (long long)pq_dim * pq_len * (long long)sizeof(float);
  return qg * per_query + (4 + qg) * (long long)sizeof(float);
}

// the largest of {8, 4, 2, 1} whose tables and residuals fit 64 KiB; 0 if the
// kernels do not serve the shape
int ivf_pq4_scan_max_qg(int pq_dim, int pq_len) {
  if (pq_dim < 1 || pq_len < 1 || pq_dim > IVF_PQ4_MAX_PQ_DIM || pq_len > IVF_PQ4_MAX_PQ_LEN)
    return 0;
  for (int qg = 8; qg >= 1; qg >>= 1)
    if (ivf_pq4_scan_lds(pq_dim, pq_len, qg) <= IVF_PQ4_LDS_BYTES) return qg;
  return 0;
}

void launch_ivf_pq4_scan(const unsigned char* codes, const long long* list_offsets,
                         const long long* indices, const float* queries,
                         const float* centroids, const float* codebooks,
                         const long long* item_list, const long long* item_pair_begin,
                         const long long* item_pair_count, const long long* n_items,
                         const long long* pair_query, const long long* pair_out_off,
                         const unsigned int* filter_words, long long filter_bits, float* out,
                         long long out_numel, long long n_lists, long long total_rows,
                         long long n_queries, long long n_pairs, long long max_items, int d,
                         int pq_dim, int pq_len, int metric, int qg, int y_split,
                         hipStream_t stream) {
  if (max_items <= 0 || n_pairs <= 0 || total_rows <= 0) return;
  if (d < 1 || pq_dim < 1 || pq_len < 1 || (long long)pq_dim * pq_len < d)
    throw std::runtime_error("ivf_pq4_scan: needs pq_dim * pq_len >= d");
  if (n_lists < 1) throw std::runtime_error("ivf_pq4_scan: n_lists must be positive");
  if (metric < 0 || metric > 2)
    throw std::runtime_error("ivf_pq4_scan: metric must be 0 (L2), 1 (L2 sqrt) or 2 (IP)");
  if (qg != 1 && qg != 2 && qg != 4 && qg != 8)
    throw std::runtime_error("ivf_pq4_scan: qg must be 1, 2, 4 or 8");
  if (qg > ivf_pq4_scan_max_qg(pq_dim, pq_len))
    throw std::runtime_error("ivf_pq4_scan: qg tables of pq_dim = " + std::to_string(pq_dim) +
                             ", pq_len = " + std::to_string(pq_len) +
                             " do not fit 64 KiB of LDS (pq_dim <= 256, pq_len <= 32)");
  if (y_split < 1 || y_split > 65535 || max_items > 2147483647ll)
    throw std::runtime_error("ivf_pq4_scan: grid out of range");
  const int chunks = ivf_pq4_row_bytes(pq_dim) / 16;
  const size_t lds = (size_t)qg * ((size_t)chunks * IVF_PQ4_QSTRIDE + (size_t)pq_dim * pq_len) *
                     sizeof(float);
  const dim3 grid((unsigned)max_items, (unsigned)y_split);
  const bool sqrt_out = metric == 1;
#define RAFT_IVF_PQ4_LAUNCH(QG, PL, IP)                                                    \
  hipLaunchKernelGGL((ivf_pq4_scan_kernel<QG, PL, IP>), grid, dim3(IVF_PQ4_BLOCK), lds,    \
                     stream, codes, list_offsets, indices, queries, centroids, codebooks,  \
                     item_list, item_pair_begin, item_pair_count, n_items, pair_query,     \
                     pair_out_off, filter_words, filter_bits, out, out_numel, n_lists,     \
                     total_rows, n_queries, n_pairs, d, pq_dim, pq_len, chunks, sqrt_out)
#define RAFT_IVF_PQ4_PL(QG, IP)                                                            \
  if (pq_len <= 2) RAFT_IVF_PQ4_LAUNCH(QG, 2, IP);                                         \
  else if (pq_len <= 8) RAFT_IVF_PQ4_LAUNCH(QG, 8, IP);                                    \
  else RAFT_IVF_PQ4_LAUNCH(QG, 32, IP)
#define RAFT_IVF_PQ4_QG(IP)                                                                \
  switch (qg) {                                                                            \
    case 8: { RAFT_IVF_PQ4_PL(8, IP); } break;                                             \
    case 4: { RAFT_IVF_PQ4_PL(4, IP); } break;                                             \
    case 2: { RAFT_IVF_PQ4_PL(2, IP); } break;                                             \
    default: { RAFT_IVF_PQ4_PL(1, IP); } break;                                            \
  }
  if (metric == 2) { RAFT_IVF_PQ4_QG(true) } else { RAFT_IVF_PQ4_QG(false) }
#undef RAFT_IVF_PQ4_QG
#undef RAFT_IVF_PQ4_PL
#undef RAFT_IVF_PQ4_LAUNCH
  HIP_CHECK(hipGetLastError());
}

}  // namespace raft_amd
