// Verified epsilon-neighborhood (squared L2) — packed-bitmap adjacency from
// the split-bf16 MFMA tile engine, plus the bitmap-row utilities that turn it
// into degrees, CSR and a dense bool matrix.
//
// Reference parity (WHAT): the historical raft::neighbors
// epsilon_neighborhood / eps_neighbors_l2sq — adj[i][j] = (||x_i - y_j||^2
// <= eps2) with vertex degrees. HOW is CDNA4-native: the 128x128 MFMA tile
// of pairwise_l2_filter_kernel (same geometry, same K-loop), but the
// epilogue turns the accumulator into BITS with wave64 ballots — the fp32
// tile never reaches HBM (1/8 B per pair instead of 4 B).
//
// Exactness for fp32 input (docs/verified_engines.md, "Eps-neighborhood
// exactness"): the emulated score s is within 2E of the true d2, with
// E = lead*sqrt(xn*yn) + tail*(xn+yn). A pair with |s - eps2| > 2E is decided
// by s; every other pair is re-decided by the unexpanded sum (x-y)^2 over the
// original fp32 rows (the definition l2nn_verify_repair_kernel uses).
//
// Bitmap ownership: the MFMA C layout is col = lane&15 (+16 fc),
// row = 4*(lane>>4) + reg (+16 fr), so for a fixed (fr, reg, fc) one 64-bit
// ballot holds 16 consecutive columns of 4 rows; two ballots (fc, fc+1) make
// an aligned 32-column word. Wave (wr, wc) owns rows wr*64.. and words
// wc*2, wc*2+1 of the tile: every word has exactly one writer, no atomics.

#include <hip/hip_runtime.h>

#include "mfma_common.h"

namespace raft_amd {

template <int NSLICE, bool VERIFY>
__launch_bounds__(256, 2)
__global__ void eps_neighbors_l2sq_kernel(const SlicePtrs p,
                                          const float* __restrict__ xn,
                                          const float* __restrict__ yn,
                                          const float* __restrict__ xf,
                                          const float* __restrict__ yf,
                                          unsigned int* __restrict__ bitmap,
                                          unsigned long long* __restrict__ rechecked,
                                          float eps2, float lead2, float tail2,
                                          long long m, long long n, int d,
                                          int df, long long n_words, int rg) {
  extern __shared__ __bf16 smem[];
  MfmaTile t;
  f32x4 acc[4][4];
  if (!mfma_tile_prologue<128>(rg, m, n, t, acc)) return;
  const int lane = t.lane, wr = t.wr, wc = t.wc;
  const long long row0 = t.row0, col0 = t.col0;
  mfma_tile_kloop<NSLICE>(p, smem, acc, t, m, n, d);

  // The K-loop LDS is dead (the loop ends on a barrier): reuse it for the
  // tile's [128][4] decision words and, when verifying, [128][4] band words.
  unsigned int* pw = reinterpret_cast<unsigned int*>(smem);
  unsigned int* iw = pw + 512;

  // out-of-range columns carry yn = +inf: their score is +inf, never <= eps2
  // (the host never launches with eps2 = +inf). Their band test may read
  // true; the recheck pass drops them by the col < n guard.
  const long long colb = col0 + wc * 64 + (lane & 15);
  float yn_r[4], sy_r[4];
#pragma unroll
  for (int fc = 0; fc < 4; fc++) {
    const long long col = colb + fc * 16;
    yn_r[fc] = col < n ? yn[col] : INFINITY;
    sy_r[fc] = VERIFY ? lead2 * sqrtf(fmaxf(yn_r[fc], 0.f)) : 0.f;
  }
  const int sel = lane & 15;
  const int sh = (lane >> 4) * 16;
#pragma unroll
  for (int fr = 0; fr < 4; fr++) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int rl = wr * 64 + fr * 16 + (lane >> 4) * 4 + reg;
      long long row = row0 + rl;
      if (row > m - 1) row = m - 1;  // rows past m are computed, never stored
      const float xv = xn[row];
      const float sx = VERIFY ? sqrtf(fmaxf(xv, 0.f)) : 0.f;
      unsigned long long pb[4], ib[4];
#pragma unroll
      for (int fc = 0; fc < 4; fc++) {
        const float t = xv + yn_r[fc];
        const float s = t - 2.f * acc[fr][fc][reg];
        pb[fc] = __ballot(s <= eps2);
        if constexpr (VERIFY) {
          // 2E = 2*lead*sqrt(xn)*sqrt(yn) + 2*tail*(xn + yn)
          const float band = fmaf(tail2, t, sx * sy_r[fc]);
          ib[fc] = __ballot(fabsf(s - eps2) <= band);
        }
      }
      if (sel < (VERIFY ? 4 : 2)) {
        unsigned long long lo = (sel & 1) ? pb[2] : pb[0];
        unsigned long long hi = (sel & 1) ? pb[3] : pb[1];
        if constexpr (VERIFY) {
          if (sel & 2) {
            lo = (sel & 1) ? ib[2] : ib[0];
            hi = (sel & 1) ? ib[3] : ib[1];
          }
        }
        const unsigned int word = (unsigned int)((lo >> sh) & 0xffffull) |
                                  ((unsigned int)((hi >> sh) & 0xffffull) << 16);
        unsigned int* dst = (sel & 2) ? iw : pw;
        dst[rl * 4 + wc * 2 + (sel & 1)] = word;
      }
    }
  }
  __syncthreads();

  // each lane now owns one row of its wave's 64x64 quadrant (2 words)
  const int rl = wr * 64 + lane;
  unsigned long long pm = (unsigned long long)pw[rl * 4 + wc * 2] |
                          ((unsigned long long)pw[rl * 4 + wc * 2 + 1] << 32);
  if constexpr (VERIFY) {
    const unsigned long long mine =
        (unsigned long long)iw[rl * 4 + wc * 2] |
        ((unsigned long long)iw[rl * 4 + wc * 2 + 1] << 32);
    // wave-cooperative exact recheck: walk the (rare) band pairs one at a
    // time; all 64 lanes stride the feature axis of that one pair.
    unsigned long long act = __ballot(mine != 0ull);
    unsigned int n_re = 0;
    while (act) {
      const int src = __ffsll((long long)act) - 1;
      act &= act - 1;
      const unsigned int b_lo = __builtin_amdgcn_readfirstlane(
          __shfl((unsigned int)mine, src, RAFT_AMD_WAVE));
      const unsigned int b_hi = __builtin_amdgcn_readfirstlane(
          __shfl((unsigned int)(mine >> 32), src, RAFT_AMD_WAVE));
      unsigned long long bits = (unsigned long long)b_lo |
                                ((unsigned long long)b_hi << 32);
      const long long row = row0 + wr * 64 + src;
      while (bits) {
        const int c = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        const long long col = col0 + wc * 64 + c;
        bool in = false;
        if (row < m && col < n) {
          const float* xp = xf + row * (long long)df;
          const float* yp = yf + col * (long long)df;
          float a = 0.f;
          for (int k = lane; k < df; k += RAFT_AMD_WAVE) {
            const float diff = xp[k] - yp[k];
            a = fmaf(diff, diff, a);
          }
          a = wave_reduce_sum(a);
          in = a <= eps2;
          n_re++;
        }
        if (lane == src) {
          const unsigned long long bit = 1ull << c;
          pm = in ? (pm | bit) : (pm & ~bit);
        }
      }
    }
    // one counter update per wave, not per pair
    if (n_re && lane == 0) atomicAdd(rechecked, (unsigned long long)n_re);
  }

  const long long row = row0 + rl;
  if (row < m) {
    const long long wi = (col0 >> 5) + wc * 2;
    unsigned int* dst = bitmap + row * n_words + wi;
    if (wi < n_words) dst[0] = (unsigned int)pm;
    if (wi + 1 < n_words) dst[1] = (unsigned int)(pm >> 32);
  }
}

void launch_eps_neighbors_l2sq(const void** xsl, const void** csl, const float* xn,
                               const float* yn, const float* xf, const float* yf,
                               unsigned int* bitmap, unsigned long long* rechecked,
                               float eps2, float lead, float tail, long long m,
                               long long n, int d, int df, long long n_words,
                               int nslice, hipStream_t stream) {
  if (m <= 0 || n <= 0) return;
  const int rg = (int)((m + 1023) / 1024);  // ceil(R/8), R = ceil(m/128)
  const int cg = (int)((n + 1023) / 1024);
  dim3 grid((unsigned)((long long)rg * cg * 64));
  const size_t lds = (size_t)nslice * 2 * 8192 * sizeof(__bf16);
  const SlicePtrs p(xsl, csl, nslice);
  const bool verify = xf != nullptr;
  if (verify && (yf == nullptr || rechecked == nullptr))
    throw std::runtime_error("eps_neighbors_l2sq: verify needs xf, yf and a counter");
  const float lead2 = 2.f * lead, tail2 = 2.f * tail;
  if (nslice == 1 && !verify) {
    hipLaunchKernelGGL((eps_neighbors_l2sq_kernel<1, false>), grid, dim3(256), lds,
                       stream, p, xn, yn, xf, yf, bitmap,
                       rechecked, eps2, lead2, tail2, m, n, d, df, n_words, rg);
  } else if (nslice == 1) {
    hipLaunchKernelGGL((eps_neighbors_l2sq_kernel<1, true>), grid, dim3(256), lds,
                       stream, p, xn, yn, xf, yf, bitmap,
                       rechecked, eps2, lead2, tail2, m, n, d, df, n_words, rg);
  } else if (nslice == 2 && verify) {
    hipLaunchKernelGGL((eps_neighbors_l2sq_kernel<2, true>), grid, dim3(256), lds,
                       stream, p, xn, yn, xf, yf, bitmap,
                       rechecked, eps2, lead2, tail2, m, n, d, df, n_words, rg);
  } else {
    throw std::runtime_error(
        "eps_neighbors_l2sq: 1 slice, or 1-2 slices with the fp32 recheck");
  }
}

// ---------------------------------------------------------------------------
// bitmap rows -> degrees / CSR / dense bool. The bitmap is row-padded: each
// row starts on a word boundary (n_words words per row), little-endian bits,
// bits at columns >= n are zero.
// ---------------------------------------------------------------------------

// one wave per row: integer popcount, no float anywhere
__global__ void bitmap_row_degrees_kernel(const unsigned int* __restrict__ bm,
                                          long long* __restrict__ deg,
                                          long long m, long long n_words) {
  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const long long wpb = blockDim.x / RAFT_AMD_WAVE;
  long long row = (long long)blockIdx.x * wpb + threadIdx.x / RAFT_AMD_WAVE;
  const long long stride = (long long)gridDim.x * wpb;
  for (; row < m; row += stride) {
    const unsigned int* r = bm + row * n_words;
    int c = 0;
    for (long long w = lane; w < n_words; w += RAFT_AMD_WAVE) c += __popc(r[w]);
    c = wave_reduce_sum(c);
    if (lane == 0) deg[row] = c;
  }
}

// one wave per row: per 64-word step, an in-wave exclusive scan of the word
// popcounts gives each lane its output offset; bits are walked low to high,
// so column ids come out strictly increasing.
__global__ void bitmap_rows_to_csr_kernel(const unsigned int* __restrict__ bm,
                                          const long long* __restrict__ indptr,
                                          int* __restrict__ indices,
                                          long long m, long long n_words) {
  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const long long wpb = blockDim.x / RAFT_AMD_WAVE;
  long long row = (long long)blockIdx.x * wpb + threadIdx.x / RAFT_AMD_WAVE;
  const long long stride = (long long)gridDim.x * wpb;
  for (; row < m; row += stride) {
    const unsigned int* r = bm + row * n_words;
    long long base = indptr[row];
    const long long end = indptr[row + 1];
    for (long long w0 = 0; w0 < n_words; w0 += RAFT_AMD_WAVE) {
      const long long w = w0 + lane;
      unsigned int word = w < n_words ? r[w] : 0u;
      const int c = __popc(word);
      int incl = c;
#pragma unroll
      for (int off = 1; off < RAFT_AMD_WAVE; off <<= 1) {
        const int t = __shfl_up(incl, off, RAFT_AMD_WAVE);
        if (lane >= off) incl += t;
      }
      const int total = __shfl(incl, RAFT_AMD_WAVE - 1, RAFT_AMD_WAVE);
      long long pos = base + (incl - c);
      const int colw = (int)(w << 5);
      while (word) {
        const int b = __ffs((int)word) - 1;
        word &= word - 1;
        // indptr comes from the same bitmap's popcounts; the guard keeps a
        // mismatched indptr from writing past the row's slot
        if (pos < end) indices[pos] = colw + b;
        pos++;
      }
      base += total;
    }
  }
}

// dense bool expand: consecutive threads write consecutive bytes of one row
__global__ void bitmap_rows_expand_kernel(const unsigned int* __restrict__ bm,
                                          unsigned char* __restrict__ out,
                                          long long m, long long n,
                                          long long n_words) {
  const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= n) return;
  for (long long row = blockIdx.y; row < m; row += gridDim.y) {
    const unsigned int word = bm[row * n_words + (col >> 5)];
    out[row * n + col] = (unsigned char)((word >> (col & 31)) & 1u);
  }
}

static int rows_grid(long long m) {
  const long long blocks = (m + 3) / 4;  // 4 waves (rows) per 256-thread block
  return (int)(blocks < 65536 ? blocks : 65536);
}

void launch_bitmap_row_degrees(const unsigned int* bm, long long* deg, long long m,
                               long long n_words, hipStream_t stream) {
  if (m <= 0) return;
  hipLaunchKernelGGL(bitmap_row_degrees_kernel, dim3(rows_grid(m)), dim3(256), 0,
                     stream, bm, deg, m, n_words);
}

void launch_bitmap_rows_to_csr(const unsigned int* bm, const long long* indptr,
                               int* indices, long long m, long long n_words,
                               hipStream_t stream) {
  if (m <= 0 || n_words <= 0) return;
  hipLaunchKernelGGL(bitmap_rows_to_csr_kernel, dim3(rows_grid(m)), dim3(256), 0,
                     stream, bm, indptr, indices, m, n_words);
}

void launch_bitmap_rows_expand(const unsigned int* bm, bool* out, long long m,
                               long long n, long long n_words, hipStream_t stream) {
  if (m <= 0 || n <= 0) return;
  const unsigned gx = (unsigned)((n + 255) / 256);
  const unsigned gy = (unsigned)(m < 65535 ? m : 65535);
  hipLaunchKernelGGL(bitmap_rows_expand_kernel, dim3(gx, gy), dim3(256), 0, stream,
                     bm, reinterpret_cast<unsigned char*>(out), m, n, n_words);
}

}  // namespace raft_amd
