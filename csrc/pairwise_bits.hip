// Bitwise Hamming distance over bit-packed rows (uint8, 8 features per byte),
// the threshold-filtered sibling that brute-force kNN runs over it, and the
// kernel that packs the sign bits of fp32 / bf16 / fp16 rows.
//
// There is no matrix instruction for xor + popcount, so the contraction runs
// on the vector ALU: per 32-bit word of a pair one v_xor_b32 and one
// v_bcnt_u32_b32, whose second source is the accumulator (the add is free).
// Everything is an exact integer; the result is converted to fp32 once.
//
// Operands: row-major bytes [rows][nbytes_pad], nbytes_pad % 16 == 0, pad
// bytes 0 on both sides (0 ^ 0 has no bits), base 16-byte aligned.
//
// Tile: 128 x 128 outputs per 256-thread block on the XCD super-tiled grid of
// the pairwise kernels (mfma_common.h). Thread (ty, tx) = (tid / 16, tid % 16)
// owns int acc[8][8]: rows gi * 64 + ty * 4 + i, columns gj * 64 + tx * 4 + j
// (gi, gj < 2; i, j < 4), so a row's four columns of one gj are one float4.
//
// K loop: a step is KW = 16 words = 64 B of every row, an 8 KiB panel per
// operand, two (A, B) buffers = 32 KiB of static LDS. Per step one wait and
// one barrier, after which every thread's loads of step t have landed and
// every wave has read step t - 1; then the loads of step t + 1 are issued
// into the other buffer ahead of the ALU work of step t (pairwise_i8.hip's
// scheme). 16-byte global_load_lds, two rounds per operand and step.
//
// LDS layout, and why it is not the XOR swizzle of mfma_common.h: a panel is
// four PLANES, plane g = the g-th 16-byte piece of all 128 rows, and inside a
// plane row r sits at slot p(r) = (r & 64) + (r & 3) * 16 + ((r & 63) >> 2),
// 16 B per slot. A thread's fragment of one row is one ds_read_b128. Its B
// rows are tx * 4 + j (+ 64 gj): for a fixed (gj, j) the 16 tx of a wave read
// 16 CONSECUTIVE slots = 256 contiguous bytes, and the wave's four ty read
// the same 256 bytes (broadcast), so every bank is asked for one address:
// no conflict, however the hardware groups lanes. Its A rows are ty * 4 + i
// (+ 64 gi): a wave's four ty read four consecutive slots, each broadcast to
// 16 lanes. With 64-byte rows stored row-major the 16 B rows of a read are
// 256 B apart, the same banks; an XOR over the four 16-byte pieces of a row
// can spread them over four positions only (the residual 4-way conflict that
// mfma_common.h records for its 64-byte rows). Here that would put LDS time
// (16 reads per 512 ALU instructions) next to ALU time; the permuted planes
// cost nothing, global_load_lds writes lane-linear and each lane fetches the
// (row, piece) that belongs at its slot. Those fetches are 16 B from 64
// different rows per wave instruction instead of whole lines; the kernel
// moves 16 KiB per 2^19 lane-operations, so the load path is far from a limit.
// Planes also make a ragged last step cheap: a step with fewer than four
// pieces left loads and reads only those planes, which is why rows are padded
// to 16 bytes and not to a whole step (a 128-bit code stays 16 B per row).
//
// Registers: 64 accumulators, the 8 B fragments of a plane (32) and 2 of the
// 8 A fragments at a time (8; with 4 at a time the kernels spilled): under
// 128 VGPRs without scratch, four blocks per CU, one wave of each per SIMD. LDS (4 x 32 KiB of 160) never limits, so the filter is not
// given a single-buffer launch at one step as the int8 filter is.
//
// Epilogues: writer -> (float)acc, interior tiles as non-temporal float4
// stores straight from registers (16 lanes x 16 B = 256 B of one row), edge
// tiles guarded scalar stores. Filter -> acc <= thr[row] appended to the
// row's bounded candidate buffer, the contract of pairwise_i8_filter_kernel.
//
// Range: 8 * nbytes_pad <= 2^24, so a count is exact in fp32 as in int32.

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mfma_common.h"

namespace raft_amd {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

namespace {

constexpr int BITS_PLANE = 128 * 16;           // one 16-byte piece of 128 rows
constexpr int BITS_PANEL = 4 * BITS_PLANE;     // one operand of one K step
constexpr int BITS_MAX_BYTES = 1 << 21;        // 2^24 bits

struct BitsTile {
  long long row0, col0;  // first row / column of the block's tile
  int ty, tx;
};

__device__ __forceinline__ bool bits_tile_prologue(int rg, long long m, long long n,
                                                   BitsTile& t, int (&acc)[8][8]) {
  t.ty = threadIdx.x / 16;
  t.tx = threadIdx.x % 16;
  long long rt, ct;
  xcd_supertile_decode(rg, &rt, &ct);
  if (rt * 128 >= m || ct * 128 >= n) return false;
  t.row0 = rt * 128;
  t.col0 = ct * 128;
#pragma unroll
  for (int a = 0; a < 8; a++)
#pragma unroll
    for (int b = 0; b < 8; b++) acc[a][b] = 0;
  return true;
}

// acc += popcount(v) as ONE instruction. From `acc += __popc(v)` the compiler
// makes v_bcnt_u32_b32 with a zero second source and joins two counts with a
// v_add3_u32: 2.5 instructions per word instead of 2.
__device__ __forceinline__ void bits_count(int& acc, unsigned int v) {
  asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(v));
}

// smem: buffer b of step parity b at b * 16 KiB, A panel then B panel. Rows
// past the edge are clamped to the last row: loaded and counted, never stored.
__device__ __forceinline__ void bits_tile_kloop(const unsigned char* __restrict__ xg,
                                                const unsigned char* __restrict__ yg,
                                                char* smem, int (&acc)[8][8],
                                                const BitsTile& t, long long m, long long n,
                                                int nbytes_pad) {
  const int tid = threadIdx.x;
  const int wv = tid / RAFT_AMD_WAVE;
  const int plane0 = tid >> 7;  // round j fills plane 2 j + plane0 (wave-uniform)
  long long ga[2], gb[2];
  int ldst[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int o = j * 4096 + tid * 16;  // linear destination byte
    const int slot = (o >> 4) & 127;    // the row whose piece belongs there
    const int r = (slot & 64) + (slot & 15) * 4 + ((slot >> 4) & 3);
    long long rx = t.row0 + r;
    if (rx > m - 1) rx = m - 1;
    ga[j] = rx * (long long)nbytes_pad + (2 * j + plane0) * 16;
    long long ry = t.col0 + r;
    if (ry > n - 1) ry = n - 1;
    gb[j] = ry * (long long)nbytes_pad + (2 * j + plane0) * 16;
    ldst[j] = j * 4096 + wv * 1024;
  }
  const int pieces = nbytes_pad / 16;
  const int steps = (pieces + 3) / 4;
  // a plane past the row's last piece is neither loaded nor read
  auto issue = [&](int step) {
    char* a = smem + (step & 1) * 2 * BITS_PANEL;
    char* b = a + BITS_PANEL;
    const long long koff = (long long)step * 64;
    const int left = pieces - step * 4;
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (2 * j + plane0 < left) {
        GLOAD_LDS(xg + ga[j] + koff, a + ldst[j]);
        GLOAD_LDS(yg + gb[j] + koff, b + ldst[j]);
      }
  };
  issue(0);
  for (int s = 0; s < steps; s++) {
    // own loads of step s landed, own LDS reads of step s - 1 returned; past
    // the barrier that holds for every thread of the block
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (s + 1 < steps) issue(s + 1);
    const char* a = smem + (s & 1) * 2 * BITS_PANEL;
    const char* b = a + BITS_PANEL;
    const int left = pieces - s * 4;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      if (g >= left) break;
      u32x4 bf[8];
#pragma unroll
      for (int c = 0; c < 8; c++)
        bf[c] = *reinterpret_cast<const u32x4*>(b + g * BITS_PLANE + (c * 16 + t.tx) * 16);
#pragma unroll
      for (int rp = 0; rp < 4; rp++) {  // A rows two at a time: r = gi * 4 + i
        u32x4 af[2];
#pragma unroll
        for (int i = 0; i < 2; i++)
          af[i] = *reinterpret_cast<const u32x4*>(
              a + g * BITS_PLANE + ((rp * 2 + i) * 16 + t.ty) * 16);
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int c = 0; c < 8; c++)
#pragma unroll
            for (int w = 0; w < 4; w++) bits_count(acc[rp * 2 + i][c], af[i][w] ^ bf[c][w]);
      }
    }
  }
}

// acc[gi * 4 + i][gj * 4 + j] is (row0 + gi * 64 + ty * 4 + i,
//                                 col0 + gj * 64 + tx * 4 + j)
__launch_bounds__(256, 4)
__global__ void pairwise_bits_kernel(const unsigned char* __restrict__ x,
                                     const unsigned char* __restrict__ y,
                                     float* __restrict__ out, long long m, long long n,
                                     int nbytes_pad, int rg) {
  __shared__ __attribute__((aligned(16))) char bits_smem[4 * BITS_PANEL];
  BitsTile t;
  int acc[8][8];
  if (!bits_tile_prologue(rg, m, n, t, acc)) return;
  bits_tile_kloop(x, y, bits_smem, acc, t, m, n, nbytes_pad);

  if (t.row0 + 128 <= m && t.col0 + 128 <= n && (n & 3) == 0) {
    // interior (non-temporal: the output is never read back)
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const long long row = t.row0 + (r >> 2) * 64 + t.ty * 4 + (r & 3);
#pragma unroll
      for (int gj = 0; gj < 2; gj++) {
        const f32x4 v4 = {(float)acc[r][gj * 4], (float)acc[r][gj * 4 + 1],
                          (float)acc[r][gj * 4 + 2], (float)acc[r][gj * 4 + 3]};
        __builtin_nontemporal_store(
            v4, reinterpret_cast<f32x4*>(out + row * n + t.col0 + gj * 64 + t.tx * 4));
      }
    }
    return;
  }
  // edge tiles: guarded scalar stores
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const long long row = t.row0 + (r >> 2) * 64 + t.ty * 4 + (r & 3);
    if (row >= m) continue;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const long long col = t.col0 + (c >> 2) * 64 + t.tx * 4 + (c & 3);
      if (col < n) out[row * n + col] = (float)acc[r][c];
    }
  }
}

// candidates with count <= thr[row] go to the row's bounded buffer; a column
// past n never passes, whatever the threshold
__launch_bounds__(256, 4)
__global__ void pairwise_bits_filter_kernel(const unsigned char* __restrict__ x,
                                            const unsigned char* __restrict__ y,
                                            const int* __restrict__ thr,
                                            float* __restrict__ out_d, int* __restrict__ out_i,
                                            int* __restrict__ cnt, int cap,
                                            long long col_offset, long long m, long long n,
                                            int nbytes_pad, int rg) {
  __shared__ __attribute__((aligned(16))) char bits_smem[4 * BITS_PANEL];
  BitsTile t;
  int acc[8][8];
  if (!bits_tile_prologue(rg, m, n, t, acc)) return;
  bits_tile_kloop(x, y, bits_smem, acc, t, m, n, nbytes_pad);

#pragma unroll
  for (int r = 0; r < 8; r++) {
    const long long row = t.row0 + (r >> 2) * 64 + t.ty * 4 + (r & 3);
    if (row >= m) continue;
    const int tv = thr[row];
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const long long col = t.col0 + (c >> 2) * 64 + t.tx * 4 + (c & 3);
      if (col < n && acc[r][c] <= tv) {
        const int pos = atomicAdd(&cnt[row], 1);
        if (pos < cap) {
          out_d[row * cap + pos] = (float)acc[r][c];
          out_i[row * cap + pos] = (int)(col + col_offset);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// bit pack: bit j % 8 of byte j / 8 of a row is x[j] > threshold, compared in
// fp32. One wave per row; lanes read 64 consecutive elements, one ballot is 8
// output bytes, written by lanes 0 .. 7 one byte each (an output row is not
// 8-byte aligned in general). Tail bits are 0.
// ---------------------------------------------------------------------------

__device__ __forceinline__ float bits_widen(float v) { return v; }
__device__ __forceinline__ float bits_widen(_Float16 v) { return (float)v; }
__device__ __forceinline__ float bits_widen(unsigned short v) {  // bf16 bits
  return __uint_as_float((unsigned int)v << 16);
}

template <typename T>
__launch_bounds__(256)
__global__ void pack_bits_kernel(const T* __restrict__ x, unsigned char* __restrict__ out,
                                 long long rows, long long d, long long ld, float threshold) {
  const int lane = threadIdx.x % RAFT_AMD_WAVE;
  const long long row = (long long)blockIdx.x * (256 / RAFT_AMD_WAVE) + threadIdx.x / RAFT_AMD_WAVE;
  if (row >= rows) return;  // the whole wave
  const long long nbytes = (d + 7) / 8;
  for (long long j0 = 0; j0 < d; j0 += RAFT_AMD_WAVE) {
    const long long j = j0 + lane;
    const bool bit = j < d && bits_widen(x[row * ld + j]) > threshold;
    const unsigned long long mask = __ballot(bit);
    const long long byte = j0 / 8 + lane;
    if (lane < 8 && byte < nbytes)
      out[row * nbytes + byte] = (unsigned char)(mask >> (8 * lane));
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

void bits_check_shape(const char* who, long long m, long long n, int nbytes_pad) {
  if (m < 1 || n < 1) throw std::runtime_error(std::string(who) + ": empty operand");
  if (m > 2147483647ll || n > 2147483647ll)
    throw std::runtime_error(std::string(who) + ": rows must be below 2^31");
  if (nbytes_pad < 16 || nbytes_pad % 16 != 0)
    throw std::runtime_error(std::string(who) +
                             ": nbytes_pad must be a positive multiple of 16");
  if (nbytes_pad > BITS_MAX_BYTES)
    throw std::runtime_error(std::string(who) + ": nbytes_pad must be <= 2^21 (fp32 exact)");
}

// blocks of the 8 x 8 super-tiled grid of 128 x 128 tiles; *rg as
// xcd_supertile_decode takes it
dim3 bits_grid(const char* who, long long m, long long n, int* rg) {
  const long long r = (m + 1023) / 1024, c = (n + 1023) / 1024;
  if (r * c * 64 > 2147483647ll)
    throw std::runtime_error(std::string(who) + ": more than 2^31 blocks, split the call");
  *rg = (int)r;
  return dim3((unsigned)(r * c * 64));
}

}  // namespace

void launch_pairwise_bits(const void* x, const void* y, float* out, long long m, long long n,
                          int nbytes_pad, hipStream_t stream) {
  bits_check_shape("pairwise_bits", m, n, nbytes_pad);
  int rg;
  const dim3 grid = bits_grid("pairwise_bits", m, n, &rg);
  rg = -rg;  // column-major walk of the super-tile, as the other writers
  hipLaunchKernelGGL(pairwise_bits_kernel, grid, dim3(256), 0, stream,
                     static_cast<const unsigned char*>(x),
                     static_cast<const unsigned char*>(y), out, m, n, nbytes_pad, rg);
  HIP_CHECK(hipGetLastError());
}

void launch_pairwise_bits_filter(const void* x, const void* y, const int* thr, float* out_d,
                                 int* out_i, int* cnt, int cap, long long col_offset,
                                 long long m, long long n, int nbytes_pad,
                                 hipStream_t stream) {
  bits_check_shape("pairwise_bits_filter", m, n, nbytes_pad);
  if (cap < 1) throw std::runtime_error("pairwise_bits_filter: cap must be positive");
  if (col_offset < 0 || col_offset + n > 2147483647ll)
    throw std::runtime_error("pairwise_bits_filter: column ids must fit int32");
  int rg;
  const dim3 grid = bits_grid("pairwise_bits_filter", m, n, &rg);
  hipLaunchKernelGGL(pairwise_bits_filter_kernel, grid, dim3(256), 0, stream,
                     static_cast<const unsigned char*>(x),
                     static_cast<const unsigned char*>(y), thr, out_d, out_i, cnt, cap,
                     col_offset, m, n, nbytes_pad, rg);
  HIP_CHECK(hipGetLastError());
}

void launch_pack_bits(const void* x, int dtype, unsigned char* out, long long rows,
                      long long d, long long ld, float threshold, hipStream_t stream) {
  if (rows < 1) return;
  if (d < 1 || ld < 0) throw std::runtime_error("pack_bits: d must be positive, ld >= 0");
  const long long blocks = (rows + 3) / 4;
  if (blocks > 2147483647ll) throw std::runtime_error("pack_bits: too many rows");
  const dim3 grid((unsigned)blocks);
  if (dtype == 0)
    hipLaunchKernelGGL(pack_bits_kernel<float>, grid, dim3(256), 0, stream,
                       static_cast<const float*>(x), out, rows, d, ld, threshold);
  else if (dtype == 1)
    hipLaunchKernelGGL(pack_bits_kernel<unsigned short>, grid, dim3(256), 0, stream,
                       static_cast<const unsigned short*>(x), out, rows, d, ld, threshold);
  else if (dtype == 2)
    hipLaunchKernelGGL(pack_bits_kernel<_Float16>, grid, dim3(256), 0, stream,
                       static_cast<const _Float16*>(x), out, rows, d, ld, threshold);
  else
    throw std::runtime_error("pack_bits: dtype must be 0 (fp32), 1 (bf16) or 2 (fp16)");
  HIP_CHECK(hipGetLastError());
}

}  // namespace raft_amd
