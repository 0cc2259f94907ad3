// Exact pairwise L2 / inner product over int8 / uint8 rows on the 8-bit
// integer MFMA (v_mfma_i32_16x16x64_i8), and the threshold-filtered sibling
// that brute-force kNN runs over it. The integer counterpart of
// pairwise_mfma.hip: same 128 x 128 tile, 2 x 2 waves, 16-byte
// global_load_lds staging, XOR swizzle (mfma_common.h) and XCD super-tiled
// grid; the K-loop, the accumulator type and the epilogues are new.
//
// Operands: row-major bytes [rows][d_pad], d_pad % 128 == 0, pad bytes at the
// dtype's zero point (0 for int8, 128 for uint8) so that they add nothing to a
// dot product, a norm or a sum. The MFMA is signed: uint8 fragments are XORed
// with 0x80808080 in registers after the LDS read, so the kernel works on
// u' = u - 128. L2 does not change under the shift; the inner product is put
// back in the epilogue, u.v = acc + 128 (sum u' + sum v') + 16384 d, with the
// real d.
//
// K-loop: one step is 128 features = 128 B per row, so an operand tile is
// [128][128 B] = 16 KiB, byte for byte the shape of the bf16 [128][64] tile.
// A step holds two MFMA K groups kf = 0, 1; a lane reads 16 B at
// swz(r * 128 + kf * 64 + (lane >> 4) * 16) for A and for B alike (which k a
// lane holds does not matter to the sum as long as both sides agree): 32 MFMA
// per step per wave. Two (A, B) buffers, 64 KiB: per step one wait and one
// barrier, after which every thread's loads of step t have landed and every
// wave has read step t - 1, then the loads of step t + 1 are issued into the
// other buffer ahead of the MFMAs of step t. The writer's interior dump needs
// [128][132] fp32 = 67.5 KiB, still two blocks per CU; the filter has no dump
// and at d_pad = 128, a single step, is launched with the one buffer it uses.
//
// Row statistics (row_stats_i8_kernel): int32 norm and sum of every row in the
// shifted domain, 8 lanes per row, 16-byte loads, 8-bit dot4 of the row with
// itself and with 0x01010101, shuffle reduce.
//
// Results: the exact integer, converted to fp32 once; L2Sqrt is the fp64 root
// rounded to fp32 (the contract of ivf_flat_scan_i8.hip).
//
// Range: d_pad <= 4096. In the shifted (or int8) domain |v| <= 128, so
// |acc|, norm <= 128^2 * 4096 = 2^26, |sum| <= 2^19, and
//   L2  = nx + ny - 2 acc              in [0, 4 * 2^26 = 2^28]
//   IP  = acc + 128 (sx + sy) + 16384 d: |128 (sx + sy)| <= 2^27,
//         16384 d <= 2^26, every partial sum below 2^28
// so nothing leaves int32 and the int32 values are the exact integers.

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "mfma_common.h"

namespace raft_amd {

typedef __attribute__((ext_vector_type(4))) int i32x4;

namespace {

constexpr unsigned int I8_FLIP = 0x80808080u;
constexpr int I8_TILE_BYTES = 128 * 128;  // one operand tile of one K step
constexpr int I8_MAX_D = 4096;
constexpr int I8_STAT_LANES = 8;          // lanes per row in the statistics kernel

template <bool SIGNED>
__device__ __forceinline__ unsigned int i8_shift(unsigned int v) {
  return SIGNED ? v : v ^ I8_FLIP;
}

// ---------------------------------------------------------------------------
// row statistics
// ---------------------------------------------------------------------------

template <bool SIGNED>
__launch_bounds__(256)
__global__ void row_stats_i8_kernel(const unsigned char* __restrict__ x,
                                    int* __restrict__ norm, int* __restrict__ sum,
                                    long long rows, int d_pad) {
  const int sub = threadIdx.x % I8_STAT_LANES;
  const long long row =
      (long long)blockIdx.x * (256 / I8_STAT_LANES) + threadIdx.x / I8_STAT_LANES;
  int nn = 0, ss = 0;
  if (row < rows) {
    const uint4* p = reinterpret_cast<const uint4*>(x + row * d_pad);
    for (int c = sub; c < d_pad / 16; c += I8_STAT_LANES) {
      const uint4 v = p[c];
      const unsigned int w[4] = {i8_shift<SIGNED>(v.x), i8_shift<SIGNED>(v.y),
                                 i8_shift<SIGNED>(v.z), i8_shift<SIGNED>(v.w)};
#pragma unroll
      for (int i = 0; i < 4; i++) {
        nn = __builtin_amdgcn_sdot4((int)w[i], (int)w[i], nn, false);
        ss = __builtin_amdgcn_sdot4((int)w[i], 0x01010101, ss, false);
      }
    }
  }
#pragma unroll
  for (int s = I8_STAT_LANES / 2; s >= 1; s >>= 1) {
    nn += __shfl_xor(nn, s);
    ss += __shfl_xor(ss, s);
  }
  if (row < rows && sub == 0) {
    norm[row] = nn;
    sum[row] = ss;
  }
}

// ---------------------------------------------------------------------------
// tile prologue and K-loop
// ---------------------------------------------------------------------------

__device__ __forceinline__ bool i8_tile_prologue(int rg, long long m, long long n,
                                                 MfmaTile& t, i32x4 (&acc)[4][4]) {
  const unsigned w = threadIdx.x / RAFT_AMD_WAVE;
  t.lane = threadIdx.x % RAFT_AMD_WAVE;
  t.wr = w / 2;
  t.wc = w % 2;
  long long rt, ct;
  xcd_supertile_decode(rg, &rt, &ct);
  if (rt * 128 >= m || ct * 128 >= n) return false;
  t.row0 = rt * 128;
  t.col0 = ct * 128;
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = i32x4{0, 0, 0, 0};
  return true;
}

// smem: buffer b of step parity b at b * 32 KiB, A tile then B tile. Rows past
// the edge are clamped to the last row: they are loaded and multiplied, never
// stored.
template <bool SIGNED>
__device__ __forceinline__ void i8_tile_kloop(const unsigned char* __restrict__ xg,
                                              const unsigned char* __restrict__ yg,
                                              char* smem, i32x4 (&acc)[4][4],
                                              const MfmaTile& t, long long m, long long n,
                                              int d_pad) {
  const int tid = threadIdx.x;
  const int wv = tid / RAFT_AMD_WAVE;
  long long ga[4], gb[4];
  int ldst[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int o = j * 4096 + tid * 16;  // linear destination byte
    const int o_src = mfma_swz(o);      // the (row, k byte) that belongs there
    const int r = o_src >> 7;
    const int kb = o_src & 127;
    long long rx = t.row0 + r;
    if (rx > m - 1) rx = m - 1;
    ga[j] = rx * (long long)d_pad + kb;
    long long ry = t.col0 + r;
    if (ry > n - 1) ry = n - 1;
    gb[j] = ry * (long long)d_pad + kb;
    ldst[j] = j * 4096 + wv * 1024;
  }
  auto issue = [&](int step) {
    char* a = smem + (step & 1) * 2 * I8_TILE_BYTES;
    char* b = a + I8_TILE_BYTES;
    const long long koff = (long long)step * 128;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      GLOAD_LDS(xg + ga[j] + koff, a + ldst[j]);
      GLOAD_LDS(yg + gb[j] + koff, b + ldst[j]);
    }
  };
  const int steps = d_pad / 128;
  issue(0);
  for (int s = 0; s < steps; s++) {
    // own loads of step s landed, own LDS reads of step s - 1 returned; past
    // the barrier that holds for every thread of the block
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (s + 1 < steps) issue(s + 1);
    const char* a = smem + (s & 1) * 2 * I8_TILE_BYTES;
    const char* b = a + I8_TILE_BYTES;
#pragma unroll
    for (int kf = 0; kf < 2; kf++) {
      const int kbyte = kf * 64 + (t.lane >> 4) * 16;
      i32x4 af[4], bf[4];
#pragma unroll
      for (int f = 0; f < 4; f++) {
        const int r = t.wr * 64 + f * 16 + (t.lane & 15);
        af[f] = *reinterpret_cast<const i32x4*>(a + mfma_swz(r * 128 + kbyte));
        const int c = t.wc * 64 + f * 16 + (t.lane & 15);
        bf[f] = *reinterpret_cast<const i32x4*>(b + mfma_swz(c * 128 + kbyte));
        if constexpr (!SIGNED) {
          af[f] ^= (int)I8_FLIP;
          bf[f] ^= (int)I8_FLIP;
        }
      }
#pragma unroll
      for (int fr = 0; fr < 4; fr++)
#pragma unroll
        for (int fc = 0; fc < 4; fc++)
          acc[fr][fc] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[fr], bf[fc],
                                                              acc[fr][fc], 0, 0, 0);
    }
  }
}

// ---------------------------------------------------------------------------
// writer. C/D layout as the fp32 MFMA: col = lane & 15 (+ fc * 16),
// row = (lane >> 4) * 4 + reg (+ fr * 16). METRIC 0 squared L2, 1 its root,
// 2 inner product. A value is rt + ct + MUL * acc: for L2 the two norms and
// MUL = -2; for the inner product MUL = 1 and, uint8 only, the shift
// correction rt = 128 sum_x + 16384 d (`bias`), ct = 128 sum_y.
// ---------------------------------------------------------------------------

template <bool SIGNED, int METRIC>
__device__ __forceinline__ int i8_term(const int* __restrict__ stat, long long i, int bias) {
  if constexpr (METRIC != 2) return stat[i];
  if constexpr (SIGNED) return 0;
  return 128 * stat[i] + bias;
}

template <int METRIC>
__device__ __forceinline__ float i8_value(int rt, int ct, int acc) {
  if constexpr (METRIC == 2) return (float)(rt + ct + acc);
  const int v = rt + ct - 2 * acc;
  if constexpr (METRIC == 1) return (float)sqrt((double)v);
  return (float)v;
}

template <bool SIGNED, int METRIC>
__launch_bounds__(256, 2)
__global__ void pairwise_i8_kernel(const unsigned char* __restrict__ x,
                                   const unsigned char* __restrict__ y,
                                   const int* __restrict__ xstat,
                                   const int* __restrict__ ystat, float* __restrict__ out,
                                   long long m, long long n, int d_pad, int bias, int rg) {
  extern __shared__ __attribute__((aligned(16))) char i8_smem[];
  MfmaTile t;
  i32x4 acc[4][4];
  if (!i8_tile_prologue(rg, m, n, t, acc)) return;
  i8_tile_kloop<SIGNED>(x, y, i8_smem, acc, t, m, n, d_pad);

  const long long colb = t.col0 + t.wc * 64 + (t.lane & 15);
  if (t.row0 + 128 <= m && t.col0 + 128 <= n && (n & 3) == 0) {
    // interior: through padded LDS [128][132] fp32, out as coalesced 16-byte
    // pieces of rows (non-temporal: the output is never read back)
    constexpr int LD = 132;
    float* tile = reinterpret_cast<float*>(i8_smem);
    int ct[4];
#pragma unroll
    for (int fc = 0; fc < 4; fc++) ct[fc] = i8_term<SIGNED, METRIC>(ystat, colb + fc * 16, 0);
    __syncthreads();  // every wave is done with the K-loop's LDS
#pragma unroll
    for (int fr = 0; fr < 4; fr++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int rl = t.wr * 64 + fr * 16 + (t.lane >> 4) * 4 + reg;
        const int rt = i8_term<SIGNED, METRIC>(xstat, t.row0 + rl, bias);
#pragma unroll
        for (int fc = 0; fc < 4; fc++)
          tile[rl * LD + t.wc * 64 + fc * 16 + (t.lane & 15)] =
              i8_value<METRIC>(rt, ct[fc], acc[fr][fc][reg]);
      }
    __syncthreads();
    const int tr = threadIdx.x / 32;        // 32 threads x 16 B cover a row
    const int tc = (threadIdx.x % 32) * 4;
#pragma unroll
    for (int rnd = 0; rnd < 16; rnd++) {
      const int rl = rnd * 8 + tr;
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(tile + rl * LD + tc);
      __builtin_nontemporal_store(
          v4, reinterpret_cast<f32x4*>(out + (t.row0 + rl) * n + t.col0 + tc));
    }
    return;
  }
  // edge tiles: guarded scalar stores
#pragma unroll
  for (int fr = 0; fr < 4; fr++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const long long row = t.row0 + t.wr * 64 + fr * 16 + (t.lane >> 4) * 4 + reg;
      if (row >= m) continue;
      const int rt = i8_term<SIGNED, METRIC>(xstat, row, bias);
#pragma unroll
      for (int fc = 0; fc < 4; fc++) {
        const long long col = colb + fc * 16;
        if (col < n)
          out[row * n + col] = i8_value<METRIC>(
              rt, i8_term<SIGNED, METRIC>(ystat, col, 0), acc[fr][fc][reg]);
      }
    }
}

// ---------------------------------------------------------------------------
// filter (squared L2): candidates with dist <= thr[row] go to the row's
// bounded buffer, as pw_filter_epilogue does for the bf16 kernels. A column
// past n never passes, whatever the threshold.
// ---------------------------------------------------------------------------

template <bool SIGNED>
__launch_bounds__(256, 2)
__global__ void pairwise_i8_filter_kernel(const unsigned char* __restrict__ x,
                                          const unsigned char* __restrict__ y,
                                          const int* __restrict__ xn,
                                          const int* __restrict__ yn,
                                          const int* __restrict__ thr,
                                          float* __restrict__ out_d, int* __restrict__ out_i,
                                          int* __restrict__ cnt, int cap, long long col_offset,
                                          long long m, long long n, int d_pad, int rg) {
  extern __shared__ __attribute__((aligned(16))) char i8_smem[];
  MfmaTile t;
  i32x4 acc[4][4];
  if (!i8_tile_prologue(rg, m, n, t, acc)) return;
  i8_tile_kloop<SIGNED>(x, y, i8_smem, acc, t, m, n, d_pad);

  const long long colb = t.col0 + t.wc * 64 + (t.lane & 15);
  int yn_r[4];
  bool ok[4];
#pragma unroll
  for (int fc = 0; fc < 4; fc++) {
    ok[fc] = colb + fc * 16 < n;
    yn_r[fc] = ok[fc] ? yn[colb + fc * 16] : 0;
  }
#pragma unroll
  for (int fr = 0; fr < 4; fr++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const long long row = t.row0 + t.wr * 64 + fr * 16 + (t.lane >> 4) * 4 + reg;
      if (row >= m) continue;
      const int xv = xn[row];
      const int tv = thr[row];
#pragma unroll
      for (int fc = 0; fc < 4; fc++) {
        const int s = xv + yn_r[fc] - 2 * acc[fr][fc][reg];
        if (ok[fc] && s <= tv) {
          const int pos = atomicAdd(&cnt[row], 1);
          if (pos < cap) {
            out_d[row * cap + pos] = (float)s;
            out_i[row * cap + pos] = (int)(colb + fc * 16 + col_offset);
          }
        }
      }
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

void i8_check_shape(const char* who, long long m, long long n, int d_pad) {
  if (m < 1 || n < 1) throw std::runtime_error(std::string(who) + ": empty operand");
  if (d_pad < 128 || d_pad % 128 != 0)
    throw std::runtime_error(std::string(who) + ": d_pad must be a positive multiple of 128");
  if (d_pad > I8_MAX_D)
    throw std::runtime_error(std::string(who) + ": d_pad must be <= 4096 (int32 range)");
}

// blocks of the 8 x 8 super-tiled grid of 128 x 128 tiles; *rg as
// xcd_supertile_decode takes it
dim3 i8_grid(const char* who, long long m, long long n, int* rg) {
  const long long r = (m + 1023) / 1024, c = (n + 1023) / 1024;
  if (r * c * 64 > 2147483647ll)
    throw std::runtime_error(std::string(who) + ": more than 2^31 blocks, split the call");
  *rg = (int)r;
  return dim3((unsigned)(r * c * 64));
}

// Launch Kernel with `lds` bytes of dynamic LDS, raising the kernel's limit
// first where it is above the default 64 KiB
template <auto Kernel, typename... Args>
void i8_launch(dim3 grid, size_t lds, hipStream_t stream, Args... args) {
  static bool raised = false;
  if (lds > 64 * 1024 && !raised) {
    HIP_CHECK(hipFuncSetAttribute((const void*)Kernel,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = true;
  }
  hipLaunchKernelGGL(Kernel, grid, dim3(256), lds, stream, args...);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_row_stats_i8(const void* x, bool is_signed, int* norm, int* sum, long long rows,
                         int d_pad, hipStream_t stream) {
  if (rows < 1) return;
  i8_check_shape("row_stats_i8", rows, 1, d_pad);
  const long long blocks = (rows + 256 / I8_STAT_LANES - 1) / (256 / I8_STAT_LANES);
  if (blocks > 2147483647ll) throw std::runtime_error("row_stats_i8: too many rows");
  const auto* xb = static_cast<const unsigned char*>(x);
  if (is_signed)
    hipLaunchKernelGGL(row_stats_i8_kernel<true>, dim3((unsigned)blocks), dim3(256), 0,
                       stream, xb, norm, sum, rows, d_pad);
  else
    hipLaunchKernelGGL(row_stats_i8_kernel<false>, dim3((unsigned)blocks), dim3(256), 0,
                       stream, xb, norm, sum, rows, d_pad);
  HIP_CHECK(hipGetLastError());
}

void launch_pairwise_i8(const void* x, const void* y, bool is_signed, const int* xnorm,
                        const int* xsum, const int* ynorm, const int* ysum, float* out,
                        long long m, long long n, int d_pad, int d_real, int metric,
                        hipStream_t stream) {
  i8_check_shape("pairwise_i8", m, n, d_pad);
  if (metric < 0 || metric > 2)
    throw std::runtime_error("pairwise_i8: metric must be 0 (L2), 1 (L2 sqrt) or 2 (IP)");
  if (d_real < 1 || d_real > d_pad)
    throw std::runtime_error("pairwise_i8: d_real must be in [1, d_pad]");
  int rg;
  const dim3 grid = i8_grid("pairwise_i8", m, n, &rg);
  rg = -rg;  // column-major walk of the super-tile, as the bf16 writer
  // K-loop 2 x (16 + 16) KiB; the interior dump [128][132] fp32 is larger
  const size_t lds = 128 * 132 * sizeof(float);
  const auto* xb = static_cast<const unsigned char*>(x);
  const auto* yb = static_cast<const unsigned char*>(y);
  const int* xs = metric == 2 ? xsum : xnorm;
  const int* ys = metric == 2 ? ysum : ynorm;
  const int bias = 16384 * d_real;
#define RAFT_PW_I8(S, M)                                                              \
  i8_launch<pairwise_i8_kernel<S, M>>(grid, lds, stream, xb, yb, xs, ys, out, m, n, \
                                      d_pad, bias, rg)
  if (is_signed) {
    if (metric == 0) RAFT_PW_I8(true, 0); else if (metric == 1) RAFT_PW_I8(true, 1);
    else RAFT_PW_I8(true, 2);
  } else {
    if (metric == 0) RAFT_PW_I8(false, 0); else if (metric == 1) RAFT_PW_I8(false, 1);
    else RAFT_PW_I8(false, 2);
  }
#undef RAFT_PW_I8
}

void launch_pairwise_i8_filter(const void* x, const void* y, bool is_signed, const int* xnorm,
                               const int* ynorm, const int* thr, float* out_d, int* out_i,
                               int* cnt, int cap, long long col_offset, long long m,
                               long long n, int d_pad, hipStream_t stream) {
  i8_check_shape("pairwise_i8_filter", m, n, d_pad);
  if (cap < 1) throw std::runtime_error("pairwise_i8_filter: cap must be positive");
  if (col_offset < 0 || col_offset + n > 2147483647ll)
    throw std::runtime_error("pairwise_i8_filter: column ids must fit int32");
  int rg;
  const dim3 grid = i8_grid("pairwise_i8_filter", m, n, &rg);
  // one K step (d_pad = 128) never touches the second buffer: 32 KiB lets
  // four blocks share a CU where 64 KiB lets two
  const size_t lds = (d_pad == 128 ? 2 : 4) * I8_TILE_BYTES;
  const auto* xb = static_cast<const unsigned char*>(x);
  const auto* yb = static_cast<const unsigned char*>(y);
  if (is_signed)
    i8_launch<pairwise_i8_filter_kernel<true>>(grid, lds, stream, xb, yb, xnorm, ynorm, thr,
                                               out_d, out_i, cnt, cap, col_offset, m, n,
                                               d_pad, rg);
  else
    i8_launch<pairwise_i8_filter_kernel<false>>(grid, lds, stream, xb, yb, xnorm, ynorm, thr,
                                                out_d, out_i, cnt, cap, col_offset, m, n,
                                                d_pad, rg);
}

}  // namespace raft_amd
